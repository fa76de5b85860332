// Pinned loads: inline-asm global loads at (uniform row base in scalar registers) + (the lane's 32-bit byte offset), and
// the waits that make their registers valid.  One lane-offset register serves every row of a segment, and the compiler
// can neither move such a load nor gather it with its neighbours: left to itself it forms thirty-two 64-bit row
// addresses per lane, keeps them across the loop and spills them (welch32k.hip), or hoists sixteen loop-invariant window
// loads into sixteen registers that two segments in flight need (welch4096.hip, welch16k1x.hip); the next segment's loads
// are spread over the step on purpose.
//
// A register written by an inline-asm load is NOT valid until the s_waitcnt that covers it, and the compiler does not
// know: to it the value exists from the asm on.  Two things follow (tools/isa_async_hazard.py checks the shipped code
// objects for both, tests/test_abi_cpu.py runs it):
//   * a wait has to NAME the registers it makes valid, or nothing keeps an instruction that reads them behind it (the
//     bare `s_waitcnt lgkmcnt(0)` in front of the last segment's tail was overtaken by the sixty instructions of its
//     first butterfly layer - late round 5; it only worked because a vmcnt wait happened to stand in between);
//   * naming them as in-out operands ("+v") is not enough when the value has to end up somewhere else (the kept half of
//     the 50 %-overlap builds): the compiler then copies the INPUT of the wait into the register it wants, i.e. reads
//     the loading register in front of the wait.  vm_arrive8 takes the loading registers as inputs only and hands out
//     fresh ones, wait and copies in one statement.
#pragma once
#include <hip/hip_runtime.h>

namespace oth {
namespace {

typedef float f2v __attribute__((ext_vector_type(2)));      // a register pair the inline asm below can name as one operand

// 8-byte load; _nt: non-temporal, for samples that are read once
__device__ __forceinline__ void load_row8(f2v &dst, unsigned lane_off, const void *row) {
    asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(dst) : "v"(lane_off), "s"(row) : "memory");
}
__device__ __forceinline__ void load_row8_nt(f2v &dst, unsigned lane_off, const void *row) {
    asm volatile("global_load_dwordx2 %0, %1, %2 nt" : "=v"(dst) : "v"(lane_off), "s"(row) : "memory");
}
// 4-byte load (window values: L2-resident, so not non-temporal)
__device__ __forceinline__ void load_row4(float &dst, unsigned lane_off, const void *row) {
    asm volatile("global_load_dword %0, %1, %2" : "=v"(dst) : "v"(lane_off), "s"(row) : "memory");
}

#define OTH_IO4(r) "+v"((r)[0]), "+v"((r)[1]), "+v"((r)[2]), "+v"((r)[3])
#define OTH_IO8(r) OTH_IO4(r), "+v"((r)[4]), "+v"((r)[5]), "+v"((r)[6]), "+v"((r)[7])
#define OTH_IO16(r) OTH_IO8(r), "+v"((r)[8]), "+v"((r)[9]), "+v"((r)[10]), "+v"((r)[11]), "+v"((r)[12]), "+v"((r)[13]), "+v"((r)[14]), "+v"((r)[15])

// every vector-memory load of this wave has landed: r[..] (pairs or single values) are valid behind this statement, in place
template <class T> __device__ __forceinline__ void vm_arrived16(T (&r)[16]) { asm volatile("s_waitcnt vmcnt(0)" : OTH_IO16(r) : : "memory"); }
template <class T> __device__ __forceinline__ void vm_arrived8(T (&r)[8]) { asm volatile("s_waitcnt vmcnt(0)" : OTH_IO8(r) : : "memory"); }
// all but the youngest eight loads have landed (the caller has issued the NEXT batch of eight behind this one)
template <class T> __device__ __forceinline__ void vm_arrived8_keep8(T (&r)[8]) { asm volatile("s_waitcnt vmcnt(8)" : OTH_IO8(r) : : "memory"); }
// wait, then out[i] = in[i] in fresh registers (eight pairs)
__device__ __forceinline__ void vm_arrive8(float2 (&out)[8], const f2v (&in)[8]) {
    f2v o[8];
    asm volatile("s_waitcnt vmcnt(0)\n\t"
                 "v_mov_b64 %0, %8\n\tv_mov_b64 %1, %9\n\tv_mov_b64 %2, %10\n\tv_mov_b64 %3, %11\n\t"
                 "v_mov_b64 %4, %12\n\tv_mov_b64 %5, %13\n\tv_mov_b64 %6, %14\n\tv_mov_b64 %7, %15"
                 : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
                 : "v"(in[0]), "v"(in[1]), "v"(in[2]), "v"(in[3]), "v"(in[4]), "v"(in[5]), "v"(in[6]), "v"(in[7])
                 : "memory");
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = make_float2(o[i].x, o[i].y);
}
// every LDS read of this wave has landed (with the workgroup barrier: lds_barrier() for a wave that holds reads in flight)
__device__ __forceinline__ void lds_arrived16(f2v (&r)[16]) { asm volatile("s_waitcnt lgkmcnt(0)" : OTH_IO16(r) : : "memory"); }
__device__ __forceinline__ void lds_barrier_arrived16(f2v (&r)[16]) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" : OTH_IO16(r) : : "memory");
}

}  // namespace
}  // namespace oth
