// The host tail every kernel file shares: the opt-in to more than 64 KiB of dynamic LDS, the occupancy calculator, the
// launch.  The kernel is a template parameter, so each instantiation owns its flags and nobody keeps a list of them.
// The device is the current one: every path to a launcher has gone through use_device / CtxGuard.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>

namespace oth {

// Opts K into lds_bytes of dynamic LDS, once per device.  A device without a slot (the query failed, or its index is past
// the table) is armed on every call; a failed call leaves its slot unarmed.
template <auto K> hipError_t arm_lds(size_t lds_bytes) {
    constexpr int kSlots = 64;
    static std::atomic<bool> opted[kSlots];
    if (lds_bytes <= 64 * 1024) return hipSuccess;
    int dev = -1;
    const bool slot = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kSlots;
    if (slot && opted[dev].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess && slot) opted[dev].store(true, std::memory_order_release);
    return e;
}

template <auto K, typename... Args>
hipError_t launch_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args &...args) {
    const hipError_t e = arm_lds<K>(lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(K, grid, block, lds_bytes, stream, args...);
    return hipGetLastError();
}

// Workgroups of K one CU holds (the occupancy calculator's answer, cached per instantiation); `fallback` where it fails.
template <auto K> int resident_blocks(int threads, size_t lds_bytes, int fallback = 1) {
    static std::atomic<int> cached{0};
    int n = cached.load(std::memory_order_acquire);
    if (n > 0) return n;
    if (arm_lds<K>(lds_bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, K, threads, lds_bytes) != hipSuccess || n < 1)
        return fallback;
    cached.store(n, std::memory_order_release);
    return n;
}

}  // namespace oth
