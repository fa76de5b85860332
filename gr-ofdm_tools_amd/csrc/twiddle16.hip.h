// The inter-pass twiddle of every radix-16 transform kernel: sixteen butterfly outputs times W^k, k = 0..15, each product
// handed to the caller's put(k, value) - a strided LDS scatter, a swizzled write, the register itself.
#pragma once
#include <type_traits>
#include "fft_lds.hip.h"

namespace oth {
namespace {

// position of output k of dft16() inside v[]
__host__ __device__ constexpr int r16(int k) { return 4 * (k & 3) + (k >> 2); }

template <int I, int N, class F> __device__ __forceinline__ void static_for(F f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// W^k is rebuilt with every call as W^(4i) W^j, k = 4i + j, from a few powers the caller keeps, instead of fifteen stored
// (30 VGPRs) or loaded values.  Loading them from an LDS table costs more than the arithmetic: hipcc issues one table
// read, waits lgkmcnt(0), multiplies and writes - fifteen exposed LDS round trips per exchange.
// The products are loop-invariant, so left alone the compiler hoists them out of the segment loop and keeps them in
// registers after all (+36 VGPRs per pass).  Each builder below therefore passes one factor of every product through an
// empty asm: an opaque copy, a v_mov per register and call, that the compiler cannot see through.
//   two seeds (W, W^4): both opaque, squared and cubed on the spot - thirteen products per call, chains of up to three.
//   six stored (W, W^2, W^3, W^4, W^8, W^12): nine products, at most ONE per twiddle, at eight more registers for the
//     caller.  Every product has a W^j factor, so those three are the opaque ones (six copies instead of twelve).  With
//     correctly rounded table values this is the form for single rows: with a strong off-bin tone in a rectangular-window
//     periodogram the rounding of a chain of three shows in every bin (the tone's bins carry 2 sqrt(N) times the noise
//     amplitude), enough to break 1e-4.
struct Pow6 {
    float2 j1, j2, j3, i1, i2, i3;      // W^1, W^2, W^3, W^4, W^8, W^12
};
__device__ __forceinline__ Pow6 pow6_load(const float2 *tw, int e) {
    return Pow6{tw[e], tw[2 * e], tw[3 * e], tw[4 * e], tw[8 * e], tw[12 * e]};
}
// What one call multiplies by: wj[j] = W^j, wi[i] = W^(4i) ([0] unused).  Built where the twiddle is applied, inside the
// segment loop, by one of the two builders: Tw16(W, W^4) or Tw16::stored(six).  (One is a constructor and the other a
// function that returns its result on purpose: written the other way round, each comes out of the compiler with the
// operands of some v_mul_f32 swapped in every kernel that uses it.  Same bits, but then no two builds compare equal.)
struct Tw16 {
    float2 wj[4], wi[4];
    __device__ __forceinline__ Tw16(float2 p1, float2 p4) {      // from two seeds
        wj[1] = p1;
        wi[1] = p4;
        asm volatile("" : "+v"(wj[1].x), "+v"(wj[1].y), "+v"(wi[1].x), "+v"(wi[1].y));
        wj[2] = cmul(wj[1], wj[1]);
        wj[3] = cmul(wj[2], wj[1]);
        wi[2] = cmul(wi[1], wi[1]);
        wi[3] = cmul(wi[2], wi[1]);
    }
    __device__ __forceinline__ Tw16() {}      // (for stored())
    static __device__ __forceinline__ Tw16 stored(const Pow6 &p) {      // from six stored
        Tw16 w;
        w.wj[1] = p.j1, w.wj[2] = p.j2, w.wj[3] = p.j3;
        w.wi[1] = p.i1, w.wi[2] = p.i2, w.wi[3] = p.i3;
        asm volatile("" : "+v"(w.wj[1].x), "+v"(w.wj[1].y), "+v"(w.wj[2].x), "+v"(w.wj[2].y), "+v"(w.wj[3].x), "+v"(w.wj[3].y));
        return w;
    }
    // v[r16(k)] * W^k, k = 1..15
    __device__ __forceinline__ float2 times(const float2 (&v)[16], int k) const {
        const int i = k >> 2, j = k & 3;
        const float2 tw = (i == 0) ? wj[j] : ((j == 0) ? wi[i] : cmul(wi[i], wj[j]));
        return cmul(v[r16(k)], tw);
    }
};

// put(k, v[r16(k)] * W^k) for k = 0..15.  k is the int of an unrolled loop, or with IMM a std::integral_constant for a put
// that needs it as an asm immediate (segfft.hip).  The compiler schedules the two halves of a product the other way round
// between the two forms, so IMM is not the form for everybody: each kernel takes the one it was tuned with.
template <bool IMM = false, class F> __device__ __forceinline__ void twiddle16(const float2 (&v)[16], const Tw16 &w, F put) {
    if constexpr (IMM) {
        put(std::integral_constant<int, 0>{}, v[0]);      // r16(0) == 0
        static_for<1, 16>([&](auto kc) { put(kc, w.times(v, decltype(kc)::value)); });
    } else {
        put(0, v[0]);
#pragma unroll
        for (int k = 1; k < 16; ++k) put(k, w.times(v, k));
    }
}

// The SYMMETRIC flavour (welch4096ws.hip's complementary-window build): the output digit k is read as a signed digit
// d = k or k - 16 in [-8, 8) and the caller measures its own index from the middle of its range, so every angle
// theta = d * (caller's step) stays inside (-0.55 pi, 0.55 pi).  There the rotation v e^(-i theta) is three shears,
//     x1 = x + t y,  y1 = y - s x1,  x2 = x1 + t y1,   t = tan(theta / 2), s = sin(theta)   (|t| < 1.2),
// three v_fma_f32 instead of cmul's four instructions, exact in real arithmetic, no scale left behind.  t and s are odd in
// theta: the eight stored pairs of |d| = 1..8 serve all fifteen rotations, the conjugate is the operand negation of
// v_fma_f32 (free).  Nothing is formed from the stored pairs, so there is nothing for the compiler to hoist and no opaque
// copy.  ts[m - 1] = (tan, sin) of m * (caller's step), signed as the step is (symtw_table(), abi_ctx.hip).
__host__ __device__ constexpr int sym16(int k) { return k < 8 ? k : k - 16; }
template <bool CONJ> __device__ __forceinline__ float2 rot3(float2 v, float2 ts) {
    const float t = CONJ ? -ts.x : ts.x, s = CONJ ? -ts.y : ts.y;
    const float x1 = fmaf(t, v.y, v.x);
    const float y1 = fmaf(-s, x1, v.y);
    return make_float2(fmaf(t, y1, x1), y1);
}
// put(k, v[r16(k)] * e^(-i sym16(k) theta)) for k = 0..15, theta the angle of ts[0]
template <class F> __device__ __forceinline__ void twiddle16_sym(const float2 (&v)[16], const float2 (&ts)[8], F put) {
    put(0, v[0]);
#pragma unroll
    for (int k = 1; k < 16; ++k) put(k, k < 8 ? rot3<false>(v[r16(k)], ts[k - 1]) : rot3<true>(v[r16(k)], ts[15 - k]));
}
template <int STRIDE> __device__ __forceinline__ void scatter_sym16(const float2 (&v)[16], float2 *out, const float2 (&ts)[8]) {
    twiddle16_sym(v, ts, [&](int k, float2 val) { out[STRIDE * k] = val; });
}

// out[STRIDE * k] = v[r16(k)] * W^k from two seeds / from six stored powers
template <int STRIDE>
__device__ __forceinline__ void scatter_pow16(const float2 (&v)[16], float2 *out, float2 p1, float2 p4) {
    twiddle16(v, Tw16(p1, p4), [&](int k, float2 val) { out[STRIDE * k] = val; });
}
template <int STRIDE> __device__ __forceinline__ void scatter_pow16_six(const float2 (&v)[16], float2 *out, const Pow6 &w) {
    twiddle16(v, Tw16::stored(w), [&](int k, float2 val) { out[STRIDE * k] = val; });
}

}  // namespace
}  // namespace oth
