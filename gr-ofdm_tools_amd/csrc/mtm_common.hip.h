// What the taper-loop kernels (mtm.hip: one channel, mtmcsd.hip: two, mtmftest.hip: the F-test, welchsk.hip: spectral
// kurtosis with the plan's window as the one taper, mtmjack.hip: the jackknife's second pass, mtmadapt.hip: the adaptive
// weighting, welchpfb.hip: the filter bank's fold, which takes the pilot and the block sum) share: the fixed-order sums
// behind a segment's pilot and residual mean, the segment entry built on them, the taper product, the rule for keeping a
// segment's samples in registers, the list of sizes with its dispatch over (size, build), and the launchers' thread and LDS rules.
#pragma once
#include "fft_lds.hip.h"

#include <type_traits>

namespace oth {

// `red` of the taper-loop kernels: red[0] holds the pilot, red[1 ..] are block_sum's T / 64 slots (base 1)
constexpr int kMtmPilot = 64;      // samples behind the pilot (the first wave's lanes)

// the mean of the segment's first min(64, nperseg) samples, the same bits in every thread (red[0])
__device__ __forceinline__ float2 mtm_pilot(const float2 *__restrict__ xs, int nperseg, float2 *red, int tid) {
    if (tid < kMtmPilot) {
        const int np = nperseg < kMtmPilot ? nperseg : kMtmPilot;
        float2 t = tid < np ? xs[tid] : make_float2(0.f, 0.f);
        t = wave_sum(t);
        const float inv = 1.0f / (float)np;
        if (tid == 0) red[0] = make_float2(t.x * inv, t.y * inv);
    }
    __syncthreads();
    return red[0];
}

// Segment entry of the taper-loop kernels as one call (mtm_kernel's arithmetic, operation for operation): the pilot comes
// off every sample, then the residual mean - a block sum in a fixed order - comes off.  KEEP: v[q] holds the detrended
// sample tid + q T (zero behind nperseg); otherwise the caller forms csub(csub(xs[n], pil), mean) again where it needs it,
// and without detrend nothing is read here.  Without detrend pil = mean = 0.  Every thread of the workgroup calls it.
template <int N, int T, bool KEEP>
__device__ __forceinline__ void mtm_segment_entry(const float2 *__restrict__ xs, int nperseg, bool detrend, float2 *red, int tid,
                                                  float2 (&v)[KEEP ? N / T : 1], float2 &pil, float2 &mean) {
    constexpr int NQ = N / T;
    pil = mean = make_float2(0.f, 0.f);
    if (detrend) pil = mtm_pilot(xs, nperseg, red, tid);
    if (!KEEP && !detrend) return;
    float2 sum = make_float2(0.f, 0.f);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int n = tid + q * T;
        const float2 r = (n < nperseg) ? csub(xs[n], pil) : make_float2(0.f, 0.f);
        if constexpr (KEEP) v[q] = r;
        sum = cadd(sum, r);
    }
    if (detrend) {
        const float2 tot = block_sum<T>(sum, red, tid, 1);
        const float inv = 1.0f / (float)nperseg;
        mean = make_float2(tot.x * inv, tot.y * inv);
    }
    if constexpr (KEEP) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int n = tid + q * T;
            v[q] = (n < nperseg) ? csub(v[q], mean) : make_float2(0.f, 0.f);
        }
    }
}

// (x - pilot - mean) v_k of one channel into buf, after mtm_segment_entry; no barrier
template <int N, int T, bool KEEP>
__device__ __forceinline__ void mtm_taper_product(const float2 *__restrict__ xs, const float *__restrict__ w, int nperseg, int tid,
                                                  float2 pil, float2 mean, const float2 (&v)[KEEP ? N / T : 1], float2 *buf) {
#pragma unroll
    for (int q = 0; q < N / T; ++q) {
        const int n = tid + q * T;
        float2 r;
        if constexpr (KEEP) {
            r = v[q];
        } else {
            r = (n < nperseg) ? csub(csub(xs[n], pil), mean) : make_float2(0.f, 0.f);      // the same arithmetic as KEEP
        }
        const float wn = w[n];
        buf[n] = make_float2(r.x * wn, r.y * wn);
    }
}

constexpr bool mtm_keep(int n) { return n < 8192; }      // mtm.hip's header: KEEP
constexpr int kMtmRedSlots = 32;                         // float2 slots of one `red` array (T / 64 + 1 <= 17 used)
// Threads of the kernels that keep several spectra or rows of sums next to the butterflies (mtmcsd, the two-channel jackknife,
// welchcyc, welchlag, welchmat): twice the coverage kernels' at 4096 and 8192 points, N / T = 8 there.  The others run
// generic_threads.
constexpr int stat_threads(int n) { return n == 4096 ? 512 : n == 8192 ? 1024 : generic_threads(n); }
// dynamic LDS of a launch: `buffers` transform buffers of nfft points and `reds` red arrays behind them
inline size_t stat_lds_bytes(int nfft, int buffers = 1, int reds = 1) {
    return (size_t)buffers * nfft * sizeof(float2) + (size_t)reds * kMtmRedSlots * sizeof(float2);
}

#define OTH_MTM_FOR_EACH_N(X) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096) X(8192) X(16384)

// f(std::integral_constant<int, N>) of the listed size nfft, `otherwise` for any other: the dispatch behind a kernel file's
// *_blocks_per_cu(nfft) and launch_*(nfft, ...), whose lambdas name the build of size N = decltype(n)::value.
template <typename R, typename F> R mtm_for_size(int nfft, R otherwise, F f) {
    switch (nfft) {
#define X(N) \
    case N: return f(std::integral_constant<int, N>{});
        OTH_MTM_FOR_EACH_N(X)
#undef X
        default: return otherwise;
    }
}

// f(std::integral_constant<int, N>, std::integral_constant<int, B>) of the listed size nfft and the build `build` out of B...
// (welchcyc's 1, 2, 4 cycle frequencies per workgroup; welchmat's capacities), `otherwise` for any other size or build.
template <int... B, typename R, typename F> R mtm_for_build(int nfft, int build, R otherwise, F f) {
    return mtm_for_size(nfft, otherwise, [&](auto n) {
        R r = otherwise;
        (void)((build == B && (r = f(n, std::integral_constant<int, B>{}), true)) || ...);
        return r;
    });
}

}  // namespace oth
