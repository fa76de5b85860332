// Spectral kurtosis (Nita & Gary) of a Welch plan: per segment m and bin j, P_m = g |FFT((x_m - mean_m) w)[j]|^2 with
// g = 1 / sum w^2, and over the M segments of a stream
//   S1 = sum_m P_m,   S2 = sum_m P_m^2;   sk_finalize_kernel turns the two rows into
//   SK = (M + 1) / (M - 1) (M S2 / S1^2 - 1)   and, where asked for, the plan's PSD row = S1 scale / (g M).
// SK does not depend on g; g keeps P near the input's variance, so P^2 overflows float32 only where |X|^2 itself is
// within a factor sum w^2 of doing so.
//
// The body is mtm_kernel's with a whole segment as the work item and the plan's window as the one taper: a stream's
// segments go to W workgroups in contiguous runs, segment entry is mtm_segment_entry (pilot, residual mean), then the
// window product into LDS, fft_lds, and per owned bin s1 += P, s2 = fma(P, P, s2).  The run's two rows leave as
// partial[stream][wg][2][N] in natural bin order; the finalize kernel adds them in double in a fixed order, so a result
// depends on the launch shape only - bit-identical from run to run.
//
// Where the state lives:
//   64 ... 2048 points    the segment's samples stay in registers between the mean and the window product (KEEP);
//                         above, they are read again (from L2: one tile against the passes a transform moves through LDS),
//                         and without detrend they are read once.
//   64 ... 8192 points    the running sums in registers, two per owned bin (ACCREG).
//   16384 points          1024 threads, 128 registers per lane: the running sums live in the workgroup's own partial rows
//                         as in mtmftest.hip - the first segment of a run stores them, every later one reads, adds and
//                         stores, each thread its own addresses, so no barrier.
#include "mtm_common.hip.h"
#include "out_stage.hip.h"
#include "launch.h"

namespace oth {
namespace {

constexpr bool sk_keep(int n) { return n <= 2048; }       // the segment's samples in registers across the mean
constexpr bool sk_accreg(int n) { return n < 16384; }     // running S1 / S2 in registers (else the partial rows)

template <int N, int T, bool KEEP, bool ACCREG> __global__ __launch_bounds__(T) void welch_sk_kernel(WelchSkArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *buf = reinterpret_cast<float2 *>(smem);
    float2 *red = buf + N;      // [0] the pilot, [1 ...] the block sum's wave rows
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y;
    const long long s0 = (p.nseg * wg) / W, s1 = (p.nseg * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    float *dst = p.partial + ((size_t)stream * W + wg) * 2 * N;      // [0] S1, [1] S2
    const float g = p.g;

    float a1[ACCREG ? NQ : 1], a2[ACCREG ? NQ : 1];
    if constexpr (ACCREG) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) a1[q] = a2[q] = 0.f;
    }
    float2 v[KEEP ? NQ : 1];

    for (long long s = s0; s < s1; ++s) {
        const bool first = s == s0;      // of the run: its sums start here
        int tid = tid0;                  // an opaque copy, as in mtm_kernel: the passes' index arithmetic is not hoisted
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step;
        float2 pil, mean;
        mtm_segment_entry<N, T, KEEP>(xs, p.nperseg, p.detrend != 0, red, tid, v, pil, mean);
        // mtm_taper_product spelled out: through the call every build of this kernel comes out scheduled differently
        const float *__restrict__ w = p.win;      // zero-extended to N
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int n = tid + q * T;
            float2 r;
            if constexpr (KEEP) {
                r = v[q];
            } else {
                r = (n < p.nperseg) ? csub(csub(xs[n], pil), mean) : make_float2(0.f, 0.f);      // the same arithmetic as KEEP
            }
            const float wn = w[n];
            buf[n] = make_float2(r.x * wn, r.y * wn);
        }
        __syncthreads();
        fft_lds<N, T>(buf, p.tw, tid);
        if constexpr (ACCREG) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float2 X = buf[tid + q * T];
                const float P = g * fmaf(X.x, X.x, X.y * X.y);
                a1[q] += P;
                a2[q] = fmaf(P, P, a2[q]);
            }
        } else {
            // four bins at a time, so that the loads in flight do not outgrow the registers
#pragma unroll 4
            for (int q = 0; q < NQ; ++q) {
                const int j = tid + q * T;
                const float2 X = buf[j];
                const float P = g * fmaf(X.x, X.x, X.y * X.y);
                float b1 = 0.f, b2 = 0.f;
                if (!first) {
                    b1 = dst[j];
                    b2 = dst[N + j];
                }
                dst[j] = b1 + P;
                dst[N + j] = fmaf(P, P, b2);
            }
        }
        __syncthreads();
    }
    if constexpr (ACCREG) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            dst[tid0 + q * T] = a1[q];
            dst[N + tid0 + q * T] = a2[q];
        }
    }
}

// The shared finalize stage (out_stage.hip.h) on the two rows S1, S2; then SK in double and the one or two rows.
__global__ __launch_bounds__(256) void sk_finalize_kernel(SkFinalizeArgs a) {
    const int k = blockIdx.x * 32 + (threadIdx.x & 31), stream = blockIdx.y;
    int i;
    const bool live = out_slot(a.out, a.nfft, k, i);
    const float *base = a.partial + (size_t)stream * a.W * 2 * a.nfft + k;
    double t[2];
    if (!slice_sums<2>(live, a.W, [&](int w, int r) { return base[((size_t)w * 2 + r) * a.nfft]; }, t)) return;
    const double t1 = t[0], t2 = t[1];
    // an empty bin (silence, a constant under detrend, the DC bin of a noiseless detrended input) reads 0: no 0 / 0
    float sk;
    if (t1 > 0.0) sk = (float)(a.mp1_over_mm1 * (a.m * t2 / (t1 * t1) - 1.0));
    else if (t1 == 0.0) sk = 0.f;
    else sk = __builtin_nanf("");      // non-finite input
    const size_t o = (size_t)stream * a.out.nout + i;
    a.sk_out[o] = sk;
    if (a.psd_out) a.psd_out[o] = psd_value(a.out, t1 * a.psd_scale);
}

}  // namespace

#define OTH_SK_KERNEL(N) welch_sk_kernel<N, generic_threads(N), sk_keep(N), sk_accreg(N)>

int welch_sk_blocks_per_cu(int nfft) {
    return mtm_for_size(nfft, 0, [](auto n) {
        constexpr int N = decltype(n)::value;
        return resident_blocks<OTH_SK_KERNEL(N)>(generic_threads(N), stat_lds_bytes(N), 0);
    });
}

hipError_t launch_welch_sk(int nfft, const WelchSkArgs &a, hipStream_t s) {
    const dim3 grid(a.wg_per_stream, a.nstreams);
    return mtm_for_size(nfft, hipErrorInvalidValue, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return launch_lds<OTH_SK_KERNEL(N)>(grid, dim3(generic_threads(N)), stat_lds_bytes(N), s, a);
    });
}

hipError_t launch_sk_finalize(const SkFinalizeArgs &a, int nstreams, hipStream_t s) {
    return launch_stat_finalize<sk_finalize_kernel>(a, nstreams, 1, s);
}

}  // namespace oth
