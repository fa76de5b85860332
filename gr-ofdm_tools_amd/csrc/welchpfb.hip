// Polyphase filter-bank (weighted overlap-add, WOLA) PSD of a Welch plan with nperseg = nfft = N: a real prototype h of
// P N taps (P taps per branch, 2 ... 16) is folded onto one transform length in front of the FFT.  Per stream and frame s,
// with n < N,
//   m_s    = (1 / (P N)) sum_{i < P N} x[s step + i]                 on a detrending plan, 0 otherwise
//   y_s[n] = sum_{p < P} h[n + p N] (x[s step + n + p N] - m_s)
//   X_s    = FFT_N(y_s),   S = sum_s |X_s|^2;
// the finalize launch turns the row into pfb = scale S / M through the shared output stage.  X_s is every P-th bin of the
// P N-point transform of h (x - m_s): a bin has the prototype's flat top and a stop band that starts one bin away, where a
// window no longer than the transform leaves a skirt.  The plan's own window takes no part.
//
// The body is welchsk.hip's (a whole frame per work item, a stream's frames to W workgroups in contiguous runs, one LDS
// buffer, fft_lds) with the fold in front of it.  The fold makes one pass over the frame's P N samples: thread tid owns the
// points n = tid + q T and for p = 0 ... P - 1 loads x[n + p N] and h[n + p N], both coalesced, and adds h (x - pil) to
// y[q] and x - pil to its part of the frame's sum.  pil is the taper-loop kernels' pilot (mtm_pilot: the mean of the frame's
// first 64 samples), taken on detrending plans only.  The residual mean m = block_sum / (P N) then comes off by linearity,
//   y[q] -= m hfold[n],   hfold[n] = sum_p h[n + p N]   (a second table of N floats, formed in double on the host),
// so a frame is read once for the mean and the fold together and N / T complex accumulators are live whatever P is.  Without
// detrend nothing is subtracted and no sum is formed.
//
// What a workgroup reads: the host counts M = (nsamples - P N) / step + 1 frames, so the furthest sample of the last frame,
// (M - 1) step + P N - 1, lies inside the stream's own nsamples.  That is the bound of every load of x here; h is read at
// n + p N < P N and hfold at n < N.
//
// Where the state lives:
//   y                     N / T complex accumulators in registers, dead once they are in LDS.
//   sums                  one running row of |X|^2 per workgroup, N / T floats per thread in registers at every size: with
//                         one row next to the butterflies every build comes out without scratch, the 1024 threads of
//                         16384 points at 117 of their 128 registers (tests/test_welch_pfb_cpu.py reads the code objects),
//                         so there is no build that keeps the row in memory as welchsk.hip's does at 16384 points.
// The rows leave as partial[stream][wg][N] in natural bin order.  The finalize launch is lag_finalize_kernel's (welchlag.hip)
// on one row per workgroup: slice_sums<1> adds the workgroups' rows in double in a fixed order, so a result depends on the
// launch shape only - bit-identical from run to run.
//
// Degenerate input.  All-zero input gives a row of exact zeros.  A constant on a detrending plan does too (-inf under dB):
// the pilot is a tree sum of 64 equal floats times 1 / 64, which is exact, so x - pil is 0 in every sample, and so are the
// sum, m and y.  A NaN or +-inf sample inside a stream's frames makes its y - and with detrend m, so all of y - non-finite;
// every bin of the transform depends on every point, so every running sum of the row is NaN or inf, and store_psd's
// finite_power turns both into NaN: the stream's row reads NaN in every bin, linear or dB, never inf.  Other streams of the
// launch share no workgroup, no sum and no partial row with it.
//
// With step = N consecutive frames of a run share (P - 1) N samples; the re-reads go to L2 (one frame of 16384 x 16 points
// is 2 MiB against 4 MiB per XCD).
//
// Not here: a sliding register window that carries P - 1 blocks across a run, complex prototypes, the bank's time-domain
// outputs in the circular-shift form that keeps phase continuity between hops (chanpfb.hip; power does not need it),
// time-sharded partials, multitaper plans, the median average, transform lengths that are not a power of two.
#include "mtm_common.hip.h"
#include "out_stage.hip.h"
#include "launch.h"

namespace oth {
namespace {

template <int N, int T> __global__ __launch_bounds__(T) void welch_pfb_kernel(WelchPfbArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *buf = reinterpret_cast<float2 *>(smem);
    float2 *red = buf + N;      // [0] the pilot, [1 ...] the block sum's wave rows
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y;
    const long long s0 = (p.nseg * wg) / W, s1 = (p.nseg * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    float *dst = p.partial + ((size_t)stream * W + wg) * N;
    const int P = p.ntaps;
    const bool detrend = p.detrend != 0;
    const float inv_len = 1.0f / (float)(P * N);

    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;

    for (long long s = s0; s < s1; ++s) {
        int tid = tid0;                  // an opaque copy, as in mtm_kernel: the passes' index arithmetic is not hoisted
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step;      // xs[i], i < P N: inside the stream, by the host's frame count
        float2 pil = make_float2(0.f, 0.f);
        if (detrend) pil = mtm_pilot(xs, N, red, tid);
        float2 y[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) y[q] = make_float2(0.f, 0.f);
        float2 sum = make_float2(0.f, 0.f);
        const float2 *__restrict__ xp = xs + tid;
        const float *__restrict__ hp = p.win + tid;
        for (int t = 0; t < P; ++t, xp += N, hp += N) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float2 r = csub(xp[q * T], pil);
                const float h = hp[q * T];
                y[q].x = fmaf(h, r.x, y[q].x);
                y[q].y = fmaf(h, r.y, y[q].y);
                sum = cadd(sum, r);
            }
        }
        if (detrend) {
            const float2 tot = block_sum<T>(sum, red, tid, 1);
            const float2 mean = make_float2(tot.x * inv_len, tot.y * inv_len);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float hf = p.hfold[tid + q * T];
                y[q] = make_float2(y[q].x - mean.x * hf, y[q].y - mean.y * hf);
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) buf[tid + q * T] = y[q];
        __syncthreads();
        fft_lds<N, T>(buf, p.tw, tid);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float2 X = buf[tid + q * T];
            acc[q] += fmaf(X.x, X.x, X.y * X.y);
        }
        __syncthreads();      // buf and red are the next frame's
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) dst[tid0 + q * T] = acc[q];
}

}  // namespace

#define OTH_PFB_KERNEL(N) welch_pfb_kernel<N, generic_threads(N)>

int welch_pfb_blocks_per_cu(int nfft) {
    return mtm_for_size(nfft, 0, [](auto n) {
        constexpr int N = decltype(n)::value;
        return resident_blocks<OTH_PFB_KERNEL(N)>(generic_threads(N), stat_lds_bytes(N), 0);
    });
}

hipError_t launch_welch_pfb(int nfft, const WelchPfbArgs &a, hipStream_t s) {
    const dim3 grid(a.wg_per_stream, a.nstreams);
    return mtm_for_size(nfft, hipErrorInvalidValue, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return launch_lds<OTH_PFB_KERNEL(N)>(grid, dim3(generic_threads(N)), stat_lds_bytes(N), s, a);
    });
}

}  // namespace oth
