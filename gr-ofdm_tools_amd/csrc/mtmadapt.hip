// Thomson's adaptive-weight multitaper PSD on the taper loop of mtm.hip, with the per-bin equivalent degrees of freedom.
// For a plan with K >= 2 tapers v_k, g_k = sum_n v_k[n]^2 and concentration ratios lambda_k (oth_mtm_set_ratios), per
// stream, segment s and bin j - segmentation, per-segment mean removal and zero padding are the plan's own:
//   P_k     = |FFT_nfft((x_s - m_s) v_k)[j]|^2 / g_k                         the eigenspectra
//   sigma^2 = (1 / nperseg) sum_n |x_s[n] - m_s|^2                           so that white noise has E P_k = sigma^2
//   S^0     = (P_0 + P_1) / 2
//   `iters` times:  b_k = S / (lambda_k S + (1 - lambda_k) sigma^2),   w_k = lambda_k b_k^2,
//                   S <- sum_k w_k P_k / sum_k w_k
//   then b_k, w_k once more from the final S, and   nu_s = 2 (sum_k w_k)^2 / sum_k w_k^2.
// Degenerate bins: where sum_k w_k is not > 0, or sigma^2 = 0, S_s = 0 and nu_s = 0 - finite input never gives NaN or
// Inf; all-zero input, and constant input on a detrending plan, give two rows of zeros.  Over the segments sum_s S_s and
// sum_s nu_s; adapt_finalize_kernel turns them into
//   psd = scale (1 / nseg) sum_s S_s     scale: 1 / fs (OTH_SCALE_DENSITY), 1 (OTH_SCALE_RAW), 1 / nfft^2 (OTH_SCALE_OVER_N2) -
//                                        for unit-norm tapers the plan's own scaling; with the plan's fftshift, trim and dB
//   dof = (1 / nseg) sum_s nu_s          fftshift and trim, always linear
// The plan's weights take no part.  The iteration count is fixed and there is no convergence test: single bins approach
// the fixed point very slowly (after 30 iterations some are still 5e-2 ... 5e+1, relative, away from the 60-iteration
// value) while the band-averaged floor settles after 3 - 4; a fixed count makes the estimator a definite function that a
// float64 computation by the definition can pin, and keeps all lanes in step.
//
// Work split: mtm_ftest_kernel's.  The weights are not linear in the tapers, so a segment's K transforms stay in one
// workgroup - the work item is a whole segment, a stream's segments go to W workgroups in contiguous runs, the two rows
// leave as partial[stream][wg][2][N] (sum S_s, sum nu_s) in natural bin order, and the finalize kernel adds them in
// double in a fixed order: a result depends on the launch shape only.  Segment entry and the taper product are
// mtm_common.hip.h's.  sigma^2 is one more block sum at segment entry, over the samples with pilot and residual mean
// already off (the direct form: the sum over the pilot-subtracted samples minus nperseg |mean|^2 cancels where the
// residual mean is large against the spread).
//
// The K eigenspectra of a bin are wanted again in every iteration.  K goes up to 64 and k is a runtime index, so they
// cannot be registers (an array indexed by k goes to scratch at once): each thread stores P_k of its own bins after
// transform k and reads them back in the iteration, the same addresses both ways, so no barrier.  Where they live:
//   64 ... 512 points (64 threads)    LDS behind the transform buffer: K N floats, at most 128 KiB (K = 64 at 512 points)
//                                     next to the 4 KiB buffer - the launch asks for the plan's K rows.
//   1024 ... 16384 points             a per-workgroup row [K][N] of a global workspace (MtmAdaptArgs.ws, d_ftest_ws's
//                                     pattern), sized by workgroups and never by segments: 64 rows of 1024 points are
//                                     256 KiB already.
// lambda_k, 1 - lambda_k and 1 / g_k are wave-uniform loads inside the k loop.  The iteration walks a thread's bins four
// at a time (S, the two or three sums: twelve to sixteen floats) in a loop that is not unrolled, so the running sums over
// a run's segments cannot be registers either (indexed by the loop): they live in the workgroup's own partial rows, as in
// mtm_ftest_kernel from 4096 points on - the first segment of a run stores, every later one reads, adds and stores.
#include "mtm_common.hip.h"
#include "out_stage.hip.h"
#include "launch.h"

#include <algorithm>

namespace oth {
namespace {

constexpr bool adapt_keep(int n) { return n <= 2048; }      // the segment's samples in registers across its tapers
constexpr bool adapt_plds(int n) { return n <= 512; }       // the eigenspectra in LDS (else MtmAdaptArgs.ws)

template <int N, int T, bool KEEP, bool PLDS>
__global__ __launch_bounds__(T) void mtm_adapt_kernel(MtmAdaptArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MtmArgs &p = a.m;
    float2 *buf = reinterpret_cast<float2 *>(smem);
    float2 *red = buf + N;                  // [0] the pilot, [1 ...] the mean's wave rows
    float2 *red2 = red + kMtmRedSlots;      // sigma^2's wave rows: a wave may be here while another still reads the mean's
    float *pl = reinterpret_cast<float *>(red2 + kMtmRedSlots);      // PLDS: [K][N]
    constexpr int NQ = N / T, C = NQ < 4 ? NQ : 4;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y, K = p.ntapers, iters = a.iters;
    const long long s0 = (p.nseg * wg) / W, s1 = (p.nseg * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    float *dst = p.partial + ((size_t)stream * W + wg) * 2 * N;      // [0] sum S_s, [1] sum nu_s
    float *pg = PLDS ? nullptr : a.ws + ((size_t)stream * W + wg) * (size_t)K * N;
    const float *__restrict__ lam = a.lam, *__restrict__ oml = a.lam + K, *__restrict__ ig = a.lam + 2 * K;
    const float inv_n = 1.0f / (float)p.nperseg;

    float2 v[KEEP ? NQ : 1];

    for (long long s = s0; s < s1; ++s) {
        const bool first = s == s0;      // of the run: its sums start here
        int tid = tid0;                  // an opaque copy, as in mtm_kernel: the passes' index arithmetic is not hoisted
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step;
        float2 pil, mean;
        mtm_segment_entry<N, T, KEEP>(xs, p.nperseg, p.detrend != 0, red, tid, v, pil, mean);
        float sig2;
        {
            float2 sq = make_float2(0.f, 0.f);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int n = tid + q * T;
                float2 r;
                if constexpr (KEEP) {
                    r = v[q];
                } else {
                    r = (n < p.nperseg) ? csub(csub(xs[n], pil), mean) : make_float2(0.f, 0.f);      // the taper product's samples
                }
                sq.x = fmaf(r.x, r.x, sq.x);
                sq.y = fmaf(r.y, r.y, sq.y);
            }
            const float2 tot = block_sum<T>(sq, red2, tid, 1);
            sig2 = (tot.x + tot.y) * inv_n;
        }
        for (int k = 0; k < K; ++k) {
            asm volatile("" : "+v"(tid));      // (nor shared between a segment's transforms)
            mtm_taper_product<N, T, KEEP>(xs, p.tapers + (size_t)k * N, p.nperseg, tid, pil, mean, v, buf);
            __syncthreads();
            fft_lds<N, T>(buf, p.tw, tid);
            const float g = ig[k];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int j = tid + q * T;
                const float2 X = buf[j];
                const float P = fmaf(X.x, X.x, X.y * X.y) * g;
                if constexpr (PLDS) pl[k * N + j] = P;
                else pg[(size_t)k * N + j] = P;
            }
            __syncthreads();
        }
        // the iteration, four of the thread's bins at a time; every P_k read here was stored above by this thread
        const bool live = sig2 > 0.f;
#pragma unroll 1
        for (int q0 = 0; q0 < NQ; q0 += C) {
            const int jb = tid + q0 * T;
            float S[C], nu[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int j = jb + c * T;
                float p0, p1;
                if constexpr (PLDS) {
                    p0 = pl[j];
                    p1 = pl[N + j];
                } else {
                    p0 = pg[j];
                    p1 = pg[(size_t)N + j];
                }
                S[c] = 0.5f * (p0 + p1);
                nu[c] = 0.f;
            }
            for (int it = 0; it <= iters; ++it) {      // `iters` updates of S, then the weights once more for nu
                float num[C], den[C], den2[C];
#pragma unroll
                for (int c = 0; c < C; ++c) num[c] = den[c] = den2[c] = 0.f;
                for (int k = 0; k < K; ++k) {
                    const float l = lam[k], noise = oml[k] * sig2;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int j = jb + c * T;
                        float P;
                        if constexpr (PLDS) P = pl[k * N + j];
                        else P = pg[(size_t)k * N + j];
                        const float d = fmaf(l, S[c], noise);
                        const float b = d > 0.f ? S[c] / d : 0.f;
                        const float w = l * b * b;
                        num[c] = fmaf(w, P, num[c]);
                        den[c] += w;
                        den2[c] = fmaf(w, w, den2[c]);
                    }
                }
                if (it < iters) {
#pragma unroll
                    for (int c = 0; c < C; ++c) S[c] = den[c] > 0.f ? num[c] / den[c] : 0.f;
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const bool ok = live && den[c] > 0.f && den2[c] > 0.f;
                        nu[c] = ok ? 2.f * den[c] * den[c] / den2[c] : 0.f;
                        if (!ok) S[c] = 0.f;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int j = jb + c * T;
                float a0 = 0.f, a1 = 0.f;
                if (!first) {
                    a0 = dst[j];
                    a1 = dst[N + j];
                }
                dst[j] = a0 + S[c];
                dst[N + j] = a1 + nu[c];
            }
        }
    }
}

// The shared finalize stage (out_stage.hip.h) on the two rows sum S_s, sum nu_s; then the PSD row with its dB and the dof row.
__global__ __launch_bounds__(256) void adapt_finalize_kernel(AdaptFinalizeArgs a) {
    const int k = blockIdx.x * 32 + (threadIdx.x & 31), stream = blockIdx.y;
    int i;
    const bool live = out_slot(a.out, a.nfft, k, i);
    const float *base = a.partial + (size_t)stream * a.W * 2 * a.nfft + k;
    double t[2];
    if (!slice_sums<2>(live, a.W, [&](int w, int r) { return base[((size_t)w * 2 + r) * a.nfft]; }, t)) return;
    const size_t o = (size_t)stream * a.out.nout + i;
    a.psd_out[o] = psd_value(a.out, t[0] * a.psd_scale);
    if (a.dof_out) a.dof_out[o] = (float)(t[1] * a.inv_nseg);
}

// the transform buffer and the two `red` arrays; the occupancy calculator is asked about this much
size_t adapt_base_lds(int nfft) { return (size_t)nfft * sizeof(float2) + 2 * kMtmRedSlots * sizeof(float2); }
constexpr size_t kAdaptLdsPerCu = 160 * 1024;
constexpr int kAdaptMaxTapers = 64;      // oth_mtm_plan's limit

}  // namespace

#define OTH_ADAPT_KERNEL(N) mtm_adapt_kernel<N, generic_threads(N), adapt_keep(N), adapt_plds(N)>

size_t mtm_adapt_lds_bytes(int nfft, int ntapers) {
    return adapt_base_lds(nfft) + (adapt_plds(nfft) ? (size_t)ntapers * nfft * sizeof(float) : 0);
}

size_t mtm_adapt_ws_floats(int nfft, int ntapers) { return adapt_plds(nfft) ? 0 : (size_t)ntapers * nfft; }

// The calculator's answer for the transform buffer alone (registers and waves; cached per build, whatever K the first
// plan had), then what the K rows of eigenspectra leave of a CU's LDS.
int mtm_adapt_blocks_per_cu(int nfft, int ntapers) {
    int n = 0;
    switch (nfft) {
#define X(N) \
    case N: n = resident_blocks<OTH_ADAPT_KERNEL(N)>(generic_threads(N), adapt_base_lds(N), 0); break;
        OTH_MTM_FOR_EACH_N(X)
#undef X
        default: return 0;
    }
    return (int)std::min<size_t>((size_t)n, kAdaptLdsPerCu / mtm_adapt_lds_bytes(nfft, ntapers));
}

// The opt-in to more than 64 KiB of LDS is made once per build and device: it asks for the most any plan can need.
hipError_t launch_mtm_adapt(int nfft, const MtmAdaptArgs &a, hipStream_t s) {
    const dim3 grid(a.m.wg_per_stream, a.m.nstreams);
    const size_t lds = mtm_adapt_lds_bytes(nfft, a.m.ntapers);
    switch (nfft) {
#define X(N)                                                                                                        \
    case N: {                                                                                                       \
        const hipError_t e = arm_lds<OTH_ADAPT_KERNEL(N)>(mtm_adapt_lds_bytes(N, kAdaptMaxTapers));                  \
        return e != hipSuccess ? e : launch_lds<OTH_ADAPT_KERNEL(N)>(grid, dim3(generic_threads(N)), lds, s, a);     \
    }
        OTH_MTM_FOR_EACH_N(X)
#undef X
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_adapt_finalize(const AdaptFinalizeArgs &a, int nstreams, hipStream_t s) {
    return launch_stat_finalize<adapt_finalize_kernel>(a, nstreams, 1, s);
}

}  // namespace oth
