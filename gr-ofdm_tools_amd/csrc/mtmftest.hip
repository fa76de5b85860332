// Thomson's harmonic F-test on the taper loop of mtm.hip: per segment s and bin j, with y_k = FFT((x_s - m_s) v_k)[j] and
// U_k = sum_n v_k[n], S = sum_k U_k^2,
//   sy = sum_k U_k y_k,   p = sum_k |y_k|^2,   num_s = |sy|^2 / S  (= S |mu_s|^2),   den_s = p - num_s,
// and over the segments sum_s num_s and sum_s den_s; ftest_finalize_kernel turns the two rows into
//   F = (K - 1) sum num / sum den,   line = sum num / (S nseg),   resid = scale sum den / ((K - 1) nseg).
// The plan's weights take no part: the test is unweighted.
//
// Work split: the step from sy to |sy|^2 is not linear, so a segment's K transforms stay in one workgroup - the work item
// is a whole segment (mtm_kernel's is a (segment, taper) pair).  A stream's segments go to W workgroups in contiguous
// runs; a workgroup forms num_s and den_s per segment in registers and adds each to its running sums - the difference
// of two long float32 sums taken at the end would be worse conditioned.  Its two rows leave as partial[stream][wg][2][N]
// in natural bin order; the finalize kernel adds them in double in a fixed order, so a result depends on the launch
// shape only.  Segment entry (pilot, residual mean) and the taper product are mtm_kernel's, the same arithmetic.
//
// State per owned bin: sy (2), p, the running num and den - five floats against mtm_kernel's one.  Where it lives:
//   64 ... 2048 points (N / T <= 8)   everything in registers, the segment's samples too (KEEP).
//   4096, 8192 points (N / T = 16)    sy / p in registers (48), the samples read again per taper (no KEEP); the running
//                                     sums live in the workgroup's own partial rows: the first segment of a run stores
//                                     them, every later one reads, adds and stores - each thread its own addresses, once
//                                     per K transforms.
//   16384 points (1024 threads)       128 registers per lane: sy / p go through three rows of the workgroup's own
//                                     global workspace (MtmFtestArgs.ws) as well - the first taper stores, the middle ones
//                                     read, add and store, the last one reads and closes the segment; again every thread
//                                     its own addresses, so no barrier, and the rows stay in L2.
#include "mtm_common.hip.h"
#include "out_stage.hip.h"
#include "launch.h"

namespace oth {
namespace {

constexpr bool ftest_keep(int n) { return n <= 2048; }        // the segment's samples in registers across its tapers
constexpr bool ftest_segreg(int n) { return n < 16384; }      // sy / p in registers (else MtmFtestArgs.ws)
constexpr bool ftest_accreg(int n) { return n <= 2048; }      // running num / den in registers (else the partial rows)

template <int N, int T, bool KEEP, bool SEGREG, bool ACCREG>
__global__ __launch_bounds__(T) void mtm_ftest_kernel(MtmFtestArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MtmArgs &p = a.m;
    float2 *buf = reinterpret_cast<float2 *>(smem);
    float2 *red = buf + N;      // [0] the pilot, [1 ...] the block sum's wave rows
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y, K = p.ntapers;
    const long long s0 = (p.nseg * wg) / W, s1 = (p.nseg * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    float *dst = p.partial + ((size_t)stream * W + wg) * 2 * N;      // [0] sum num, [1] sum den
    float *ws = SEGREG ? nullptr : a.ws + ((size_t)stream * W + wg) * 3 * N;      // sy.re, sy.im, p
    const float inv_s = a.inv_s;

    float num[ACCREG ? NQ : 1], den[ACCREG ? NQ : 1];
    if constexpr (ACCREG) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) num[q] = den[q] = 0.f;
    }
    float2 sy[SEGREG ? NQ : 1];
    float pw[SEGREG ? NQ : 1];
    float2 v[KEEP ? NQ : 1];

    for (long long s = s0; s < s1; ++s) {
        const bool first = s == s0;      // of the run: its sums start here
        int tid = tid0;                  // an opaque copy, as in mtm_kernel: the passes' index arithmetic is not hoisted
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step;
        float2 pil = make_float2(0.f, 0.f), mean = make_float2(0.f, 0.f);
        if (p.detrend) pil = mtm_pilot(xs, p.nperseg, red, tid);
        {
            float2 sum = make_float2(0.f, 0.f);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int n = tid + q * T;
                const float2 r = (n < p.nperseg) ? csub(xs[n], pil) : make_float2(0.f, 0.f);
                if constexpr (KEEP) v[q] = r;
                sum = cadd(sum, r);
            }
            if (p.detrend) {
                const float2 tot = block_sum<T>(sum, red, tid, 1);
                const float inv = 1.0f / (float)p.nperseg;
                mean = make_float2(tot.x * inv, tot.y * inv);
            }
            if constexpr (KEEP) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int n = tid + q * T;
                    v[q] = (n < p.nperseg) ? csub(v[q], mean) : make_float2(0.f, 0.f);
                }
            }
        }
        if constexpr (SEGREG) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                sy[q] = make_float2(0.f, 0.f);
                pw[q] = 0.f;
            }
        }
        for (int k = 0; k < K; ++k) {
            asm volatile("" : "+v"(tid));      // (nor shared between a segment's transforms)
            const float *__restrict__ w = p.tapers + (size_t)k * N;      // zero-extended to N
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
            const float u = a.u[k];
            if constexpr (SEGREG) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const float2 X = buf[tid + q * T];
                    sy[q].x = fmaf(u, X.x, sy[q].x);
                    sy[q].y = fmaf(u, X.y, sy[q].y);
                    pw[q] = fmaf(X.x, X.x, fmaf(X.y, X.y, pw[q]));
                }
            } else {
                // the workspace rows: stored by the first taper, closed by the last (K >= 2); four bins at a time, so
                // that the loads in flight do not outgrow the registers
                const bool open = k == 0, close = k == K - 1;
#pragma unroll 4
                for (int q = 0; q < NQ; ++q) {
                    const int j = tid + q * T;
                    const float2 X = buf[j];
                    float sr = 0.f, si = 0.f, pp = 0.f;
                    if (!open) {
                        sr = ws[j];
                        si = ws[N + j];
                        pp = ws[2 * N + j];
                    }
                    sr = fmaf(u, X.x, sr);
                    si = fmaf(u, X.y, si);
                    pp = fmaf(X.x, X.x, fmaf(X.y, X.y, pp));
                    if (!close) {
                        ws[j] = sr;
                        ws[N + j] = si;
                        ws[2 * N + j] = pp;
                    } else {
                        const float line = fmaf(sr, sr, si * si) * inv_s;
                        float n0 = 0.f, d0 = 0.f;
                        if (!first) {
                            n0 = dst[j];
                            d0 = dst[N + j];
                        }
                        dst[j] = n0 + line;
                        dst[N + j] = d0 + (pp - line);
                    }
                }
            }
            __syncthreads();
        }
        if constexpr (SEGREG) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int j = tid + q * T;
                const float line = fmaf(sy[q].x, sy[q].x, sy[q].y * sy[q].y) * inv_s;
                if constexpr (ACCREG) {
                    num[q] += line;
                    den[q] += pw[q] - line;
                } else {
                    float n0 = 0.f, d0 = 0.f;
                    if (!first) {
                        n0 = dst[j];
                        d0 = dst[N + j];
                    }
                    dst[j] = n0 + line;
                    dst[N + j] = d0 + (pw[q] - line);
                }
            }
        }
    }
    if constexpr (ACCREG) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            dst[tid0 + q * T] = num[q];
            dst[N + tid0 + q * T] = den[q];
        }
    }
}

// The shared finalize stage (out_stage.hip.h) on the two rows sum num, sum den; then the three rows.
__global__ __launch_bounds__(256) void ftest_finalize_kernel(FtestFinalizeArgs a) {
    const int k = blockIdx.x * 32 + (threadIdx.x & 31), stream = blockIdx.y;
    int i;
    const bool live = out_slot(a.out, a.nfft, k, i);
    const float *base = a.partial + (size_t)stream * a.W * 2 * a.nfft + k;
    double t[2];
    if (!slice_sums<2>(live, a.W, [&](int w, int r) { return base[((size_t)w * 2 + r) * a.nfft]; }, t)) return;
    const double sn = t[0], sd = t[1];
    // degenerate bins: nothing left beside the line (or nothing at all) - no 0 / 0, and no negative power
    float f;
    if (sd > 0.0) f = (float)(a.km1 * sn / sd);
    else if (sd <= 0.0) f = sn > 0.0 ? __builtin_inff() : 0.f;
    else f = __builtin_nanf("");      // non-finite input
    const size_t o = (size_t)stream * a.out.nout + i;
    a.f_out[o] = f;
    if (a.line_out) a.line_out[o] = (float)(sn * a.line_scale);
    if (a.resid_out) a.resid_out[o] = (float)(sd > 0.0 || sd != sd ? sd * a.resid_scale : 0.0);
}

}  // namespace

#define OTH_FTEST_KERNEL(N) mtm_ftest_kernel<N, generic_threads(N), ftest_keep(N), ftest_segreg(N), ftest_accreg(N)>

size_t mtm_ftest_ws_floats(int nfft) { return ftest_segreg(nfft) ? 0 : 3 * (size_t)nfft; }

int mtm_ftest_blocks_per_cu(int nfft) {
    return mtm_for_size(nfft, 0, [](auto n) {
        constexpr int N = decltype(n)::value;
        return resident_blocks<OTH_FTEST_KERNEL(N)>(generic_threads(N), stat_lds_bytes(N), 0);
    });
}

hipError_t launch_mtm_ftest(int nfft, const MtmFtestArgs &a, hipStream_t s) {
    const dim3 grid(a.m.wg_per_stream, a.m.nstreams);
    return mtm_for_size(nfft, hipErrorInvalidValue, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return launch_lds<OTH_FTEST_KERNEL(N)>(grid, dim3(generic_threads(N)), stat_lds_bytes(N), s, a);
    });
}

hipError_t launch_ftest_finalize(const FtestFinalizeArgs &a, int nstreams, hipStream_t s) {
    return launch_stat_finalize<ftest_finalize_kernel>(a, nstreams, 1, s);
}

}  // namespace oth
