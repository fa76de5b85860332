// Cyclic spectrum and cyclic coherence of a Welch plan (the time-smoothed cyclic cross periodogram): for a set of A cycle
// frequencies alpha_a in cycles per sample, per stream, segment s and bin j, with m_s the segment mean on a detrending plan,
//   X_s[j]   = FFT((x_s[n] - m_s) w[n])[j]
//   U_s,a[j] = FFT((x_s[n] - m_s) w[n] e^{-j 2 pi alpha_a (n + s step)})[j]      X at frequency j / nfft + alpha_a, global time
//   Sxx = sum_s |X_s|^2,   Suu_a = sum_s |U_s,a|^2,   Sux_a = sum_s U_s,a conj(X_s);
// cyc_finalize_kernel turns the rows into scf_a = scale Sux_a / M, coh_a = |Sux_a|^2 / (Suu_a Sxx) and the plan's PSD row.
//
// The body is welchsk.hip's (a whole segment per work item, a stream's segments to W workgroups in contiguous runs, segment
// entry by mtm_segment_entry) with mtmcsd.hip's second transform: the second "channel" is the same segment under a complex
// taper c_a[n] = w[n] e^{-j 2 pi alpha_a n}, built on the host in double and rounded once.  The segment's own factor
// e^{-j 2 pi alpha_a s step} is constant over the segment, so it rotates the segment's cross product once per owned bin instead
// of every sample: its angle is the fractional part of alpha_a s step taken in double - s step passes 2^24, where a float32
// product is useless - and only that fraction, in [-1/2, 1/2], is rounded to float32 for sincospif.
//
// Grid (W, nstreams, G): the A cycle frequencies are split into G groups of at most GA consecutive ones.  A workgroup
// transforms X once per segment and keeps it for the whole group, so a segment costs 1 + GA transforms instead of 2 GA.
// GA = 1 is mtmcsd_kernel's item exactly (two transforms per (segment, alpha)); GA = 2 and GA = 4 are the grouped builds.  Which
// one runs is the host's choice per size and A, from a measurement (cyc_group, abi_cyc.hip).
//
// Where the state lives:
//   64 ... 8192 points    two LDS buffers: X stays in the first, every U of the group goes through the second.
//   16384 points          one 128 KiB buffer.  X goes through a row of global memory that belongs to the workgroup
//                         (WelchCycArgs.ws): every thread writes the bins it owns and reads the same addresses back - no
//                         barrier, and the row stays in L2 (mtmcsd.hip's single-buffer path).
//   samples               in registers across the segment's transforms below 8192 points (mtm_keep), read again above.
//   sums                  1 + 3 GA rows (|X|^2; per alpha |U|^2, Re and Im Sux).  In registers where that builds without
//                         scratch (cyc_accreg: GA = 1, 2 up to 8192 points, GA = 4 up to 4096); otherwise in the workgroup's
//                         own partial rows - the first segment of a run stores, every later one reads, adds and stores,
//                         each thread at its own addresses.
// The rows leave as partial[stream][group][wg][1 + 3 GA][N] in natural bin order; row 0 is written by group 0 only.  The
// finalize kernel adds the workgroups' rows in double in a fixed order: a result depends on the launch shape only.
//
// Arithmetic the tests rely on: Re U conj(X) = fma(Ur, Xr, Ui Xi) has the expression shape of |X|^2 = fma(Xr, Xr, Xi Xi) and
// Im U conj(X) is cross_im's two rounded products (mtmcsd.hip); at alpha = 0 the taper is (w, 0), the rotation (1, 0), so
// U = X bit for bit, the three rows are identical and the imaginary part is exactly 0.
//
// Not here: the conjugate cyclic spectrum E[X(f + alpha) X(-f)], a search over alpha (the caller supplies the cycle
// frequencies), multitaper plans, transform lengths that are not a power of two.
#include "mtm_common.hip.h"
#include "out_stage.hip.h"
#include "launch.h"

#include <type_traits>

namespace oth {
namespace {

constexpr bool cyc_two_buffers(int n) { return n <= 8192; }
// the sums in registers: what builds without scratch (tests/test_welch_cyclic_cpu.py reads the code objects)
constexpr bool cyc_accreg(int n, int ga) { return ga <= 2 ? n <= 8192 : n <= 4096; }

// (x - pilot - mean) c_a of the segment into buf, after mtm_segment_entry; no barrier.  mtm_taper_product with a complex taper.
template <int N, int T, bool KEEP>
__device__ __forceinline__ void cyc_taper_product(const float2 *__restrict__ xs, const float2 *__restrict__ c, int nperseg, int tid,
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
        buf[n] = cmul(r, c[n]);      // c = (w, 0): r.x w and r.y w, the bits of the window product
    }
}

template <int N, int T, int GA, bool KEEP, bool TWO, bool ACCREG> __global__ __launch_bounds__(T) void welch_cyc_kernel(WelchCycArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *bufx = reinterpret_cast<float2 *>(smem);
    float2 *bufu = TWO ? bufx + N : bufx;
    int red0 = 0;      // off an opaque vector register (mtmcsd.hip's header: scalar registers)
    asm volatile("" : "+v"(red0));
    float2 *red = bufu + N + red0;      // [0] the pilot, [1 ...] the block sum's wave rows
    constexpr int NQ = N / T;
    constexpr int R = 1 + 3 * GA;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y, grp = blockIdx.z, G = gridDim.z;
    const int a0 = grp * GA;
    const int na = p.ncyc - a0 < GA ? p.ncyc - a0 : GA;      // the last group may be a partial one
    const long long s0 = (p.nseg * wg) / W, s1 = (p.nseg * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    const size_t slot = ((size_t)stream * G + grp) * W + wg;
    float *dst = p.partial + slot * R * N;
    float2 *ws = TWO ? nullptr : p.ws + slot * N;

    float acc[ACCREG ? R : 1][ACCREG ? NQ : 1];
    if constexpr (ACCREG) {
#pragma unroll
        for (int c = 0; c < R; ++c)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[c][q] = 0.f;
    }
    float2 v[KEEP ? NQ : 1];

    for (long long s = s0; s < s1; ++s) {
        const bool first = s == s0;      // of the run: its sums start here
        int tid = tid0;                  // an opaque copy, as in mtm_kernel: the passes' index arithmetic is not hoisted
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step;
        float2 pil, mean;
        mtm_segment_entry<N, T, KEEP>(xs, p.nperseg, p.detrend != 0, red, tid, v, pil, mean);
        mtm_taper_product<N, T, KEEP>(xs, p.win, p.nperseg, tid, pil, mean, v, bufx);
        __syncthreads();
        fft_lds<N, T>(bufx, p.tw, tid);
        if constexpr (!TWO) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) ws[tid + q * T] = bufx[tid + q * T];      // this thread's bins, read back below
        }
        if (grp == 0) {
            // |X|^2: group 0 alone (a uniform branch)
            if constexpr (ACCREG) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const float2 X = bufx[tid + q * T];
                    acc[0][q] += fmaf(X.x, X.x, X.y * X.y);
                }
            } else {
#pragma unroll 4
                for (int q = 0; q < NQ; ++q) {
                    const int j = tid + q * T;
                    const float2 X = bufx[j];
                    const float b = first ? 0.f : dst[j];
                    dst[j] = b + fmaf(X.x, X.x, X.y * X.y);
                }
            }
        }
        if constexpr (!TWO) __syncthreads();
#pragma unroll
        for (int g = 0; g < GA; ++g) {
            if (g < na) {      // uniform
                asm volatile("" : "+v"(tid));      // nor shared between the transforms of a segment (mtmcsd.hip)
                cyc_taper_product<N, T, KEEP>(xs, p.ctap + (size_t)(a0 + g) * N, p.nperseg, tid, pil, mean, v, bufu);
                __syncthreads();
                fft_lds<N, T>(bufu, p.tw, tid);
                // the segment's factor e^{-j 2 pi alpha s step}: the fraction in double, its sine and cosine in float32
                const double turns = p.alpha[a0 + g] * (double)(s * (long long)p.step);
                const float frac = (float)(turns - rint(turns));
                float sn, cs;
                sincospif(2.0f * frac, &sn, &cs);
                auto sum = [&](auto load) {
#pragma unroll ACCREG ? NQ : 4
                    for (int q = 0; q < NQ; ++q) {
                        const int j = tid + q * T;
                        const float2 X = TWO ? bufx[j] : ws[j];
                        const float2 U = bufu[j];
                        float r[3] = {0.f, 0.f, 0.f};
                        if constexpr (decltype(load)::value) {
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch)
                                r[ch] = ACCREG ? acc[ACCREG ? 1 + 3 * g + ch : 0][ACCREG ? q : 0] : dst[(size_t)(1 + 3 * g + ch) * N + j];
                        }
                        const float re = fmaf(U.x, X.x, U.y * X.y);      // U conj(X)
                        const float im = cross_im(X, U);
                        r[0] += fmaf(U.x, U.x, U.y * U.y);
                        r[1] = fmaf(cs, re, fmaf(sn, im, r[1]));         // (cs - j sn)(re + j im)
                        r[2] = fmaf(cs, im, fmaf(-sn, re, r[2]));
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            if constexpr (ACCREG) acc[ACCREG ? 1 + 3 * g + ch : 0][ACCREG ? q : 0] = r[ch];
                            else dst[(size_t)(1 + 3 * g + ch) * N + j] = r[ch];
                        }
                    }
                };
                if (ACCREG || !first) sum(std::true_type{});
                else sum(std::false_type{});
                __syncthreads();
            }
        }
    }
    if constexpr (ACCREG) {
#pragma unroll
        for (int c = 0; c < R; ++c)
#pragma unroll
            for (int q = 0; q < NQ; ++q) dst[(size_t)c * N + tid0 + q * T] = acc[c][q];
    }
}

// The shared finalize stage (out_stage.hip.h), one cycle frequency per blockIdx.z, on the |X|^2 row of group 0 and the
// frequency's own three rows; then scf, coh and (with the first cycle frequency) the PSD row.
__global__ __launch_bounds__(256) void cyc_finalize_kernel(CycFinalizeArgs a) {
    const int k = blockIdx.x * 32 + (threadIdx.x & 31), stream = blockIdx.y, cyc = blockIdx.z;
    int i;
    const bool live = out_slot(a.out, a.nfft, k, i);
    const int R = 1 + 3 * a.ga, grp = cyc / a.ga, g = cyc - grp * a.ga;
    const size_t row = (size_t)a.nfft, wgrows = (size_t)R * row;
    const float *bx = a.partial + (size_t)stream * a.G * a.W * wgrows + k;                       // group 0, row 0
    const float *bu = a.partial + ((size_t)stream * a.G + grp) * a.W * wgrows + (size_t)(1 + 3 * g) * row + k;
    double t[4];
    if (!slice_sums<4>(live, a.W, [&](int w, int r) { return r ? bu[(size_t)w * wgrows + (size_t)(r - 1) * row] : bx[(size_t)w * wgrows]; }, t))
        return;
    // an empty bin (silence, a constant under detrend) reads scf = 0, coh = 0: no 0 / 0; non-finite input stays non-finite
    const double den = t[0] * t[1];
    double coh = 0.0, sr = 0.0, si = 0.0;
    if (!(den <= 0.0)) {
        coh = (t[2] * t[2] + t[3] * t[3]) / den;
        if (coh > 1.0) coh = 1.0;      // Cauchy-Schwarz up to the float32 rounding of the three rows
        sr = t[2] * a.scf_scale;
        si = t[3] * a.scf_scale;
    }
    const size_t o = ((size_t)stream * a.ncyc + cyc) * a.out.nout + i;
    a.coh_out[o] = (float)coh;
    if (a.scf_out) {
        a.scf_out[2 * o] = (float)sr;
        a.scf_out[2 * o + 1] = (float)si;
    }
    if (a.psd_out && cyc == 0) a.psd_out[(size_t)stream * a.out.nout + i] = psd_value(a.out, t[0] * a.scf_scale);
}

size_t cyc_lds_bytes(int nfft) { return stat_lds_bytes(nfft, cyc_two_buffers(nfft) ? 2 : 1); }

}  // namespace

#define OTH_CYC_KERNEL(N, GA) welch_cyc_kernel<N, stat_threads(N), GA, mtm_keep(N), cyc_two_buffers(N), cyc_accreg(N, GA)>

size_t welch_cyc_ws_points(int nfft) { return cyc_two_buffers(nfft) ? 0 : (size_t)nfft; }

int welch_cyc_blocks_per_cu(int nfft, int ga) {
    return mtm_for_build<1, 2, kCycGroup>(nfft, ga, 0, [](auto n, auto g) {
        constexpr int N = decltype(n)::value, GA = decltype(g)::value;
        return resident_blocks<OTH_CYC_KERNEL(N, GA)>(stat_threads(N), cyc_lds_bytes(N), 0);
    });
}

hipError_t launch_welch_cyc(int nfft, int ga, int groups, const WelchCycArgs &a, hipStream_t s) {
    if (ga != 1 && ga != 2 && ga != kCycGroup) return hipErrorInvalidValue;
    const dim3 grid(a.wg_per_stream, a.nstreams, groups);
    return mtm_for_build<1, 2, kCycGroup>(nfft, ga, hipErrorInvalidValue, [&](auto n, auto g) {
        constexpr int N = decltype(n)::value, GA = decltype(g)::value;
        return launch_lds<OTH_CYC_KERNEL(N, GA)>(grid, dim3(stat_threads(N)), cyc_lds_bytes(N), s, a);
    });
}

hipError_t launch_cyc_finalize(const CycFinalizeArgs &a, int nstreams, hipStream_t s) {
    return launch_stat_finalize<cyc_finalize_kernel>(a, nstreams, a.ncyc, s);
}

}  // namespace oth
