// Cyclic autocorrelation of a Welch plan as a Welch PSD of the lag product: for a set of L lags tau_l >= 0, per stream,
// segment s and lag l, with n < nperseg,
//   z_s,l[n] = x[s step + n + tau_l] conj(x[s step + n])
//   mbar_s,l = (1 / nperseg) sum_n z_s,l[n]
//   Z_s,l[q] = FFT((z_s,l[n] - m) w[n])[q]          m = mbar_s,l on a detrending plan, 0 otherwise
//   S_l = sum_s |Z_s,l|^2,   R_l = sum_s mbar_s,l;
// lag_finalize_kernel turns the rows into caf_l = scale S_l / M through the shared output stage and r_l = R_l / M.
// Bin q of caf_l is the cycle frequency alpha = q / nfft: a CP-OFDM signal shows lines at k / (Tu + Tcp) in the row of
// tau = Tu and a non-zero r there; stationary noise shows neither at any lag but 0.
//
// The body is welchcyc.hip's (a whole segment per work item, a stream's segments to W workgroups in contiguous runs) with
// the product in front of the taper loop's segment entry: what mtm_segment_entry does to samples, lag_segment_entry does to
// products - the pilot (the mean of the first min(64, nperseg) products) comes off every product, then the residual mean as
// a block sum in a fixed order.  Lag 0 and a DC offset in x both give z a mean far above its fluctuation, which is what
// the pilot is for.  mbar is always formed, pilot + residual mean added in double, since it feeds r also where the plan
// does not detrend; there the pilot is 0 and nothing is subtracted.
//
// Grid (W, nstreams, G): the L lags are split into G groups of at most GL consecutive ones.  A workgroup loads the base
// segment x_s[n] once per segment for the whole group - into registers where mtm_keep(N) holds, read again above - and per
// lag loads the lagged samples (8-byte loads at any tau), forms z, takes the means, applies the window, transforms in the
// one LDS buffer and adds |Z|^2 to the lag's running row.  GL = 1 and GL = 2 are the two builds; which one runs is the
// host's choice, from a measurement (lag_group, abi_lag.hip: GL = 1 wherever the library chooses).
//
// What a workgroup reads: the host counts M segments on nsamples - max_l tau_l samples, so the furthest sample of the last
// segment, (M - 1) step + nperseg - 1 + tau_l, lies inside the stream's own nsamples.  That is the bound of every load here.
//
// Where the state lives:
//   products              in registers across the mean and the taper below 8192 points (mtm_keep), formed again above.
//   sums                  one row per lag of the group.  In registers where that builds without scratch (lag_accreg:
//                         every build but GL = 2 at 16384 points); otherwise in the workgroup's own partial rows - the
//                         first segment of a run stores, every later one reads, adds and stores, each thread at its own
//                         addresses.
//   mbar                  the run's sum in double, the same bits in every thread; thread 0 stores it.
// The rows leave as partial[stream][group][wg][GL][N] in natural bin order and means[stream][group][wg][GL] as re, im
// doubles.  The finalize kernel adds the workgroups' rows in double in a fixed order: a result depends on the launch shape
// only.
//
// Arithmetic the tests rely on: Re z = fma(ar, br, ai bi) and Im z = ai br - ar bi with both products rounded before the
// subtraction (cross_im), so at tau = 0 the imaginary part is exactly 0 in every product, every mean and r.
//
// Not here: the conjugate lag product x[n + tau] x[n], negative lags, coherent averaging across segments, multitaper plans,
// transform lengths that are not a power of two.
#include "mtm_common.hip.h"
#include "out_stage.hip.h"
#include "launch.h"

namespace oth {
namespace {

// the sums in registers: what builds without scratch (tests/test_welch_caf_cpu.py reads the code objects)
constexpr bool lag_accreg(int n, int gl) { return gl == 1 || n <= 8192; }

// x[n + tau] conj(x[n]): a the lagged sample, b the base one
__device__ __forceinline__ float2 lag_product(float2 a, float2 b) { return make_float2(fmaf(a.x, b.x, a.y * b.y), cross_im(b, a)); }

// product n of the segment; xs + n + tau stays inside the stream (the file header's bound)
template <bool KEEP> __device__ __forceinline__ float2 lag_z(const float2 *__restrict__ xs, const float2 *__restrict__ xl, int n, float2 base) {
    return lag_product(xl[n], KEEP ? base : xs[n]);
}

// mtm_segment_entry on products.  pil: the mean of the first min(64, nperseg) products on a detrending plan, else 0; mean:
// the mean of z - pil as a fixed-order block sum, always formed; KEEP: v[q] holds z - pil of product tid + q T (zero behind
// nperseg) - the caller takes `mean` off where the plan detrends.  Every thread of the workgroup calls it.
template <int N, int T, bool KEEP>
__device__ __forceinline__ void lag_segment_entry(const float2 *__restrict__ xs, const float2 *__restrict__ xl, int nperseg, bool detrend,
                                                  float2 *red, int tid, const float2 (&b)[KEEP ? N / T : 1], float2 (&v)[KEEP ? N / T : 1],
                                                  float2 &pil, float2 &mean) {
    constexpr int NQ = N / T;
    pil = make_float2(0.f, 0.f);
    if (detrend) {
        if (tid < kMtmPilot) {
            const int np = nperseg < kMtmPilot ? nperseg : kMtmPilot;
            float2 t = tid < np ? lag_product(xl[tid], xs[tid]) : make_float2(0.f, 0.f);
            t = wave_sum(t);
            const float inv = 1.0f / (float)np;
            if (tid == 0) red[0] = make_float2(t.x * inv, t.y * inv);
        }
        __syncthreads();
        pil = red[0];
    }
    float2 sum = make_float2(0.f, 0.f);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int n = tid + q * T;
        const float2 r = (n < nperseg) ? csub(lag_z<KEEP>(xs, xl, n, b[KEEP ? q : 0]), pil) : make_float2(0.f, 0.f);
        if constexpr (KEEP) v[q] = r;
        sum = cadd(sum, r);
    }
    const float2 tot = block_sum<T>(sum, red, tid, 1);
    const float inv = 1.0f / (float)nperseg;
    mean = make_float2(tot.x * inv, tot.y * inv);
}

template <int N, int T, int GL, bool KEEP, bool ACCREG> __global__ __launch_bounds__(T) void welch_lag_kernel(WelchLagArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *buf = reinterpret_cast<float2 *>(smem);
    int red0 = 0;      // off an opaque vector register (mtmcsd.hip's header: scalar registers)
    asm volatile("" : "+v"(red0));
    float2 *red = buf + N + red0;      // [0] the pilot, [1 ...] the block sum's wave rows
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y, grp = blockIdx.z, G = gridDim.z;
    const int l0 = grp * GL;
    const int nl = p.nlags - l0 < GL ? p.nlags - l0 : GL;      // the last group may be a partial one
    const long long s0 = (p.nseg * wg) / W, s1 = (p.nseg * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    const size_t slot = ((size_t)stream * G + grp) * W + wg;
    float *dst = p.partial + slot * GL * N;
    const bool detrend = p.detrend != 0;

    float acc[ACCREG ? GL : 1][ACCREG ? NQ : 1];
    if constexpr (ACCREG) {
#pragma unroll
        for (int g = 0; g < GL; ++g)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[g][q] = 0.f;
    }
    double mre[GL], mim[GL];
#pragma unroll
    for (int g = 0; g < GL; ++g) mre[g] = mim[g] = 0.0;
    float2 b[KEEP ? NQ : 1], v[KEEP ? NQ : 1];

    for (long long s = s0; s < s1; ++s) {
        const bool first = s == s0;      // of the run: its sums start here
        int tid = tid0;                  // an opaque copy, as in mtm_kernel: the passes' index arithmetic is not hoisted
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step;
        if constexpr (KEEP) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int n = tid + q * T;
                b[q] = (n < p.nperseg) ? xs[n] : make_float2(0.f, 0.f);
            }
        }
#pragma unroll
        for (int g = 0; g < GL; ++g) {
            if (g < nl) {      // uniform
                asm volatile("" : "+v"(tid));      // nor shared between the transforms of a segment (mtmcsd.hip)
                const float2 *xl = xs + p.lags[l0 + g];      // n < nperseg: inside the stream, by the host's segment count
                float2 pil, mean;
                lag_segment_entry<N, T, KEEP>(xs, xl, p.nperseg, detrend, red, tid, b, v, pil, mean);
                mre[g] += (double)pil.x + (double)mean.x;
                mim[g] += (double)pil.y + (double)mean.y;
                const float2 off = detrend ? mean : make_float2(0.f, 0.f);
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int n = tid + q * T;
                    float2 r;
                    if constexpr (KEEP) {
                        r = (n < p.nperseg) ? csub(v[q], off) : make_float2(0.f, 0.f);
                    } else {
                        r = (n < p.nperseg) ? csub(csub(lag_z<false>(xs, xl, n, b[0]), pil), off) : make_float2(0.f, 0.f);      // the same arithmetic
                    }
                    const float wn = p.win[n];
                    buf[n] = make_float2(r.x * wn, r.y * wn);
                }
                __syncthreads();
                fft_lds<N, T>(buf, p.tw, tid);
                if constexpr (ACCREG) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const float2 Z = buf[tid + q * T];
                        acc[g][q] += fmaf(Z.x, Z.x, Z.y * Z.y);
                    }
                } else {
                    float *row = dst + (size_t)g * N;
#pragma unroll 4
                    for (int q = 0; q < NQ; ++q) {
                        const int j = tid + q * T;
                        const float2 Z = buf[j];
                        const float before = first ? 0.f : row[j];
                        row[j] = before + fmaf(Z.x, Z.x, Z.y * Z.y);
                    }
                }
                __syncthreads();      // buf and red are the next lag's
            }
        }
    }
    if constexpr (ACCREG) {
#pragma unroll
        for (int g = 0; g < GL; ++g)
#pragma unroll
            for (int q = 0; q < NQ; ++q) dst[(size_t)g * N + tid0 + q * T] = acc[g][q];
    }
    if (tid0 == 0) {
        double *m = p.means + slot * GL * 2;
#pragma unroll
        for (int g = 0; g < GL; ++g) {
            m[2 * g] = mre[g];
            m[2 * g + 1] = mim[g];
        }
    }
}

// The shared finalize stage (out_stage.hip.h), one lag per blockIdx.z, on the lag's row; the first wave of the first
// workgroup of a (stream, lag) adds the workgroups' mbar sums - lane i takes w = i, i + 64, ..., then the wave's fixed tree.
__global__ __launch_bounds__(256) void lag_finalize_kernel(LagFinalizeArgs a) {
    const int k = blockIdx.x * 32 + (threadIdx.x & 31), stream = blockIdx.y, lag = blockIdx.z;
    const int grp = lag / a.gl, g = lag - grp * a.gl;
    const size_t slot0 = ((size_t)stream * a.G + grp) * a.W;
    if (a.r_out && blockIdx.x == 0 && threadIdx.x < 64) {
        double re = 0.0, im = 0.0;
        for (int w = threadIdx.x; w < a.W; w += 64) {
            const double *m = a.means + ((slot0 + w) * a.gl + g) * 2;
            re += m[0];
            im += m[1];
        }
        re = wave_sum(re);
        im = wave_sum(im);
        if (threadIdx.x == 0) {
            float *r = a.r_out + ((size_t)stream * a.nlags + lag) * 2;
            r[0] = (float)(re * a.inv_m);
            r[1] = (float)(im * a.inv_m);
        }
    }
    int i;
    const bool live = out_slot(a.out, a.nfft, k, i);
    const size_t row = (size_t)a.nfft, wgrows = (size_t)a.gl * row;
    const float *base = a.partial + (slot0 * a.gl + g) * row + k;
    double t[1];
    if (!slice_sums<1>(live, a.W, [&](int w, int) { return base[(size_t)w * wgrows]; }, t)) return;
    store_psd(a.caf_out, ((size_t)stream * a.nlags + lag) * a.out.nout + i, t[0], a.scale, 0, a.out);
}

}  // namespace

#define OTH_LAG_KERNEL(N, GL) welch_lag_kernel<N, stat_threads(N), GL, mtm_keep(N), lag_accreg(N, GL)>

int welch_lag_blocks_per_cu(int nfft, int gl) {
    return mtm_for_build<1, kLagGroup>(nfft, gl, 0, [](auto n, auto g) {
        constexpr int N = decltype(n)::value, GL = decltype(g)::value;
        return resident_blocks<OTH_LAG_KERNEL(N, GL)>(stat_threads(N), stat_lds_bytes(N), 0);
    });
}

hipError_t launch_welch_lag(int nfft, int gl, int groups, const WelchLagArgs &a, hipStream_t s) {
    if (gl != 1 && gl != kLagGroup) return hipErrorInvalidValue;
    const dim3 grid(a.wg_per_stream, a.nstreams, groups);
    return mtm_for_build<1, kLagGroup>(nfft, gl, hipErrorInvalidValue, [&](auto n, auto g) {
        constexpr int N = decltype(n)::value, GL = decltype(g)::value;
        return launch_lds<OTH_LAG_KERNEL(N, GL)>(grid, dim3(stat_threads(N)), stat_lds_bytes(N), s, a);
    });
}

hipError_t launch_lag_finalize(const LagFinalizeArgs &a, int nstreams, hipStream_t s) {
    return launch_stat_finalize<lag_finalize_kernel>(a, nstreams, a.nlags, s);
}

}  // namespace oth
