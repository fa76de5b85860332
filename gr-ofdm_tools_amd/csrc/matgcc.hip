// Generalized cross-correlation (Knapp & Carter: PHAT, SCOT, plain) and the delay of every pair a < b of C coherent channels,
// 2 <= C <= 8, from the totals row [C][C][nfft] in double that welchmat.hip's mat_finalize_kernel leaves on the device
// (launch_mat_totals with every bin live: the plan's shift and trim take no part).  With k the signed bins of the band
// band_lo ... band_hi of the nfft-point transform, NI = U nfft the build's length and l the lag in units of 1 / U sample:
//   u_k = T_ab[k] / |T_ab[k]|        0 where |T_ab[k]| = 0 or T_aa[k] <= 0 or T_bb[k] <= 0
//   w_k = 1 (PHAT), |T_ab| / sqrt(T_aa T_bb) (SCOT), |T_ab| (plain)
//   Z   = the count of in-band bins with u_k != 0 (PHAT, SCOT); sqrt(sum_k T_aa[k] sum_k T_bb[k]) over the band (plain)
//   R_ab[l] = (1 / Z) sum_k w_k u_k e^(+j 2 pi k l / NI),      l = -maxlag ... maxlag
// Signed bin k sits at index k mod NI of the NI-point inverse transform: band-limited interpolation by U.  Channel c carries
// s(t - tau_c), T_ab = sum conj(X_a) X_b carries e^(-j 2 pi f_k (tau_b - tau_a)), so |R_ab| peaks at l / U = tau_b - tau_a.
//
// One workgroup per pair, generic_threads(NI) threads, NI float2 of LDS and the reductions' slots behind them.
//   1. Z: a thread walks the tile indices i = tid, tid + T, ... - consecutive lanes on consecutive doubles of the four totals
//      rows the pair reads - and adds its in-band bins' terms of Z and a count of non-finite entries; one fixed-order block
//      sum of the three in double (xor-shuffles inside a wave, then the waves' slots in index order).
//   2. The fill: the same walk again (the rows are L2-resident: 32 B per bin), w_k u_k / Z formed in double and stored as
//      float2 at i, 0 outside the band.  Every LDS entry is written once by the lane that owns it - consecutive lanes on
//      consecutive 8-byte words, no strided scatter and no clearing pass.  The 1 / Z goes in here and not after the
//      transform: every entry is at most 1 in magnitude and their sum at most 1 whatever the input's scale, so a capture
//      whose float32 sums are finite cannot overflow the float32 transform.
//   3. fft_lds<NI, T, true> with the NI-entry table of the context's per-length cache.
//   4. The window's lags leave as they stand in LDS, and each thread keeps the largest |R|^2 (double, from the float pair)
//      of its lags, the lowest lag among equals.
//   5. A fixed-order block argmax - the order is total (value, then lowest lag), so the result does not depend on how the
//      waves fold -, then thread 0 reads |R| at i - 1, i, i + 1 and writes (i + d) / U, |R[i]|, arg R[i] with
//      d = 0.5 (y- - y+) / (y- - 2 y0 + y+), d = 0 at a window edge or where the denominator is not negative.
//   6. A pair with a non-finite total inside the band reads NaN in every output; Z = 0 (or not above 0) reads 0 everywhere.
//      Both are uniform over the workgroup and taken before the fill.
// The outputs are a function of the totals and the arguments only: the same bits run to run, and gcc_out and peak_out each
// the same bits with and without the other.  Not here: the ML / Hannan-Thomson weighting, coherence-gated weights, more than
// 8 channels.
#include "fft_lds.hip.h"
#include "oth_internal.h"
#include "launch.h"

namespace oth {
namespace {

constexpr int kGccSlots = 3 * 16;      // three doubles per wave, 16 waves at most
constexpr size_t mat_gcc_lds(int ni) { return sizeof(float2) * (size_t)ni + sizeof(double) * kGccSlots; }

// the totals of one in-band bin of the pair
struct GccBin {
    double re, im, taa, tbb;
    __device__ __forceinline__ bool finite() const { return isfinite(re) && isfinite(im) && isfinite(taa) && isfinite(tbb); }
    __device__ __forceinline__ bool live() const { return taa > 0.0 && tbb > 0.0 && (re != 0.0 || im != 0.0); }
};

// signed bin of tile index i, and whether the band holds it
template <int NI> __device__ __forceinline__ bool gcc_in_band(const MatGccArgs &a, int i, int &k) {
    k = i < NI / 2 ? i : i - NI;
    return k >= a.band_lo && k <= a.band_hi;
}

template <int NI, int T> __global__ __launch_bounds__(T) void mat_gcc_kernel(MatGccArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *buf = reinterpret_cast<float2 *>(smem);
    double *red = reinterpret_cast<double *>(buf + NI);      // [3][NW]
    constexpr int NQ = NI / T, NW = T / 64;
    static_assert(3 * NW <= kGccSlots, "a slot per wave and value");
    const int tid = threadIdx.x, C = a.nchan, L = a.maxlag, nlag = 2 * L + 1;
    const size_t n = (size_t)a.nfft;
    int ca = 0, cb = blockIdx.x;      // pair (ca, cb) of the order (0,1), (0,2), ..., (C-2,C-1)
    while (cb >= C - 1 - ca) {
        cb -= C - 1 - ca;
        ++ca;
    }
    cb += ca + 1;
    const double *raa = a.totals + (size_t)(ca * C + ca) * n, *rbb = a.totals + (size_t)(cb * C + cb) * n;
    const double *rre = a.totals + (size_t)(ca * C + cb) * n, *rim = a.totals + (size_t)(cb * C + ca) * n;
    auto bin = [&](int k) {
        const int kn = k < 0 ? k + a.nfft : k;
        return GccBin{rre[kn], rim[kn], raa[kn], rbb[kn]};
    };
    const bool plain = a.weighting == 0, phat = a.weighting == 1;

    // 1. Z and the count of non-finite bins
    double s0 = 0.0, s1 = 0.0, nbad = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        int k;
        if (gcc_in_band<NI>(a, tid + q * T, k)) {
            const GccBin t = bin(k);
            if (!t.finite()) nbad += 1.0;
            if (plain) {
                s0 += t.taa;
                s1 += t.tbb;
            } else if (t.live()) {
                s0 += 1.0;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off, 64);
        s1 += __shfl_xor(s1, off, 64);
        nbad += __shfl_xor(nbad, off, 64);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = s0;
        red[NW + (tid >> 6)] = s1;
        red[2 * NW + (tid >> 6)] = nbad;
    }
    __syncthreads();
    s0 = s1 = nbad = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        s0 += red[w];
        s1 += red[NW + w];
        nbad += red[2 * NW + w];
    }
    const double z = plain ? sqrt(s0 * s1) : s0;

    // 6. the degenerate pairs, uniform over the workgroup
    float *row = a.gcc_out ? a.gcc_out + 2 * (size_t)blockIdx.x * nlag : nullptr;
    float *peak = a.peak_out ? a.peak_out + 3 * (size_t)blockIdx.x : nullptr;
    if (nbad != 0.0 || !(z > 0.0)) {
        const float v = nbad != 0.0 ? __builtin_nanf("") : 0.f;
        if (row)
            for (int j = tid; j < 2 * nlag; j += T) row[j] = v;
        if (peak && tid < 3) peak[tid] = v;
        return;
    }

    // 2. the fill
    const double inv = 1.0 / z;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int i = tid + q * T;
        int k;
        float2 v = make_float2(0.f, 0.f);
        if (gcc_in_band<NI>(a, i, k)) {
            const GccBin t = bin(k);
            if (t.live()) {
                const double s = plain ? inv : phat ? inv / sqrt(t.re * t.re + t.im * t.im) : inv / sqrt(t.taa * t.tbb);
                v = make_float2((float)(t.re * s), (float)(t.im * s));
            }
        }
        buf[i] = v;
    }
    __syncthreads();

    // 3. the inverse transform
    fft_lds<NI, T, true>(buf, a.tw, tid);

    // 4. the window leaves; 5. the peak
    double best = -1.0;
    int at = 0x7fffffff;
    for (int j = tid; j < nlag; j += T) {      // ascending lags: the first of equals stays
        const int l = j - L;
        const float2 r = buf[l < 0 ? l + NI : l];
        if (row) {
            row[2 * j] = r.x;
            row[2 * j + 1] = r.y;
        }
        const double m2 = (double)r.x * (double)r.x + (double)r.y * (double)r.y;
        if (m2 > best) {
            best = m2;
            at = l;
        }
    }
    if (!peak) return;      // uniform
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(at, off, 64);
        if (ob > best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
        }
    }
    // the slots of the first sum are free: every thread read them before the fill's barrier
    if ((tid & 63) == 0) {
        red[tid >> 6] = best;
        red[NW + (tid >> 6)] = (double)at;
    }
    __syncthreads();
    if (tid != 0) return;
    best = red[0];
    at = (int)red[NW];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        const double ob = red[w];
        const int oa = (int)red[NW + w];
        if (ob > best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
        }
    }
    auto mag = [&](int l) {
        const float2 r = buf[l < 0 ? l + NI : l];
        return sqrt((double)r.x * (double)r.x + (double)r.y * (double)r.y);
    };
    const float2 top = buf[at < 0 ? at + NI : at];
    const double y0 = mag(at);
    double d = 0.0;
    if (at > -L && at < L) {
        const double ym = mag(at - 1), yp = mag(at + 1), den = ym - 2.0 * y0 + yp;
        if (den < 0.0) d = 0.5 * (ym - yp) / den;
    }
    peak[0] = (float)(((double)at + d) * (double)a.nfft / (double)NI);
    peak[1] = (float)y0;
    peak[2] = (float)atan2((double)top.y, (double)top.x);
}

}  // namespace

#define OTH_GCC_FOR_EACH_N(X) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096) X(8192) X(16384)

hipError_t launch_mat_gcc(int ni, const MatGccArgs &a, hipStream_t s) {
    if (a.nchan < 2 || a.nchan > kMatChanMax || !a.totals || !a.tw || (!a.gcc_out && !a.peak_out) || a.weighting < 0 || a.weighting > 2)
        return hipErrorInvalidValue;
    if (a.nfft < 64 || ni < a.nfft || ni > kGccPointsMax || ni % a.nfft || ni / a.nfft > kGccUpsampleMax) return hipErrorInvalidValue;
    if (a.band_lo < -a.nfft / 2 || a.band_hi > a.nfft / 2 - 1 || a.band_lo > a.band_hi || a.maxlag < 0 || a.maxlag > ni / 2 - 1)
        return hipErrorInvalidValue;
    const dim3 grid(a.nchan * (a.nchan - 1) / 2);
    switch (ni) {
#define X(N) \
    case N: return launch_lds<mat_gcc_kernel<N, generic_threads(N)>>(grid, dim3(generic_threads(N)), mat_gcc_lds(N), s, a);
        OTH_GCC_FOR_EACH_N(X)
#undef X
        default:
            return hipErrorInvalidValue;
    }
}

}  // namespace oth
