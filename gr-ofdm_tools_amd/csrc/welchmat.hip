// Spectral matrix and generalized coherence of C coherent channels on a Welch plan, 2 <= C <= 8: per segment s, channel a
// and bin j, with m_s,a the segment's mean on a detrending plan,
//   X_s,a[j] = FFT((x_a,s[n] - m_s,a) w[n])[j]
//   T_ab[j]  = sum_s conj(X_s,a[j]) X_s,b[j]      a <= b; T_aa real
// mat_finalize_kernel adds the workgroups' rows in double; mat_det_kernel turns them into S_ab = scale T_ab / M, the coherence
// matrix G_ab = T_ab / sqrt(T_aa T_bb) and gcoh = 1 - det G (the Hadamard ratio, the GLRT for a common signal in
// uncalibrated receivers).
//
// The body is welchsk.hip's (a whole segment per work item, the segments to W workgroups in contiguous runs, segment entry by
// mtm_segment_entry, the window product into the one LDS buffer, fft_lds) once per channel of the segment: a channel of a
// segment is transformed once and read from HBM once.  A thread keeps the bins it owns of every channel, and after the last
// channel adds the C squares and the C (C - 1) / 2 cross products of each owned bin.
//
// Builds: a channel capacity CC of 2, 4 or 8 per size, the loops over channels unrolled to CC under a uniform c < nchan guard -
// 27 kernels instead of 63.  Where the state lives, per (N, CC), is whichever builds without scratch
// (tests/test_welch_matrix_cpu.py reads the code objects):
//   in registers (mat_reg)   the owned bins of the C spectra, 2 CC N / T registers, and the C^2 running rows, CC^2 N / T:
//                            CC = 2 up to 8192 points, CC = 4 up to 4096, CC = 8 at 64, 128, 256 and 1024 points.
//   in memory                everywhere else.  The spectra go through a row of global memory that belongs to the workgroup
//                            (WelchMatArgs.ws): every thread writes the bins it owns and reads the same addresses back - no
//                            barrier (welchcyc.hip's 16384-point path).  The sums live in the workgroup's own partial rows:
//                            the first segment of a run stores, every later one reads, adds and stores, each thread its own
//                            addresses (welchsk.hip's 16384-point path), pair by pair.
//                            Spectra in registers next to sums in memory was tried at (512, 8), (2048, 8), (4096, 8) and
//                            (8192, 4): every one of them spilled, so the two go together.
//   samples                  in registers between the mean and the window product below 8192 points (mtm_keep), read again
//                            above.
// The rows leave as partial[wg][C][C][N] in natural bin order: entry [a][b] with a <= b is Re T_ab, [b][a] with a < b is
// Im T_ab.  The finalize launches add them in double in a fixed order: a result depends on the launch shape only.
//
// Arithmetic the tests rely on: |X|^2 = fma(Xr, Xr, Xi Xi), Re conj(A) B = fma(Ar, Br, Ai Bi) - the same expression shape, so
// two identical channels give three bit-identical rows - and Im conj(A) B is cross_im's two rounded products (fft_lds.hip.h):
// exactly 0 on identical channels and exactly negated when the two channels change places.
//
// Not here: partial sums for time-sharded runs, multitaper plans, transform lengths that are not a power of two, more than 8
// channels.  The eigenvalues of S and G are mateig.hip's, from the totals row of launch_mat_totals.
#include "mtm_common.hip.h"
#include "out_stage.hip.h"
#include "launch.h"

namespace oth {
namespace {

// registers a lane may hold at this workgroup size (stat_threads: N / T <= 8 up to 8192 points), and what the transform, the
// samples and the addresses take of them
constexpr int mat_regs(int n) { return stat_threads(n) <= 256 ? 512 : stat_threads(n) == 512 ? 256 : 128; }
constexpr int kMatReserve = 64;
constexpr int mat_nq(int n) { return n / stat_threads(n); }
// the owned bins of the C spectra (2 C N / T registers) and the C^2 running rows (C^2 N / T) in registers
constexpr bool mat_reg(int n, int cc) { return n < 16384 && (2 * cc + cc * cc) * mat_nq(n) + kMatReserve <= mat_regs(n); }

template <int N, int T, int CC, bool KEEP, bool REG> __global__ __launch_bounds__(T) void welch_mat_kernel(WelchMatArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *buf = reinterpret_cast<float2 *>(smem);
    float2 *red = buf + N;      // [0] the pilot, [1 ...] the block sum's wave rows
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_count, C = p.nchan;
    const long long s0 = (p.nseg * wg) / W, s1 = (p.nseg * (wg + 1)) / W;
    float *dst = p.partial + (size_t)wg * C * C * N;
    float2 *ws = REG ? nullptr : p.ws + (size_t)wg * C * N;

    float acc[REG ? CC * CC : 1][REG ? NQ : 1];      // [a CC + b]: Re T_ab (a <= b), Im T_ba (a > b)
    if constexpr (REG) {
#pragma unroll
        for (int r = 0; r < CC * CC; ++r)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[r][q] = 0.f;
    }
    float2 spec[REG ? CC : 1][REG ? NQ : 1];
    float2 v[KEEP ? NQ : 1];

    for (long long s = s0; s < s1; ++s) {
        const bool first = s == s0;      // of the run: its sums start here
#pragma unroll REG ? CC : 1      // the registers are indexed by c
        for (int c = 0; c < CC; ++c) {
            if (c < C) {      // uniform
                int tid = tid0;      // an opaque copy, as in mtm_kernel: the passes' index arithmetic is not hoisted nor shared
                asm volatile("" : "+v"(tid));
                const float2 *xs = p.x + (size_t)c * p.chan_stride + s * p.step;
                float2 pil, mean;
                mtm_segment_entry<N, T, KEEP>(xs, p.nperseg, p.detrend != 0, red, tid, v, pil, mean);
                mtm_taper_product<N, T, KEEP>(xs, p.win, p.nperseg, tid, pil, mean, v, buf);
                __syncthreads();
                fft_lds<N, T>(buf, p.tw, tid);
#pragma unroll
                for (int q = 0; q < NQ; ++q) {      // this thread's bins
                    if constexpr (REG) spec[REG ? c : 0][REG ? q : 0] = buf[tid + q * T];
                    else ws[(size_t)c * N + tid + q * T] = buf[tid + q * T];
                }
                __syncthreads();
            }
        }
        if constexpr (REG) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
#pragma unroll
                for (int a = 0; a < CC; ++a) {
                    if (a < C) {      // uniform
                        const float2 A = spec[REG ? a : 0][REG ? q : 0];
                        acc[REG ? a * CC + a : 0][REG ? q : 0] += fmaf(A.x, A.x, A.y * A.y);
#pragma unroll
                        for (int b = a + 1; b < CC; ++b) {
                            if (b < C) {
                                const float2 B = spec[REG ? b : 0][REG ? q : 0];
                                acc[REG ? a * CC + b : 0][REG ? q : 0] += fmaf(A.x, B.x, A.y * B.y);      // conj(X_a) X_b
                                acc[REG ? b * CC + a : 0][REG ? q : 0] += cross_im(A, B);
                            }
                        }
                    }
                }
            }
        } else {
            // pair by pair, four bins at a time, so that the loads in flight do not outgrow the registers; X_a and X_b come
            // back from the workgroup's row (L1 / L2) for every pair
            auto sum = [&](auto load) {
                auto add = [&](float *at, float val) {
                    float b = 0.f;
                    if constexpr (decltype(load)::value) b = *at;
                    *at = b + val;
                };
                for (int a = 0; a < C; ++a) {
                    const float2 *wa = ws + (size_t)a * N;
                    for (int b = a; b < C; ++b) {
                        const float2 *wb = ws + (size_t)b * N;
                        float *re = dst + (size_t)(a * C + b) * N, *im = dst + (size_t)(b * C + a) * N;
                        if (a == b) {
#pragma unroll 4
                            for (int q = 0; q < NQ; ++q) {
                                const int j = tid0 + q * T;
                                const float2 A = wa[j];
                                add(re + j, fmaf(A.x, A.x, A.y * A.y));
                            }
                        } else {
#pragma unroll 4
                            for (int q = 0; q < NQ; ++q) {
                                const int j = tid0 + q * T;
                                const float2 A = wa[j], B = wb[j];
                                add(re + j, fmaf(A.x, B.x, A.y * B.y));      // conj(X_a) X_b
                                add(im + j, cross_im(A, B));
                            }
                        }
                    }
                }
            };
            if (!first) sum(std::true_type{});
            else sum(std::false_type{});
        }
    }
    if constexpr (REG) {
#pragma unroll
        for (int a = 0; a < CC; ++a)
#pragma unroll
            for (int b = 0; b < CC; ++b)
                if (a < C && b < C) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) dst[(size_t)(a * C + b) * N + tid0 + q * T] = acc[REG ? a * CC + b : 0][REG ? q : 0];
                }
    }
}

// The shared finalize stage (out_stage.hip.h), one of the C^2 rows per blockIdx.z: the W workgroups' sums of a live bin in
// double in a fixed order into the totals row [C][C][nfft] (natural bin order) mat_det_kernel reads.
__global__ __launch_bounds__(256) void mat_finalize_kernel(MatFinalizeArgs a) {
    const int k = blockIdx.x * 32 + (threadIdx.x & 31), row = blockIdx.z;
    int i;
    const bool live = out_slot(a.out, a.nfft, k, i);
    const size_t n = (size_t)a.nfft, wgrows = (size_t)a.nchan * a.nchan * n;
    const float *base = a.partial + (size_t)row * n + k;
    double t[1];
    if (!slice_sums<1>(live, a.W, [&](int w, int) { return base[(size_t)w * wgrows]; }, t)) return;
    a.totals[(size_t)row * n + k] = t[0];
}

// One thread per bin on the totals: S_ab = scale T_ab / M into the packed upper triangle, then G in double in this thread's
// column of LDS, its determinant by LDL^H without square roots (the Schur complement, pivot by pivot), and gcoh = 1 - det G.
//   a channel without power in the bin (T_aa <= 0: silence, a constant under detrend)   its rows read 0, gcoh reads 0
//   a channel whose T_aa is not finite (a NaN or inf sample)                             its rows and gcoh read NaN
// Every other entry is the bin's own totals times the scale: untouched bit for bit by what another channel holds.
constexpr int kMatDetThreads = 64;
constexpr int kMatPairsMax = kMatChanMax * (kMatChanMax + 1) / 2;
__global__ __launch_bounds__(kMatDetThreads) void mat_det_kernel(MatFinalizeArgs a) {
    __shared__ double gre[kMatPairsMax][kMatDetThreads], gim[kMatPairsMax][kMatDetThreads];
    const int t = threadIdx.x, k = blockIdx.x * kMatDetThreads + t, C = a.nchan;
    int i;
    if (!out_slot(a.out, a.nfft, k, i)) return;      // no barrier below: a thread works in its own column
    const size_t n = (size_t)a.nfft;
    const double *tot = a.totals + k;
    bool empty = false, bad = false;
    for (int c = 0; c < C; ++c) {
        const double d = tot[(size_t)(c * C + c) * n];
        if (!isfinite(d)) bad = true;
        else if (d <= 0.0) empty = true;
    }
    const float nanf32 = __builtin_nanf("");
    int pr = 0;      // the pair's place in the upper triangle, row by row
    for (int r = 0; r < C; ++r) {
        const double trr = tot[(size_t)(r * C + r) * n];
        for (int c = r; c < C; ++c, ++pr) {
            const double tcc = tot[(size_t)(c * C + c) * n];
            const double re = tot[(size_t)(r * C + c) * n], im = c > r ? tot[(size_t)(c * C + r) * n] : 0.0;
            if (a.s_out) {
                float sr, si;
                if (!isfinite(trr) || !isfinite(tcc)) sr = si = nanf32;
                else if (trr <= 0.0 || tcc <= 0.0) sr = si = 0.f;
                else sr = (float)(re * a.s_scale), si = (float)(im * a.s_scale);
                if (c == r) si = 0.f;
                const size_t o = (size_t)pr * a.out.nout + i;
                a.s_out[2 * o] = sr;
                a.s_out[2 * o + 1] = si;
            }
            if (!bad && !empty) {
                const double inv = 1.0 / sqrt(trr * tcc);
                gre[pr][t] = c == r ? 1.0 : re * inv;
                gim[pr][t] = im * inv;
            }
        }
    }
    if (!a.gcoh_out) return;
    float g;
    if (bad) {
        g = nanf32;
    } else if (empty) {
        g = 0.f;
    } else {
        auto at = [C](int r, int c) { return r * C - r * (r - 1) / 2 + (c - r); };      // r <= c
        double det = 1.0;
        for (int piv = 0; piv < C; ++piv) {
            const double d = gre[at(piv, piv)][t];
            if (!(d > 0.0)) {      // singular up to rounding (M < C, identical channels): det G = 0
                det = 0.0;
                break;
            }
            det *= d;
            const double invd = 1.0 / d;
            for (int r = piv + 1; r < C; ++r) {
                // A_rc -= conj(A_piv,r) A_piv,c / A_piv,piv
                const double ur = gre[at(piv, r)][t] * invd, ui = gim[at(piv, r)][t] * invd;
                for (int c = r; c < C; ++c) {
                    const double vr = gre[at(piv, c)][t], vi = gim[at(piv, c)][t];
                    gre[at(r, c)][t] -= ur * vr + ui * vi;
                    gim[at(r, c)][t] -= ur * vi - ui * vr;
                }
            }
        }
        double gc = 1.0 - det;
        gc = gc < 0.0 ? 0.0 : gc > 1.0 ? 1.0 : gc;      // Hadamard's inequality up to the float32 rounding of the rows
        g = (float)gc;
    }
    a.gcoh_out[i] = g;
}

}  // namespace

#define OTH_MAT_KERNEL(N, CC) welch_mat_kernel<N, stat_threads(N), CC, mtm_keep(N), mat_reg(N, CC)>

int welch_mat_capacity(int nchan) { return nchan <= 2 ? 2 : nchan <= 4 ? 4 : kMatChanMax; }

size_t welch_mat_ws_points(int nfft, int cc) {
    return mtm_for_build<2, 4, kMatChanMax>(nfft, cc, (size_t)0, [](auto n, auto c) { return mat_reg(n(), c()) ? (size_t)0 : (size_t)n(); });
}

int welch_mat_blocks_per_cu(int nfft, int cc) {
    return mtm_for_build<2, 4, kMatChanMax>(nfft, cc, 0, [](auto n, auto c) {
        constexpr int N = decltype(n)::value, CC = decltype(c)::value;
        return resident_blocks<OTH_MAT_KERNEL(N, CC)>(stat_threads(N), stat_lds_bytes(N), 0);
    });
}

hipError_t launch_welch_mat(int nfft, int cc, const WelchMatArgs &a, hipStream_t s) {
    if (cc != 2 && cc != 4 && cc != kMatChanMax) return hipErrorInvalidValue;
    if (a.nchan < 2 || a.nchan > cc) return hipErrorInvalidValue;
    const dim3 grid(a.wg_count);
    return mtm_for_build<2, 4, kMatChanMax>(nfft, cc, hipErrorInvalidValue, [&](auto n, auto c) {
        constexpr int N = decltype(n)::value, CC = decltype(c)::value;
        return launch_lds<OTH_MAT_KERNEL(N, CC)>(grid, dim3(stat_threads(N)), stat_lds_bytes(N), s, a);
    });
}

hipError_t launch_mat_totals(const MatFinalizeArgs &a, hipStream_t s) {
    if (a.nchan < 2 || a.nchan > kMatChanMax) return hipErrorInvalidValue;
    return launch_stat_finalize<mat_finalize_kernel>(a, 1, a.nchan * a.nchan, s);
}

hipError_t launch_mat_finalize(const MatFinalizeArgs &a, hipStream_t s) {
    const hipError_t e = launch_mat_totals(a, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mat_det_kernel, dim3((a.nfft + kMatDetThreads - 1) / kMatDetThreads), dim3(kMatDetThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace oth
