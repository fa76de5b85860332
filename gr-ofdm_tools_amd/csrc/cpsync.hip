// Cyclic-prefix symbol timing and carrier offset (oth_cp_sync): the correlator of van de Beek, Sandell and Boerjesson (1997),
// folded over all symbols of a capture.  Per stream x and hypothesis (Tu, cp), Ts = Tu + cp, S = floor((nsamples - Tu) / Ts):
//   z[n]     = x[n + Tu] conj(x[n])                 welchlag.hip's lag product: re = fma(ar, br, ai bi), im = ai br - ar bi
//   e[n]     = (|x[n]|^2 + |x[n + Tu]|^2) / 2
//   F[r]     = sum_{s < S} z[r + s Ts]              G[r] = sum_{s < S} e[r + s Ts]                 r < Ts
//   Gamma[t] = sum_{j < cp} F[(t + j) mod Ts]       Phi[t] = sum_{j < cp} G[(t + j) mod Ts]        t < Ts
//   Lambda[t]= |Gamma[t]| - rho Phi[t],   theta = the lowest t that maximises Lambda,
//   eps = arg(Gamma[theta]) / (2 pi),   rho_hat = |Gamma[theta]| / Phi[theta]   (0 where Phi == 0)
// No transform: a memory-bound fold with a residue-indexed accumulator, then two small launches.
//
// cps_fold_kernel<TILE, T>, grid (W tiles, streams, hypotheses).  A workgroup takes a tile of TILE = 4 T consecutive residues
// and a contiguous run of the stream's symbols; thread tid owns the residues tile TILE + tid + q T (q < 4), so consecutive
// threads read consecutive samples, 8 bytes each, and the lagged read of one symbol is the base read of a later one (L2).
// The three sums of a residue run in float32 over blocks of at most kCpsSymBlock = 64 symbols, counted from the run's first
// symbol; the blocks are added in double (65536 additions of 1.21 in float32 are off by 6.1e-4, of 64 by less than 3e-6).  A
// run leaves as one row [3][Ts] of doubles.  No atomics: a result depends on the launch shape (W per hypothesis) alone.
// T is 64, 128 or 256 by the launch's largest Ts, so that a short symbol still fills its waves.
//
// What a workgroup reads: the samples s Ts + r and s Ts + r + Tu for s < S, r < Ts; the furthest is S Ts - 1 + Tu, which the
// host's S keeps below nsamples.  What it writes: its own row of the partial buffer.
//
// cps_total_kernel, grid (blocks of 64 residues, streams, hypotheses x groups): the W rows of a (stream, hypothesis) go to NG
// groups of contiguous rows (NG about W / 32, at most 32), and a workgroup adds the rows of one group for 64 residues in double,
// four threads per residue, into the group's row - so that the rows of a long capture (W in the thousands at a short symbol)
// are read by NG times as many workgroups as a symbol has blocks.
//
// cps_window_kernel, grid (streams, hypotheses), 1024 threads: first the groups' rows are added in order into the totals
// [3][Ts] and the sums of each block of kCpsBlock = 64 residues (lanes ascending) are formed, both in the totals buffer, which
// the workgroup that wrote them reads back behind a barrier.  Then the circular window of an entry is at most two linear ranges,
// each summed in double as edge + whole blocks + edge - never as a difference of prefix sums, so an entry depends on the
// residues of its own window alone.  An entry one of whose three sums is not finite is stored as NaN (Gamma and Phi both);
// Lambda is formed in double from the unrounded sums and reduced to its lowest-index maximum; thread 0 forms the window at
// theta again (the same function, the same bits) and writes est = theta, eps, rho_hat, Lambda[theta] - four NaNs where the row
// holds a non-finite entry.
//
// Degenerate input.  All-zero input gives exact zeros and est = (0, 0, 0, 0).  A sample with a NaN or +-inf part makes the
// float32 sums of the residues n mod Ts and (n - Tu) mod Ts non-finite (every product with it is inf or NaN, and so is e);
// exactly the entries whose window covers such a residue are NaN, and every other entry takes the sums it takes in the clean
// run, in the same order.
#include "fft_lds.hip.h"
#include "oth_internal.h"
#include "launch.h"

namespace oth {
namespace {

constexpr int kCpsWinThreads = 1024;

template <int TILE, int T> __global__ __launch_bounds__(T) void cps_fold_kernel(CpsArgs p) {
    constexpr int Q = TILE / T;
    const int h = blockIdx.z, stream = blockIdx.y;
    const int tile = (int)(blockIdx.x % (unsigned)p.tiles_max), w = (int)(blockIdx.x / (unsigned)p.tiles_max);
    const int Tu = p.tu[h], Ts = Tu + p.cp[h], W = p.w[h];
    if (w >= W || tile * TILE >= Ts) return;
    const long long S = p.nsym[h];
    const long long s0 = (S * w) / W, s1 = (S * (w + 1)) / W;
    const int r0 = tile * TILE + (int)threadIdx.x;
    const float2 *__restrict__ xs = p.x + (size_t)stream * p.stream_stride;
    double dr[Q], di[Q], dg[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) dr[q] = di[q] = dg[q] = 0.0;
    for (long long sb = s0; sb < s1; sb += kCpsSymBlock) {
        const long long se = sb + kCpsSymBlock < s1 ? sb + kCpsSymBlock : s1;
        float fr[Q], fi[Q], fg[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) fr[q] = fi[q] = fg[q] = 0.f;
        for (long long s = sb; s < se; ++s) {
            const float2 *__restrict__ row = xs + (size_t)s * (size_t)Ts;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int r = r0 + q * T;
                if (r < Ts) {
                    const float2 b = row[r], a = row[r + Tu];      // a the lagged sample, b the base one
                    fr[q] += fmaf(a.x, b.x, a.y * b.y);
                    fi[q] += cross_im(b, a);
                    fg[q] += 0.5f * (fmaf(b.x, b.x, b.y * b.y) + fmaf(a.x, a.x, a.y * a.y));
                }
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            dr[q] += (double)fr[q];
            di[q] += (double)fi[q];
            dg[q] += (double)fg[q];
        }
    }
    double *__restrict__ out = p.rows + p.part_off[h] + ((size_t)stream * W + w) * 3 * (size_t)Ts;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int r = r0 + q * T;
        if (r < Ts) {
            out[r] = dr[q];
            out[(size_t)Ts + r] = di[q];
            out[2 * (size_t)Ts + r] = dg[q];
        }
    }
}

// totals of (stream, hypothesis h): [3][Ts] F re, F im, G, then [3][nb] the sums of their blocks of kCpsBlock residues
__device__ __forceinline__ double *cps_totals(const CpsArgs &p, int h, int stream, int Ts, int nb) {
    return p.rows + p.tot_off[h] + (size_t)stream * 3 * ((size_t)Ts + nb);
}

// the W rows of a hypothesis go to NG groups of contiguous rows; a workgroup adds the rows of one group for a block of kCpsBlock
// residues - four threads per residue, each a contiguous quarter of the group's rows, the quarters in order - into the row
// [3][Ts] of its group
__global__ __launch_bounds__(4 * kCpsBlock) void cps_total_kernel(CpsArgs p) {
    __shared__ double sh[3][4][kCpsBlock];
    const int h = blockIdx.z / (unsigned)p.ng_max, g = blockIdx.z % (unsigned)p.ng_max, stream = blockIdx.y, k = blockIdx.x;
    const int Ts = p.tu[h] + p.cp[h], W = p.w[h], NG = p.ng[h];
    if (g >= NG || k * kCpsBlock >= Ts) return;      // uniform: the barrier below is met by the whole workgroup or by nobody
    const int lane = threadIdx.x & (kCpsBlock - 1), sub = threadIdx.x / kCpsBlock;
    const int r = k * kCpsBlock + lane;
    const int g0 = (int)(((long long)W * g) / NG), g1 = (int)(((long long)W * (g + 1)) / NG);
    double a[3] = {0.0, 0.0, 0.0};
    if (r < Ts) {
        const int w0 = g0 + ((g1 - g0) * sub) / 4, w1 = g0 + ((g1 - g0) * (sub + 1)) / 4;
        const double *__restrict__ src = p.rows + p.part_off[h] + ((size_t)stream * W + w0) * 3 * (size_t)Ts + r;
#pragma unroll 4
        for (int w = w0; w < w1; ++w, src += 3 * (size_t)Ts) {
            a[0] += src[0];
            a[1] += src[(size_t)Ts];
            a[2] += src[2 * (size_t)Ts];
        }
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) sh[v][sub][lane] = a[v];
    __syncthreads();
    if (sub == 0 && r < Ts) {
        double *__restrict__ dst = p.rows + p.grp_off[h] + ((size_t)stream * NG + g) * 3 * (size_t)Ts + r;
#pragma unroll
        for (int v = 0; v < 3; ++v) dst[(size_t)v * Ts] = ((sh[v][0][lane] + sh[v][1][lane]) + sh[v][2][lane]) + sh[v][3][lane];
    }
}

// g += the residues a ... b - 1 of the three totals: edge, whole blocks, edge
__device__ __forceinline__ void cps_range(const double *tot, int Ts, int nb, int a, int b, double (&g)[3]) {
    if (a >= b) return;
    const int first = (a + kCpsBlock - 1) & ~(kCpsBlock - 1), last = b & ~(kCpsBlock - 1);
    const bool blocks = first < last;
    const int e0 = blocks ? first : b;
    for (int j = a; j < e0; ++j) {
        g[0] += tot[j];
        g[1] += tot[(size_t)Ts + j];
        g[2] += tot[2 * (size_t)Ts + j];
    }
    if (!blocks) return;
    const double *bs = tot + 3 * (size_t)Ts;
    for (int k = first / kCpsBlock; k < last / kCpsBlock; ++k) {
        g[0] += bs[k];
        g[1] += bs[nb + k];
        g[2] += bs[2 * nb + k];
    }
    for (int j = last; j < b; ++j) {
        g[0] += tot[j];
        g[1] += tot[(size_t)Ts + j];
        g[2] += tot[2 * (size_t)Ts + j];
    }
}

// the circular window of entry t: F re, F im and G summed over the residues t ... t + cp - 1 mod Ts
__device__ __forceinline__ void cps_window(const double *tot, int Ts, int nb, int cp, int t, double (&g)[3]) {
    g[0] = g[1] = g[2] = 0.0;
    const int end = t + cp;
    cps_range(tot, Ts, nb, t, end < Ts ? end : Ts, g);
    cps_range(tot, Ts, nb, 0, end - Ts, g);
}

__device__ __forceinline__ bool cps_finite(const double (&g)[3]) { return isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]); }

__global__ __launch_bounds__(kCpsWinThreads) void cps_window_kernel(CpsArgs p) {
    __shared__ double best_l[kCpsWinThreads];
    __shared__ int best_t[kCpsWinThreads];
    const int h = blockIdx.y, stream = blockIdx.x, tid = threadIdx.x;
    const int cp = p.cp[h], Ts = p.tu[h] + cp;
    const int nb = (Ts + kCpsBlock - 1) / kCpsBlock;
    double *tot = cps_totals(p, h, stream, Ts, nb);
    {      // the groups' rows added in order into the totals, then the sums of their blocks of kCpsBlock residues, lanes ascending
        const int NG = p.ng[h];
        const double *__restrict__ grp = p.rows + p.grp_off[h] + (size_t)stream * NG * 3 * (size_t)Ts;
        for (int i = tid; i < 3 * Ts; i += kCpsWinThreads) {
            double t = 0.0;
#pragma unroll 4
            for (int g = 0; g < NG; ++g) t += grp[(size_t)g * 3 * Ts + i];
            tot[i] = t;
        }
        __syncthreads();
        for (int i = tid; i < 3 * nb; i += kCpsWinThreads) {
            const int v = i / nb, k = i - v * nb;
            const int end = (k + 1) * kCpsBlock < Ts ? (k + 1) * kCpsBlock : Ts;
            double t = 0.0;
            for (int j = k * kCpsBlock; j < end; ++j) t += tot[(size_t)v * Ts + j];
            tot[3 * (size_t)Ts + i] = t;
        }
        __syncthreads();
    }
    const size_t row = ((size_t)stream * p.nhyp + h) * p.row_stride;
    const float nanf_ = __builtin_nanf("");
    double bl = -INFINITY;
    int bt = 0x7fffffff, bad = 0;
    for (int t = tid; t < Ts; t += kCpsWinThreads) {
        double g[3];
        cps_window(tot, Ts, nb, cp, t, g);
        const bool ok = cps_finite(g);
        if (p.gamma) p.gamma[row + t] = ok ? make_float2((float)g[0], (float)g[1]) : make_float2(nanf_, nanf_);
        if (p.phi) p.phi[row + t] = ok ? (float)g[2] : nanf_;
        if (ok) {
            const double lam = sqrt(g[0] * g[0] + g[1] * g[1]) - p.rho * g[2];
            if (lam > bl) bl = lam, bt = t;      // t ascends: the lowest index of a thread's maximum stays
        } else {
            bad = 1;
        }
    }
    bad = __syncthreads_or(bad);
    best_l[tid] = bl;
    best_t[tid] = bt;
    __syncthreads();
    for (int half = kCpsWinThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
            const double ol = best_l[tid + half];
            const int ot = best_t[tid + half];
            if (ol > best_l[tid] || (ol == best_l[tid] && ot < best_t[tid])) best_l[tid] = ol, best_t[tid] = ot;
        }
        __syncthreads();
    }
    if (tid == 0) {
        float *__restrict__ est = p.est + ((size_t)stream * p.nhyp + h) * 4;
        if (bad) {
            est[0] = est[1] = est[2] = est[3] = nanf_;
        } else {
            const int theta = best_t[0];
            double g[3];
            cps_window(tot, Ts, nb, cp, theta, g);
            const double mag = sqrt(g[0] * g[0] + g[1] * g[1]);
            est[0] = (float)theta;
            est[1] = (float)(atan2(g[1], g[0]) * 0.15915494309189535);      // 1 / (2 pi)
            est[2] = g[2] == 0.0 ? 0.f : (float)(mag / g[2]);
            est[3] = (float)(mag - p.rho * g[2]);
        }
    }
}

#define OTH_CPS_FOLD(T) cps_fold_kernel<4 * T, T>

}  // namespace

int cps_fold_threads(int ts_max) { return ts_max <= 256 ? 64 : (ts_max <= 512 ? 128 : 256); }

int cps_fold_blocks_per_cu(int threads) {
    switch (threads) {
        case 64: return resident_blocks<OTH_CPS_FOLD(64)>(64, 0, 0);
        case 128: return resident_blocks<OTH_CPS_FOLD(128)>(128, 0, 0);
        case 256: return resident_blocks<OTH_CPS_FOLD(256)>(256, 0, 0);
        default: return 0;
    }
}

hipError_t launch_cps_fold(int threads, const CpsArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.w_max * (unsigned)a.tiles_max, (unsigned)a.nstreams, (unsigned)a.nhyp);
    switch (threads) {
        case 64: return launch_lds<OTH_CPS_FOLD(64)>(grid, dim3(64), 0, s, a);
        case 128: return launch_lds<OTH_CPS_FOLD(128)>(grid, dim3(128), 0, s, a);
        case 256: return launch_lds<OTH_CPS_FOLD(256)>(grid, dim3(256), 0, s, a);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_cps_finalize(const CpsArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.nb_max, (unsigned)a.nstreams, (unsigned)a.nhyp * (unsigned)a.ng_max);
    const hipError_t e = launch_lds<cps_total_kernel>(grid, dim3(4 * kCpsBlock), 0, s, a);
    if (e != hipSuccess) return e;
    return launch_lds<cps_window_kernel>(dim3((unsigned)a.nstreams, (unsigned)a.nhyp), dim3(kCpsWinThreads), 0, s, a);
}

}  // namespace oth
