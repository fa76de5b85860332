// Bartlett, Capon (MVDR) and MUSIC direction spectra, per bin and per direction, of the spectral matrix S or of the coherence
// matrix G of C coherent channels, 2 <= C <= 8, from the eigenbasis that mateig.hip's basis build leaves on the device
// (launch_mat_eig_basis: the eigenvalues l_1 >= ... >= l_C clamped at 0 and their vectors v_i, in double, [entry][bin]) and a
// steering table of D directions: per direction d and channel c a delay tau in samples and frac(fc tau), the carrier's
// whole cycles taken off on the host.  Channel c carries s(t - tau_c), so at bin k, whose signed frequency is
// f_k = k / nfft below nfft / 2 and (k - nfft) / nfft from there on, X_c = X_s e^(-j 2 pi (fc + f_k) tau_c); the family's
// matrix is S_ab = E[conj(X_a) X_b], so the vector of the quadratic forms is
//   w_c(d, k) = e^(+j 2 pi (frac(fc tau_dc) + f_k tau_dc))      the phase in double, sincospi of twice it: no recurrence over bins
// and with y_i = v_i^H w, p_i = |y_i|^2, delta = loading sum_i l_i / C:
//   Bartlett   sum_i l_i p_i / C^2                    = w^H A w / C^2
//   Capon      1 / sum_i p_i / (l_i + delta)          = 1 / w^H (A + delta I)^-1 w;  exactly 0 in a bin where l_C + delta <= 0
//   MUSIC      C / sum_{i > nsrc} p_i                  +inf where the sum is exactly 0
// One projection onto the eigenbasis serves the three.  A bin whose first eigenvalue is NaN (the basis build's mark of a
// non-finite channel) reads NaN in every row.
//
// Grid: (tiles of 64 bins) x (tiles of kDoaTile directions).  256 threads = 64 bins x 4 direction lanes: a wave is 64
// consecutive bins on one direction lane.  The workgroup stages its bins' basis into LDS as it lies in memory, [entry][bin]
// (consecutive lanes on consecutive 8-byte words: coalesced loads, no bank conflict on either side; the waves of a workgroup
// read the same words) - CC + 2 CC^2 doubles per bin, 68 KiB at CC = 8 (dynamic LDS through launch_lds), 18 KiB at 4, 5 KiB
// at 2 -, then a thread walks the directions of its lane: C sincospi for w, and for each vector the C complex multiply-adds
// of y_i with V read from LDS, its p_i folded into the three sums at once.  The table's entries are wave-uniform.
// The loops over channels are unrolled to the capacity CC under uniform guards against nchan, so every LDS index is a
// constant plus the lane and nothing is indexed dynamically.  All arithmetic is double; float appears in the stores only.
// A direction's values are a function of its own table row and the bin's basis: they do not depend on which other
// directions share the table or the tile.  Deterministic: same basis, same table, same bits.
//
// Not here: a wideband combination over bins, tabulated array manifolds, more than 8 channels.
#include "out_stage.hip.h"
#include "launch.h"

namespace oth {
namespace {

constexpr int kDoaBins = 64;       // bins of a workgroup: a wave
constexpr int kDoaLanes = 4;       // direction lanes of a workgroup: its waves
constexpr int kDoaTile = 32;       // directions of a workgroup
constexpr int kDoaThreads = kDoaBins * kDoaLanes;

template <int CC> constexpr size_t mat_doa_lds() { return sizeof(double) * kDoaBins * (CC + 2 * CC * CC); }

template <int CC, int T> __global__ __launch_bounds__(T) void mat_doa_kernel(MatDoaArgs a) {
    static_assert(T == kDoaThreads, "64 bins x the direction lanes");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int E = CC + 2 * CC * CC, B = kDoaBins;
    double *lds = reinterpret_cast<double *>(smem);
    const int b = threadIdx.x % B, lane = threadIdx.x / B, C = a.nchan;
    const int k = blockIdx.x * B + b;
    const size_t n = (size_t)a.nfft, nout = (size_t)a.out.nout;
    // the entries the basis build wrote (rank and channel below C); a bin it left out is staged as it lies and never read
    if (k < a.nfft) {
        for (int e = lane; e < E; e += kDoaLanes) {
            const int v = (e - CC) / 2;
            const bool live = e < CC ? e < C : (v / CC < C && v % CC < C);
            if (live) lds[e * B + b] = a.basis[(size_t)e * n + k];
        }
    }
    __syncthreads();
    int slot;
    if (!out_slot(a.out, a.nfft, k, slot)) return;      // no barrier below
    const double *col = lds + b;
    const int d0 = blockIdx.y * kDoaTile, d1 = min(a.ndir, d0 + kDoaTile);
    if (isnan(col[0])) {
        const float nanf32 = __builtin_nanf("");
        for (int d = d0 + lane; d < d1; d += kDoaLanes) {
            if (a.bartlett_out) a.bartlett_out[d * nout + slot] = nanf32;
            if (a.capon_out) a.capon_out[d * nout + slot] = nanf32;
            if (a.music_out) a.music_out[d * nout + slot] = nanf32;
        }
        return;
    }
    double lam[CC], inv[CC], trace = 0.0, low = 0.0;
#pragma unroll
    for (int i = 0; i < CC; ++i) {
        if (i < C) {      // uniform
            lam[i] = low = col[i * B];
            trace += lam[i];
        }
    }
    const double delta = a.loading * trace / (double)C;
    const bool capon_zero = low + delta <= 0.0;      // the rows descend: l_C is the last one read
#pragma unroll
    for (int i = 0; i < CC; ++i)
        if (i < C) inv[i] = 1.0 / (lam[i] + delta);
    const double fk = (double)(k < a.nfft / 2 ? k : k - a.nfft) / (double)a.nfft;
    const double inv_c2 = 1.0 / (double)(C * C);

    for (int d = d0 + lane; d < d1; d += kDoaLanes) {
        const double *tau = a.tau + (size_t)d * C, *frac = a.frac + (size_t)d * C;
        double wr[CC], wi[CC];
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            if (c < C) {
                const double phase = frac[c] + fk * tau[c];
                sincospi(2.0 * phase, &wi[c], &wr[c]);
            }
        }
        double bart = 0.0, cap = 0.0, noise = 0.0;
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            if (i < C) {
                double yr = 0.0, yi = 0.0;      // y_i = sum_c conj(v_ic) w_c
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    if (c < C) {
                        const double vr = col[mat_basis_at(CC, i, c) * B], vi = col[(mat_basis_at(CC, i, c) + 1) * B];
                        yr += vr * wr[c] + vi * wi[c];
                        yi += vr * wi[c] - vi * wr[c];
                    }
                }
                const double p = yr * yr + yi * yi;
                bart += lam[i] * p;
                cap += p * inv[i];
                if (i >= a.nsrc) noise += p;
            }
        }
        if (a.bartlett_out) a.bartlett_out[d * nout + slot] = (float)(bart * inv_c2);
        if (a.capon_out) a.capon_out[d * nout + slot] = capon_zero ? 0.0f : (float)(1.0 / cap);
        if (a.music_out) a.music_out[d * nout + slot] = noise == 0.0 ? __builtin_inff() : (float)((double)C / noise);
    }
}

}  // namespace

hipError_t launch_mat_doa(int cc, const MatDoaArgs &a, hipStream_t s) {
    if (a.nchan < 2 || a.nchan > cc || a.ndir < 1 || a.ndir > kDoaDirsMax || !a.basis || !a.tau || !a.frac ||
        (!a.bartlett_out && !a.capon_out && !a.music_out))
        return hipErrorInvalidValue;
    const dim3 grid((a.nfft + kDoaBins - 1) / kDoaBins, (a.ndir + kDoaTile - 1) / kDoaTile), block(kDoaThreads);
    if (cc == 2) return launch_lds<mat_doa_kernel<2, kDoaThreads>>(grid, block, mat_doa_lds<2>(), s, a);
    if (cc == 4) return launch_lds<mat_doa_kernel<4, kDoaThreads>>(grid, block, mat_doa_lds<4>(), s, a);
    if (cc == kMatChanMax) return launch_lds<mat_doa_kernel<kMatChanMax, kDoaThreads>>(grid, block, mat_doa_lds<kMatChanMax>(), s, a);
    return hipErrorInvalidValue;
}

}  // namespace oth
