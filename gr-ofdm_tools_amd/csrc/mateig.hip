// Eigenvalues and the principal eigenvector, per bin, of the spectral matrix S = scale T / M or of the coherence matrix
// G_ab = T_ab / sqrt(T_aa T_bb) of C coherent channels, 2 <= C <= 8, from the totals row [C][C][nfft] in double that
// welchmat.hip's mat_finalize_kernel leaves on the device (launch_mat_totals).
//
// One thread per live bin (out_slot, as mat_det_kernel).  The thread's Hermitian matrix lives in double in its own column of
// LDS, [entry][thread]: the packed upper triangle row by row at the build's channel capacity CC (re and im planes), and where
// the vector is asked for the C x C rotation product V behind it.  Consecutive lanes read consecutive 8-byte words, so no
// access has a bank conflict, and no thread reads another's column: there is no barrier.  The matrix is built from the totals
// exactly as mat_det_kernel builds S and G, with its `empty` and `bad` rules:
//   a channel whose T_aa is not finite               every eig and vec entry of the bin reads NaN
//   of S, a channel with T_aa <= 0                   its row and column of S are 0 (as s_out reads): one eigenvalue is exactly 0
//   of G, any channel with T_aa <= 0                 G is the identity (gcoh = 0): every eigenvalue 1, vec = e_0
//
// The solver is the cyclic Hermitian Jacobi: sweeps over p < q in row-cyclic order; for a_pq = g e^(i phi), g > 0,
//   tau = (a_qq - a_pp) / (2 g),  t = sign(tau) / (|tau| + sqrt(1 + tau^2)),  c = 1 / sqrt(1 + t^2),  s = t c   (Rutishauser)
//   J_pp = J_qq = c,  J_pq = s e^(i phi),  J_qp = -s e^(-i phi);  A <- J^H A J:  a_pp -= t g,  a_qq += t g,  a_pq = 0,
//   a_kp <- c a_kp - s e^(-i phi) a_kq,  a_kq <- s e^(i phi) a_kp + c a_kq   (k != p, q);  V <- V J the same way on every row.
// A rotation whose |a_pq| is exactly 0 is skipped: a zero row stays zero and its eigenvalue exactly 0.  A thread leaves the
// sweep loop when 2 sum_{p<q} |a_pq|^2 <= 2^-104 sum_p a_pp^2, tested in front of every sweep, and after kMatEigSweepCap sweeps
// at the latest (the float64 transcription of this loop in tests/: the worst count over the CPU test's matrices plus 2).  The eigenvalues are the diagonal: each goes to the row of its rank in descending order (ties: the lower Jacobi
// index first), clamped at 0, then cast to float.  The vector is the column of V at the largest eigenvalue's index (the lowest
// such index), rotated so that component 0 is real and >= 0 with an imaginary part stored as exactly 0; where component 0 is
// exactly 0 it leaves as computed.
//
// Builds: the channel capacity CC of welch_mat_capacity (2, 4, 8) x with / without the vector.  The loops over channels are
// unrolled to CC under uniform guards against nchan, so every LDS index is a constant plus the lane.  64 threads; LDS is
// 16 T (CC (CC + 1) / 2 + (vector ? CC^2 : 0)) bytes: 100 KiB at (8, vector) - dynamic LDS through launch_lds -, 36 KiB at 8
// without it, 26 / 10 KiB at 4, 7 / 3 KiB at 2.  An eigenvalue-only call takes the build without V: it pays nothing for the
// vector, and its A is updated by the same expressions, so the eigenvalue rows are the same bits either way.
// All arithmetic is double; float appears in the two stores only.  Deterministic: same totals, same bits.
//
// Not here: all C eigenvectors, more than 8 channels.
#include "out_stage.hip.h"
#include "launch.h"

namespace oth {
namespace {

constexpr int kMatEigThreads = 64;
constexpr int kMatEigSweepCap = 9;      // tests/test_welch_eig_cpu.py: the emulation's worst sweep count, 7, plus 2
constexpr double kMatEigTol = 0x1p-104;      // of the off-diagonal norm squared against the diagonal norm squared

// the place of (r, c), r <= c, in the upper triangle row by row at capacity CC
template <int CC> __device__ __forceinline__ constexpr int eig_at(int r, int c) { return r * CC - r * (r - 1) / 2 + (c - r); }

template <int CC, bool VEC> constexpr size_t mat_eig_lds(int threads) {
    return sizeof(double) * 2 * (size_t)threads * (CC * (CC + 1) / 2 + (VEC ? CC * CC : 0));
}

template <int CC, int T, bool VEC> __global__ __launch_bounds__(T) void mat_eig_kernel(MatEigArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int P = CC * (CC + 1) / 2;
    const int t = threadIdx.x, k = blockIdx.x * T + t, C = a.nchan;
    double *are = reinterpret_cast<double *>(smem) + t, *aim = are + P * T;      // [entry] at entry * T
    double *vre = aim + P * T, *vim = vre + (VEC ? CC * CC * T : 0);             // [row CC + column], with VEC only
    int i;
    if (!out_slot(a.out, a.nfft, k, i)) return;      // no barrier below: a thread works in its own column
    const size_t n = (size_t)a.nfft, nout = (size_t)a.out.nout;
    const double *tot = a.totals + k;
    bool empty = false, bad = false;
    for (int c = 0; c < C; ++c) {
        const double d = tot[(size_t)(c * C + c) * n];
        if (!isfinite(d)) bad = true;
        else if (d <= 0.0) empty = true;
    }
    if (bad) {
        const float nanf32 = __builtin_nanf("");
        for (int c = 0; c < C; ++c) {
            if (a.eig_out) a.eig_out[c * nout + i] = nanf32;
            if (VEC) a.vec_out[2 * (c * nout + i)] = a.vec_out[2 * (c * nout + i) + 1] = nanf32;
        }
        return;
    }
    const bool ofg = a.of != 0;
#pragma unroll
    for (int r = 0; r < CC; ++r) {
        if (r < C) {      // uniform
            const double trr = tot[(size_t)(r * C + r) * n];
#pragma unroll
            for (int c = r; c < CC; ++c) {
                if (c < C) {
                    const double tcc = tot[(size_t)(c * C + c) * n];
                    const double re = tot[(size_t)(r * C + c) * n], im = c > r ? tot[(size_t)(c * C + r) * n] : 0.0;
                    double xr, xi;
                    if (ofg) {
                        const double inv = empty ? 0.0 : 1.0 / sqrt(trr * tcc);
                        xr = c == r ? 1.0 : empty ? 0.0 : re * inv;
                        xi = c == r || empty ? 0.0 : im * inv;
                    } else {
                        const bool zero = trr <= 0.0 || tcc <= 0.0;
                        xr = zero ? 0.0 : re * a.s_scale;
                        xi = zero || c == r ? 0.0 : im * a.s_scale;
                    }
                    are[eig_at<CC>(r, c) * T] = xr;
                    aim[eig_at<CC>(r, c) * T] = xi;
                }
            }
        }
    }
    if constexpr (VEC) {
#pragma unroll
        for (int r = 0; r < CC; ++r)
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (r < C && c < C) {
                    vre[(r * CC + c) * T] = r == c ? 1.0 : 0.0;
                    vim[(r * CC + c) * T] = 0.0;
                }
    }

    for (int sweep = 0; sweep < kMatEigSweepCap; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int r = 0; r < CC; ++r) {
            if (r < C) {
                const double d = are[eig_at<CC>(r, r) * T];
                diag += d * d;
#pragma unroll
                for (int c = r + 1; c < CC; ++c) {
                    if (c < C) {
                        const double x = are[eig_at<CC>(r, c) * T], y = aim[eig_at<CC>(r, c) * T];
                        off += x * x + y * y;
                    }
                }
            }
        }
        if (2.0 * off <= kMatEigTol * diag) break;
#pragma unroll
        for (int p = 0; p < CC - 1; ++p) {
#pragma unroll
            for (int q = p + 1; q < CC; ++q) {
                if (q < C) {      // uniform
                    const double x = are[eig_at<CC>(p, q) * T], y = aim[eig_at<CC>(p, q) * T];
                    const double g = sqrt(x * x + y * y);
                    if (g != 0.0) {
                        const double app = are[eig_at<CC>(p, p) * T], aqq = are[eig_at<CC>(q, q) * T];
                        const double tau = (aqq - app) / (2.0 * g);
                        const double tt = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = tt * cs;
                        const double sr = sn * (x / g), si = sn * (y / g);      // s e^(i phi)
                        are[eig_at<CC>(p, p) * T] = app - tt * g;
                        are[eig_at<CC>(q, q) * T] = aqq + tt * g;
                        are[eig_at<CC>(p, q) * T] = 0.0;
                        aim[eig_at<CC>(p, q) * T] = 0.0;
#pragma unroll
                        for (int r = 0; r < CC; ++r) {
                            if (r != p && r != q && r < C) {
                                // a_rp and a_rq from the upper triangle: the stored entry, or its conjugate below the diagonal
                                const int ip = (r < p ? eig_at<CC>(r, p) : eig_at<CC>(p, r)) * T;
                                const int iq = (r < q ? eig_at<CC>(r, q) : eig_at<CC>(q, r)) * T;
                                const double fp = r < p ? 1.0 : -1.0, fq = r < q ? 1.0 : -1.0;
                                const double pr = are[ip], pi = fp * aim[ip], qr = are[iq], qi = fq * aim[iq];
                                const double npr = cs * pr - (sr * qr + si * qi), npi = cs * pi - (sr * qi - si * qr);
                                const double nqr = (sr * pr - si * pi) + cs * qr, nqi = (sr * pi + si * pr) + cs * qi;
                                are[ip] = npr;
                                aim[ip] = fp * npi;
                                are[iq] = nqr;
                                aim[iq] = fq * nqi;
                            }
                        }
                        if constexpr (VEC) {
#pragma unroll
                            for (int r = 0; r < CC; ++r) {
                                if (r < C) {
                                    const int ip = (r * CC + p) * T, iq = (r * CC + q) * T;
                                    const double pr = vre[ip], pi = vim[ip], qr = vre[iq], qi = vim[iq];
                                    vre[ip] = cs * pr - (sr * qr + si * qi);
                                    vim[ip] = cs * pi - (sr * qi - si * qr);
                                    vre[iq] = (sr * pr - si * pi) + cs * qr;
                                    vim[iq] = (sr * pi + si * pr) + cs * qi;
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    // every eigenvalue to the row of its rank, descending; the largest one's index (the lowest of equals) picks V's column
    int top = 0;
#pragma unroll
    for (int j = 0; j < CC; ++j) {
        if (j < C) {
            const double d = are[eig_at<CC>(j, j) * T];
            int rank = 0;
#pragma unroll
            for (int m = 0; m < CC; ++m) {
                if (m < C && m != j) {
                    const double e = are[eig_at<CC>(m, m) * T];
                    rank += (e > d || (e == d && m < j)) ? 1 : 0;
                }
            }
            if (rank == 0) top = j;
            if (a.eig_out) a.eig_out[rank * nout + i] = (float)(d < 0.0 ? 0.0 : d);
        }
    }
    if constexpr (VEC) {
        const double zr = vre[top * T], zi = vim[top * T];      // component 0
        const double z = sqrt(zr * zr + zi * zi);
        const double ur = z != 0.0 ? zr / z : 1.0, ui = z != 0.0 ? -zi / z : 0.0;      // conj(v_0) / |v_0|
#pragma unroll
        for (int r = 0; r < CC; ++r) {
            if (r < C) {
                const double xr = vre[(r * CC + top) * T], xi = vim[(r * CC + top) * T];
                double wr = xr * ur - xi * ui, wi = xr * ui + xi * ur;
                if (r == 0 && z != 0.0) wr = z, wi = 0.0;
                a.vec_out[2 * (r * nout + i)] = (float)wr;
                a.vec_out[2 * (r * nout + i) + 1] = (float)wi;
            }
        }
    }
}

}  // namespace

hipError_t launch_mat_eig(int cc, const MatEigArgs &a, hipStream_t s) {
    if (a.nchan < 2 || a.nchan > cc || (!a.eig_out && !a.vec_out)) return hipErrorInvalidValue;
    const dim3 grid((a.nfft + kMatEigThreads - 1) / kMatEigThreads), block(kMatEigThreads);
    auto go = [&](auto c, auto v) {
        constexpr int CC = decltype(c)::value;
        constexpr bool VEC = decltype(v)::value;
        return launch_lds<mat_eig_kernel<CC, kMatEigThreads, VEC>>(grid, block, mat_eig_lds<CC, VEC>(kMatEigThreads), s, a);
    };
    auto cap = [&](auto v) {
        if (cc == 2) return go(std::integral_constant<int, 2>{}, v);
        if (cc == 4) return go(std::integral_constant<int, 4>{}, v);
        if (cc == kMatChanMax) return go(std::integral_constant<int, kMatChanMax>{}, v);
        return hipErrorInvalidValue;
    };
    return a.vec_out ? cap(std::true_type{}) : cap(std::false_type{});
}

}  // namespace oth
