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
// The basis build (mat_eig_basis_kernel, one per capacity; launch_mat_eig_basis) is the with-vector build up to the end of
// the sweep loop - the same body, the same LDS - and then stores, in double, the C eigenvalues clamped at 0 to the rows of
// their rank and every column of V to the rows of its eigenvalue's rank in a workspace [CC + 2 CC^2][nfft] ([entry][bin]:
// mat_basis_at), which matdoa.hip's direction stage reads with consecutive lanes on consecutive bins.  A bin that reads NaN
// stores a NaN first eigenvalue and nothing else; a trimmed bin stores nothing.
//
// Not here: all C eigenvectors as an output row, more than 8 channels.
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

// The two kernels' body is one text, mateig_body.hip.h (it says why it is no function), included under OTH_MAT_EIG_BASIS.
template <int CC, int T, bool VEC> __global__ __launch_bounds__(T) void mat_eig_kernel(MatEigArgs a) {
#define OTH_MAT_EIG_BASIS 0
#include "mateig_body.hip.h"
#undef OTH_MAT_EIG_BASIS
}

// the basis build: the with-vector body and LDS, a kernel name of its own - the six builds above keep theirs
template <int CC, int T> __global__ __launch_bounds__(T) void mat_eig_basis_kernel(MatEigArgs a, double *basis) {
    constexpr bool VEC = true;
#define OTH_MAT_EIG_BASIS 1
#include "mateig_body.hip.h"
#undef OTH_MAT_EIG_BASIS
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

size_t mat_eig_basis_entries(int cc) { return (size_t)cc + 2 * (size_t)cc * cc; }

hipError_t launch_mat_eig_basis(int cc, const MatEigArgs &a, double *basis, hipStream_t s) {
    if (a.nchan < 2 || a.nchan > cc || !basis) return hipErrorInvalidValue;
    const dim3 grid((a.nfft + kMatEigThreads - 1) / kMatEigThreads), block(kMatEigThreads);
    auto go = [&](auto c) {
        constexpr int CC = decltype(c)::value;
        return launch_lds<mat_eig_basis_kernel<CC, kMatEigThreads>>(grid, block, mat_eig_lds<CC, true>(kMatEigThreads), s, a, basis);
    };
    if (cc == 2) return go(std::integral_constant<int, 2>{});
    if (cc == 4) return go(std::integral_constant<int, 4>{});
    if (cc == kMatChanMax) return go(std::integral_constant<int, kMatChanMax>{});
    return hipErrorInvalidValue;
}

}  // namespace oth
