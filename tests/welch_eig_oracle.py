"""float64 oracle of the eigenvalues and the principal eigenvector of the spectral matrix S and of the coherence matrix G of C
channels on a Welch plan (oth_welch_matrix_eig): numpy.linalg.eigh per bin on tests/welch_matrix_oracle.py's S, and on
G_ab = T_ab / sqrt(T_aa T_bb) formed from its T, with the library's rules - rows descending, values below 0 clamped to 0, the
vector of the largest eigenvalue with unit norm and component 0 real and >= 0; a non-finite channel reads NaN everywhere; a
silent channel leaves a zero row and column in S and turns G into the identity (vec = e_0 where the matrix is 0 or the identity).
jacobi_emulation is a float64 transcription of the loop of csrc/mateig.hip: its sweep count sets the kernel's cap."""
import numpy as np

import welch_matrix_oracle as XO

TOL = 2.0 ** -104      # off-diagonal norm squared against the diagonal norm squared: where a thread leaves the sweep loop


def fix_phase(v):
    """v [..., C]: rotated so that component 0 is real and >= 0 (imaginary part exactly 0); left alone where it is exactly 0"""
    v = np.array(v, np.complex128)
    z = np.abs(v[..., 0])
    ok = z != 0
    u = np.ones(z.shape, np.complex128)
    u[ok] = np.conj(v[..., 0][ok]) / z[ok]
    v = v * u[..., None]
    v[..., 0][ok] = z[ok]
    return v


def decompose(A):
    """A [m, C, C] Hermitian -> (eigenvalues [m, C] descending and clamped at 0, unit vector of the largest [m, C])"""
    A = np.asarray(A, np.complex128)
    w, V = np.linalg.eigh(A)
    lam = np.maximum(w[:, ::-1], 0.0)
    silent = (~A.any(axis=2)).sum(axis=1)      # zero rows: as many eigenvalues - the smallest, S is positive - are exactly 0
    for k in range(A.shape[1]):
        lam[silent > k, A.shape[1] - 1 - k] = 0.0
    vec = fix_phase(V[:, :, -1])
    diagonal = ~(A * (1.0 - np.eye(A.shape[1]))[None]).any(axis=(1, 2))
    equal = diagonal & np.all(np.einsum('jaa->ja', A) == A[:, :1, 0], axis=1)      # 0 and the identity: the lowest index
    vec[equal] = 0.0
    vec[equal, 0] = 1.0
    return lam, vec


def matrices(ref, of):
    """the matrix the library decomposes per bin, [nfft, C, C], from welch_matrix_oracle.matrix's dict, and the bins that read NaN"""
    T = ref['T']
    C = T.shape[0]
    d = np.einsum('aaj->aj', T).real
    with np.errstate(all='ignore'):
        bad = (~np.isfinite(d)).any(axis=0)
        empty = (~bad[None, :] & (d <= 0.0)).any(axis=0)
        if of == 'S':
            A = np.moveaxis(ref['S'], 2, 0).copy()
        else:
            A = np.moveaxis(T / np.sqrt(d[:, None, :] * d[None, :, :]), 2, 0).copy()
            A[:, np.arange(C), np.arange(C)] = 1.0
            A[empty] = np.eye(C)
    A[bad] = 0.0
    return A, bad


def eig(x, nfft, nperseg=None, noverlap=0, window='hann', detrend=True, scaling='density', fs=1.0, of='S', ref=None):
    """-> dict: eig [C, nfft] float64 (natural bin order, rows descending), vec [C, nfft] complex, A [nfft, C, C] the matrix
    decomposed, M, ref (welch_matrix_oracle.matrix's dict)"""
    ref = XO.matrix(x, nfft, nperseg, noverlap, window, detrend, scaling, fs) if ref is None else ref
    A, bad = matrices(ref, of)
    lam, vec = decompose(A)
    lam[bad] = np.nan
    vec[bad] = np.nan + 1j * np.nan
    return {'eig': lam.T.copy(), 'vec': vec.T.copy(), 'A': A, 'M': ref['M'], 'ref': ref, 'bad': bad}


def jacobi_emulation(A, cap):
    """csrc/mateig.hip's loop in float64 on a batch A [B, C, C] (or one matrix [C, C]): row-cyclic sweeps over p < q with
    Rutishauser's rotation, a rotation skipped where |a_pq| is exactly 0, a matrix leaving the loop in front of the sweep at
    which 2 sum_{p<q} |a_pq|^2 <= 2^-104 sum_p a_pp^2, `cap` sweeps at most.
    -> (eigenvalues [B, C] descending and clamped, vector of the largest [B, C], sweeps used [B])"""
    A = np.array(A, np.complex128)
    single = A.ndim == 2
    A = A[None] if single else A
    B, C, _ = A.shape
    V = np.tile(np.eye(C, dtype=np.complex128), (B, 1, 1))
    sweeps = np.zeros(B, int)
    live = np.ones(B, bool)
    iu = np.triu_indices(C, 1)
    with np.errstate(all='ignore'):
        for _ in range(cap):
            d = np.einsum('baa->ba', A).real
            off = (A[:, iu[0], iu[1]].real ** 2 + A[:, iu[0], iu[1]].imag ** 2).sum(axis=1)
            live &= ~(2.0 * off <= TOL * (d * d).sum(axis=1))
            if not live.any():
                break
            sweeps[live] += 1
            for p in range(C - 1):
                for q in range(p + 1, C):
                    x, y = A[:, p, q].real, A[:, p, q].imag
                    g = np.sqrt(x * x + y * y)
                    act = live & (g != 0.0)
                    if not act.any():
                        continue
                    a = A[act]
                    ga = g[act]
                    app, aqq = a[:, p, p].real.copy(), a[:, q, q].real.copy()
                    tau = (aqq - app) / (2.0 * ga)
                    t = np.copysign(1.0, tau) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    se = (t * cs) * (a[:, p, q] / ga)      # s e^(i phi)
                    kp, kq = a[:, :, p].copy(), a[:, :, q].copy()
                    a[:, :, p] = cs[:, None] * kp - np.conj(se)[:, None] * kq
                    a[:, :, q] = se[:, None] * kp + cs[:, None] * kq
                    a[:, p, :] = np.conj(a[:, :, p])
                    a[:, q, :] = np.conj(a[:, :, q])
                    a[:, p, p] = app - t * ga
                    a[:, q, q] = aqq + t * ga
                    a[:, p, q] = a[:, q, p] = 0.0
                    A[act] = a
                    v = V[act]
                    kp, kq = v[:, :, p].copy(), v[:, :, q].copy()
                    v[:, :, p] = cs[:, None] * kp - np.conj(se)[:, None] * kq
                    v[:, :, q] = se[:, None] * kp + cs[:, None] * kq
                    V[act] = v
    d = np.einsum('baa->ba', A).real
    order = np.argsort(-d, axis=1, kind='stable')      # ties: the lower Jacobi index first
    lam = np.maximum(np.take_along_axis(d, order, axis=1), 0.0)
    vec = fix_phase(V[np.arange(B), :, order[:, 0]])
    return (lam[0], vec[0], sweeps[0]) if single else (lam, vec, sweeps)
