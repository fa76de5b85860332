"""float64 oracles of the cyclic-prefix synchroniser (oth_cp_sync, include/ofdm_tools_hip.h), computed from the complex64 input:
    S = (nsamples - Tu) // Ts,  z[n] = x[n + Tu] conj(x[n]),  e[n] = (|x[n]|^2 + |x[n + Tu]|^2) / 2
    F[r] = sum_s z[r + s Ts],  G[r] = sum_s e[r + s Ts],  Gamma[t] = sum_{j < cp} F[(t + j) mod Ts],  Phi likewise from G
    Lambda = |Gamma| - rho Phi,  theta = the lowest argmax,  eps = arg Gamma[theta] / 2 pi,  rho_hat = |Gamma[theta]| / Phi[theta]
definition(): the direct sums over s and j.  fold(): F / G and then the circular window, which is what the GPU tests compare
against (tests/test_cp_sync_cpu.py holds the two together at 1e-12 of A).  A[t] is Gamma's sum with |z| in place of z: the size
every rounding of Gamma is relative to.  cp_ofdm_sync() makes the CP-OFDM captures of the estimator tests."""
import numpy as np


def nsym(nsamples, tu, cp):
    return (int(nsamples) - int(tu)) // (int(tu) + int(cp)) if nsamples >= tu else 0


def products(x, tu, cp):
    """-> (z, e, |z|) of the S Ts samples the fold reads, each [S, Ts] float64 / complex128"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    ts, S = tu + cp, nsym(len(x), tu, cp)
    assert S >= 1
    base, lag = x[:S * ts], x[tu:tu + S * ts]
    z = lag * np.conj(base)
    e = 0.5 * (base.real ** 2 + base.imag ** 2 + lag.real ** 2 + lag.imag ** 2)
    return z.reshape(S, ts), e.reshape(S, ts), np.abs(z).reshape(S, ts)


def definition(x, tu, cp):
    """Gamma, Phi, A by the direct sums over s and j (small shapes: cp S vector operations) -> dict"""
    z, e, a = products(x, tu, cp)
    S, ts = z.shape
    t = np.arange(ts)
    gamma, phi, A = np.zeros(ts, np.complex128), np.zeros(ts), np.zeros(ts)
    for j in range(cp):
        r = (t + j) % ts
        for s in range(S):
            gamma += z[s, r]
            phi += e[s, r]
            A += a[s, r]
    return {'gamma': gamma, 'phi': phi, 'A': A, 'S': S}


def window(v, cp, direct=True):
    """the circular window sum_{j < cp} v[(t + j) mod Ts].  direct: every entry summed on its own (an entry is non-finite
    exactly where its window holds a non-finite value); else by differences of a running sum (finite input, large shapes:
    float64 leaves 1e-12 of the sum)"""
    ts = len(v)
    vv = np.concatenate([v, v[:cp - 1]]) if cp > 1 else v
    if direct:
        return np.lib.stride_tricks.sliding_window_view(vv, cp).sum(axis=1)
    c = np.concatenate([[0], np.cumsum(vv)])
    return c[cp:cp + ts] - c[:ts]


def fold(x, tu, cp, direct=None):
    """F / G / sum |z| over the symbols, then the circular window -> dict gamma, phi, A [Ts], F, G [Ts], S"""
    z, e, a = products(x, tu, cp)
    if direct is None:
        direct = (tu + cp) * cp <= (1 << 24)
    F, G, B = z.sum(axis=0), e.sum(axis=0), a.sum(axis=0)
    return {'gamma': window(F, cp, direct), 'phi': window(G, cp, direct), 'A': window(B, cp, direct), 'F': F, 'G': G, 'S': z.shape[0]}


def estimate(gamma, phi, rho):
    """-> (theta, eps, rho_hat, Lambda[theta], Lambda) of float64 rows"""
    lam = np.abs(gamma) - float(rho) * phi
    theta = int(np.argmax(lam))      # numpy's argmax is the lowest index of the maximum
    g, p = gamma[theta], phi[theta]
    return theta, float(np.angle(g) / (2.0 * np.pi)), float(abs(g) / p) if p != 0.0 else 0.0, float(lam[theta]), lam


def poisoned(n, nsamples, tu, cp):
    """the residues a non-finite sample n enters: n mod Ts as the base sample, (n - Tu) mod Ts as the lagged one - each only
    where the fold reads it in that role"""
    ts, S = tu + cp, nsym(nsamples, tu, cp)
    out = set()
    if n < S * ts:
        out.add(n % ts)
    if tu <= n < S * ts + tu:
        out.add((n - tu) % ts)
    return out


def covered(residues, tu, cp):
    """the entries t whose window t ... t + cp - 1 mod Ts holds one of `residues` -> bool [Ts]"""
    ts = tu + cp
    hit = np.zeros(ts, bool)
    for r in residues:
        hit[(r - np.arange(cp)) % ts] = True
    return hit


def cp_ofdm_sync(seed, tu, cp, symbols, snr_db, theta0, eps0, noise=True):
    """A CP-OFDM capture of `symbols` Ts + Tu samples (S = symbols): QPSK on every subcarrier, ifft, the prefix in front, cut so
    that the first sample of a prefix is sample theta0 (< Ts), a carrier offset of eps0 subcarrier spacings, and complex white
    noise `snr_db` below the signal's unit power -> complex64"""
    rng = np.random.default_rng([seed, tu, cp])
    ts = tu + cp
    n = symbols * ts + tu
    count = symbols + 3
    q = (rng.integers(0, 2, (count, tu)) * 2 - 1 + 1j * (rng.integers(0, 2, (count, tu)) * 2 - 1)) / np.sqrt(2.0)
    body = np.fft.ifft(q, axis=1) * np.sqrt(tu)
    sig = np.concatenate([body[:, tu - cp:], body], axis=1).reshape(-1)
    start = (ts - theta0) % ts
    x = sig[start:start + n] * np.exp(2j * np.pi * eps0 * np.arange(n) / tu)
    if noise:
        sigma = 10.0 ** (-snr_db / 20.0)
        x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    return x.astype(np.complex64)
