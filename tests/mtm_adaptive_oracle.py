"""float64 oracle of Thomson's adaptive-weight multitaper PSD (oth_mtm_adaptive, csrc/mtmadapt.hip) by the DEFINITION of
include/ofdm_tools_hip.h: per segment the eigenspectra P_k = |FFT((x_s - m_s) v_k, nfft)|^2 / g_k on
mtm_ftest_oracle.eigencoefficients (median_oracle's segmentation), sigma^2, S^0 = (P_0 + P_1) / 2, `iters` updates with
b_k = S / (lambda_k S + (1 - lambda_k) sigma^2), w_k = lambda_k b_k^2, and nu = 2 (sum w)^2 / sum w^2 from the final S.  The
tapers are the plan's: ofdm_tools.windows.dpss rounded to float32 (g_k is their energy), the ratios dpss's, in double.

emulate32 is the same estimate as the kernel forms it - pilot and residual mean in float32, complex64 pocketfft, float32
arithmetic in the kernel's order - and sets the GPU gate.  A float32 transform leaves an absolute error of the size of the
spectrum's rms in every bin, so a deep bin's relative error grows like sqrt(Pbar / S); with Pbar the mean of P_k over
segments, tapers and bins, and S, nu the means over the segments (what the call returns), parity is asked as
    |S - S_ref|   <= 1e-4 S_ref + G_S sqrt(S_ref Pbar)
    |nu - nu_ref| <= G_NU nu_ref (1 + sqrt(Pbar / S_ref))
in every bin, none excluded.  The gates are 3 x the emulation's worst over the parity cases of tests/test_mtm_adaptive_gpu.py
(PARITY_CASES and EXTRA_CASES below, each at 1 and 4 iterations, the band capture at D = 40): the GPU's Stockham transform sums in another
order than pocketfft.  The emulation is measured with a relative part of 1e-5 instead of 1e-4.  Measured (this file's
measure(), tests/test_mtm_adaptive_cpu.py::test_float32_emulation_sets_the_gpu_gate prints it): worst G_S 2.21e-6
((16384, 16384, 0, 1, 4, 7) at 4 iterations; 1.5e-7 at 64 points, 5.8e-7 at 1024, 2.4e-7 at 4096, 1.27e-6 at 8192), worst
G_NU 5.02e-7 ((4096, 4096, 50, 9, 2.5, 4) at 4 iterations; 6.1e-8 at 64 points, 1.0e-7 ... 2.5e-7 elsewhere)."""
import numpy as np

import mtm_ftest_oracle as FO
import mtm_oracle as O
from oracle import ref_cpu as R

G_S = 6.7e-6       # 3 x 2.21e-6
G_NU = 1.51e-6     # 3 x 5.02e-7
REL_S = 1e-4       # the relative part of the S bound
REL_EMU = 1e-5     # ... with which the emulation is measured

PARITY_CASES = [  # nfft, nperseg, overlap %, segments, NW, K, scaling, fftshift, trim, offset
    (64, 64, 0, 5, 2, 3, 'density', False, 0, 0.0),
    (512, 512, 50, 3, 2.5, 4, 'raw', True, 0, 0.0),
    (1024, 1024, 0, 1, 4, 7, 'density', False, 0, 0.0),
    (4096, 4096, 50, 9, 2.5, 4, 'over_n2', False, 0, 0.0),
    (4096, 1000, 0, 3, 3, 5, 'density', True, 100, 0.0),          # zero-padded
    (8192, 8192, 0, 1, 4, 7, 'density', False, 0, 0.0),
    (16384, 16384, 0, 1, 4, 7, 'raw', False, 0, 0.0),
    (16384, 16384, 50, 3, 8, 15, 'density', True, 0, 0.0),
    (256, 200, 0, 3, 2.5, 4, 'density', False, 0, 35.0),          # an offset of 35
]
PARITY_ITERS = (1, 4)
EXTRA_CASES = [(512, 512, 0, 2, 24, 40, 'density', False, 0, 0.0)]      # 40 rows of eigenspectra: 80 KiB of LDS
BAND = (0.1, 0.06)      # centre and half-width of the band capture's occupied band, cycles per sample


_tapers = {}


def plan_tapers(nperseg, nw, K):
    """-> (tapers as the plan holds them: float32 values in float64 [K, nperseg], ratios float64 [K]); computed once"""
    from ofdm_tools import windows
    key = (int(nperseg), float(nw), int(K))
    if key not in _tapers:
        tapers, ratios = windows.dpss(nperseg, nw, K, return_ratios=True)
        _tapers[key] = (np.asarray(tapers, np.float32).astype(np.float64), np.asarray(ratios, np.float64))
        for a in _tapers[key]:
            a.setflags(write=False)
    return _tapers[key]


def on_off_tones(nfft):
    """one tone on a bin of the transform, one between bins (test_mtm_ftest_gpu.on_off_tones' frequencies), amplitude 0.3"""
    return ((0.3, round(0.123 * nfft) / float(nfft)), (0.3, -0.31))


def band_capture(n, seed, D=40.0, nfft=None, offset=0.0):
    """The band capture: a band-limited complex Gaussian of unit power on |f - 0.1| <= 0.06 (white noise through a brick
    wall on a grid of 4 n points, n samples from its middle: not periodic in the capture), a white floor D dB below it,
    with nfft given the two tones of on_off_tones(nfft), and an offset.  -> complex64 [n]"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(4 * n) + 1j * rng.standard_normal(4 * n)
    f = np.fft.fftfreq(4 * n)
    sig = np.fft.ifft(np.fft.fft(w) * (np.abs(f - BAND[0]) <= BAND[1]))[n:2 * n]
    sig = sig / np.sqrt(np.mean(np.abs(sig) ** 2))
    floor = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5 * 10.0 ** (-D / 10.0))
    x = sig + floor
    if nfft is not None:
        t = np.arange(n)
        for a, fr in on_off_tones(nfft):
            x = x + a * np.exp(2j * np.pi * fr * t)
    return (x + offset).astype(np.complex64)


def outside_band(nfft, nw):
    """natural-order mask of the bins more than 2 NW bins outside the occupied band"""
    f = np.fft.fftfreq(nfft)
    return np.abs(f - BAND[0]) > BAND[1] + 2.0 * nw / nfft


def parity_capture(case, seed=None):
    """-> (x, noverlap) of one PARITY_CASES row: the band capture at D = 40 with the tones and the row's offset"""
    nfft, nperseg, ov, nseg, nw, K, scaling, fftshift, trim, offset = case
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    seed = 7 * nfft + ov + K if seed is None else seed
    return band_capture(noverlap + nseg * step + step // 3, seed, 40.0, nfft, offset), noverlap


def iterate(P, sigma2, lam, iters, dtype=np.float64):
    """P [nseg, K, nfft], sigma2 [nseg], lam [K] (or a pair (lambda, 1 - lambda)) -> (S, nu) [nseg, nfft] by the definition,
    in `dtype` arithmetic with the sums over k taken in order (the kernel's)."""
    if isinstance(lam, tuple):
        l, oml = (np.asarray(v, dtype) for v in lam)
    else:
        l = np.asarray(lam, np.float64)
        l, oml = l.astype(dtype), np.maximum(1.0 - l, 0.0).astype(dtype)
    P = np.asarray(P, dtype)
    sig = np.asarray(sigma2, dtype)[:, None]
    K = P.shape[1]
    zero = np.zeros_like(P[:, 0])

    def sums(S):
        num, den, den2 = zero.copy(), zero.copy(), zero.copy()
        for k in range(K):
            d = l[k] * S + oml[k] * sig
            with np.errstate(divide='ignore', invalid='ignore'):
                b = np.where(d > 0, S / d, 0).astype(dtype)
            w = l[k] * b * b
            num, den, den2 = num + w * P[:, k], den + w, den2 + w * w
        return num, den, den2

    S = (dtype(0.5) * (P[:, 0] + P[:, 1])).astype(dtype)
    for _ in range(iters):
        num, den, _ = sums(S)
        with np.errstate(divide='ignore', invalid='ignore'):
            S = np.where(den > 0, num / den, 0).astype(dtype)
    _, den, den2 = sums(S)
    ok = (den > 0) & (den2 > 0) & (sig > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        nu = np.where(ok, dtype(2.0) * den * den / den2, 0).astype(dtype)
    return np.where(ok, S, 0).astype(dtype), nu


def adaptive(x, nfft, nperseg=None, noverlap=0, nw=4.0, K=None, iters=4, detrend=True, scaling='density', fs=1.0, tapers=None,
             ratios=None):
    """One stream.  -> dict: S, nu [nseg, nfft], P [nseg, K, nfft], sigma2 [nseg] per segment; psd, dof [nfft] (the call's
    rows before shift, trim and dB); Sm = mean_s S_s; Pbar; nseg.  float64, natural bin order."""
    nperseg = nfft if nperseg is None else nperseg
    K = int(2 * nw) - 1 if K is None else K
    if tapers is None:
        tapers, ratios = plan_tapers(nperseg, nw, K)
    tapers = np.asarray(tapers, np.float64)
    g = np.sum(tapers * tapers, axis=1)
    y = FO.eigencoefficients(x, nfft, nperseg, noverlap, tapers, detrend)
    P = np.abs(y) ** 2 / g[None, :, None]
    xs = R._segments(np.asarray(x).astype(np.complex128), nperseg, noverlap)
    if detrend:
        xs = xs - xs.mean(axis=1, keepdims=True)
    sigma2 = np.mean(np.abs(xs) ** 2, axis=1)
    S, nu = iterate(P, sigma2, ratios, iters)
    Sm = S.mean(axis=0)
    return dict(S=S, nu=nu, P=P, sigma2=sigma2, Sm=Sm, psd=FO.SCALE[scaling](fs, nfft) * Sm, dof=nu.mean(axis=0), Pbar=float(P.mean()),
                nseg=S.shape[0])


def adaptive_streams(x, nstreams, **kw):
    """x: nstreams equal captures back to back -> list of adaptive() results"""
    n = len(x) // nstreams
    return [adaptive(x[s * n:(s + 1) * n], **kw) for s in range(nstreams)]


def unity_psd(x, nfft, nw=4.0, K=None, fs=1.0):
    """the fixed-weight ('unity') estimate of one full-length segment plan, float64 [nfft]"""
    return O.mtm_psd(x, nfft, nfft, 0, nw, K, fs=fs)


def emulate32(x, nfft, nperseg=None, noverlap=0, nw=4.0, K=None, iters=4, detrend=True):
    """The estimate as mtm_adapt_kernel forms it, on the CPU: the pilot (mean of the segment's first 64 samples) and the
    residual mean come off in float32, the taper product, a complex64 transform (pocketfft), P_k, sigma^2 and the iteration
    in float32.  -> (Sm, dof) float64 [nfft]: the means over the segments (summed in double, as the finalize kernel does)."""
    from scipy import fft as sfft
    nperseg = nfft if nperseg is None else nperseg
    K = int(2 * nw) - 1 if K is None else K
    tapers, ratios = plan_tapers(nperseg, nw, K)
    t32 = tapers.astype(np.float32)
    inv_g = (1.0 / np.sum(tapers * tapers, axis=1)).astype(np.float32)
    lam = (ratios.astype(np.float32), np.maximum(1.0 - ratios, 0.0).astype(np.float32))
    xs = R._segments(np.asarray(x, np.complex64), nperseg, noverlap).astype(np.complex64)
    if detrend:
        npil = min(64, nperseg)
        pil = (xs[:, :npil].sum(axis=1, dtype=np.complex64) * np.float32(1.0 / npil)).astype(np.complex64)
        xs = xs - pil[:, None]
        mean = (xs.sum(axis=1, dtype=np.complex64) * np.float32(1.0 / nperseg)).astype(np.complex64)
        xs = (xs - mean[:, None]).astype(np.complex64)
    sigma2 = ((xs.real * xs.real).sum(axis=1, dtype=np.float32) + (xs.imag * xs.imag).sum(axis=1, dtype=np.float32)) * np.float32(1.0 / nperseg)
    y = sfft.fft((xs[:, None, :] * t32[None, :, :]).astype(np.complex64), nfft, axis=2)
    assert y.dtype == np.complex64
    P = ((y.real * y.real + y.imag * y.imag) * inv_g[None, :, None]).astype(np.float32)
    S, nu = iterate(P, sigma2.astype(np.float32), lam, iters, np.float32)
    assert S.dtype == np.float32 and nu.dtype == np.float32
    return S.astype(np.float64).mean(axis=0), nu.astype(np.float64).mean(axis=0)


def gate_shares(Sm, dof, ref, rel=REL_S):
    """Sm, dof: the rows under test, natural order, unscaled; ref: adaptive()'s dict.  -> (g_s, g_nu) [nfft]: per bin
    (|dS| - rel S_ref) / sqrt(S_ref Pbar), not below 0, and |d nu| / (nu_ref (1 + sqrt(Pbar / S_ref))) - to be held against
    G_S and G_NU."""
    Sr, nr, Pbar = ref['Sm'], ref['dof'], ref['Pbar']
    g_s = np.maximum(np.abs(Sm - Sr) - rel * Sr, 0.0) / np.sqrt(Sr * Pbar)
    g_nu = np.abs(dof - nr) / (nr * (1.0 + np.sqrt(Pbar / Sr)))
    return g_s, g_nu


def measure(cases=PARITY_CASES + EXTRA_CASES, iters=PARITY_ITERS):
    """The emulation's worst shares over the parity cases -> (worst g_s, its case, worst g_nu, its case), printed per case"""
    best = [0.0, None, 0.0, None]
    for case in cases:
        nfft, nperseg, ov, nseg, nw, K = case[:6]
        x, noverlap = parity_capture(case)
        for it in iters:
            ref = adaptive(x, nfft, nperseg, noverlap, nw, K, it)
            g_s, g_nu = gate_shares(*emulate32(x, nfft, nperseg, noverlap, nw, K, it), ref, rel=REL_EMU)
            print('adaptive emulation %s iters %d: G_S %.2e G_NU %.2e' % (case[:6], it, g_s.max(), g_nu.max()))
            if g_s.max() > best[0]:
                best[0:2] = [float(g_s.max()), case[:6] + (it,)]
            if g_nu.max() > best[2]:
                best[2:4] = [float(g_nu.max()), case[:6] + (it,)]
    return tuple(best)


if __name__ == '__main__':
    print(measure())
