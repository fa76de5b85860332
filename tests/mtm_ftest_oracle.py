"""float64 oracle of Thomson's harmonic F-test (oth_mtm_ftest, csrc/mtmftest.hip) by the DEFINITION: per segment and bin the
eigencoefficients y_k = FFT((x_s - m_s) v_k, nfft), the line amplitude mu = sum_k U_k y_k / S, and the residual as the
explicit sum_k |y_k - mu U_k|^2 - not the subtracted form sum_k |y_k|^2 - S |mu|^2 the kernel uses.  Tapers from
mtm_oracle.tapers_and_weights (the weights are not used: the test is unweighted)."""
import numpy as np

import mtm_oracle as O
from oracle import ref_cpu as R

SCALE = {'density': lambda fs, nfft: 1.0 / fs, 'raw': lambda fs, nfft: 1.0, 'over_n2': lambda fs, nfft: 1.0 / (float(nfft) ** 2)}


def eigencoefficients(x, nfft, nperseg, noverlap, tapers, detrend=True):
    """-> complex128 [nseg, K, nfft], natural bin order"""
    xs = R._segments(np.asarray(x).astype(np.complex128), nperseg, noverlap)
    if detrend:
        xs = xs - xs.mean(axis=1, keepdims=True)
    return np.fft.fft(xs[:, None, :] * np.asarray(tapers, np.float64)[None, :, :], nfft, axis=2)


def ftest(x, nfft, nperseg=None, noverlap=0, nw=4.0, K=None, detrend=True, scaling='density', fs=1.0, tapers=None,
          subtracted=False):
    """One stream.  -> dict(num, den, F, line, resid, nseg, S): float64 [nfft] rows in natural bin order; num and den are
    the sums over the segments.  subtracted=True: den as sum_k |y_k|^2 - num (the kernel's form) instead of the definition."""
    nperseg = nfft if nperseg is None else nperseg
    K = int(2 * nw) - 1 if K is None else K
    if tapers is None:
        tapers, _ = O.tapers_and_weights(nperseg, nw, K)
    tapers = np.asarray(tapers, np.float64)
    K = len(tapers)
    U = tapers.sum(axis=1)
    S = float(np.sum(U * U))
    y = eigencoefficients(x, nfft, nperseg, noverlap, tapers, detrend)
    nseg = y.shape[0]
    mu = np.einsum('k,skj->sj', U, y) / S
    num_s = S * np.abs(mu) ** 2
    if subtracted:
        den_s = np.sum(np.abs(y) ** 2, axis=1) - num_s
    else:
        den_s = np.sum(np.abs(y - mu[:, None, :] * U[None, :, None]) ** 2, axis=1)
    num, den = num_s.sum(axis=0), den_s.sum(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        F = np.where(den > 0.0, (K - 1) * num / den, np.where(num > 0.0, np.inf, 0.0))
    return dict(num=num, den=den, F=F, line=num / (S * nseg), resid=SCALE[scaling](fs, nfft) * den / ((K - 1) * nseg),
                nseg=nseg, S=S, K=K)


def ftest_streams(x, nstreams, **kw):
    """x: nstreams equal captures back to back -> list of ftest() results"""
    n = len(x) // nstreams
    return [ftest(x[s * n:(s + 1) * n], **kw) for s in range(nstreams)]


def hump_capture(seed, n=1024):
    """The case the feature exists for: unit-variance complex noise shaped by 1 + 9 exp(-((k - 200) / 60)^2 / 2) in the
    frequency domain - a broadband signal 20 dB over the floor around bin 200 - with a line of amplitude 4.0 at bin 200, on
    the hump, and one of amplitude 0.5 at bin -300.  -> complex64 [n]"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    k = np.arange(n)
    k = np.where(k >= n // 2, k - n, k)
    shape = 1.0 + 9.0 * np.exp(-0.5 * ((k - 200) / 60.0) ** 2)
    x = np.fft.ifft(np.fft.fft(w) * shape)
    t = np.arange(n)
    x = x + 4.0 * np.exp(2j * np.pi * 200 * t / n) + 0.5 * np.exp(-2j * np.pi * 300 * t / n)
    return x.astype(np.complex64)


HUMP_LINES = (200, -300)      # bins of hump_capture's lines
