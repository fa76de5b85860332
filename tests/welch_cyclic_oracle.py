"""float64 oracle of the cyclic spectrum and cyclic coherence of a Welch plan (the time-smoothed cyclic cross periodogram),
by the definition: per segment s and cycle frequency alpha (cycles per sample), with m_s the segment mean when the plan
detrends,
  X_s = FFT_nfft((x_s - m_s) w),   U_s = FFT_nfft((x_s - m_s) w e^{-j 2 pi alpha (n + s step)}),
  Sxx = sum_s |X_s|^2,  Suu = sum_s |U_s|^2,  Sux = sum_s U_s conj(X_s),
  scf = scale Sux / M,  coh = |Sux|^2 / (Suu Sxx),  psd = scale Sxx / M;  a bin with Suu Sxx <= 0 reads scf = coh = 0."""
import numpy as np

import median_oracle as MO
from oracle import ref_cpu as R


def cyclic(x, nfft, alphas, nperseg=None, noverlap=0, window='hann', detrend=True, scaling='density', fs=1.0):
    """-> dict: M, Sxx [nfft], Suu [A, nfft], Sux [A, nfft] complex, scf, coh, psd - natural bin order, linear."""
    nperseg = nfft if nperseg is None else nperseg
    step = nperseg - noverlap
    x = np.asarray(x).astype(np.complex128)
    win = R.get_window(window, nperseg) if isinstance(window, str) else np.asarray(window, np.float64)
    xs = R._segments(x, nperseg, noverlap)
    M = xs.shape[0]
    if detrend:
        xs = xs - xs.mean(axis=1, keepdims=True)
    xw = xs * win
    X = np.fft.fft(xw, nfft, axis=1)
    Sxx = (X.real * X.real + X.imag * X.imag).sum(axis=0)
    alphas = np.atleast_1d(np.asarray(alphas, np.float64))
    n = np.arange(nperseg, dtype=np.float64)[None, :] + (np.arange(M, dtype=np.float64) * step)[:, None]
    Suu, Sux = np.empty((len(alphas), nfft)), np.empty((len(alphas), nfft), np.complex128)
    for a, alpha in enumerate(alphas):
        turns = alpha * n                      # exact products up to 2^53: the fraction keeps 1e-9 at 2^24 samples
        U = np.fft.fft(xw * np.exp(-2j * np.pi * (turns - np.rint(turns))), nfft, axis=1)
        Suu[a] = (U.real * U.real + U.imag * U.imag).sum(axis=0)
        Sux[a] = (U * np.conj(X)).sum(axis=0)
    scale = MO.plan_scale(win, scaling, fs, nfft)
    den = Suu * Sxx[None, :]
    live = den > 0.0
    coh = np.where(live, np.abs(Sux) ** 2 / np.where(live, den, 1.0), 0.0)
    scf = np.where(live, Sux * scale / M, 0.0)
    return {'M': M, 'Sxx': Sxx, 'Suu': Suu, 'Sux': Sux, 'scf': scf, 'coh': coh, 'psd': Sxx * scale / M, 'scale': scale}


def profile(x, nfft, alphas, **kw):
    """mean over bins of each coherence row"""
    return cyclic(x, nfft, alphas, **kw)['coh'].mean(axis=1)

