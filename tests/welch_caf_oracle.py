"""float64 oracle of the cyclic autocorrelation of a Welch plan (the plan's PSD of the lag product), by the definition: with
T the largest lag, M the plan's segment count for an input of len(x) - T samples, per segment s and lag tau,
  z_s[n] = x[s step + n + tau] conj(x[s step + n]),  n < nperseg,     mbar_s = mean_n z_s[n],
  Z_s = FFT_nfft((z_s - m) w),  m = mbar_s when the plan detrends, else 0,
  caf = scale sum_s |Z_s|^2 / M,   r = sum_s mbar_s / M."""
import numpy as np

import median_oracle as MO
from oracle import ref_cpu as R


def nseg(nsamples, lags, nperseg, noverlap=0):
    """the segment count: the plan's, on nsamples - max(lags) samples"""
    return (nsamples - int(max(lags)) - noverlap) // (nperseg - noverlap)


def products(x, tau, nperseg, noverlap, M):
    """-> complex128 [M, nperseg]: the lag products of the M segments"""
    x = np.asarray(x).astype(np.complex128)
    need = (M - 1) * (nperseg - noverlap) + nperseg
    z = x[tau:tau + need] * np.conj(x[:need])
    return R._segments(z, nperseg, noverlap)[:M]


def caf(x, nfft, lags, nperseg=None, noverlap=0, window='hann', detrend=True, scaling='density', fs=1.0):
    """-> dict: M, caf [L, nfft] (natural bin order, linear), r [L] complex, zabs [L] (mean |z|), scale."""
    nperseg = nfft if nperseg is None else nperseg
    lags = [int(t) for t in lags]
    M = nseg(len(x), lags, nperseg, noverlap)
    assert M >= 1
    win = R.get_window(window, nperseg) if isinstance(window, str) else np.asarray(window, np.float64)
    scale = MO.plan_scale(win, scaling, fs, nfft)
    rows, r, zabs = np.empty((len(lags), nfft)), np.empty(len(lags), np.complex128), np.empty(len(lags))
    for i, tau in enumerate(lags):
        zs = products(x, tau, nperseg, noverlap, M)
        assert zs.shape == (M, nperseg)
        mbar = zs.mean(axis=1, keepdims=True)
        r[i] = mbar.mean()
        zabs[i] = np.abs(zs).mean()
        Z = np.fft.fft((zs - mbar if detrend else zs) * win, nfft, axis=1)
        rows[i] = (Z.real * Z.real + Z.imag * Z.imag).sum(axis=0) * scale / M
    return {'M': M, 'caf': rows, 'r': r, 'zabs': zabs, 'scale': scale}
