"""float64 oracle of the multitaper (Thomson) PSD plans: per taper median_oracle.welch_rows with window = v_k, the mean
over the segments' rows, the weighted sum over tapers - tapers and concentration ratios from ofdm_tools.windows.dpss
(checked against scipy.signal.windows.dpss in tests/test_mtm_cpu.py)."""
import math

import numpy as np

import median_oracle as M
from oracle import ref_cpu as R


def tapers_and_weights(nperseg, nw, K, weights='unity'):
    """-> (float64 tapers [K, nperseg], weights a_k normalised to sum 1)"""
    from ofdm_tools import windows
    tapers, ratios = windows.dpss(nperseg, nw, K, return_ratios=True)
    if isinstance(weights, str):
        a = np.ones(K) if weights == 'unity' else np.asarray(ratios, np.float64)
    else:
        a = np.asarray(weights, np.float64)
    return tapers, a / a.sum()


def mtm_psd(x, nfft, nperseg=None, noverlap=0, nw=4.0, K=None, weights='unity', detrend=True, scaling='density', fs=1.0,
            tapers=None):
    """-> float64 [nfft], natural bin order: mean over segments of sum_k c_k |FFT((x_s - m_s) v_k, nfft)|^2 with
    c_k = a_k / sum(v_k^2) / fs ('density'), a_k ('raw'), a_k / nfft^2 ('over_n2') - welch_rows' own scalings."""
    nperseg = nfft if nperseg is None else nperseg
    K = int(2 * nw) - 1 if K is None else K
    if tapers is None:
        tapers, a = tapers_and_weights(nperseg, nw, K, weights)
    else:
        tapers = np.asarray(tapers, np.float64)
        a = np.ones(len(tapers)) if isinstance(weights, str) else np.asarray(weights, np.float64)
        a = a / a.sum()
    out = np.zeros(nfft)
    for v, ak in zip(tapers, a):
        rows = M.welch_rows(x, fs, v, nperseg, noverlap, nfft, 'constant' if detrend else False, scaling)
        out += ak * rows.mean(axis=0)
    return out


def scan_psd(vector, nFFT, Sf, NW=4.0, K=None):
    """The helpers' estimate: nperseg = min(nFFT, len), one pass without overlap, density, fftshift."""
    nperseg = min(int(nFFT), len(vector))
    return np.fft.fftshift(mtm_psd(vector, nFFT, nperseg, 0, NW, K, fs=float(Sf)))


def src_power_mtm(vector, npts, nFFT, Fr, Sf, bb_freqs, srch_bins, NW=4.0, K=None):
    psd = scan_psd(vector, nFFT, Sf, NW, K)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf))
    return psd, axis, R._channel_sums(psd, Fr, Sf, bb_freqs, srch_bins)


def fast_spectrum_scan_mtm(vct_sample, fc, channel_rate, srch_bw, n_fft, samp_rate, thr_leveler, noise_estimate, alpha_avg):
    """oracle.ref_cpu.fast_spectrum_scan with the multitaper estimate (NW 4, K 7) as the PSD."""
    npts = len(vct_sample)
    nFFT = int(2 ** math.ceil(math.log(npts, 2))) if n_fft == 0 else n_fft
    Fr = float(samp_rate) / float(nFFT)
    half = R._py2div(samp_rate, 2)
    bb_freqs = R.frange(R._py2div(-samp_rate, 2), half, channel_rate)
    psd, axis, plc = src_power_mtm(vct_sample, npts, nFFT, Fr, samp_rate, bb_freqs, srch_bw / Fr, 4.0, 7)
    ax_ch = R.frange(fc - half, fc + half, channel_rate)
    noise_estimate = (1 - alpha_avg) * noise_estimate + alpha_avg * np.amin(plc)
    thr = noise_estimate * thr_leveler
    return thr, plc, noise_estimate, [ax_ch[i] for i, item in enumerate(plc) if item > thr]
