"""float64 oracle of the two-channel path (scipy.signal.csd / coherence / welch, two-sided): Pxx, Pyy, Pxy = mean over
segments of conj(X) Y, and Cxy = |Pxy|^2 / (Pxx Pyy), with every scaling a plan accepts - built from oracle.ref_cpu's
segmentation and windows and median_oracle's scale factor and output stage."""
import numpy as np

import median_oracle as M
from oracle import ref_cpu as R


def csd_sums(x, y, window='hann', nperseg=256, noverlap=None, nfft=None, detrend='constant'):
    """-> (sxx, syy, sxy, nseg): the unscaled sums over segments of |X|^2, |Y|^2 and conj(X) Y, natural bin order - what
    oth_csd_partial_dev leaves (its third row interleaves re, im)."""
    x = np.asarray(x).astype(np.complex128)
    y = np.asarray(y).astype(np.complex128)
    noverlap = nperseg // 2 if noverlap is None else noverlap
    nfft = nperseg if nfft is None else nfft
    win = R.get_window(window, nperseg) if isinstance(window, str) else np.asarray(window, np.float64)
    xs, ys = R._segments(x, nperseg, noverlap), R._segments(y, nperseg, noverlap)
    if detrend == 'constant':
        xs = xs - xs.mean(axis=1, keepdims=True)
        ys = ys - ys.mean(axis=1, keepdims=True)
    X = np.fft.fft(xs * win, nfft, axis=1)
    Y = np.fft.fft(ys * win, nfft, axis=1)
    sxx = (X.real * X.real + X.imag * X.imag).sum(axis=0)
    syy = (Y.real * Y.real + Y.imag * Y.imag).sum(axis=0)
    return sxx, syy, (np.conj(X) * Y).sum(axis=0), xs.shape[0]


def csd(x, y, fs=1.0, window='hann', nperseg=256, noverlap=None, nfft=None, detrend='constant', scaling='density'):
    """-> float64 pxx, pyy, complex128 pxy, float64 cxy, each [nfft] in natural bin order."""
    nfft = nperseg if nfft is None else nfft
    win = R.get_window(window, nperseg) if isinstance(window, str) else np.asarray(window, np.float64)
    sxx, syy, sxy, nseg = csd_sums(x, y, win, nperseg, noverlap, nfft, detrend)
    k = M.plan_scale(win, scaling, fs, nfft) / nseg
    pxx, pyy, pxy = sxx * k, syy * k, sxy * k
    with np.errstate(invalid='ignore', divide='ignore'):
        cxy = (pxy.real * pxy.real + pxy.imag * pxy.imag) / (pxx * pyy)
    return pxx, pyy, pxy, cxy


def shift_trim(rows, fftshift=False, trim=0):
    """The plan's output stage (median_oracle.shift_trim_db without the dB step)."""
    return M.shift_trim_db(rows, fftshift, trim, False)
