"""float64 oracle of the median average (scipy.signal.welch average='median', two-sided) and of the per-segment
periodogram rows it takes the median of - built from oracle.ref_cpu's segmentation and windows."""
import numpy as np

from oracle import ref_cpu as R


def median_bias(n):
    """scipy.signal._spectral_helper._median_bias: the median of n chi^2_2 / 2 variates over their mean."""
    ii_2 = 2.0 * np.arange(1.0, (n - 1) // 2 + 1)
    return 1.0 + np.sum(1.0 / (ii_2 + 1.0) - 1.0 / ii_2)


def plan_scale(win, scaling, fs=1.0, nfft=None):
    if scaling == 'density':
        return 1.0 / (fs * np.sum(win * win))
    if scaling == 'spectrum':
        return 1.0 / np.sum(win) ** 2
    if scaling == 'over_n2':
        return 1.0 / (float(nfft) * float(nfft))
    return 1.0      # 'raw'


def welch_rows(x, fs=1.0, window='hann', nperseg=256, noverlap=None, nfft=None, detrend='constant', scaling='density'):
    """-> float64 [nseg, nfft]: the scaled periodogram of every segment, natural bin order."""
    x = np.asarray(x).astype(np.complex128)
    noverlap = nperseg // 2 if noverlap is None else noverlap
    nfft = nperseg if nfft is None else nfft
    win = R.get_window(window, nperseg) if isinstance(window, str) else np.asarray(window, np.float64)
    xs = R._segments(x, nperseg, noverlap)
    if detrend == 'constant':
        xs = xs - xs.mean(axis=1, keepdims=True)
    X = np.fft.fft(xs * win, nfft, axis=1)
    return (X.real * X.real + X.imag * X.imag) * plan_scale(win, scaling, fs, nfft)


def welch_median(x, fs=1.0, window='hann', nperseg=256, noverlap=None, nfft=None, detrend='constant', scaling='density'):
    """-> float64 [nfft]: scipy.signal.welch(x, ..., average='median', return_onesided=False)[1]."""
    rows = welch_rows(x, fs, window, nperseg, noverlap, nfft, detrend, scaling)
    return np.median(rows, axis=0) / median_bias(rows.shape[0])


def shift_trim_db(rows, fftshift=False, trim=0, db=False):
    """The plan's output stage on float64 rows [..., nfft]."""
    rows = np.fft.fftshift(rows, axes=-1) if fftshift else rows
    if trim:
        rows = rows[..., trim:rows.shape[-1] - trim]
    return 10.0 * np.log10(rows) if db else rows
