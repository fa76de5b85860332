"""float64 oracle of the spectral kurtosis estimator (Nita & Gary) on a Welch plan's periodograms, by the definition:
P_m[j] = g |FFT_nfft((x_m - mean_m) w)[j]|^2 with g = 1 / sum w^2 (the mean only when the plan detrends),
S1 = sum_m P_m, S2 = sum_m P_m^2, R = M S2 / S1^2, SK = (M + 1) / (M - 1) (R - 1); a bin with S1 = 0 reads R = SK = 0."""
import numpy as np

import median_oracle as MO


def sk_rows(x, nfft, nperseg=None, noverlap=0, window='hann', detrend=True):
    """-> float64 [M, nfft]: P_m, natural bin order."""
    nperseg = nfft if nperseg is None else nperseg
    return MO.welch_rows(x, 1.0, window, nperseg, noverlap, nfft, 'constant' if detrend else None, 'density')


def sk_of_rows(P):
    """P: [M, nfft] periodograms -> dict with S1, S2, R, SK (natural bin order) and M."""
    P = np.asarray(P, np.float64)
    M = P.shape[0]
    S1, S2 = P.sum(axis=0), (P * P).sum(axis=0)
    live = S1 > 0.0
    R = np.where(live, M * S2 / np.where(live, S1, 1.0) ** 2, 0.0)
    SK = np.where(live, (M + 1.0) / (M - 1.0) * (R - 1.0), 0.0)
    return {'S1': S1, 'S2': S2, 'R': R, 'SK': SK, 'M': M}


def sk(x, nfft, nperseg=None, noverlap=0, window='hann', detrend=True):
    return sk_of_rows(sk_rows(x, nfft, nperseg, noverlap, window, detrend))


def psd(ref, window, nperseg, scaling, fs, nfft):
    """The plan's PSD row (linear, natural order) from the oracle's S1: P carries g = 1 / sum w^2 already."""
    from oracle import ref_cpu as R
    win = R.get_window(window, nperseg) if isinstance(window, str) else np.asarray(window, np.float64)
    return ref['S1'] / ref['M'] * np.sum(win * win) * MO.plan_scale(win, scaling, fs, nfft)


def r_of_sk(sk_row, M):
    """R = M S2 / S1^2 recovered from a returned SK row."""
    return np.asarray(sk_row, np.float64) * (M - 1.0) / (M + 1.0) + 1.0
