"""float64 oracle of the spectral matrix and the generalized coherence of C channels on a Welch plan, by the definition: M
the plan's segment count, per segment s, channel a and bin j
  X_s,a = FFT_nfft((x_a,s - m_s,a) w),   m_s,a the segment's mean when the plan detrends, else 0,
  T_ab = sum_s conj(X_s,a) X_s,b,   S = scale T / M,   G_ab = T_ab / sqrt(T_aa T_bb),   gcoh = 1 - det G (numpy.linalg.det),
with the library's degenerate rules: a bin in which a channel holds no power reads 0 in the channel's rows and in gcoh; a
non-finite channel reads NaN in its rows and in gcoh."""
import numpy as np

import median_oracle as MO
from oracle import ref_cpu as R


def nseg(nsamples, nperseg, noverlap=0):
    return (nsamples - noverlap) // (nperseg - noverlap)


def null_mean(nchan, M):
    """E[1 - det G] of independent noise over M independent segments: 1 - prod_{k=1}^{C-1} (M - k) / M"""
    prod = 1.0
    for k in range(1, nchan):
        prod *= max(M - k, 0) / float(M)
    return 1.0 - prod


def pairs(nchan):
    """the packed rows' order: the upper triangle row by row"""
    return [(a, b) for a in range(nchan) for b in range(a, nchan)]


def matrix(x, nfft, nperseg=None, noverlap=0, window='hann', detrend=True, scaling='density', fs=1.0):
    """x: (C, n) -> dict: M, T [C, C, nfft] complex (the raw sums), S [C, C, nfft] complex, gcoh [nfft] (natural bin order),
    scale."""
    x = np.asarray(x)
    C = x.shape[0]
    nperseg = nfft if nperseg is None else nperseg
    M = nseg(x.shape[1], nperseg, noverlap)
    assert M >= 1
    win = R.get_window(window, nperseg) if isinstance(window, str) else np.asarray(window, np.float64)
    scale = MO.plan_scale(win, scaling, fs, nfft)
    X = np.empty((C, M, nfft), np.complex128)
    with np.errstate(all='ignore'):
        for a in range(C):
            seg = R._segments(x[a].astype(np.complex128), nperseg, noverlap)[:M]
            assert seg.shape == (M, nperseg)
            if detrend:
                seg = seg - seg.mean(axis=1, keepdims=True)
            X[a] = np.fft.fft(seg * win, nfft, axis=1)
        T = np.einsum('asj,bsj->abj', np.conj(X), X)
        d = np.einsum('aaj->aj', T).real
        bad = ~np.isfinite(d)                      # [C, nfft]
        empty = ~bad & (d <= 0.0)
        S = T * (scale / M)
        for a in range(C):
            S[a][:, empty[a]] = 0.0
            S[:, a][:, empty[a]] = 0.0
        for a in range(C):
            S[a][:, bad[a]] = np.nan + 1j * np.nan
            S[:, a][:, bad[a]] = np.nan + 1j * np.nan
        gcoh = np.zeros(nfft)
        ok = ~(bad.any(axis=0) | empty.any(axis=0))
        if ok.any():
            dd = d[:, ok]
            G = T[:, :, ok] / np.sqrt(dd[:, None, :] * dd[None, :, :])
            det = np.linalg.det(np.moveaxis(G, 2, 0)).real
            gcoh[ok] = np.clip(1.0 - det, 0.0, 1.0)
        gcoh[bad.any(axis=0)] = np.nan
    return {'M': M, 'T': T, 'S': S, 'gcoh': gcoh, 'scale': scale}


def shape_out(row, fftshift=False, trim=0):
    """a natural-order row (last axis nfft) as the plan hands it out"""
    row = np.fft.fftshift(row, axes=-1) if fftshift else row
    return row[..., trim:row.shape[-1] - trim] if trim else row
