"""float64 oracle of the multitaper jackknife (oth_mtm_jackknife, oth_mtm_csd_jackknife; csrc/mtmjack.hip) by the
definitions in include/ofdm_tools_hip.h, literally: the M = K nseg (segment, taper) items' transforms, their weighted
powers and cross terms, the totals, and per item the clamped ratio, log1p, the delete-one coherence and its atanh.  Tapers and
weights from mtm_csd_oracle.taper_table, segments and mean removal from mtm_ftest_oracle.eigencoefficients."""
import numpy as np

import mtm_csd_oracle as MC
import mtm_ftest_oracle as FO

CL = 1.0 - 2.0 ** -24


def items(x, nfft, nperseg=None, noverlap=0, nw=4.0, K=None, detrend=True, scaling='density', tapers=None):
    """-> (X complex128 [M, nfft] in natural bin order, items ordered (segment, taper) with the taper fastest; c [M])"""
    nperseg = nfft if nperseg is None else nperseg
    tapers, a = MC.taper_table(nperseg, nw, K, 'unity', tapers)
    c = np.array([ak / np.sum(v * v) if scaling == 'density' else ak for v, ak in zip(tapers, a)])
    y = FO.eigencoefficients(x, nfft, nperseg, noverlap, tapers, detrend)      # [nseg, K, nfft]
    nseg, K = y.shape[:2]
    return y.reshape(nseg * K, nfft), np.tile(c, nseg)


def _var(v, M):
    return np.maximum((M - 1.0) / M * (np.sum(v * v, axis=0) - np.sum(v, axis=0) ** 2 / M), 0.0)


def _ratios(p, S):
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.minimum(p / S[None, :], CL)
    return np.where(S[None, :] > 0.0, t, 0.0)


def lnpsd(p):
    """p: [M, nfft] item powers -> (lnsd [nfft], tmax [nfft])"""
    M = p.shape[0]
    S = p.sum(axis=0)
    t = _ratios(p, S)
    return np.sqrt(_var(np.log1p(-t), M)), t.max(axis=0)


def lnpsd_literal(p):
    """The same variance from the delete-one estimates themselves, ln((S - p_i) / (M - 1)); needs S - p_i > 0."""
    M = p.shape[0]
    return np.sqrt(_var(np.log((p.sum(axis=0)[None, :] - p) / (M - 1.0)), M))


def z_of(c):
    return np.arctanh(np.minimum(np.sqrt(c), CL))


def jackknife(x, nfft, **kw):
    """One channel.  -> dict(lnsd, tmax, S, M): float64 [nfft] rows in natural bin order"""
    X, c = items(x, nfft, **kw)
    p = c[:, None] * np.abs(X) ** 2
    lnsd, tmax = lnpsd(p)
    return dict(lnsd=lnsd, tmax=tmax, S=p.sum(axis=0), M=p.shape[0])


def csd_jackknife(x, y, nfft, **kw):
    """Two channels.  -> dict(cxy, z, zsd, lnsd_x, lnsd_y, tmax_x, tmax_y, cmax, M): float64 [nfft], natural bin order"""
    X, c = items(x, nfft, **kw)
    Y, _ = items(y, nfft, **kw)
    p, q, r = c[:, None] * np.abs(X) ** 2, c[:, None] * np.abs(Y) ** 2, c[:, None] * np.conj(X) * Y
    M = p.shape[0]
    Sxx, Syy, Sxy = p.sum(axis=0), q.sum(axis=0), r.sum(axis=0)
    lx, tmx = lnpsd(p)
    ly, tmy = lnpsd(q)
    ok = (Sxx > 0.0) & (Syy > 0.0)
    tx, ty = _ratios(p, Sxx), _ratios(q, Syy)
    with np.errstate(divide='ignore', invalid='ignore'):
        C = np.where(ok, np.abs(Sxy) ** 2 / (Sxx * Syy), 0.0)
        Ci = np.where(ok[None, :], np.abs(Sxy[None, :] - r) ** 2 / (Sxx[None, :] * (1.0 - tx) * Syy[None, :] * (1.0 - ty)), 0.0)
    d = np.where(ok[None, :], z_of(Ci) - z_of(C)[None, :], 0.0)
    return dict(cxy=C, z=z_of(C), zsd=np.sqrt(_var(d, M)), lnsd_x=lx, lnsd_y=ly, tmax_x=tmx, tmax_y=tmy,
                cmax=np.maximum(C, Ci.max(axis=0)), M=M)


def shift_trim(v, fftshift, trim):
    v = np.fft.fftshift(v) if fftshift else v
    return v[trim:len(v) - trim] if trim else v
