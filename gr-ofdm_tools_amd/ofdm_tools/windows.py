"""Window tables handed to the HIP plans (host side, float64 -> float32).

``get_window`` mirrors the periodic windows ``scipy.signal.welch`` builds from a
string (``window='hann'`` default at ofdm_cr_tools.py:322,342, ``'flattop'`` at
ofdm_cr_tools.py:214 and spectrum_sweeper.py:263); ``blackmanharris`` mirrors
``gnuradio.filter.window.blackmanharris`` (symmetric, psd_logger.py:47,
local_worker.py:62) and ``flattop`` the symmetric ``sg.flattop(npts)`` of
ofdm_cr_tools.py:175.  ``dpss`` returns the Slepian tapers of the multitaper plans
(``scipy.signal.windows.dpss`` with ``Kmax``), computed by the library's host-only ``oth_dpss``.
"""
import ctypes

import numpy as np

_FLATTOP = (0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368)
_BH92 = (0.35875, 0.48829, 0.14128, 0.01168)


def _cosine_sum(coeffs, n, denom):
    f = 2.0 * np.pi * np.arange(n) / float(denom)
    w = np.zeros(n)
    for i, a in enumerate(coeffs):
        w += ((-1) ** i) * a * np.cos(i * f)
    return w


def get_window(name, nperseg):
    """Periodic (DFT-even) window, as scipy.signal.get_window(name, nperseg)."""
    if name in ('hann', 'hanning'):
        return _cosine_sum((0.5, 0.5), nperseg, nperseg)
    if name == 'flattop':
        return _cosine_sum(_FLATTOP, nperseg, nperseg)
    if name == 'blackmanharris':
        return _cosine_sum(_BH92, nperseg, nperseg)
    if name in ('boxcar', 'rect', 'rectangular'):
        return np.ones(nperseg)
    raise ValueError('unknown window %r' % (name,))


def blackmanharris(ntaps):
    """gnuradio.filter.window.blackmanharris(ntaps): symmetric 4-term, 92 dB."""
    return _cosine_sum(_BH92, ntaps, max(ntaps - 1, 1))


def flattop(npts):
    """Symmetric flat-top, ``sg.flattop(npts)``."""
    if npts == 1:
        return np.ones(1)
    return _cosine_sum(_FLATTOP, npts, npts - 1)


def pfb_prototype(nfft, ntaps, beta=None, cutoff=1.0):
    """The prototype of a polyphase filter bank of nfft channels with ntaps taps per branch (WelchPlan.set_prototype): a
    Kaiser-windowed sinc, sinc(cutoff (i - (L - 1) / 2) / nfft) kaiser(L, beta) over L = ntaps nfft taps, beta = 2.5 ntaps
    by default; float64, symmetric.  cutoff 1 puts the sinc's first nulls one transform length from the centre: a bin of the
    bank has a flat top and a stop band one bin away (noise bandwidth 0.78 ... 0.86 bins for 4 ... 16 taps)."""
    nfft, ntaps = int(nfft), int(ntaps)
    if nfft < 1 or ntaps < 1:
        raise ValueError('pfb_prototype needs nfft >= 1 and ntaps >= 1 (got nfft=%d, ntaps=%d)' % (nfft, ntaps))
    L = nfft * ntaps
    beta = 2.5 * ntaps if beta is None else float(beta)
    t = (np.arange(L, dtype=np.float64) - 0.5 * (L - 1)) / nfft
    return np.sinc(float(cutoff) * t) * np.kaiser(L, beta)


def dpss(n, nw, kmax, return_ratios=False):
    """scipy.signal.windows.dpss(n, nw, kmax, return_ratios=...): the kmax Slepian sequences of length n with the largest
    concentration in [-nw / n, nw / n], float64 [kmax, n], unit L2 norm, SciPy's signs; with return_ratios also their
    concentration ratios, float64 [kmax].  Runs on the host (oth_dpss: no context, no GPU)."""
    from . import _hip
    n, kmax, nw = int(n), int(kmax), float(nw)
    if n < 2 or not 0.0 < nw < 0.5 * n or not 1 <= kmax <= n:
        raise ValueError('dpss needs n >= 2, 0 < nw < n / 2 and 1 <= kmax <= n (got n=%d, nw=%r, kmax=%d)' % (n, nw, kmax))
    lib = _hip.load()
    tapers = np.empty((kmax, n), np.float64)
    ratios = np.empty(kmax, np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.oth_dpss(n, nw, kmax, tapers.ctypes.data_as(dp), ratios.ctypes.data_as(dp) if return_ratios else None)
    if rc != _hip.OK:
        raise _hip.HipError(rc, 'oth_dpss', lib.oth_last_error(None).decode())
    return (tapers, ratios) if return_ratios else tapers
