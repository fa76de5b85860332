"""float64 oracle of the two-channel multitaper plans (oth_mtm_csd_plan): csd_oracle.csd_sums once per taper with
window = v_k, the sums weighted by c_k (mtm_oracle's tapers and weights; the taper's energy under 'density'), then
median_oracle's scale and output stage."""
import numpy as np

import csd_oracle as C
import median_oracle as M
import mtm_oracle as O


def taper_table(nperseg, nw=4.0, K=None, weights='unity', tapers=None):
    """-> (float64 tapers [K, nperseg], weights a_k normalised to sum 1) as mtm_oracle.mtm_psd takes them"""
    if tapers is None:
        return O.tapers_and_weights(nperseg, nw, int(2 * nw) - 1 if K is None else K, weights)
    tapers = np.asarray(tapers, np.float64)
    a = np.ones(len(tapers)) if isinstance(weights, str) else np.asarray(weights, np.float64)
    return tapers, a / a.sum()


def mtm_csd_sums(x, y, nfft, nperseg=None, noverlap=0, nw=4.0, K=None, weights='unity', detrend=True, scaling='density',
                 tapers=None):
    """-> (sxx, syy, sxy, nseg): sum over segments and tapers of c_k |X_k|^2, c_k |Y_k|^2, c_k conj(X_k) Y_k in natural
    bin order - what oth_csd_partial_dev leaves on such a plan; c_k = a_k / sum(v_k^2) under 'density', a_k otherwise."""
    nperseg = nfft if nperseg is None else nperseg
    tapers, a = taper_table(nperseg, nw, K, weights, tapers)
    sxx, syy, sxy, nseg = np.zeros(nfft), np.zeros(nfft), np.zeros(nfft, np.complex128), 0
    for v, ak in zip(tapers, a):
        ck = ak / np.sum(v * v) if scaling == 'density' else ak
        txx, tyy, txy, nseg = C.csd_sums(x, y, v, nperseg, noverlap, nfft, 'constant' if detrend else False)
        sxx += ck * txx
        syy += ck * tyy
        sxy += ck * txy
    return sxx, syy, sxy, nseg


def mtm_csd(x, y, nfft, nperseg=None, noverlap=0, nw=4.0, K=None, weights='unity', detrend=True, scaling='density', fs=1.0,
            tapers=None, fftshift=False, trim=0):
    """-> [pxx, pyy, pxy (complex128), cxy], each [nfft - 2 trim] after the plan's fftshift and trim."""
    sxx, syy, sxy, nseg = mtm_csd_sums(x, y, nfft, nperseg, noverlap, nw, K, weights, detrend, scaling, tapers)
    # the tapers' energies are in c_k: what is left of median_oracle.plan_scale is that of a unit-energy window
    k = M.plan_scale(np.ones(1), scaling, fs, nfft) / nseg
    pxx, pyy, pxy = sxx * k, syy * k, sxy * k
    with np.errstate(invalid='ignore', divide='ignore'):
        cxy = (pxy.real * pxy.real + pxy.imag * pxy.imag) / (pxx * pyy)
    return [C.shift_trim(v, fftshift, trim) for v in (pxx, pyy, pxy, cxy)]
