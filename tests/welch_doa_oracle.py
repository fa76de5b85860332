"""float64 oracle of the Bartlett, Capon (MVDR) and MUSIC direction spectra of the spectral matrix S or of the coherence matrix
G of C channels on a Welch plan (oth_welch_set_steering, oth_welch_matrix_doa), by the header's definitions on
tests/welch_matrix_oracle.py's dict and tests/welch_eig_oracle.py's matrices: channel c of direction d carries s(t - tau_dc),
the steering vector at bin k is w_c = exp(+j 2 pi (fc + f_k) tau_dc) with f_k the signed bin frequency in cycles per sample,
and with l_i (descending, clamped at 0) and v_i the eigenpairs of the bin's matrix A (numpy.linalg.eigh), p_i = |v_i^H w|^2 and
delta = loading trace(A) / C:
  bartlett = sum_i l_i p_i / C^2,   capon = 1 / sum_i p_i / (l_i + delta) (0 where l_C + delta <= 0),
  music = C / sum_{i > nsrc} p_i (+inf where the sum is exactly 0);   a non-finite channel reads NaN in every row.
Bartlett and Capon are also formed the direct way - w^H A w / C^2 and 1 / w^H inv(A + delta I) w (numpy.linalg.inv) -, so the
eigen-form is checked against an independent formula.  doa_capture synthesises a line array's capture by physically delaying
each source per channel; combine is the band combination of ofdm_cr_tools.doa_scan; peaks lists a row's local maxima."""
import numpy as np

import welch_eig_oracle as EO
import welch_matrix_oracle as XO


def bin_freqs(nfft):
    """the signed bin frequencies in cycles per sample, natural order: k / nfft below nfft / 2, (k - nfft) / nfft from there on"""
    k = np.arange(nfft)
    return np.where(k < nfft // 2, k, k - nfft) / float(nfft)


def steering(delays, fc, nfft):
    """delays [D, C] in samples, fc in cycles per sample -> w [D, nfft, C] = exp(+j 2 pi (fc + f_k) tau_dc)"""
    tau = np.asarray(delays, np.float64)
    phase = np.mod(fc * tau, 1.0)[:, None, :] + bin_freqs(nfft)[None, :, None] * tau[:, None, :]
    return np.exp(2j * np.pi * phase)


def doa(x, nfft, delays, fc, nperseg=None, noverlap=0, window='hann', detrend=True, scaling='density', fs=1.0, of='S', nsrc=1,
        loading=0.0, ref=None, direct=False):
    """-> dict: bartlett, capon, music [D, nfft] float64 in natural bin order; lam [C, nfft] the eigenvalues (descending, clamped),
    delta [nfft], A [nfft, C, C], bad [nfft], M, ref; with direct=True also bartlett_direct and capon_direct (the bins where
    A + delta I is singular read 0 there too)"""
    ref = XO.matrix(x, nfft, nperseg, noverlap, window, detrend, scaling, fs) if ref is None else ref
    A, bad = EO.matrices(ref, of)
    C = A.shape[1]
    lam = EO.decompose(A)[0]                               # [nfft, C] descending, clamped, exact zeros of silent channels
    V = np.linalg.eigh(A)[1][:, :, ::-1]                   # [nfft, C, C]: column i the vector of the i-th largest
    w = steering(delays, fc, nfft)                         # [D, nfft, C]
    p = np.abs(np.einsum('jci,djc->dji', np.conj(V), w)) ** 2
    trace = np.einsum('jaa->j', A).real
    delta = loading * trace / C
    with np.errstate(all='ignore'):
        bartlett = (lam[None] * p).sum(axis=2) / C ** 2
        den = lam + delta[:, None]
        singular = den[:, C - 1] <= 0.0
        capon = 1.0 / (p / np.where(den > 0.0, den, 1.0)[None]).sum(axis=2)
        capon[:, singular] = 0.0
        noise = p[:, :, nsrc:].sum(axis=2)
        music = np.where(noise == 0.0, np.inf, C / np.where(noise == 0.0, 1.0, noise))
    out = {'bartlett': bartlett, 'capon': capon, 'music': music}
    if direct:
        out['bartlett_direct'] = np.einsum('dja,jab,djb->dj', np.conj(w), A, w).real / C ** 2
        loaded = A + delta[:, None, None] * np.eye(C)[None]
        loaded[singular] = np.eye(C)
        q = np.einsum('dja,jab,djb->dj', np.conj(w), np.linalg.inv(loaded), w).real
        out['capon_direct'] = np.where(singular[None, :], 0.0, 1.0 / q)
    for r in out.values():
        r[:, bad] = np.nan
    out.update(lam=lam.T.copy(), delta=delta, A=A, bad=bad, M=ref['M'], ref=ref)
    return out


def combine(rows, band=None):
    """dict method -> [D, m] -> dict method -> [D] over the bins band = (lo, hi) of the last axis (None: all): the mean for
    bartlett, 1 / mean(1 / P) for capon and music"""
    out = {}
    for name in ('bartlett', 'capon', 'music'):
        if name in rows:
            r = np.asarray(rows[name], np.float64)
            r = r if band is None else r[:, band[0]:band[1]]
            out[name] = r.mean(axis=1) if name == 'bartlett' else 1.0 / (1.0 / r).mean(axis=1)
    return out


def peaks(row):
    """the interior local maxima of a row (above the left neighbour, not below the right one), the highest first"""
    r = np.asarray(row, np.float64)
    at = [i for i in range(1, len(r) - 1) if r[i] > r[i - 1] and r[i] >= r[i + 1]]
    return sorted(at, key=lambda i: -r[i])


def ula_delays(nchan, angles_deg, fc, spacing=0.5):
    """tau[d, c] = c spacing sin(theta_d) / fc: a line array of `spacing` wavelengths at the carrier fc (cycles per sample)"""
    return np.arange(nchan)[None, :] * (spacing * np.sin(np.deg2rad(np.asarray(angles_deg, np.float64))) / fc)[:, None]


def doa_capture(C, nfft, M, angles, snr_db, seed, fc=2.0):
    """unit complex noise per channel plus, per source, white complex Gaussian noise of the given SNR (dB, per channel) that
    reaches channel c later by tau_c = c sin(theta) / (2 fc) samples - a half-wavelength line array at the carrier fc -, the
    delay applied in the frequency domain of the whole capture to the pass-band signal: X_c(f) = S(f) exp(-j 2 pi (fc + f) tau_c)
    -> complex64 (C, nfft M)"""
    rng = np.random.default_rng(seed)
    n = nfft * M
    x = (rng.standard_normal((C, n)) + 1j * rng.standard_normal((C, n))) / np.sqrt(2.0)
    f = np.fft.fftfreq(n)
    for theta, snr in zip(angles, snr_db):
        s = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5 * 10.0 ** (snr / 10.0))
        spec = np.fft.fft(s)
        tau = np.arange(C) * np.sin(np.deg2rad(theta)) / (2.0 * fc)
        x = x + np.fft.ifft(spec[None, :] * np.exp(-2j * np.pi * (fc + f)[None, :] * tau[:, None]), axis=1)
    return x.astype(np.complex64)
