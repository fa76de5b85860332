"""float64 oracle of the generalized cross-correlation of the spectral matrix's pairs (oth_welch_matrix_gcc) by the header's
definitions, from the raw sums T of tests/welch_matrix_oracle.py: per pair a < b, over the signed bins k of the band,
  u_k = T_ab / |T_ab| (0 where |T_ab| = 0 or T_aa <= 0 or T_bb <= 0),  w_k = 1 | |T_ab| / sqrt(T_aa T_bb) | |T_ab|,
  Z = count of u_k != 0 (PHAT, SCOT) | sqrt(sum T_aa sum T_bb) (PLAIN),  R[l] = (1 / Z) sum_k w_k u_k e^(+j 2 pi k l / NI)
by numpy.fft.ifft of NI = U nfft points with bin k at index k mod NI, the window -maxlag ... maxlag, and the peak: the lowest
lag of the largest |R|, the parabola through |R| at its neighbours.  Next to it the gates of the GPU suite, which follow from
the matrix family's contract |dT_ab| <= RTOL sqrt(T_aa T_bb) and from no measured number, and the captures and cases both
suites share (the CPU suite checks the cases' conditions on the oracle alone)."""
import numpy as np

import welch_matrix_oracle as XO

WEIGHTINGS = ('plain', 'phat', 'scot')      # in the order of OTH_GCC_PLAIN, OTH_GCC_PHAT, OTH_GCC_SCOT


def pairs(nchan):
    """the rows' order: (0,1), (0,2), ..., (C-2,C-1)"""
    return [(a, b) for a in range(nchan) for b in range(a + 1, nchan)]


def parabola(y, i):
    """the offset d of the parabola's top through y[i - 1], y[i], y[i + 1] and its denominator; (0, 0) where i is an edge of
    y, d = 0 where the denominator is not negative"""
    if i == 0 or i == len(y) - 1:
        return 0.0, 0.0
    den = y[i - 1] - 2.0 * y[i] + y[i + 1]
    return (0.5 * (y[i - 1] - y[i + 1]) / den if den < 0.0 else 0.0), den


def gcc(T, weighting='phat', band=None, upsample=1, maxlag=None):
    """T: [C, C, nfft] complex raw sums, natural bin order (welch_matrix_oracle.matrix(...)['T']).  -> dict over the P pairs:
    'R' [P, 2 maxlag + 1] complex, 'peak' [P, 3] (delay in samples, |R|, arg R at the peak), 'lag' [P] the peak's lag i,
    'den' [P] the parabola's denominator (0 at a window edge), 'lead' [P] what the top of |R| leads every other lag of the
    window by (inf with one lag), 'wsum' [P] sum_k w_k / Z, 'coh' [P, bins] |T_ab| / sqrt(T_aa T_bb) of the in-band bins (0
    where u = 0), 'Z' [P]; a pair with a non-finite sum reads NaN, one with Z = 0 reads 0 (and peak (0, 0, 0))."""
    T = np.asarray(T)
    C, nfft = T.shape[0], T.shape[2]
    U = int(upsample)
    NI = U * nfft
    lo, hi = (-(nfft // 2), nfft // 2 - 1) if band is None else band
    L = NI // 2 - 1 if maxlag is None else int(maxlag)
    assert weighting in WEIGHTINGS and -(nfft // 2) <= lo <= hi <= nfft // 2 - 1 and 0 <= L <= NI // 2 - 1
    k = np.arange(lo, hi + 1)
    lags = np.arange(-L, L + 1)
    P = len(pairs(C))
    out = {'R': np.zeros((P, 2 * L + 1), np.complex128), 'peak': np.zeros((P, 3)), 'lag': np.zeros(P, np.int64), 'den': np.zeros(P),
           'lead': np.full(P, np.inf), 'wsum': np.zeros(P), 'coh': np.zeros((P, len(k))), 'Z': np.zeros(P), 'lags': lags}
    with np.errstate(all='ignore'):
        for p, (a, b) in enumerate(pairs(C)):
            tab, taa, tbb = T[a, b, k % nfft], T[a, a, k % nfft].real, T[b, b, k % nfft].real
            if not (np.all(np.isfinite(tab)) and np.all(np.isfinite(taa)) and np.all(np.isfinite(tbb))):
                for name in ('R', 'peak', 'den', 'lead', 'wsum', 'coh', 'Z'):
                    out[name][p] = np.nan
                continue
            mag = np.abs(tab)
            live = (mag > 0) & (taa > 0) & (tbb > 0)
            safe = np.where(live, mag, 1.0)
            root = np.where(live, np.sqrt(taa * tbb), 1.0)
            u = np.where(live, tab / safe, 0.0)
            out['coh'][p] = np.where(live, mag / root, 0.0)
            if weighting == 'phat':
                w, Z = live.astype(np.float64), float(live.sum())
            elif weighting == 'scot':
                w, Z = out['coh'][p], float(live.sum())
            else:
                w, Z = np.where(live, mag, 0.0), float(np.sqrt(taa.sum() * tbb.sum()))
            out['Z'][p] = Z
            if not Z > 0:
                continue
            spec = np.zeros(NI, np.complex128)
            spec[k % NI] = w * u
            R = (np.fft.ifft(spec) * (NI / Z))[lags % NI]
            y = np.abs(R)
            i = int(np.argmax(y))      # the first of equals: the lowest lag
            d, den = parabola(y, i)
            out['R'][p], out['lag'][p], out['den'][p], out['wsum'][p] = R, lags[i], den, w.sum() / Z
            out['peak'][p] = (lags[i] + d) / U, y[i], np.angle(R[i])
            if len(y) > 1:
                out['lead'][p] = y[i] - np.delete(y, i).max()
    return out


def gates(want, weighting, NI, rtol):
    """The absolute gate on R of each pair, [P]: from |dT_ab| <= rtol sqrt(T_aa T_bb) per bin,
      plain   3 rtol: every term of the sum moves by rtol sqrt(T_aa T_bb), their sum by at most rtol Z (Cauchy-Schwarz), and
              Z itself moves by rtol Z relatively (T_aa and T_bb by rtol each, under the root) - with |R| <= 1 and the second order
      scot    2 rtol: a term T_ab / sqrt(T_aa T_bb) moves by rtol from T_ab and by rtol from the root, the mean of such by the same
      phat    the mean over the in-band bins of min(2, 2 rtol / |G_ab|): a unit phasor turns by at most its relative error
              (twice it covers the chord to second order), and by no more than 2 whatever happens
    each with the float32 transform's worst case added, 16 2^-24 log2(NI) sum_k w_k / Z."""
    coh = want['coh']
    with np.errstate(all='ignore'):
        if weighting == 'plain':
            g = np.full(len(coh), 3.0 * rtol)
        elif weighting == 'scot':
            g = np.full(len(coh), 2.0 * rtol)
        else:
            g = np.mean(np.minimum(2.0, 2.0 * rtol / np.where(coh > 0, coh, 1e-300)), axis=1)
    return g + 16.0 * 2.0 ** -24 * np.log2(NI) * want['wsum']


def delay_gate(want, g, U):
    """-> (the gate on the delay in samples per pair, [P]: 3 g / (|den| - 4 g) / U - the parabola's numerator moves by g, its
    denominator by 4 g and |d| <= 1 / 2 -, the conditions per pair, [P] bool: the oracle's top leads every other lag of the
    window by more than 2 g, so the device picks the same lag, and |den| > 8 g unless the top is a window edge, where d = 0 on
    both sides)"""
    edge = (np.abs(want['lag']) == (len(want['lags']) - 1) // 2)
    den = np.abs(want['den'])
    with np.errstate(all='ignore'):
        gate = np.where(edge, 0.0, 3.0 * g / (den - 4.0 * g) / U)
    return gate, (want['lead'] > 2.0 * g) & (edge | (den > 8.0 * g))


# ---- the captures and cases of the two suites ------------------------------------------------------------------------------------

BASE_DELAYS = (0.0, 3.0, -7.0, 5.0, -2.0, 8.0, -4.0, 1.0)      # whole samples per channel; the grid fractions come on top


def channel_delays(nchan, U):
    """per-channel delays in samples whose differences lie near the lag grid of 1 / U sample - whole samples, c mod U grid
    steps and 0.04 c of a step on top -, so that the top of |R| leads its neighbours and the parabola still has an offset
    to find"""
    c = np.arange(nchan)
    return np.array(BASE_DELAYS[:nchan]) + ((c % U) + 0.04 * c) / U


def delayed_capture(delays, n, seed, snr_db=0.0, band=None, offset=0.0, dtype=np.complex64):
    """len(delays) channels of n samples: a common complex white signal of unit power, channel c carrying s(t - delays[c])
    (a phase ramp on a transform of a power of two at least n + 64 points, cut to n), limited to the frequencies
    band = (f_lo, f_hi) cycles per sample (hi excluded) where given, at snr_db over independent unit noise per channel"""
    rng = np.random.default_rng(seed)
    C = len(delays)
    nfast = 1 << (n + 63).bit_length()
    f = np.fft.fftfreq(nfast)
    spec = np.fft.fft(rng.standard_normal(nfast) + 1j * rng.standard_normal(nfast))
    if band is not None:
        spec[~((f >= band[0]) & (f < band[1]))] = 0.0
    spec /= np.sqrt(np.mean(np.abs(spec) ** 2) / nfast)      # unit power in time
    s = np.fft.ifft(spec[None, :] * np.exp(-2j * np.pi * f[None, :] * np.asarray(delays, np.float64)[:, None]), axis=1)[:, :n]
    x = (rng.standard_normal((C, n)) + 1j * rng.standard_normal((C, n))) / np.sqrt(2.0) + 10.0 ** (snr_db / 20.0) * s
    return (x + offset).astype(dtype)


# nfft, U, C, M, option (of the matrix suite's list: OPTIONS of tests/test_welch_matrix_gpu.py), narrow (the common signal in f in [-0.25, 0) and the band set to its bins but the outermost), maxlag
# (None: the largest).  One case per NI build 64 ... 16384 (twice at 256 and 4096); C cycles through 2, 3, 5, 8; the narrow
# cases stay at U <= 2, where the peak of a quarter band is still sharp against the gate; then the small windows: maxlag = 0,
# and a window of +-2 samples that the delays of -7 and 3 samples leave on either edge.
PARITY = [
    (64, 1, 2, 1, 0, False, None),
    (64, 2, 3, 4, 1, True, None),
    (64, 4, 5, 12, 2, False, None),
    (128, 4, 8, 7, 3, False, None),
    (256, 4, 2, 9, 4, False, None),
    (256, 8, 3, 11, 5, False, None),
    (4096, 1, 5, 3, 6, True, None),
    (2048, 4, 8, 5, 0, False, None),
    (16384, 1, 2, 2, 1, False, None),
    (2048, 8, 3, 6, 2, False, None),
    (64, 1, 2, 8, 3, False, 0),
    (64, 2, 3, 10, 4, False, 4),
]


def parity_input(nfft, U, C, M, option, narrow, maxlag):
    """-> x [C, n] complex64, the plan's (nperseg, noverlap, detrend, scaling, fftshift, trim, db), band in signed bins or None"""
    from test_welch_matrix_gpu import OPTIONS      # nperseg x / 16 of nfft, overlap %, detrend, scaling, fftshift, trim x nfft / 64, db, offset
    frac, ov, detrend, scaling, fftshift, trim64, db, offset = OPTIONS[option]
    nperseg = nfft * frac // 16
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    n = noverlap + M * step + step // 3
    x = delayed_capture(channel_delays(C, U), n, 11 * nfft + 17 * C + M + U, 0.0, (-0.25, 0.0) if narrow else None, offset)
    band = (-nfft // 4 + 1, -2) if narrow else None
    return x, (nperseg, noverlap, detrend, scaling, fftshift, trim64 * nfft // 64, db), band
