"""float64 oracle of the polyphase filter-bank (WOLA) PSD of a Welch plan, by the definition: with N = nfft, P = ntaps, a real
prototype h of P N taps, step = N - noverlap and M = (len(x) - P N) // step + 1 frames, per frame s
  m_s    = mean_{i < P N} x[s step + i] when the plan detrends, else 0
  y_s[n] = sum_{p < P} h[n + p N] (x[s step + n + p N] - m_s),  n < N
  pfb    = scale sum_s |FFT_N(y_s)|^2 / M,   scale the plan's with h in the window's place
- and emulate32, the same in the kernel's precision and order (complex64 samples, float32 taps and accumulators, the pilot
then the residual mean, a complex64 transform), which says what float32 itself loses on an input."""
import numpy as np

import median_oracle as MO

PILOT = 64      # samples behind the pilot (csrc/mtm_common.hip.h)


def nseg(nsamples, nfft, ntaps, noverlap=0):
    """the frame count (0 where the input is shorter than one frame)"""
    return (nsamples - ntaps * nfft) // (nfft - noverlap) + 1 if nsamples >= ntaps * nfft else 0


def frames(x, nfft, ntaps, noverlap, M):
    """-> [M, P N]: the frames' samples, in x's type"""
    step, L = nfft - noverlap, ntaps * nfft
    return np.stack([x[s * step:s * step + L] for s in range(M)])


def pfb(x, nfft, ntaps, h, noverlap=0, detrend=True, scaling='density', fs=1.0):
    """-> dict: M, pfb [nfft] (natural bin order, linear), scale."""
    h = np.asarray(h, np.float64)
    assert h.shape == (ntaps * nfft,)
    M = nseg(len(x), nfft, ntaps, noverlap)
    assert M >= 1
    xs = frames(np.asarray(x).astype(np.complex128), nfft, ntaps, noverlap, M)
    if detrend:
        xs = xs - xs.mean(axis=1, keepdims=True)
    y = (xs * h).reshape(M, ntaps, nfft).sum(axis=1)
    X = np.fft.fft(y, axis=1)
    scale = MO.plan_scale(h, scaling, fs, nfft)
    return {'M': M, 'pfb': (X.real * X.real + X.imag * X.imag).sum(axis=0) * scale / M, 'scale': scale}


def emulate32(x, nfft, ntaps, h, noverlap=0, detrend=True, scaling='density', fs=1.0):
    """pfb() as float32 arithmetic forms it -> float64 [nfft] (the scale and the sum over frames applied in double, as the
    finalize launch does)."""
    import scipy.fft
    h64 = np.asarray(h, np.float64)
    h32 = h64.astype(np.float32)
    hfold = h32.astype(np.float64).reshape(ntaps, nfft).sum(axis=0).astype(np.float32)
    M = nseg(len(x), nfft, ntaps, noverlap)
    xs = frames(np.asarray(x, np.complex64), nfft, ntaps, noverlap, M)
    total = np.zeros(nfft, np.float64)
    for s in range(M):
        r = xs[s]
        if detrend:
            pil = np.complex64(r[:PILOT].sum(dtype=np.complex64) * np.float32(1.0 / PILOT))
            r = (r - pil).astype(np.complex64)
        y = np.zeros(nfft, np.complex64)
        for p in range(ntaps):
            y = (y + h32[p * nfft:(p + 1) * nfft] * r[p * nfft:(p + 1) * nfft]).astype(np.complex64)
        if detrend:
            mean = np.complex64(r.sum(dtype=np.complex64) * np.float32(1.0 / (ntaps * nfft)))
            y = (y - mean * hfold).astype(np.complex64)
        X = scipy.fft.fft(y)
        assert X.dtype == np.complex64
        total += (X.real * X.real + X.imag * X.imag).astype(np.float32)
    return total * MO.plan_scale(h32.astype(np.float64), scaling, fs, nfft) / M


def hann_welch(x, nfft, fs=1.0):
    """-> float64 [nfft]: the Hann Welch PSD without overlap, constant detrend, density scaling, natural bin order"""
    return MO.welch_rows(x, fs, 'hann', nfft, 0, nfft).mean(axis=0)


# ---- the leakage capture: a strong band next to empty channels -----------------------------------------------------------------
LEAK_NFFT, LEAK_TAPS, LEAK_M, LEAK_SEED = 256, 8, 64, 20
LEAK_BAND = (100, 109)                      # the bins the tones fill
LEAK_EMPTY = (96, 97, 98, 112, 113, 114)    # empty bins two and more away from the band's edge bins
LEAK_DB = 60.0                              # the band's level per bin over the noise's


def leak_capture(seed=LEAK_SEED):
    """LEAK_M frames of LEAK_TAPS x LEAK_NFFT at hop LEAK_NFFT: unit complex noise and forty tones, a quarter of a bin apart
    from bin 99.625 to bin 109.375, random phases, together LEAK_DB above the noise in each of the band's ten bins"""
    n = LEAK_NFFT * (LEAK_TAPS + LEAK_M - 1)
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    nbins, ntones = LEAK_BAND[1] - LEAK_BAND[0] + 1, 40
    amp = np.sqrt(10.0 ** (LEAK_DB / 10.0) * nbins / LEAK_NFFT / ntones)
    t = np.arange(n)
    for i in range(ntones):
        f = (LEAK_BAND[0] - 0.375 + 0.25 * i) / LEAK_NFFT
        x = x + amp * np.exp(2j * np.pi * (f * t + rng.random()))
    return x.astype(np.complex64)


def check_leakage(pfb_row, hann_row, what=''):
    """natural-order linear rows of the capture: every empty PFB bin within 3 dB of the row's median; Hann at least 10 dB
    above its median at bin 98"""
    rel = lambda row: 10.0 * np.log10(np.asarray(row, np.float64) / np.median(row))      # noqa: E731
    p, w = rel(pfb_row), rel(hann_row)
    print('leakage %s: PFB at bins %s: %s dB of the median; Hann at 98 / 112: %+.1f / %+.1f dB' %
          (what, LEAK_EMPTY, np.round(p[list(LEAK_EMPTY)], 2), w[98], w[112]))
    assert np.all(np.abs(p[list(LEAK_EMPTY)]) <= 3.0)
    assert w[98] >= 10.0
    assert p[LEAK_BAND[0]:LEAK_BAND[1] + 1].min() >= LEAK_DB - 3.0      # ... and the band itself reads its level
