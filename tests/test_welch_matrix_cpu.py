"""CPU checks of the spectral-matrix addition (no GPU): the float64 oracle by the definition (tests/welch_matrix_oracle.py)
against SciPy, on two identities and on the detection case, the Python helper's refusals, the declared surface, and the
resource figures of every welch_mat_kernel build and its finalize kernels read from the code objects of the built library."""
import numpy as np
import pytest

import welch_matrix_oracle as XO
from stat_support import POWERS, check_builds, check_surface

SYMBOLS = ('oth_welch_matrix_dev', 'oth_welch_matrix')
DET_C, DET_NFFT, DET_M = 4, 256, 32
DET_BAND = DET_NFFT // 4      # the common component fills the lowest quarter: fftshifted bins 0 ... 63
DET_GUARD = 2                 # bins on either side of a band edge (the Hann main lobe: +-2 bins) that belong to neither mean


def noise(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def detection_capture(seed, nchan=DET_C, nfft=DET_NFFT, M=DET_M, signal=True):
    """unit complex noise per channel plus a common component of unit power (0 dB per channel) in the lowest quarter of the
    band, [-1/2, -1/4) cycles per sample, with a random phase per channel -> complex64 (C, nfft M)"""
    rng = np.random.default_rng(seed)
    n = nfft * M
    x = noise(rng, (nchan, n))
    if signal:
        spec = np.fft.fft(noise(rng, n))
        f = np.fft.fftfreq(n)
        spec[~(f < -0.25)] = 0.0
        s = np.fft.ifft(spec)
        s /= np.sqrt(np.mean(np.abs(s) ** 2))
        x = x + s[None, :] * np.exp(2j * np.pi * rng.random(nchan))[:, None]
    return x.astype(np.complex64)


def check_detection(gcoh_shifted, null_mean, what=''):
    """the detection condition on a fftshifted gcoh row of the detection capture: the mean over the band's bins at least 0.9,
    the mean over the bins outside it within 25 % of null_mean.  DET_GUARD bins on either side of each band edge (the lower
    edge is the row's wrap-around) count for neither: the Hann window spreads a band edge over its main lobe."""
    g = np.asarray(gcoh_shifted, np.float64)
    assert g.shape == (DET_NFFT,)
    inband = g[DET_GUARD:DET_BAND - DET_GUARD].mean()
    outband = g[DET_BAND + DET_GUARD:DET_NFFT - DET_GUARD].mean()
    print('gcoh %s: in band %.4f, outside %.4f, null mean %.4f' % (what, inband, outband, null_mean))
    assert inband >= 0.9, inband
    assert abs(outband - null_mean) <= 0.25 * null_mean, (outband, null_mean)


# ---- 1. the oracle against SciPy ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nchan,nfft,nperseg,noverlap,detrend,scaling', [
    (2, 64, 64, 0, True, 'density'), (3, 128, 100, 50, True, 'spectrum'), (4, 256, 256, 128, False, 'density'),
    (5, 64, 48, 0, False, 'spectrum')])
def test_oracle_is_scipys_csd_welch_and_coherence(nchan, nfft, nperseg, noverlap, detrend, scaling):
    from scipy import signal
    rng = np.random.default_rng(nchan)
    n = nperseg + 9 * (nperseg - noverlap) + 3
    x = noise(rng, (nchan, n)) + 0.7 * noise(rng, n)[None, :] + (0.3 - 0.2j)
    ref = XO.matrix(x, nfft, nperseg, noverlap, detrend=detrend, scaling=scaling, fs=2.0)
    assert ref['M'] == 10
    kw = dict(fs=2.0, window='hann', nperseg=nperseg, noverlap=noverlap, nfft=nfft, detrend='constant' if detrend else False,
              return_onesided=False, scaling=scaling)
    worst = 0.0
    for a in range(nchan):
        pa = signal.welch(x[a], **kw)[1]
        worst = max(worst, np.max(np.abs(ref['S'][a, a].real - pa) / pa), np.max(np.abs(ref['S'][a, a].imag)))
        for b in range(a + 1, nchan):
            pab = signal.csd(x[a], x[b], **kw)[1]
            worst = max(worst, np.max(np.abs(ref['S'][a, b] - pab) / np.sqrt(pa * signal.welch(x[b], **kw)[1])))
            worst = max(worst, np.max(np.abs(ref['S'][b, a] - np.conj(pab))))
    print('oracle against scipy csd / welch, C = %d: worst %.1e' % (nchan, worst))
    assert worst <= 1e-12
    if nchan == 2:
        kw.pop('scaling')
        coh = signal.coherence(x[0], x[1], **{k: v for k, v in kw.items() if k != 'return_onesided'})[1]
        err = np.max(np.abs(ref['gcoh'] - coh))
        print('C = 2 gcoh against scipy coherence: %.1e' % err)
        assert err <= 1e-12


# ---- 2. two identities -----------------------------------------------------------------------------------------------------------

def test_oracle_gcoh_ignores_per_channel_gains():
    rng = np.random.default_rng(7)
    x = noise(rng, (5, 128 * 12)) + 0.8 * noise(rng, 128 * 12)[None, :]
    gains = rng.uniform(0.01, 100.0, 5) * np.exp(2j * np.pi * rng.random(5))
    a, b = XO.matrix(x, 128, detrend=False), XO.matrix(x * gains[:, None], 128, detrend=False)
    err = np.max(np.abs(a['gcoh'] - b['gcoh']))
    print('gcoh under per-channel complex gains: %.1e' % err)
    assert err <= 1e-12
    assert np.max(np.abs(b['S'][1, 3] - np.conj(gains[1]) * gains[3] * a['S'][1, 3])) <= 1e-12 * np.max(np.abs(b['S'][1, 3]))


def test_oracle_null_mean_on_independent_noise():
    C, M, nfft = 4, 64, 256
    want = XO.null_mean(C, M)
    assert abs(want - (1.0 - 63.0 * 62.0 * 61.0 / 64.0 ** 3)) <= 1e-15 and XO.null_mean(2, M) == 1.0 / M
    assert XO.null_mean(4, 3) == 1.0 and XO.null_mean(3, 1) == 1.0
    # a rectangular window: no-overlap segments of white noise are independent and so are a segment's bins
    got = XO.matrix(noise(np.random.default_rng(3), (C, nfft * M)), nfft, window=np.ones(nfft), detrend=False)['gcoh'].mean()
    print('mean gcoh on independent noise, (C, M) = (4, 64): %.4f against %.4f' % (got, want))
    assert abs(got - want) <= 0.1 * want
    from ofdm_tools import ofdm_cr_tools as T
    for c, m in ((2, 1), (2, 7), (4, 3), (4, 64), (8, 12), (8, 200)):
        assert T.multiantenna_null_mean(c, m) == XO.null_mean(c, m)


def test_oracle_degenerate_rules():
    rng = np.random.default_rng(11)
    x = noise(rng, (3, 64 * 6))
    x[1] = 0.0
    r = XO.matrix(x, 64)
    assert not r['gcoh'].any() and not r['S'][1].any() and not r['S'][:, 1].any() and np.all(r['S'][0, 2] != 0)
    x[1] = noise(rng, 64 * 6)
    base = XO.matrix(x, 64)
    x[1, 100] = np.nan
    r = XO.matrix(x, 64)
    assert np.isnan(r['gcoh']).all() and np.isnan(r['S'][1]).all() and np.isnan(r['S'][:, 1]).all()
    assert np.array_equal(r['S'][0, 2], base['S'][0, 2]) and np.array_equal(r['S'][2, 2], base['S'][2, 2])
    one = XO.matrix(noise(rng, (4, 64)), 64, detrend=False)      # M = 1: rank one
    assert one['M'] == 1 and np.max(np.abs(one['gcoh'] - 1.0)) <= 1e-12
    few = XO.matrix(noise(rng, (4, 64 * 3)), 64)                 # M < C: singular
    assert few['M'] == 3 and np.max(np.abs(few['gcoh'] - 1.0)) <= 1e-9


# ---- 3. the detection condition ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1, 2])
def test_oracle_meets_the_detection_condition(seed):
    ref = XO.matrix(detection_capture(seed), DET_NFFT, detrend=False)
    assert ref['M'] == DET_M
    check_detection(np.fft.fftshift(ref['gcoh']), XO.null_mean(DET_C, DET_M), 'oracle, seed %d' % seed)
    off = XO.matrix(detection_capture(seed, signal=False), DET_NFFT, detrend=False)
    every = np.fft.fftshift(off['gcoh']).mean()
    assert abs(every - XO.null_mean(DET_C, DET_M)) <= 0.25 * XO.null_mean(DET_C, DET_M), every


# ---- 4. the helper's refusals, before a context exists --------------------------------------------------------------------------

def test_multiantenna_scan_refuses_in_python():
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros((4, 256 * 8), np.complex64)
    for nfft in (100, 32, 32768):
        with pytest.raises(ValueError) as ei:
            T.multiantenna_scan(x, nfft, 1.0)
        assert 'power of two' in str(ei.value)
    for bad in (x[0], x[:1], np.zeros((9, 2048), np.complex64)):
        with pytest.raises(ValueError) as ei:
            T.multiantenna_scan(bad, 256, 1.0)
        assert '2 ... 8 channels' in str(ei.value)
    with pytest.raises(ValueError) as ei:
        T.multiantenna_scan(x[:, :255], 256, 1.0)
    assert 'at least nFFT' in str(ei.value)
    with pytest.raises(ValueError) as ei:
        T.multiantenna_scan(x, 256, 0.0)
    assert 'Sf > 0' in str(ei.value)


def test_unpack_matrix_is_hermitian():
    from ofdm_tools import _hip
    packed = (np.arange(6 * 5) + 1j * np.arange(6 * 5)[::-1]).reshape(6, 5).astype(np.complex64)
    S = _hip.unpack_matrix(packed, 3)
    assert S.shape == (3, 3, 5) and S.dtype == np.complex64
    for k, (a, b) in enumerate(XO.pairs(3)):
        assert np.array_equal(S[a, b], packed[k]) and (a == b or np.array_equal(S[b, a], np.conj(packed[k])))


# ---- 5. surface, 6. resources --------------------------------------------------------------------------------------------------

def test_surface_is_declared_and_exported():
    check_surface(SYMBOLS, 'WelchPlan', ('matrix', 'matrix_dev'), ['float *s_out_dev, float *gcoh_out_dev, uint64_t *nseg_out);'])


def test_every_welch_mat_kernel_build_has_no_scratch():
    """the owned bins of up to 8 spectra and up to 64 running rows next to the butterflies, or both in memory where they do
    not fit: read from the code objects inside the built library, three builds (channel capacity 2, 4, 8) per power of two
    64 ... 16384 and the two finalize kernels, each with a private segment of 0 bytes and no spilled register; the
    1024-thread builds inside their 128 registers, the 512-thread builds inside 256."""
    check_builds('welch_mat_kernel', [(n, cc) for n in POWERS for cc in (2, 4, 8)], {64: 512, 256: 512, 512: 256, 1024: 128},
                 extra_kernels=('mat_finalize_kernel', 'mat_det_kernel'))
