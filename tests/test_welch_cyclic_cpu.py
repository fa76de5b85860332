"""CPU checks of the cyclic spectrum / cyclic coherence addition (no GPU): the float64 oracle by the definition
(tests/welch_cyclic_oracle.py) on its identities and on a CP-OFDM signal, the Python helpers, the declared surface, and the
resource figures of every welch_cyc_kernel build read from the code objects of the built library."""
import numpy as np
import pytest

import welch_cyclic_oracle as CO
from stat_support import POWERS, check_builds, check_surface

SYMBOLS = ('oth_welch_set_cycles', 'oth_welch_cyclic_dev', 'oth_welch_cyclic')
TU, TCP, NFFT, M = 64, 16, 256, 60
ON = (1.0 / 80.0, -1.0 / 80.0)
OFF = (1.0 / 77.0, 1.0 / 80.0 + 1.0 / (M * NFFT))      # another period; one resolution cell 1 / (M step) off the true one


def cp_ofdm(seed, nsamples=NFFT * M, tu=TU, tcp=TCP, used=48, snr_db=20.0, signal=True):
    """CP-OFDM, `used` QPSK carriers around an empty DC carrier of a tu-point symbol with a tcp-sample prefix, unit power
    times snr_db, over unit complex noise -> complex64 [nsamples].  signal=False: the noise alone."""
    rng = np.random.default_rng(seed)
    nsym = -(-nsamples // (tu + tcp))
    k = np.r_[1:used // 2 + 1, tu - used // 2:tu]
    S = np.zeros((nsym, tu), np.complex128)
    S[:, k] = ((2 * rng.integers(0, 2, (nsym, used)) - 1) + 1j * (2 * rng.integers(0, 2, (nsym, used)) - 1)) / np.sqrt(2.0)
    s = np.fft.ifft(S, axis=1) * tu / np.sqrt(used)
    s = np.concatenate([s[:, tu - tcp:], s], axis=1).reshape(-1)[:nsamples]
    w = (rng.standard_normal(nsamples) + 1j * rng.standard_normal(nsamples)) / np.sqrt(2.0)
    return ((10.0 ** (snr_db / 20.0) * s if signal else 0.0) + w).astype(np.complex64)


def check_detection(prof_on, prof_off, what=''):
    """the on / off conditions of the CP-OFDM case: every on-cycle profile entry at least 5 x every off-cycle one, and the
    off-cycle entries at the null level, at most 2.5 / M"""
    print('cyclic profile %s: on %s, off %s, null 1 / M = %.4f' % (what, np.round(prof_on, 4), np.round(prof_off, 4), 1.0 / M))
    assert min(prof_on) >= 5.0 * max(prof_off), (prof_on, prof_off)
    assert max(prof_off) <= 2.5 / M, prof_off


def test_oracle_alpha_zero_is_the_psd():
    x = cp_ofdm(5, 256 * 7 + 40)
    for kw in (dict(), dict(nperseg=200, noverlap=100, detrend=False, scaling='raw')):
        ref = CO.cyclic(x, 256, [0.0], **kw)
        assert np.max(np.abs(ref['coh'][0] - 1.0)) <= 1e-12
        assert np.max(np.abs(ref['scf'][0] - ref['psd'])) <= 1e-12 * ref['psd'].max()


@pytest.mark.parametrize('m', [1, -3, 17])
def test_oracle_integer_bin_shift_rolls_the_spectrum(m):
    """alpha = m / nfft: U_s[j] = e^{-j phase_s} X_s[j + m], so Suu = roll(Sxx, -m)"""
    nfft = 128
    x = cp_ofdm(9, nfft * 11)
    ref = CO.cyclic(x, nfft, [m / float(nfft)], noverlap=nfft // 2)
    err = np.max(np.abs(ref['Suu'][0] - np.roll(ref['Sxx'], -m))) / ref['Sxx'].max()
    print('Suu against roll(Sxx, %d): %.1e' % (-m, err))
    assert err <= 1e-12


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_oracle_detects_cp_ofdm_at_its_cycle_frequencies_only(seed):
    x = cp_ofdm(seed)
    prof = CO.profile(x, NFFT, ON + OFF)
    check_detection(prof[:2], prof[2:], 'seed %d' % seed)
    noise = CO.profile(cp_ofdm(seed, signal=False), NFFT, ON + OFF)
    print('noise alone: %s' % np.round(noise, 4))
    assert max(noise) <= 2.5 / M


def test_ofdm_cycle_frequencies():
    from ofdm_tools import ofdm_cr_tools as T
    f = T.ofdm_cycle_frequencies(64, 16, 20e6)
    assert f.dtype == np.float64 and np.allclose(f, [250e3, -250e3, 500e3, -500e3], rtol=1e-15)
    assert np.allclose(T.ofdm_cycle_frequencies(2048, 144, 30.72e6, harmonics=1), [30.72e6 / 2192, -30.72e6 / 2192], rtol=1e-15)
    assert len(T.ofdm_cycle_frequencies(64, 16, 1.0, harmonics=3)) == 6
    for bad in ((0, 16, 1.0), (64, 0, 1.0), (64, 16, 0.0), (64, 16, 1.0, 0)):
        with pytest.raises(ValueError):
            T.ofdm_cycle_frequencies(*bad)


def test_cyclic_scan_refuses_in_python():
    """before a context exists: a bad size, an empty or oversized cycle list, |cycle| > Sf / 2, a non-finite cycle, a capture
    shorter than one segment"""
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros(256 * 8, np.complex64)
    for nfft in (100, 32, 32768):
        with pytest.raises(ValueError) as ei:
            T.cyclic_scan(x, nfft, 1.0, [0.0125])
        assert 'power of two' in str(ei.value)
    for cycles in ([], np.zeros(65)):
        with pytest.raises(ValueError) as ei:
            T.cyclic_scan(x, 256, 1.0, cycles)
        assert '64' in str(ei.value)
    for cycles in ([0.0125, 0.51], [-1.1e6], [float('nan')], [float('inf')]):
        with pytest.raises(ValueError) as ei:
            T.cyclic_scan(x, 256, 2.0e6 if abs(cycles[0]) > 1 else 1.0, cycles)
        assert 'Sf / 2' in str(ei.value)
    with pytest.raises(ValueError):
        T.cyclic_scan(x[:255], 256, 1.0, [0.0125])


def test_surface_is_declared_and_exported():
    check_surface(SYMBOLS, 'WelchPlan', ('set_cycles', 'cyclic', 'cyclic_dev'))


def test_every_welch_cyc_kernel_build_has_no_scratch():
    """1 + 3 GA running sums per owned bin next to the butterflies (or the partial rows where they do not fit): read from the
    code objects inside the built library, three builds (GA = 1, 2, 4) per power of two 64 ... 16384, each with a private segment
    of 0 bytes and no spilled register; the 1024-thread builds inside their 128 registers."""
    check_builds('welch_cyc_kernel', [(n, ga) for n in POWERS for ga in (1, 2, 4)], {1024: 128})
