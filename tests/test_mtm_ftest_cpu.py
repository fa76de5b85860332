"""CPU checks of the harmonic F-test addition (no GPU): the threshold (the F quantile without SciPy) against SciPy, the
float64 oracle (tests/mtm_ftest_oracle.py) against itself and on the case the feature exists for, and the resource
figures of every mtm_ftest_kernel build read from the code objects of the built library."""
import numpy as np
import pytest

import mtm_ftest_oracle as FO
from stat_support import POWERS, check_builds


@pytest.mark.parametrize('nseg,K,p', [(1, 7, 1e-3), (1, 2, 1e-2), (1, 3, 1e-5), (4, 7, 1e-6), (20, 3, 1e-4), (2047, 4, 1e-9)])
def test_threshold_is_the_f_quantile(nseg, K, p):
    from scipy import stats
    from ofdm_tools import ofdm_cr_tools as T
    got, ref = T.ftest_threshold(p, nseg, K), float(stats.f.isf(p, 2 * nseg, 2 * nseg * (K - 1)))
    print('ftest_threshold %s: %.12g against %.12g, %.2e' % ((nseg, K, p), got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-9 * ref


def test_threshold_closed_form_and_arguments():
    """F(2, 2): P(F > f) = 1 / (1 + f), so the 1 % point is exactly 99."""
    from ofdm_tools import ofdm_cr_tools as T
    assert abs(T.ftest_threshold(0.01, 1, 2) - 99.0) <= 1e-9 * 99.0
    for bad in ((0.0, 1, 7), (1.0, 1, 7), (1e-3, 0, 7), (1e-3, 1, 1)):
        with pytest.raises(ValueError):
            T.ftest_threshold(*bad)


def test_surface():
    from ofdm_tools import _hip
    for name in ('oth_mtm_ftest', 'oth_mtm_ftest_dev'):
        assert name in _hip.SIGNATURES
    for name in ('ftest', 'ftest_dev', 'dof'):
        assert hasattr(_hip.MtmPlan, name) and hasattr(_hip.MtmCsdPlan, name)
    assert not hasattr(_hip.WelchPlan, 'ftest')


def test_oracle_definition_equals_its_subtracted_form():
    """sum_k |y_k - mu U_k|^2 = sum_k |y_k|^2 - S |mu|^2 (U_k real): the two forms of the oracle agree to 1e-10 of
    num + den, on several segments, zero padding and a strong line included."""
    def noise_tones(n, seed, tones):
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
        for a, f in tones:
            x = x + a * np.exp(2j * np.pi * f * np.arange(n))
        return (x + 0.3 - 0.1j).astype(np.complex64)

    for nfft, nperseg, ov, nseg, nw, K in ((256, 256, 50, 3, 2.5, 4), (512, 300, 0, 2, 3, 5), (1024, 1024, 0, 1, 4, 7)):
        noverlap = nperseg * ov // 100
        x = noise_tones(noverlap + nseg * (nperseg - noverlap) + 7, 5 + nfft, tones=((100.0, 0.125), (0.5, -0.31)))
        a = FO.ftest(x, nfft, nperseg, noverlap, nw, K)
        b = FO.ftest(x, nfft, nperseg, noverlap, nw, K, subtracted=True)
        err = float(np.max(np.abs(a['den'] - b['den']) / (a['num'] + a['den'])))
        print('ftest oracle, definition against subtracted form %s: %.2e' % ((nfft, nperseg, ov, nseg, nw, K), err))
        assert a['nseg'] == nseg and err < 1e-10 and np.array_equal(a['num'], b['num'])


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_oracle_finds_the_line_on_the_hump(seed):
    """1024 points, NW 4, K 7, one segment: a line of amplitude 4 on a hump 20 dB over the floor and one of 0.5 on the
    floor both stand at least 1.5 x over the 1e-3 / 1024 threshold (54.2), and every bin farther than 4 from a line stays
    under half of it."""
    from ofdm_tools import ofdm_cr_tools as T
    n = 1024
    thr = T.ftest_threshold(1e-3 / n, 1, 7)
    assert abs(thr - 54.2) < 0.05
    F = FO.ftest(FO.hump_capture(seed, n), n, nw=4.0, K=7)['F']
    k = np.arange(n)
    far = np.ones(n, bool)
    for b in FO.HUMP_LINES:
        far &= np.abs((k - b + n // 2) % n - n // 2) > 4
    print('hump seed %d: F %.1f / %.1f at the lines, %.1f at most elsewhere' % (seed, F[200], F[-300], F[far].max()))
    assert min(F[200], F[-300]) >= 1.5 * thr and F[far].max() <= 0.5 * thr


def test_every_mtm_ftest_kernel_build_has_no_scratch():
    """Five floats of state per owned bin next to the butterflies: read from the code objects inside the built library,
    one build per power of two 64 ... 16384, each with a private segment of 0 bytes and no spilled register; the
    1024-thread build at 16384 points inside its 128 registers."""
    check_builds('mtm_ftest_kernel', POWERS, {1024: 128})
