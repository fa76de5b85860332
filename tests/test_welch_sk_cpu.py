"""CPU checks of the spectral kurtosis addition (no GPU): the float64 oracle (tests/welch_sk_oracle.py) on Gaussian noise
against the estimator's exact null moments, sk_limits (a Pearson type IV fit of those moments, no SciPy) against a seeded
Monte Carlo of the null, the refusals that happen in Python, and the resource figures of every welch_sk_kernel build read
from the code objects of the built library."""
import os

import numpy as np
import pytest

import welch_sk_oracle as SO
from stat_support import POWERS, check_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_on_noise_has_the_null_moments():
    """complex Gaussian noise, 64 points, M = 64, 4000 trials (boxcar, no overlap: every bin of every trial is one draw of
    the null): the mean of SK within 0.01 of 1, its variance within 5 % of mu2 = 4 M^2 / ((M - 1)(M + 2)(M + 3))."""
    from ofdm_tools import ofdm_cr_tools as T
    n, M, trials = 64, 64, 4000
    rng = np.random.default_rng(2024)
    sk = np.empty((trials, n))
    for t in range(trials):
        x = (rng.standard_normal(n * M) + 1j * rng.standard_normal(n * M)) / np.sqrt(2.0)
        sk[t] = SO.sk(x, n, window='boxcar', detrend=False)['SK']
    mu2 = T.sk_null_moments(M)[0]
    mean, var = float(sk.mean()), float(sk.var())
    print('oracle on noise: mean SK %.5f, variance %.5f against mu2 %.5f (%.3f)' % (mean, var, mu2, var / mu2))
    assert abs(mean - 1.0) <= 0.01 and abs(var / mu2 - 1.0) <= 0.05


def test_oracle_by_hand():
    """one bin, by hand: P = (1, 1, 1, 1) is a steady line, R = 1 and SK = 0; P = (4, 0, 0, 0) is a burst, R = 4 and
    SK = 5 / 3 * 3 = 5; an empty bin reads 0."""
    ref = SO.sk_of_rows(np.array([[1.0, 4.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]))
    assert ref['M'] == 4 and np.allclose(ref['R'], [1.0, 4.0, 0.0]) and np.allclose(ref['SK'], [0.0, 5.0, 0.0])
    assert np.allclose(SO.r_of_sk(ref['SK'][:2], 4), ref['R'][:2])


_null = {}


def null_draws(M):
    """10^6 seeded draws of the null: SK of M i.i.d. unit exponentials (a noise bin's periodograms).  Sorted, read-only."""
    if M not in _null:
        rng = np.random.default_rng(1000 + M)
        out = np.empty(1000000)
        for i in range(0, len(out), 50000):
            P = rng.standard_exponential((50000, M))
            s1 = P.sum(axis=1)
            out[i:i + 50000] = (M + 1.0) / (M - 1.0) * (M * (P * P).sum(axis=1) / (s1 * s1) - 1.0)
        out.sort()
        out.setflags(write=False)
        _null[M] = out
    return _null[M]


@pytest.mark.parametrize('M', [32, 64, 256])
@pytest.mark.parametrize('p', [1e-2, 1.35e-3])
def test_limits_against_a_monte_carlo_of_the_null(M, p):
    """The Monte Carlo is the truth (its own standard error: at most 3 % of p at 10^6 trials); the rate measured on each
    side lies in [0.5 p, 1.5 p].  Measured with the fit: 0.62 ... 1.06 of p, the worst the lower side at M = 64."""
    from ofdm_tools import ofdm_cr_tools as T
    lower, upper = T.sk_limits(M, p)
    draws = null_draws(M)
    below = np.searchsorted(draws, lower, side='left') / float(len(draws))
    above = (len(draws) - np.searchsorted(draws, upper, side='right')) / float(len(draws))
    print('sk_limits(%d, %g) = (%.4f, %.4f): rates %.3f / %.3f of p' % (M, p, lower, upper, below / p, above / p))
    assert 0.0 < lower < 1.0 < upper
    assert 0.5 * p <= below <= 1.5 * p and 0.5 * p <= above <= 1.5 * p


def test_limits_arguments():
    from ofdm_tools import ofdm_cr_tools as T
    for M in (2, 16, 31):
        with pytest.raises(ValueError) as ei:
            T.sk_limits(M, 1e-3)
        assert '32' in str(ei.value)
    for p in (0.0, 1.0, -1e-3, 1.5):
        with pytest.raises(ValueError):
            T.sk_limits(64, p)
    with pytest.raises(ValueError):
        T.sk_limits(64.5, 1e-3)
    lo1, hi1 = T.sk_limits(64, 1e-3)
    lo2, hi2 = T.sk_limits(1024, 1e-3)
    assert lo1 < lo2 < 1.0 < hi2 < hi1                    # the limits close in on 1 with more segments
    assert abs(lo1 - 0.48) < 0.02 and abs(hi1 - 2.23) < 0.05      # M = 64 at 1e-3 per side


def test_surface_and_python_level_refusals():
    """the entry points are declared, and sk_scan refuses in Python - before a context exists - what sk_limits or the
    kernel list cannot serve"""
    from ofdm_tools import _hip
    from ofdm_tools import ofdm_cr_tools as T
    for name in ('oth_welch_sk', 'oth_welch_sk_dev'):
        assert name in _hip.SIGNATURES
    for name in ('sk', 'sk_dev'):
        assert hasattr(_hip.WelchPlan, name)
    header = open(os.path.join(ROOT, 'include', 'ofdm_tools_hip.h')).read()
    assert 'int oth_welch_sk_dev(' in header and 'int oth_welch_sk(' in header
    x = np.zeros(256 * 64, np.complex64)
    for nfft in (100, 32, 32768):
        with pytest.raises(ValueError) as ei:
            T.sk_scan(x, nfft, 1.0)
        assert 'power of two' in str(ei.value)
    with pytest.raises(ValueError) as ei:
        T.sk_scan(x[:256 * 31], 256, 1.0)                 # 31 segments
    assert '32' in str(ei.value)
    with pytest.raises(ValueError):
        T.sk_scan(x, 256, 1.0, p_false=0.0)


def test_every_welch_sk_kernel_build_has_no_scratch():
    """Two running sums per owned bin next to the butterflies: read from the code objects inside the built library, one
    build per power of two 64 ... 16384, each with a private segment of 0 bytes and no spilled register; the 1024-thread
    build at 16384 points inside its 128 registers."""
    check_builds('welch_sk_kernel', POWERS, {1024: 128})
