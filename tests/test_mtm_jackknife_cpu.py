"""CPU checks of the multitaper jackknife addition (no GPU): the surface, the Student-t quantile without SciPy against
SciPy, the float64 oracle (tests/mtm_jackknife_oracle.py) against the literal delete-one form and on what the feature exists
for - the share of bins whose interval holds the truth - and the resource figures of every mtm_jack_kernel and
mtmcsd_jack_kernel build read from the code objects of the built library."""
import math

import numpy as np
import pytest

import mtm_jackknife_oracle as JO
from stat_support import POWERS, check_builds


def white(n, seed):
    """unit-variance complex white noise, float64"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)


def test_surface():
    from ofdm_tools import _hip
    for name in ('oth_mtm_jackknife', 'oth_mtm_jackknife_dev', 'oth_mtm_csd_jackknife', 'oth_mtm_csd_jackknife_dev'):
        assert name in _hip.SIGNATURES
    for name in ('jackknife', 'jackknife_dev'):
        assert hasattr(_hip.MtmPlan, name) and hasattr(_hip.MtmCsdPlan, name) and not hasattr(_hip.WelchPlan, name)
    for name in ('csd_jackknife', 'csd_jackknife_dev'):
        assert hasattr(_hip.MtmCsdPlan, name) and not hasattr(_hip.WelchPlan, name)


@pytest.mark.parametrize('dof', [1, 2, 6, 27, 2047])
def test_t_quantile_against_scipy(dof):
    from scipy import stats
    from ofdm_tools import ofdm_cr_tools as T
    worst = 0.0
    for p in (0.25, 0.1, 0.05, 0.025, 0.005, 1e-3, 1e-4, 1e-6, 1e-9):
        got, ref = T.student_t_quantile(p, dof), float(stats.t.isf(p, dof))
        worst = max(worst, abs(got - ref) / ref)
        assert abs(got - ref) <= 1e-9 * ref, (dof, p, got, ref)
    print('student_t_quantile dof %d: %.2e' % (dof, worst))


def test_t_quantile_closed_form_and_arguments():
    """t(1) is Cauchy: isf(p) = cot(pi p)."""
    from ofdm_tools import ofdm_cr_tools as T
    for p in (0.25, 0.01, 1e-6):
        ref = 1.0 / math.tan(math.pi * p)
        assert abs(T.student_t_quantile(p, 1) - ref) <= 1e-9 * ref
    assert T.student_t_quantile(0.5, 3) == 0.0 and T.student_t_quantile(0.9, 3) == -T.student_t_quantile(1.0 - 0.9, 3)
    for bad in ((0.0, 5), (1.0, 5), (-0.1, 5), (0.05, 0), (0.05, 0.5)):
        with pytest.raises(ValueError):
            T.student_t_quantile(*bad)


def test_oracle_equals_the_literal_delete_one_form():
    """log1p(-p_i / S) = ln((S - p_i) / (M - 1)) + a constant of the bin: the two variances agree to 1e-10, over several
    segments and with zero padding."""
    for nfft, nperseg, ov, nseg, nw, K in ((256, 256, 50, 3, 2.5, 4), (512, 300, 0, 2, 3, 5), (1024, 1024, 0, 1, 4, 7)):
        noverlap = nperseg * ov // 100
        x = white(noverlap + nseg * (nperseg - noverlap) + 7, 5 + nfft) + 0.3 - 0.1j
        X, c = JO.items(x, nfft, nperseg=nperseg, noverlap=noverlap, nw=nw, K=K)
        p = c[:, None] * np.abs(X) ** 2
        assert p.shape == (nseg * K, nfft)
        a, b = JO.lnpsd(p)[0], JO.lnpsd_literal(p)
        err = float(np.max(np.abs(a - b) / b))
        print('jackknife oracle, log1p form against the literal form %s: %.2e' % ((nfft, nperseg, ov, nseg, nw, K), err))
        assert err < 1e-10


def psd_coverage(n, nw, K, nseg, seed, confidence=0.95):
    """share of the non-DC bins whose interval psd exp(-+ q lnsd) holds the true density of unit white noise (fs = 1: 1)"""
    from ofdm_tools import ofdm_cr_tools as T
    x = white(n * nseg, seed)
    r = JO.jackknife(x, n, nw=nw, K=K)
    psd = r['S'] / nseg
    q = T.student_t_quantile(0.5 * (1.0 - confidence), r['M'] - 1)
    inside = (psd * np.exp(-q * r['lnsd']) <= 1.0) & (1.0 <= psd * np.exp(q * r['lnsd']))
    return float(np.mean(inside[1:]))


@pytest.mark.parametrize('n,nw,K,nseg', [(1024, 4.0, 7, 1), (256, 2.5, 4, 3)])
def test_psd_interval_covers_the_truth(n, nw, K, nseg):
    """What the feature exists for, on the oracle: unit complex white noise, whose true density is the plan's level; over
    seeds 0 ... 7 the 95 % interval holds it in 90 ... 99 % of the non-DC bins (the DC bin is the detrend's)."""
    got = [psd_coverage(n, nw, K, nseg, seed) for seed in range(8)]
    print('psd coverage at %s: %s' % ((n, nw, K, nseg), ' '.join('%.3f' % g for g in got)))
    assert all(0.90 <= g <= 0.99 for g in got), got


def test_coherence_interval_covers_the_truth():
    """y = x + independent unit noise: the true magnitude-squared coherence is 0.5 in every bin.  The two-sided 95 % interval
    on z = atanh|gamma| holds atanh(sqrt(0.5)) in 90 ... 99 % of the bins over seeds 0 ... 7.  A true coherence of 0 is NOT
    covered at that rate - |gamma| is biased upwards there, and z cannot go below 0 - and is not tested."""
    from ofdm_tools import ofdm_cr_tools as T
    n, truth, got = 1024, math.atanh(math.sqrt(0.5)), []
    for seed in range(8):
        x = white(n, seed)
        y = x + white(n, 1000 + seed)
        r = JO.csd_jackknife(x, y, n, nw=4.0, K=7)
        q = T.student_t_quantile(0.025, r['M'] - 1)
        got.append(float(np.mean(np.abs(r['z'] - truth) <= q * r['zsd'])))
    print('coherence coverage: %s' % ' '.join('%.3f' % g for g in got))
    assert all(0.90 <= g <= 0.99 for g in got), got


def test_every_jackknife_kernel_build_has_no_scratch():
    """Two (one channel) or six (two channels) floats of state per owned bin next to the butterflies and a log1p / atanh per
    bin: read from the code objects inside the built library, one build per power of two 64 ... 16384 of each kernel, each
    with a private segment of 0 bytes and no spilled register; the 1024-thread builds inside their 128 registers."""
    check_builds('mtm_jack_kernel', POWERS, {1024: 128})
    check_builds('mtmcsd_jack_kernel', POWERS, {1024: 128})
