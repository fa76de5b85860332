"""CPU checks of the adaptive-weight multitaper addition (no GPU): the float64 oracle (tests/mtm_adaptive_oracle.py) on its
fixed point and on the case the feature exists for, the chi-square quantile (no SciPy at run time) against SciPy and the
interval's coverage, the float32 emulation that sets the GPU gate, the ABI surface, and the resource figures of every
mtm_adapt_kernel build read from the code objects of the built library."""
import os
import re

import numpy as np
import pytest

import mtm_adaptive_oracle as AO
from stat_support import POWERS, check_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ('oth_mtm_set_ratios', 'oth_mtm_adaptive_dev', 'oth_mtm_adaptive')


@pytest.mark.parametrize('iters', [1, 4, 40])
def test_equal_eigenspectra_are_a_fixed_point(iters):
    """P_k = sigma^2 in every taper: b_k = 1, so S = sigma^2 and nu = 2 (sum lambda)^2 / sum lambda^2 whatever the count."""
    _, lam = AO.plan_tapers(256, 4.0, 7)
    sigma2 = np.array([0.37, 5.0])
    P = np.broadcast_to(sigma2[:, None, None], (2, 7, 256)).copy()
    S, nu = AO.iterate(P, sigma2, lam, iters)
    want = 2.0 * lam.sum() ** 2 / np.sum(lam * lam)
    assert np.max(np.abs(S / sigma2[:, None] - 1.0)) < 1e-14 and np.max(np.abs(nu / want - 1.0)) < 1e-14
    assert 13.9 < want < 14.0


def test_oracle_degenerate_bins_read_zero():
    _, lam = AO.plan_tapers(64, 2.0, 3)
    P = np.zeros((2, 3, 64))
    P[1, :, 5] = 1.0
    S, nu = AO.iterate(P, np.array([0.0, 1.0]), lam, 4)
    assert not S[0].any() and not nu[0].any() and S[1, 5] > 0 and nu[1, 5] > 2.0 and not S[1, :5].any() and not nu[1, :5].any()
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(nu))


def leakage_db(psd, nfft, nw, D):
    """mean of psd (natural order, density at fs = 1) over the bins more than 2 NW bins outside the band, in dB over the floor"""
    return 10.0 * np.log10(psd[AO.outside_band(nfft, nw)].mean()) + D


def test_adaptive_weights_see_the_floor_next_to_a_band():
    """The point of the feature: 1024 points, NW 4, K 7, one segment, the band capture at D = 40 without its tones (their
    own 2 NW-bin lobes are not floor).  Over the bins more than 2 NW bins outside the band the adaptive estimate at 4
    iterations reads the floor to 1.5 dB; the fixed unit weights sit at least 4 dB above it.  Measured: 0.53 dB and 8.0 dB
    (seed 1; 0.3 ... 1.0 and 4.2 ... 10.2 over seeds 0 ... 3)."""
    n, nw, K, D = 1024, 4.0, 7, 40.0
    x = AO.band_capture(n, 1, D)
    a = leakage_db(AO.adaptive(x, n, nw=nw, K=K, iters=4)['psd'], n, nw, D)
    u = leakage_db(AO.unity_psd(x, n, nw, K), n, nw, D)
    print('floor at -40 dB: adaptive %+.2f dB, unity %+.2f dB' % (a, u))
    assert abs(a) <= 1.5 and u >= 4.0


@pytest.mark.parametrize('nu', [2, 3.3, 14, 30.7, 400])
def test_chi2_quantile_against_scipy(nu):
    from scipy import stats
    from ofdm_tools import ofdm_cr_tools as T
    p = np.array([0.005, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 0.995])
    ref = stats.chi2.ppf(p, nu)
    got = T.chi2_quantile(p, nu)
    one = np.array([T.chi2_quantile(float(q), nu) for q in p[::4]])
    err = float(np.max(np.abs(got - ref) / ref))
    print('chi2_quantile nu = %g: %.2e' % (nu, err))
    assert err <= 1e-9 and np.array_equal(one, got[::4]) and isinstance(T.chi2_quantile(0.5, nu), float)


def test_chi2_quantile_closed_form_and_arguments():
    """nu = 2 is the exponential distribution: the p-quantile is -2 ln(1 - p)."""
    from ofdm_tools import ofdm_cr_tools as T
    assert abs(T.chi2_quantile(0.9, 2) + 2.0 * np.log(0.1)) <= 1e-12
    for bad in ((0.0, 2), (1.0, 2), (0.5, 0.0), (0.5, -1.0), (0.5, float('nan'))):
        with pytest.raises(ValueError):
            T.chi2_quantile(*bad)
    with pytest.raises(ValueError):
        T.mtm_adaptive_interval(np.ones(4), np.full(4, 14.0), 1, confidence=1.0)
    lo, hi = T.mtm_adaptive_interval(np.array([0.0, 2.0]), np.array([0.0, 14.0]), 3)      # a bin without degrees of freedom
    assert lo[0] == hi[0] == 0.0 and lo[1] < 2.0 < hi[1]


def test_interval_coverage_on_white_noise():
    """95 % intervals from the oracle's psd and dof on unit white noise (1024 points, NW 4, K 7, one segment, density at
    fs = 1: the truth is 1 in every bin but DC, where the mean came off) hold the truth in 0.90 ... 0.98 of the non-DC
    bins over seeds 0 ... 7.  Measured: 0.957 (0.944 ... 0.973 per seed)."""
    from ofdm_tools import ofdm_cr_tools as T
    n, hits = 1024, []
    for seed in range(8):
        rng = np.random.default_rng(seed)
        x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)
        r = AO.adaptive(x, n, nw=4.0, K=7, iters=4)
        lo, hi = T.mtm_adaptive_interval(r['psd'], r['dof'], r['nseg'], 0.95)
        hits.append(((lo <= 1.0) & (1.0 <= hi))[1:])
    cover = float(np.mean(hits))
    print('coverage of the 95 %% interval: %.3f' % cover)
    assert 0.90 <= cover <= 0.98


def test_float32_emulation_sets_the_gpu_gate():
    """The gates G_S and G_NU of the oracle module are 3 x the float32 emulation's worst over the GPU file's parity inputs
    (its docstring has the form and the figures); re-measured here, the emulation stays under a third of them - and not
    under a tenth: a gate that loose would be checking nothing."""
    g_s, at_s, g_nu, at_nu = AO.measure()
    print('emulation: worst G_S %.3e at %s, worst G_NU %.3e at %s; gates %.2e, %.2e' % (g_s, at_s, g_nu, at_nu, AO.G_S, AO.G_NU))
    assert AO.G_S / 10.0 < g_s <= AO.G_S / 3.0 and AO.G_NU / 10.0 < g_nu <= AO.G_NU / 3.0


def test_surface():
    """the three symbols: declared in the header, in the ctypes table, exported by the built library; the Python calls"""
    from ofdm_tools import _hip
    from ofdm_tools import ofdm_cr_tools as T
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ofdm_tools_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(oth_[a-z0-9_]+)\s*\(', src))
    for name in SYMBOLS:
        assert name in declared and name in _hip.SIGNATURES, name
    assert '#define OTH_ABI_VERSION 6 ' in src
    for name in ('set_ratios', 'adaptive', 'adaptive_dev'):
        assert hasattr(_hip.MtmPlan, name) and hasattr(_hip.MtmCsdPlan, name)
    assert not hasattr(_hip.WelchPlan, 'adaptive')
    for name in ('mtm_adaptive_estimate', 'chi2_quantile', 'mtm_adaptive_interval'):
        assert callable(getattr(T, name))
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    import subprocess
    out = subprocess.run(['nm', '-D', '--defined-only', _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert set(SYMBOLS) <= exported


def test_every_mtm_adaptive_kernel_build_has_no_scratch():
    """K eigenspectra per owned bin cannot be registers (K <= 64, indexed at run time): they sit in LDS up to 512 points and
    in a workspace row from 1024 on, and the iteration's sums are twelve to sixteen floats.  Read from the code objects
    inside the built library: one build per power of two 64 ... 16384, each with a private segment of 0 bytes and no
    spilled register; the 1024-thread build at 16384 points inside its 128 registers."""
    check_builds('mtm_adapt_kernel', POWERS, {1024: 128})
