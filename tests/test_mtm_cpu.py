"""CPU checks of the multitaper additions (no GPU): oth_dpss against scipy.signal.windows.dpss, the Python surface's
argument checks, and the resource figures of every mtm_kernel build read from the code objects of the built library."""
import ctypes
import os
import sys

import numpy as np
import pytest

from stat_support import POWERS, check_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

DPSS_CASES = [(64, 2, 3), (256, 2.5, 4), (1000, 3.5, 6), (4096, 4, 7), (4096, 4, 8), (16384, 4, 7), (16384, 8, 15)]
# Largest absolute difference to SciPy over DPSS_CASES as measured: tapers 2.3e-12 at (16384, 4, 7),
# concentration ratios 1.4e-14 at (16384, 8, 15).  Asserted at ten times that; the plans use the tapers as float32
# (epsilon 1.2e-7), so neither bound may ever be looser than 1e-7.
TAPER_ATOL = 10 * 2.3e-12
RATIO_ATOL = 10 * 1.4e-14
assert TAPER_ATOL <= 1e-7 and RATIO_ATOL <= 1e-7


def _lib():
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet (run __graft_entry__.build())')
    return _hip.load()


def _dpss(lib, n, nw, kmax, want_ratios=True):
    dp = ctypes.POINTER(ctypes.c_double)
    tapers = np.full((max(kmax, 1), max(n, 1)), np.nan)
    ratios = np.full(max(kmax, 1), np.nan)
    rc = lib.oth_dpss(n, nw, kmax, tapers.ctypes.data_as(dp), ratios.ctypes.data_as(dp) if want_ratios else None)
    return rc, tapers, ratios


@pytest.mark.parametrize('n,nw,kmax', DPSS_CASES)
def test_oth_dpss_matches_scipy(n, nw, kmax):
    from scipy.signal.windows import dpss
    lib = _lib()
    rc, tapers, ratios = _dpss(lib, n, float(nw), kmax)
    assert rc == 0
    ref, ref_ratios = dpss(n, nw, kmax, return_ratios=True)
    dt, dr = np.max(np.abs(tapers - ref)), np.max(np.abs(ratios - ref_ratios))
    gram = np.max(np.abs(tapers @ tapers.T - np.eye(kmax)))
    print('dpss(%d, %g, %d): tapers %.2e ratios %.2e gram %.2e' % (n, nw, kmax, dt, dr, gram))
    assert dt <= TAPER_ATOL and dr <= RATIO_ATOL
    # signs: SciPy's convention, checked on the definition and entry by entry wherever SciPy's value is not rounding noise
    thresh = max(1e-7, 1.0 / n)
    for k in range(kmax):
        if k % 2 == 0:
            assert tapers[k].sum() > 0
        else:
            assert tapers[k][tapers[k] ** 2 > thresh][0] > 0
    big = np.abs(ref) > 1e-9
    assert np.array_equal(np.sign(tapers[big]), np.sign(ref[big]))
    assert gram <= 1e-10
    # by falling concentration (the leading ones equal 1 to rounding)
    assert np.all(np.diff(ratios) < 1e-12) and np.all(ratios > 0) and np.all(ratios < 1 + 1e-12)
    # ratios == NULL leaves the tapers the same
    rc2, tapers2, _ = _dpss(lib, n, float(nw), kmax, want_ratios=False)
    assert rc2 == 0 and np.array_equal(tapers, tapers2)


def test_oth_dpss_refuses_invalid_arguments():
    lib = _lib()
    lib.oth_last_error.restype = ctypes.c_char_p
    for n, nw, kmax in ((1, 0.25, 1), (0, 1.0, 1), (-5, 1.0, 1), (64, 0.0, 3), (64, -1.0, 3), (64, 32.0, 3), (64, 40.0, 3),
                        (64, float('nan'), 3), (64, float('inf'), 3), (64, 2.0, 0), (64, 2.0, 65), (64, 2.0, -1)):
        rc, tapers, _ = _dpss(lib, n, nw, kmax)
        assert rc == -1, (n, nw, kmax, rc)
        assert b'oth_dpss' in lib.oth_last_error(None)
        assert np.all(np.isnan(tapers))                     # nothing written
    assert lib.oth_dpss(64, 2.0, 3, None, None) == -1
    rc, tapers, _ = _dpss(lib, 2, 0.5, 2)                   # the smallest problem: (1, 1) / sqrt 2 and (1, -1) / sqrt 2
    assert rc == 0 and np.allclose(np.abs(tapers), np.sqrt(0.5), atol=1e-15) and tapers[0].sum() > 0
    rc, tapers, _ = _dpss(lib, 64, 31.9, 64)                # kmax = n, nw just below n / 2
    assert rc == 0 and np.max(np.abs(tapers @ tapers.T - np.eye(64))) < 1e-10


def test_windows_dpss_shapes_and_dtypes():
    from ofdm_tools import windows
    _lib()
    t = windows.dpss(1000, 3.5, 6)
    assert isinstance(t, np.ndarray) and t.shape == (6, 1000) and t.dtype == np.float64
    t2, r = windows.dpss(1000, 3.5, 6, return_ratios=True)
    assert np.array_equal(t, t2) and r.shape == (6,) and r.dtype == np.float64
    assert np.allclose(np.sum(t * t, axis=1), 1.0, atol=1e-13)
    assert windows.dpss(64, 2, 1).shape == (1, 64)
    for bad in ((1, 0.25, 1), (64, 0, 3), (64, 32, 3), (64, 2, 0), (64, 2, 65)):
        with pytest.raises(ValueError):
            windows.dpss(*bad)


def test_bad_weights_and_unknown_scan_method_raise_before_the_library_is_called():
    """No context, no GPU: Context.mtm_plan checks its weights (and the taper table's shape) before anything touches the
    library, and SpectrumScan still refuses a method it does not know."""
    from ofdm_tools import _hip
    from ofdm_tools import ofdm_cr_tools as T

    class NoLibrary(object):
        """stands in for the context: any use of it is an error"""
        def __getattr__(self, name):
            raise AssertionError('the library was reached: ' + name)

    plan = _hip.Context.mtm_plan
    for bad in ([1, 1, -1, 1, 1, 1, 1], [0] * 7, [1, 1, 1], [1, 1, 1, float('nan'), 1, 1, 1], [float('inf')] + [1] * 6,
                'eigenvalues', np.ones((7, 1))):
        with pytest.raises(ValueError):
            plan(NoLibrary(), 1024, nw=4.0, weights=bad)
    with pytest.raises(ValueError):
        plan(NoLibrary(), 1024, tapers=np.ones((3, 1024), np.float32), weights='eigen')      # no ratios for foreign tapers
    with pytest.raises(ValueError):
        plan(NoLibrary(), 1024, tapers=np.ones((3, 1000), np.float32))
    with pytest.raises(ValueError):
        plan(NoLibrary(), 1024, nw=0.5)                                                       # int(2 nw) - 1 = 0 tapers
    assert _hip.mtm_weights('unity', 7) is None and _hip.mtm_weights('eigen', 7) == 'eigen'
    w = _hip.mtm_weights([1, 2, 3], 3)
    assert w.dtype == np.float32 and np.array_equal(w, [1, 2, 3])
    for method in ('mtm ', 'multitaper', 'median', None):
        with pytest.raises(ValueError):
            T.SpectrumScan(np.zeros(2048, np.complex64), 0, 50e3, 25e3, 1024, 1e6, method, 5, 1, ctx=NoLibrary())
    assert set(T.SpectrumScan._ENQUEUE) == {'welch', 'fft', 'mtm'}


def test_every_mtm_kernel_build_has_no_scratch():
    """The taper loop keeps its accumulators (and, below 16384 points, the detrended samples) in registers across the
    transforms of a run: a spilled register would come back at memory latency K times per segment.  Read from the code
    objects inside the built library: one build per power of two 64 ... 16384, each with a private segment of 0 bytes."""
    check_builds('mtm_kernel', POWERS, {1024: 128})      # 1024 threads: four waves per SIMD
