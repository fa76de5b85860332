"""CPU checks of the two-channel multitaper addition (no GPU): the float64 oracle (tests/mtm_csd_oracle.py) against
SciPy and against the one-channel oracle, the declared surface, the Python argument checks, and the resource figures of
every mtmcsd_kernel build read from the code objects of the built library."""
import os
import re

import numpy as np
import pytest

import mtm_csd_oracle as MC
import mtm_oracle as O
from stat_support import POWERS, check_builds
from oracle import ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ofdm_tools_hip.h')


def _pair(n, seed):
    x = R.synth_iq(n, seed, dc=2 - 1j)
    y = (0.7 * np.roll(x, 5) + 0.5 * R.synth_iq(n, seed + 1000, tones=(), dc=0.5 + 0.25j)).astype(np.complex64)
    return x, y


def test_oracle_with_one_hann_taper_is_scipy():
    """256 points, 50 % overlap, 5 segments, constant detrend, two-sided: one taper and unit weight is the Welch estimate
    of that window."""
    from scipy import signal
    n, noverlap, fs = 256, 128, 2.5e6
    x, y = _pair(noverlap + 5 * (n - noverlap), 11)
    x, y = x.astype(np.complex128), y.astype(np.complex128)
    w = signal.get_window('hann', n)
    kw = dict(fs=fs, window=w, nperseg=n, noverlap=noverlap, nfft=n, detrend='constant', return_onesided=False)
    for scaling in ('density', 'raw'):
        pxx, pyy, pxy, cxy = MC.mtm_csd(x, y, n, noverlap=noverlap, tapers=w[None, :], scaling=scaling, fs=fs)
        k = 1.0 if scaling == 'density' else fs * np.sum(w * w)      # 'raw': the unscaled sums over nseg
        _, sxy = signal.csd(x, y, scaling='density', **kw)
        _, sxx = signal.welch(x, scaling='density', **kw)
        _, syy = signal.welch(y, scaling='density', **kw)
        _, sc = signal.coherence(x, y, **{q: v for q, v in kw.items() if q not in ('return_onesided',)})
        e = (np.max(np.abs(pxx - k * sxx) / (k * sxx)), np.max(np.abs(pyy - k * syy) / (k * syy)),
             np.max(np.abs(pxy - k * sxy) / np.sqrt(k * sxx * k * syy)), np.max(np.abs(cxy - sc)))
        print('mtm csd oracle against scipy (%s): Pxx %.2e Pyy %.2e Pxy %.2e Cxy %.2e' % ((scaling,) + e))
        assert max(e) < 1e-12


def test_oracle_with_identical_channels_is_the_one_channel_oracle():
    for nfft, nperseg, ov, nseg, nw, K, weights, scaling in ((256, 256, 50, 3, 2.5, 4, 'eigen', 'density'),
                                                             (512, 300, 0, 2, 3, 5, 'unity', 'over_n2'),
                                                             (1024, 1024, 0, 1, 4, None, 'unity', 'raw')):
        noverlap = nperseg * ov // 100
        x, _ = _pair(noverlap + nseg * (nperseg - noverlap) + 7, 5 + nfft)
        pxx, pyy, pxy, cxy = MC.mtm_csd(x, x, nfft, nperseg, noverlap, nw, K, weights, True, scaling, 3.0)
        ref = O.mtm_psd(x, nfft, nperseg, noverlap, nw, K, weights, True, scaling, 3.0)
        e = np.max(np.abs(pxx - ref) / ref)
        print('mtm csd oracle against mtm_psd %s: %.2e' % ((nfft, nperseg, ov, nseg, nw, K), e))
        assert e < 1e-12 and np.array_equal(pxx, pyy)
        assert np.max(np.abs(pxy - pxx) / pxx) < 1e-12 and np.max(np.abs(cxy - 1.0)) < 1e-12


def test_header_and_signatures_declare_the_constructor():
    from ofdm_tools import _hip
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    decl = re.search(r'int oth_mtm_csd_plan\(([^;]*)\);', src)
    ref = re.search(r'int oth_mtm_plan\(([^;]*)\);', src)
    assert decl and ref and ' '.join(decl.group(1).split()) == ' '.join(ref.group(1).split())      # the same arguments
    assert _hip.SIGNATURES['oth_mtm_csd_plan'] == _hip.SIGNATURES['oth_mtm_plan']
    assert '#define OTH_ABI_VERSION 6' in ' '.join(open(HEADER).read().split()).replace('  ', ' ')
    assert issubclass(_hip.MtmCsdPlan, _hip.MtmPlan)
    for name in ('csd', 'csd_exec_dev', 'csd_partial_dev', 'csd_scale_dev'):
        assert hasattr(_hip.MtmCsdPlan, name)


def test_bad_arguments_raise_before_the_library_is_called():
    """No context, no GPU: Context.mtm_csd_plan has Context.mtm_plan's checks, and coherence_estimator refuses a method
    it does not know - and a block shorter than one segment under 'mtm' - before anything touches the library."""
    import ofdm_tools
    from ofdm_tools import _hip

    class NoLibrary(object):
        """stands in for the context: any use of it is an error"""
        def __getattr__(self, name):
            raise AssertionError('the library was reached: ' + name)

    plan = _hip.Context.mtm_csd_plan
    for bad in ([1, 1, -1, 1, 1, 1, 1], [0] * 7, [1, 1, 1], [1, 1, 1, float('nan'), 1, 1, 1], [float('inf')] + [1] * 6,
                'eigenvalues', np.ones((7, 1))):
        with pytest.raises(ValueError):
            plan(NoLibrary(), 1024, nw=4.0, weights=bad)
    with pytest.raises(ValueError):
        plan(NoLibrary(), 1024, tapers=np.ones((3, 1024), np.float32), weights='eigen')      # no ratios for foreign tapers
    with pytest.raises(ValueError):
        plan(NoLibrary(), 1024, tapers=np.ones((3, 1000), np.float32))
    with pytest.raises(ValueError):
        plan(NoLibrary(), 1024, tapers=np.ones((3, 1024), np.float32), ntapers=4)
    with pytest.raises(ValueError):
        plan(NoLibrary(), 1024, nw=0.5)                                                       # int(2 nw) - 1 = 0 tapers
    for method in ('mtm ', 'multitaper', 'Welch', 'median', None, 1):
        with pytest.raises(ValueError):
            ofdm_tools.coherence_estimator(1024, 1e6, ctx=NoLibrary(), method=method)
    for block_len in (1023, 1, 0):
        with pytest.raises(ValueError):
            ofdm_tools.coherence_estimator(1024, 1e6, block_len=block_len, ctx=NoLibrary(), method='mtm')


def test_every_mtmcsd_kernel_build_has_no_scratch():
    """The two-channel taper loop keeps 4 N / T accumulators in registers across the transforms of a run: a spilled
    register would come back at memory latency 2 K times per segment.  Read from the code objects inside the built
    library: one build per power of two 64 ... 16384, each with a private segment of 0 bytes and no spilled register;
    the 1024-thread build inside its 128 registers; dynamic LDS (not in the code object) at most 160 KiB by the launcher's
    own arithmetic - 2 N float2 up to 8192 points, N float2 at 16384, and 64 float2 of reduction slots."""
    for (size, _, _, two, _), _ in check_builds('mtmcsd_kernel', POWERS, {1024: 128}):      # 1024 threads: four waves per SIMD
        assert two == (size <= 8192), size
        assert (2 if two else 1) * size * 8 + 64 * 8 <= 160 * 1024, size
