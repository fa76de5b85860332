"""CPU checks of the polyphase filter-bank addition (no GPU): the float64 oracle by the definition
(tests/welch_pfb_oracle.py) against the scipy.signal.welch identity it rests on, the frame count at its edges, the
prototype of windows.pfb_prototype, the leakage property the feature exists for, what float32 itself loses on the exact
inputs of the GPU parity cases (emulate32 against float64 stays inside half the GPU gate), the Python helpers' refusals,
the declared surface, and the resource figures of every welch_pfb_kernel build read from the code objects of the built
library."""
import numpy as np
import pytest

import welch_pfb_oracle as PO
from stat_support import FS, POWERS, check_builds, check_surface
from test_median_gpu import noise_tones

SYMBOLS = ('oth_welch_set_prototype', 'oth_welch_pfb_dev', 'oth_welch_pfb')
RTOL = 1e-4      # the project's parity tolerance (tests/test_hip_parity.py), spelled out: this file runs without a GPU

# The parity cases of tests/test_welch_pfb_gpu.py: nfft, ntaps, hop, M, detrend, scaling, fftshift, trim, db, offset
PARITY_CASES = [
    (64, 2, 64, 9, True, 'density', False, 0, False, 0.0),
    (128, 3, 77, 7, True, 'raw', True, 10, False, 0.0),                       # an odd hop, fftshift with trim
    (256, 4, 128, 9, True, 'density', False, 0, True, 0.0),                   # the 2x oversampled bank, dB
    (512, 2, 512, 1, False, 'density', False, 0, False, 0.0),                 # one frame, detrend off
    (1024, 5, 512, 5, True, 'density', False, 0, False, 35.0 - 20.0j),        # a 35-sigma complex offset under detrend
    (2048, 8, 2048, 3, True, 'spectrum', False, 0, False, 0.0),
    (4096, 4, 2048, 9, True, 'density', False, 0, False, 0.0),
    (4096, 8, 4096, 4, False, 'over_n2', False, 0, False, 0.0),
    (8192, 16, 5001, 6, True, 'density', False, 0, False, 35.0 - 20.0j),      # an odd hop, the offset
    (16384, 16, 16384, 3, True, 'density', False, 0, False, 0.0),
    (16384, 2, 8192, 5, False, 'density', False, 0, False, 0.0),
]


def prototype(nfft, ntaps):
    from ofdm_tools import windows
    return windows.pfb_prototype(nfft, ntaps)


def parity_input(nfft, ntaps, hop, M, offset):
    """the capture of a parity case: exactly M frames and a third of a hop more"""
    n = ntaps * nfft + (M - 1) * hop + hop // 3
    return (noise_tones(n, 7 * nfft + ntaps + M) + np.complex64(offset)).astype(np.complex64)


# ---- 1. the identity the oracle and the composition test rest on -----------------------------------------------------------------

@pytest.mark.parametrize('nfft,ntaps,step', [(64, 4, 64), (128, 3, 64), (256, 8, 100)])
def test_oracle_is_every_pth_bin_of_a_long_welch(nfft, ntaps, step):
    import scipy.signal as sg
    L = nfft * ntaps
    x = noise_tones(L + 6 * step + 5, 3 + nfft).astype(np.complex128)
    h = prototype(nfft, ntaps)
    worst = 0.0
    for scaling in ('density', 'spectrum'):
        for detrend in (True, False):
            got = PO.pfb(x, nfft, ntaps, h, nfft - step, detrend, scaling, FS)
            want = sg.welch(x, FS, window=h, nperseg=L, noverlap=L - step, nfft=L, detrend='constant' if detrend else False,
                            return_onesided=False, scaling=scaling)[1][::ntaps]
            assert got['M'] == 7
            worst = max(worst, float(np.max(np.abs(got['pfb'] - want) / want)))
    print('oracle against scipy.signal.welch(...)[::%d] at %d points, hop %d: %.1e' % (ntaps, nfft, step, worst))
    assert worst <= 1e-12


def test_oracle_counts_frames():
    assert PO.nseg(4 * 64, 64, 4) == 1 and PO.nseg(4 * 64 - 1, 64, 4) == 0      # one frame; one sample fewer is the refusal's case
    assert PO.nseg(4 * 64 + 63, 64, 4) == 1 and PO.nseg(5 * 64, 64, 4) == 2
    assert PO.nseg(3 * 128 + 76, 128, 3, 128 - 77) == 1 and PO.nseg(3 * 128 + 77, 128, 3, 128 - 77) == 2      # an odd hop
    assert PO.nseg(3 * 128 + 6 * 77 + 25, 128, 3, 128 - 77) == 7
    assert PO.nseg(1 << 24, 4096, 8) == 4096 - 7
    x = noise_tones(4 * 64, 1)
    assert PO.pfb(x, 64, 4, prototype(64, 4))['M'] == 1
    for nfft, ntaps, hop, M, _, _, _, _, _, off in PARITY_CASES:
        assert PO.nseg(len(parity_input(nfft, ntaps, hop, M, off)), nfft, ntaps, nfft - hop) == M


# ---- 2. the prototype --------------------------------------------------------------------------------------------------------------

def test_prototype_is_a_flat_narrow_filter():
    """symmetric; the folded taps flat to 1 % from 8 taps on (0.924 / 0.994 / 0.99995 min over max at 4 / 8 / 16 taps); the
    noise bandwidth at 256 points 0.780 / 0.806 / 0.859 bins"""
    for nfft in (64, 256, 4096):
        for ntaps, fold_floor in ((4, 0.9), (8, 0.99), (16, 0.99)):
            h = prototype(nfft, ntaps)
            assert h.dtype == np.float64 and h.shape == (nfft * ntaps,)
            assert np.array_equal(h, h[::-1]) and h.max() <= 1.0 and abs(h[len(h) // 2] - 1.0) < 1e-3
            fold = h.reshape(ntaps, nfft).sum(axis=0)
            enbw = np.sum(h * h) / np.sum(h) ** 2 * nfft      # in bins of the nfft-point bank
            print('prototype %d x %d: hfold min / max %.5f, noise bandwidth %.3f bins' % (nfft, ntaps, fold.min() / fold.max(), enbw))
            assert fold.min() / fold.max() >= fold_floor
            if nfft == 256:
                assert 0.78 <= round(enbw, 3) <= 0.86      # at the three digits it is read to: 4 taps give 0.7796
    from ofdm_tools import windows
    assert np.array_equal(windows.pfb_prototype(64, 4, beta=10.0), prototype(64, 4))      # beta = 2.5 ntaps by default
    assert not np.array_equal(windows.pfb_prototype(64, 4, cutoff=0.9), prototype(64, 4))
    with pytest.raises(ValueError):
        windows.pfb_prototype(0, 4)


# ---- 3. what the feature exists for --------------------------------------------------------------------------------------------------

def test_oracle_keeps_a_strong_band_out_of_its_neighbours():
    x = PO.leak_capture()
    ref = PO.pfb(x, PO.LEAK_NFFT, PO.LEAK_TAPS, prototype(PO.LEAK_NFFT, PO.LEAK_TAPS))
    assert ref['M'] == PO.LEAK_M
    PO.check_leakage(ref['pfb'], PO.hann_welch(x, PO.LEAK_NFFT), 'float64 oracle')


# ---- 4. float32's own loss on the GPU suite's inputs -------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,ntaps,hop,M,detrend,scaling,fftshift,trim,db,offset', PARITY_CASES)
def test_float32_stays_inside_half_the_gpu_gate(nfft, ntaps, hop, M, detrend, scaling, fftshift, trim, db, offset):
    x = parity_input(nfft, ntaps, hop, M, offset)
    h = prototype(nfft, ntaps).astype(np.float32)
    ref = PO.pfb(x, nfft, ntaps, h, nfft - hop, detrend, scaling, FS)
    assert ref['M'] == M
    emu = PO.emulate32(x, nfft, ntaps, h, nfft - hop, detrend, scaling, FS)
    err = float(np.max(np.abs(emu - ref['pfb']) / ref['pfb']))
    print('float32 emulation against float64, %d x %d, hop %d, M %d: %.1e per bin' % (nfft, ntaps, hop, M, err))
    assert err <= RTOL / 2


# ---- 5. the helpers' refusals, before a context exists ---------------------------------------------------------------------------

def test_helpers_refuse_in_python():
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros(256 * 8, np.complex64)
    calls = (lambda n, t, v=x: T.pfb_power_estimate(v, n, 1.0, ntaps=t),
             lambda n, t, v=x: T.pfb_plot_dB(v, 1.0, 0.0, n, ntaps=t),
             lambda n, t, v=x: T.src_power_pfb(v, len(v), n, 1.0 / n, 1.0, [0.0], 4, ntaps=t))
    for call in calls:
        for nfft in (100, 32, 32768):
            with pytest.raises(ValueError) as ei:
                call(nfft, 2)
            assert 'power of two' in str(ei.value)
        for ntaps in (1, 17, 0):
            with pytest.raises(ValueError) as ei:
                call(64, ntaps)
            assert '2 ... 16' in str(ei.value)
        with pytest.raises(ValueError) as ei:
            call(256, 8, x[:-1])      # one sample short of a frame
        assert 'ntaps * nFFT' in str(ei.value)
    import inspect
    for f in (T.pfb_power_estimate, T.pfb_plot_dB, T.src_power_pfb):
        assert inspect.signature(f).parameters['ntaps'].default == 8


# ---- 6. surface, 7. resources ------------------------------------------------------------------------------------------------------

def test_surface_is_declared_and_exported():
    check_surface(SYMBOLS, 'WelchPlan', ('set_prototype', 'pfb', 'pfb_dev'))


def test_every_welch_pfb_kernel_build_has_no_scratch():
    """N / T complex accumulators of the fold and one running row next to the butterflies: read from the code objects inside
    the built library, one build per power of two 64 ... 16384, each with a private segment of 0 bytes and no spilled
    register.  The compiler reports (vgpr, printed per build): 32 / 33 / 47 / 70 on 64 threads, 51 / 77 / 117 on 256, 116 on
    512, 117 on 1024.  Budgets per thread count: 128 from 256 threads on - all a lane of a 1024-thread workgroup can have,
    and what keeps the four 4096-point workgroups per CU the launch counts on - and 80 on 64 threads."""
    check_builds('welch_pfb_kernel', list(POWERS), {64: 80, 256: 128, 512: 128, 1024: 128})
