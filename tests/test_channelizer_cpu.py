"""CPU checks of the polyphase channelizer addition (no GPU): the float64 oracle by the definition
(tests/channelizer_oracle.py) against scipy.signal.lfilter on the mixed signal, against the fold / circular shift / transform
form the kernel computes (1e-10 of the output's size) and, with one tap per branch, against windowed-frame transforms with
the phase of the absolute time; the frame arithmetic of a push against a brute-force count; the declared surface; the
ValueErrors the Python layer raises before a context exists; and the resource figures of every chan_pfb_kernel build read
from the code objects of the built library."""
import os

import numpy as np
import pytest

import channelizer_oracle as CO
from stat_support import ROOT, check_builds, check_surface

SYMBOLS = ('oth_channelizer_create', 'oth_channelizer_destroy', 'oth_channelizer_reset', 'oth_channelizer_frames',
           'oth_channelizer_push_dev', 'oth_channelizer_push', 'oth_channelizer_pending')
METHODS = ('push', 'push_dev', 'frames_for', 'pending', 'reset', 'close', '__del__', 'channel_freqs', 'channel_rate')
SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
TILE = 8                 # kChanTile: frames of a tile
PARITY_FRAMES = 37       # no multiple of the tile, more than one tile

# the parity cases of tests/test_channelizer_gpu.py: every size x every hop, the taps per branch cycling through 1, 2, 8, 16 -
# 4 and 3 are coprime, so any 12 consecutive cases hold every (taps, hop) pair
PARITY_CASES = [(M, M // r, (1, 2, 8, 16)[(3 * i + j) % 4]) for i, M in enumerate(SIZES) for j, r in enumerate((1, 2, 4))]


def prototype(nchan, taps):
    """the float32 taps a channelizer holds: the oracles run on the same values"""
    from ofdm_tools import windows
    return windows.pfb_prototype(nchan, taps).astype(np.float32)


def noise(n, seed):
    """unit complex noise, complex64"""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)


def parity_input(nchan, decim, taps, frames=PARITY_FRAMES):
    """exactly `frames` frames: unit complex noise, a tone on the centre of channel 3, one 0.25 channel above the centre of
    channel nchan - 7 (a negative frequency) and a 35 - 20j offset"""
    n = taps * nchan + (frames - 1) * decim
    t = np.arange(n, dtype=np.float64)
    x = noise(n, 11 * nchan + decim + taps).astype(np.complex128)
    x += 3.0 * np.exp(2j * np.pi * 3.0 / nchan * t) + 0.5 * np.exp(2j * np.pi * (nchan - 7 + 0.25) / nchan * t) + (35.0 - 20.0j)
    return x.astype(np.complex64)


# ---- 1. the oracle -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nchan,decim,taps', [(64, 32, 8), (64, 16, 3), (128, 128, 2)])
def test_oracle_is_mix_filter_decimate(nchan, decim, taps):
    """scipy.signal.lfilter on the mixed signal, every decim-th output from the first full one"""
    import scipy.signal as sg
    h = prototype(nchan, taps).astype(np.float64)
    h[::3] *= 0.7      # not symmetric: the filter's direction shows
    L = len(h)
    x = parity_input(nchan, decim, taps, 9).astype(np.complex128)
    got = CO.channelize(x, nchan, decim, h)
    assert got.shape == (nchan, 9)
    t = np.arange(len(x))
    size = CO.bound(x, decim, h)      # sum |h| |x| per frame: each of the two sums of L products is good to L 2^-53 of it
    worst = 0.0
    for k in (0, 1, 3, nchan // 2, nchan - 7, nchan - 1):
        want = sg.lfilter(h[::-1], 1.0, x * np.exp(-2j * np.pi * ((k * t) % nchan) / nchan))[L - 1::decim]
        worst = max(worst, float(np.max(np.abs(got[k] - want) / size)))
    print('oracle against lfilter + slicing at %d / %d x %d: %.1e of sum |h| |x|' % (nchan, decim, taps, worst))
    assert worst <= 2.0 * L * 2.0 ** -53
    # an absolute time origin: the frames of x[t0:] with t0 a multiple of decim are the later frames of x
    late = CO.channelize(x[2 * decim:], nchan, decim, h, channels=(3, nchan - 7), t0=2 * decim)
    assert np.max(np.abs(late - got[[3, nchan - 7], 2:])) <= 1e-9 * np.max(np.abs(got))


@pytest.mark.parametrize('nchan,decim,taps', [(64, 64, 2), (64, 32, 8), (128, 32, 1), (256, 64, 3), (512, 256, 16)])
def test_fold_shift_transform_is_the_definition(nchan, decim, taps):
    h = prototype(nchan, taps)
    x = parity_input(nchan, decim, taps, 13)
    want = CO.channelize(x, nchan, decim, h)
    got = CO.channelize_fold(x, nchan, decim, h)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print('fold / shift / transform against the definition at %d / %d x %d: %.1e of the output' % (nchan, decim, taps, err))
    assert got.shape == want.shape == (nchan, 13) and err <= 1e-10
    # frame0: the absolute frame index behind the shift
    part = CO.channelize_fold(x[5 * decim:], nchan, decim, h, frame0=5)
    assert np.max(np.abs(part - want[:, 5:])) <= 1e-10 * np.max(np.abs(want))


@pytest.mark.parametrize('nchan,decim', [(64, 64), (64, 16), (256, 128)])
def test_one_tap_is_the_phase_continuous_stft(nchan, decim):
    h = prototype(nchan, 1)
    x = parity_input(nchan, decim, 1, 11).astype(np.complex128)
    got = CO.channelize(x, nchan, decim, h)
    k = np.arange(nchan)
    for m in range(11):
        want = np.fft.fft(x[m * decim:m * decim + nchan] * h) * np.exp(-2j * np.pi * ((k * m * decim) % nchan) / nchan)
        assert np.max(np.abs(got[:, m] - want)) <= 1e-10 * np.max(np.abs(want))


def test_a_tone_off_centre_advances_delta_d_over_m_cycles_per_output():
    nchan, decim, taps = 64, 32, 8
    t = np.arange(taps * nchan + 20 * decim)
    y = CO.channelize(np.exp(2j * np.pi * 5.25 / nchan * t), nchan, decim, prototype(nchan, taps), channels=(5,))[0]
    step = np.angle(y[1:] * np.conj(y[:-1])) / (2.0 * np.pi)
    assert np.max(np.abs(step - 0.25 * decim / nchan)) <= 1e-12


# ---- 2. the frame arithmetic of a push ------------------------------------------------------------------------------------------------

def test_frames_of_a_push_against_a_brute_force_count():
    for L, D in ((512, 32), (512, 64), (128, 128), (64, 16), (4096, 256)):
        for pending in (0, 1, D - 1, D, L - D, L - 2, L - 1):
            for n in (0, 1, D - 1, D, D + 1, L - pending - 1, L - pending, L - pending + 1, L - 1, L, L + 1, 3 * L + 7, 10 * L + D - 1):
                if n < 0:
                    continue
                total = pending + n
                brute = sum(1 for m in range(total // D + 1) if m * D + L <= total)
                assert CO.frames(pending, n, L, D) == brute, (L, D, pending, n)
                left = total - brute * D      # what stays pending behind the push
                assert left <= L - 1 and (brute == 0 or left >= L - D)
    assert CO.frames(0, 511, 512, 32) == 0 and CO.frames(0, 512, 512, 32) == 1 and CO.frames(0, 543, 512, 32) == 1
    assert CO.frames(0, 544, 512, 32) == 2 and CO.frames(511, 1, 512, 32) == 1 and CO.frames(511, 0, 512, 32) == 0
    for nchan, decim, taps in PARITY_CASES:
        assert CO.frames(0, len(parity_input(nchan, decim, taps)), taps * nchan, decim) == PARITY_FRAMES
    assert len(PARITY_CASES) == 21 and {(t, M // D) for M, D, t in PARITY_CASES} == {(t, r) for t in (1, 2, 8, 16) for r in (1, 2, 4)}


# ---- 3. surface, 4. the Python layer's refusals -----------------------------------------------------------------------------------------

def test_surface_is_declared_and_exported():
    check_surface(SYMBOLS, 'Channelizer', METHODS)
    from ofdm_tools import _hip, ofdm_cr_tools
    assert hasattr(_hip.Context, 'channelizer') and callable(ofdm_cr_tools.channelized_scan)
    header = open(os.path.join(ROOT, 'include', 'ofdm_tools_hip.h')).read()
    assert 'typedef struct oth_channelizer oth_channelizer;' in header
    assert not [ln for ln in header.splitlines() if ln.startswith('int oth_channelizer') and 'oth_plan' in ln]


def test_argument_errors_are_value_errors_without_a_context():
    from ofdm_tools import _hip
    from ofdm_tools import ofdm_cr_tools as T
    for nchan in (0, 32, 100, 8192, 96):
        with pytest.raises(ValueError) as ei:
            _hip.Channelizer(None, nchan)
        assert 'power of two from 64 to 4096' in str(ei.value)
    for decim in (0, 8, 63, 128, 48):
        with pytest.raises(ValueError) as ei:
            _hip.Channelizer(None, 64, decim=decim)
        assert 'decim must be nchan, nchan / 2 or nchan / 4' in str(ei.value)
    for taps in (0, 17, -1):
        with pytest.raises(ValueError) as ei:
            _hip.Channelizer(None, 64, taps=taps)
        assert '1 ... 16' in str(ei.value)
    for proto, text in ((np.ones(100), 'taps * nchan = 512'), (np.zeros(512), 'all zero'),
                        (np.where(np.arange(512) == 9, np.nan, 1.0), 'finite'), (np.where(np.arange(512) == 9, np.inf, 1.0), 'finite')):
        with pytest.raises(ValueError) as ei:
            _hip.Channelizer(None, 64, prototype=proto)
        assert text in str(ei.value)
    nchan, decim, taps, h = _hip.channelizer_args(128)
    assert (nchan, decim, taps) == (128, 64, 8) and h.dtype == np.float32 and np.array_equal(h, prototype(128, 8))
    assert _hip.channelizer_args(64, 16, 1, np.arange(1, 65))[3].shape == (64,)
    # channelized_scan: before anything runs
    x = np.zeros(512 + (48 * 64 - 1) * 32, np.complex64)
    for kw, text in ((dict(nchan=64, nFFT=100), 'power of two from 64 to 16384'), (dict(nchan=64, nFFT=32), 'power of two from 64 to 16384'),
                     (dict(nchan=96, nFFT=64), 'power of two from 64 to 4096'), (dict(nchan=64, nFFT=64, decim=7), 'decim must be'),
                     (dict(nchan=64, nFFT=64, taps=0), '1 ... 16'), (dict(nchan=64, nFFT=128), 'at least 32 fine segments')):
        with pytest.raises(ValueError) as ei:
            T.channelized_scan(x, Sf=1.0, **kw)
        assert text in str(ei.value)
    with pytest.raises(ValueError) as ei:
        T.channelized_scan(x[:-32 * 1025], 64, 64, 1.0)      # 2047 frames: 31 segments
    assert 'at least 32 fine segments' in str(ei.value)


# ---- 5. resources -------------------------------------------------------------------------------------------------------------------------

def test_every_chan_pfb_kernel_build_has_no_scratch():
    """One build per channel count 64 ... 4096, each with the tile of 8 frames: a tile of 8 M / T <= 32 complex registers next
    to the fold and the butterflies, read from the code objects inside the built library - a private segment of 0 bytes and
    no spilled register.  The compiler reports (vgpr, printed per build): 38 / 58 / 96 on 64 threads (64 / 128 / 256
    channels), 96 on 128, 96 on 256, 94 on 512, 95 on 1024.  Budget 128 at every thread count: all a lane of a 1024-thread
    workgroup can have, and what keeps four waves on a SIMD for the smaller workgroups."""
    builds = check_builds('chan_pfb_kernel', [(M, TILE) for M in SIZES], {64: 128, 128: 128, 256: 128, 512: 128, 1024: 128})
    assert sorted(a[1] for a, _ in builds) == sorted(max(64, M // 4) for M in SIZES)
