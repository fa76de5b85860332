"""GPU tests of the polyphase channelizer (oth_channelizer_*, csrc/chanpfb.hip, Context.channelizer) against the float64
oracles of tests/channelizer_oracle.py: the definition (mix, filter, decimate - no fold) on a sample of channels and the
fold / shift / transform form, which tests/test_channelizer_cpu.py holds to the definition at 1e-10, on all of them.
The gate, per output: |y_k[m] - oracle| <= RTOL sum_n |h[n]| |x[m D + n]| with the project's RTOL = 1e-4 - that sum is the
size of the worst-case result, and every rounding of the fold and of the butterflies is relative to at most that.  A wrong
rotation, twiddle or tap is an error of order 1 of it.  Input of the parity cases: unit complex noise, a tone of amplitude 3
on a channel centre, one of 0.5 a quarter channel off a centre at a negative frequency, and a 35 - 20j offset.
Measured on an MI355X, worst readings of this file (gate 1e-4 of sum |h| |x|): the 21 parity cases 1.03e-7 (4096 / 2048 x
16; the smallest 6.1e-8), which is 2.2e-4 of a channel's rms at worst - the offset's and the strong tone's rounding in a
channel that holds only their stop-band residue; one push of 5000 and of 40000 noise samples 4.2e-8 and 1.4e-8 (4.7e-7 of
the rms); 63 frames across 2^21 samples at 64 x 2 4.2e-8, 62 frames across 2^20 at 4096 x 16 6.5e-9, the same bytes with
16 workgroups and with the library's own split; after the refusals 6.7e-8.  exec_dev on the rows of push_dev against the
float64 Welch oracle of those rows: 2.8e-5 and 1.0e-6 per bin (gate 1e-4).  channelized_scan on the seed-0 capture: min SK of
channel 10 0.0075, max SK of channel 40 12.09, 2 of 3712 quiet cells flagged - the float64 oracles' figures - and its rows
against the SK oracle of the channel rows PSD 1.5e-5, R 2.6e-5 (gates 1e-4, 3e-4).  The phase step of a tone a quarter
channel off: 0.125000 cycles, spread below 1e-8.
Streaming in pieces, reset, the x0.125 gain, the frames a NaN does not cover and push against push_dev: the same bytes."""
import ctypes as C
import gc

import numpy as np
import pytest

import channelizer_oracle as CO
import median_oracle as MO
import welch_sk_oracle as SO
from stat_support import forced_env, recipe_field
from test_channelizer_cpu import PARITY_CASES, PARITY_FRAMES, TILE, noise, parity_input, prototype
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
SENTINEL = np.float32(-7.25)


def check_against(got, want, size, what):
    """got, want [channels, frames]; size [frames] = sum |h| |x|: the gate of the file header on every output -> the worst
    reading as a fraction of that size; prints it next to the worst reading as a fraction of a channel's rms"""
    assert got.shape == want.shape and got.dtype == np.complex64 and np.all(np.isfinite(got))
    err = np.abs(got.astype(np.complex128) - want)
    worst = float(np.max(err / size[None, :]))
    rms = np.sqrt(np.mean(np.abs(want) ** 2, axis=1))
    print('channelizer parity %s: %.2e of sum |h| |x|, %.2e of the channel rms' % (what, worst, float(np.max(np.max(err, axis=1) / rms))))
    assert worst <= RTOL, (what, worst)
    return worst


def run_dev(ctx, chan, x, stride, behind=64):
    """push_dev of the whole of x into a buffer [nchan][stride] full of SENTINEL with `behind` floats of it behind
    -> (rows [nchan, stride] complex64, the floats behind, frames)"""
    M = chan.nchan
    total = 2 * M * stride + behind
    d_x, d_out = ctx.alloc(max(x.nbytes, 8)), ctx.alloc(4 * total)
    try:
        ctx.h2d(d_x, x)
        ctx.h2d(d_out, np.full(total, SENTINEL, np.float32))
        frames = chan.push_dev(d_x, len(x), d_out, stride)
        flat = ctx.d2h(d_out, (total,), np.float32)
    finally:
        ctx.free(d_x)
        ctx.free(d_out)
    return flat[:2 * M * stride].view(np.complex64).reshape(M, stride), flat[2 * M * stride:], frames


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- 1. parity at every size, hop and tap count -------------------------------------------------------------------------------------

@pytest.mark.parametrize('nchan,decim,taps', PARITY_CASES)
def test_parity_with_the_float64_oracles(ctx, hip, nchan, decim, taps):
    x = parity_input(nchan, decim, taps)
    h = prototype(nchan, taps)
    chan = ctx.channelizer(nchan, decim, taps)
    assert chan.frames_for(len(x)) == PARITY_FRAMES and chan.frames_for(len(x) - 1) == PARITY_FRAMES - 1 and chan.pending == 0
    got = chan.push(x)
    assert got.shape == (nchan, PARITY_FRAMES) and chan.pending == taps * nchan - decim
    recipe = chan.last_recipe()
    tiles = (PARITY_FRAMES + TILE - 1) // TILE
    assert recipe.startswith('kernel=chanpfb nchan=%d decim=%d ntaps=%d tile=%d W=%d frames=%d tiles=%d pending=0 bpc=' %
                             (nchan, decim, taps, TILE, tiles, PARITY_FRAMES, tiles)), recipe
    size = CO.bound(x, decim, h)
    what = str((nchan, decim, taps))
    check_against(got, CO.channelize_fold(x, nchan, decim, h), size, what + ' all channels, fold form')
    some = sorted({0, 1, 3, nchan // 2 - 1, nchan // 2, nchan - 7, nchan - 1})
    check_against(got[some], CO.channelize(x, nchan, decim, h, channels=some), size, what + ' %d channels, definition' % len(some))
    # the same bytes through push_dev at an even stride on an aligned buffer (16-byte stores) and at an odd one (8-byte stores)
    for stride in (PARITY_FRAMES + 3, PARITY_FRAMES + 4):
        chan.reset()
        rows, behind, frames = run_dev(ctx, chan, x, stride)
        assert frames == PARITY_FRAMES and same_bytes(rows[:, :frames], got)
        assert np.all(rows[:, frames:].view(np.float32) == SENTINEL) and np.all(behind == SENTINEL)
    chan.close()


# ---- 2. streaming -----------------------------------------------------------------------------------------------------------------------

def cuts_for(n, L, D, seed):
    """push lengths that add up to n: the edges of the frame arithmetic, empty pushes, a run of pushes shorter than D, then
    random lengths up to 2 L"""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, D - 1, L - 1, L, L + 1, 0] + [int(v) for v in rng.integers(1, D, 12)] + [0]
    assert sum(sizes) < n
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 2 * L)), n - sum(sizes)))
    return sizes


@pytest.mark.parametrize('nchan,decim,taps,n', [(64, 32, 8, 5000), (1024, 256, 4, 40000)])
def test_any_split_into_pushes_gives_the_same_bytes(ctx, hip, nchan, decim, taps, n):
    L = taps * nchan
    x = noise(n, 5 + nchan)
    chan = ctx.channelizer(nchan, decim, taps)
    whole = chan.push(x)
    assert whole.shape == (nchan, CO.frames(0, n, L, decim)) and chan.pending == n - whole.shape[1] * decim
    check_against(whole, CO.channelize_fold(x, nchan, decim, prototype(nchan, taps)), CO.bound(x, decim, prototype(nchan, taps)),
                  'one push of %d samples at %s' % (n, (nchan, decim, taps)))
    for seed in (1, 2):
        chan.reset()
        assert chan.pending == 0
        parts, at, pending = [], 0, 0
        for size in cuts_for(n, L, decim, seed):
            want = CO.frames(pending, size, L, decim)
            assert chan.frames_for(size) == want
            part = chan.push(x[at:at + size])
            assert part.shape == (nchan, want)
            parts.append(part)
            at += size
            pending += size - want * decim
            assert chan.pending == pending <= L - 1
        assert at == n and same_bytes(np.concatenate(parts, axis=1), whole)
    # device pushes into one buffer at a moving column - a tile is aligned on each push's own column 0 - give them too
    chan.reset()
    stride = whole.shape[1] + 1
    d_x, d_out = ctx.alloc(x.nbytes), ctx.alloc(8 * nchan * stride)
    try:
        ctx.h2d(d_x, x)
        at = col = 0
        for size in cuts_for(n, L, decim, 3):
            col += chan.push_dev(d_x + 8 * at, size, d_out + 8 * col, stride)      # (the rows' pitch stays the buffer's)
            at += size
        rows = ctx.d2h(d_out, (nchan, stride), np.complex64)
    finally:
        ctx.free(d_x)
        ctx.free(d_out)
    assert col == whole.shape[1] and same_bytes(rows[:, :col], whole)
    # after a reset the first push repeats the first result bit for bit
    chan.reset()
    assert same_bytes(chan.push(x[:L + 3 * decim]), whole[:, :4])
    chan.close()


# ---- 3. phase continuity and exact properties -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('nchan,decim,taps', [(64, 32, 8), (256, 128, 8)])
def test_a_tone_keeps_its_phase_across_hops_and_pushes(ctx, hip, nchan, decim, taps):
    n = taps * nchan + 63 * decim
    x = np.exp(2j * np.pi * 5.25 / nchan * np.arange(n)).astype(np.complex64)
    chan = ctx.channelizer(nchan, decim, taps)
    y = np.concatenate([chan.push(x[:n // 3]), chan.push(x[n // 3:n // 3 + 7]), chan.push(x[n // 3 + 7:])], axis=1)[5].astype(np.complex128)
    assert len(y) == 64
    step = np.angle(y[1:] * np.conj(y[:-1])) / (2.0 * np.pi)
    print('phase step of a tone 0.25 channel off at %d / %d: mean %.6f cycles (%.6f), spread %.1e' %
          (nchan, decim, step.mean(), 0.25 * decim / nchan, np.ptp(step)))
    assert abs(step.mean() - 0.25 * decim / nchan) <= 1e-4 and np.max(np.abs(step - 0.25 * decim / nchan)) <= 1e-4
    chan.close()


@pytest.mark.parametrize('nchan,decim,taps', [(64, 16, 8), (512, 512, 3), (4096, 2048, 2)])
def test_zeros_a_gain_and_a_nan(ctx, hip, nchan, decim, taps):
    L, frames = taps * nchan, 21
    n = L + (frames - 1) * decim + 5
    x = parity_input(nchan, decim, taps, frames + 1)[:n]
    chan = ctx.channelizer(nchan, decim, taps)
    zero = chan.push(np.zeros(n, np.complex64))
    assert zero.shape == (nchan, frames) and np.all(zero == 0)
    chan.reset()
    clean = chan.push(x)
    chan.reset()
    assert same_bytes(chan.push((x * np.float32(0.125)).astype(np.complex64)), clean * np.float32(0.125))
    for at in (0, L - 1, L + 5 * decim + 1, n - 6, n - 1):
        bad = x.copy()
        bad[at] = np.complex64(complex(np.nan, 1.0)) if at % 2 else np.complex64(complex(2.0, np.inf))
        chan.reset()
        got = chan.push(bad)
        covered = np.array([m * decim <= at < m * decim + L for m in range(frames)])      # (none for the last samples)
        assert not np.isfinite(got[:, covered]).any()
        assert same_bytes(got[:, ~covered], clean[:, ~covered])
        chan.reset()
        assert same_bytes(chan.push(x), clean)      # nothing of the poisoned push stays behind a reset
    chan.close()


# ---- 4. a long push: a workgroup walks several tiles ------------------------------------------------------------------------------------

@pytest.mark.parametrize('nchan,decim,taps,n', [(64, 64, 2, 1 << 21), (4096, 1024, 16, 1 << 20)])
def test_a_workgroup_walks_several_tiles(ctx, hip, nchan, decim, taps, n):
    L = taps * nchan
    x = noise(n, 77 + nchan)
    h = prototype(nchan, taps)
    frames = CO.frames(0, n, L, decim)
    picks = sorted(set([0, 1, TILE - 1, TILE, frames - TILE - 1, frames - 2, frames - 1] +
                       [int(v) for v in np.random.default_rng(3).integers(0, frames, 57)]))[:64]
    want = CO.channelize_fold(x, nchan, decim, h, frame_list=picks)
    size = CO.bound(x, decim, h, frame_list=picks)
    results = []
    for cap in (16, None):      # at most 16 workgroups, then the library's own split
        with forced_env('OTH_CHAN_WG', cap):
            chan = ctx.channelizer(nchan, decim, taps)
        rows, behind, got_frames = run_dev(ctx, chan, x, frames)
        recipe = chan.last_recipe()
        assert got_frames == frames and np.all(behind == SENTINEL)
        W, tiles = recipe_field(recipe, 'W'), recipe_field(recipe, 'tiles')
        assert tiles == (frames + TILE - 1) // TILE and recipe_field(recipe, 'frames') == frames
        if cap:
            assert W == cap and tiles >= 4 * W, recipe      # every workgroup walks at least four tiles
        check_against(rows[:, picks], want, size, '%d frames of %d [%s]' % (len(picks), frames, recipe))
        results.append(rows)
        chan.close()
    assert same_bytes(results[0], results[1])      # a result does not depend on the split


# ---- 5. the device form feeds the _dev statistics ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('nchan,decim,taps,frames', [(64, 32, 8, 330), (128, 128, 2, 331)])
def test_push_dev_writes_its_columns_only_and_feeds_exec_dev(ctx, hip, nchan, decim, taps, frames):
    from test_median_gpu import window
    nfft, fs = 64, 2.5
    x = (noise(taps * nchan + (frames - 1) * decim + 7, 31 + nchan) +
         0.5 * np.exp(2j * np.pi * 9.3 / nchan * np.arange(taps * nchan + (frames - 1) * decim + 7))).astype(np.complex64)
    chan = ctx.channelizer(nchan, decim, taps)
    host = chan.push(x)
    assert host.shape == (nchan, frames)
    chan.reset()
    stride = frames + 129
    total = 2 * nchan * stride + 64
    d_x, d_out, d_psd = ctx.alloc(x.nbytes), ctx.alloc(4 * total), ctx.alloc(4 * nchan * nfft)
    plan = ctx.welch_plan(nfft, nperseg=nfft, noverlap=0, window=window('hann', nfft), detrend=hip.DETREND_CONSTANT,
                          scaling=hip.SCALE_DENSITY, fs=fs)
    try:
        ctx.h2d(d_x, x)
        ctx.h2d(d_out, np.full(total, SENTINEL, np.float32))
        assert chan.push_dev(d_x, len(x), d_out, stride) == frames
        nseg = plan.exec_dev(d_out, frames, d_psd, nstreams=nchan, stream_stride=stride)      # straight from the rows
        flat = ctx.d2h(d_out, (total,), np.float32)
        psd = ctx.d2h(d_psd, (nchan, nfft), np.float32).astype(np.float64)
    finally:
        for d in (d_x, d_out, d_psd):
            ctx.free(d)
    rows = flat[:2 * nchan * stride].view(np.complex64).reshape(nchan, stride)
    assert same_bytes(rows[:, :frames], host)
    assert np.all(rows[:, frames:].view(np.float32) == SENTINEL) and np.all(flat[2 * nchan * stride:] == SENTINEL)
    assert nseg == frames // nfft
    worst = 0.0
    for k in range(nchan):      # the float64 Welch oracle of the channelizer's own rows
        ref = MO.welch_rows(host[k], fs, 'hann', nfft, 0, nfft, 'constant', 'density').mean(axis=0)
        worst = max(worst, float(np.max(np.abs(psd[k] - ref) / ref)))
    print('exec_dev on the rows of push_dev, %d channels x %d segments of %d: %.2e per bin' % (nchan, nseg, nfft, worst))
    assert worst <= RTOL
    plan.close()
    chan.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def refused(ctx, rc, code, text):
    assert rc == code and ctx.lib.oth_last_error(ctx.h).decode() == text, (rc, ctx.lib.oth_last_error(ctx.h))


def test_refusals_leave_nothing_behind_and_the_handle_usable(ctx, hip):
    ctx.channelizer(64, 32, 8).close()      # (the context keeps the twiddles of a length once a handle has asked for them)
    gc.collect()
    lib, live0 = ctx.lib, hip.live_resources()
    fp = C.POINTER(C.c_float)
    good = prototype(64, 8)

    def create(nchan, decim, ntaps, h):
        out = C.c_void_p()
        rc = lib.oth_channelizer_create(ctx.h, nchan, decim, ntaps, h.ctypes.data_as(fp) if h is not None else None, C.byref(out))
        assert rc != 0 and not out.value and hip.live_resources() == live0
        return rc

    for nchan in (0, 32, 96, 8192, -64):
        refused(ctx, create(nchan, nchan // 2, 8, good), UNSUPPORTED,
                'the channelizer takes a channel count that is a power of two from 64 to 4096, not %d' % nchan)
    for decim in (0, 8, 48, 128):
        refused(ctx, create(64, decim, 8, good), INVALID, 'decim must be nchan, nchan / 2 or nchan / 4')
    for ntaps in (0, 17, -3):
        refused(ctx, create(64, 32, ntaps, good), INVALID, 'ntaps must lie in 1 ... 16')
    refused(ctx, create(64, 32, 8, None), INVALID, 'h is NULL')
    for v in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[100] = v
        refused(ctx, create(64, 32, 8, bad), INVALID, 'every tap of the prototype must be finite')
    refused(ctx, create(64, 32, 8, np.zeros(512, np.float32)), INVALID, 'the prototype is all zero')
    # the order: the channel count before the hop before the taps before h
    refused(ctx, create(96, 7, 0, None), UNSUPPORTED, 'the channelizer takes a channel count that is a power of two from 64 to 4096, not 96')
    refused(ctx, create(64, 7, 0, None), INVALID, 'decim must be nchan, nchan / 2 or nchan / 4')
    refused(ctx, create(64, 64, 0, None), INVALID, 'ntaps must lie in 1 ... 16')

    chan = ctx.channelizer(64, 32, 8)
    assert hip.live_resources() != live0
    x = parity_input(64, 32, 8, 12)
    first = chan.push(x[:700])
    want = CO.channelize_fold(x, 64, 32, good)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.full((64, 8), SENTINEL + 0j, np.complex64)
    n = C.c_uint64(99)
    rest = x[700:]
    nrest = want.shape[1] - first.shape[1]
    assert chan.frames_for(len(rest)) == nrest == 6
    attempts = (
        (lambda: lib.oth_channelizer_push(chan.h, None, 5, 0, vp(out), 8, C.byref(n)), 'bad argument'),
        (lambda: lib.oth_channelizer_push(chan.h, vp(rest), len(rest), 0, vp(out), 8, None), 'bad argument'),
        (lambda: lib.oth_channelizer_push_dev(chan.h, None, 5, None, 8, C.byref(n)), 'bad argument'),
        (lambda: lib.oth_channelizer_push(chan.h, vp(rest), len(rest), 0, None, 8, C.byref(n)), 'the output is NULL'),
        (lambda: lib.oth_channelizer_push_dev(chan.h, C.c_void_p(4096), len(rest), None, 8, C.byref(n)), 'the output is NULL'),
        (lambda: lib.oth_channelizer_push(chan.h, vp(rest), len(rest), 0, vp(out), 5, C.byref(n)), 'out_stride < frames of this push'),
        (lambda: lib.oth_channelizer_push_dev(chan.h, C.c_void_p(4096), len(rest), C.c_void_p(4096), 5, C.byref(n)), 'out_stride < frames of this push'),
    )
    pending = chan.pending
    for call, text in attempts:
        refused(ctx, call(), INVALID, text)
        assert chan.pending == pending and chan.frames_for(len(rest)) == nrest and np.all(out == np.complex64(SENTINEL))
    # nsamples == 0 is no error, with or without pointers
    n.value = 99
    assert lib.oth_channelizer_push(chan.h, None, 0, 0, None, 0, C.byref(n)) == 0 and n.value == 0
    n.value = 99
    assert lib.oth_channelizer_push_dev(chan.h, None, 0, None, 0, C.byref(n)) == 0 and n.value == 0
    # ... and after all of them the handle gives the right answer
    got = np.concatenate([first, chan.push(rest)], axis=1)
    check_against(got, want, CO.bound(x, 32, good), 'after the refusals')
    chan.close()
    gc.collect()
    assert hip.live_resources() == live0


# ---- 7. the pipeline the feature exists for ---------------------------------------------------------------------------------------------

def scan_capture(seed):
    """unit complex noise, a carrier of amplitude 0.5 just off the centre of channel 10 of 64, and a unit-power noise band of
    half-width 1 / 512 cycles per sample on the centre of channel 40 that is on a quarter of the time"""
    n = 512 + (48 * 64 - 1) * 32
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    x += 0.5 * np.exp(2j * np.pi * (10.0 / 64.0 + 0.0017) * t)
    B = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    B[np.abs(np.fft.fftfreq(n)) > 1.0 / 512.0] = 0.0
    band = np.fft.ifft(B)
    band /= np.sqrt(np.mean(np.abs(band) ** 2))
    x += band * np.exp(2j * np.pi * 40.0 / 64.0 * t) * ((t // 4096) % 4 == 0)
    return x.astype(np.complex64)


def test_channelized_scan_tells_a_carrier_from_a_burst_per_channel(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    from test_welch_sk_gpu import check_rows
    nchan, decim, taps, nfft, Sf, fc = 64, 32, 8, 64, 6.4e6, 100e6
    x = scan_capture(0)
    centres, offsets, psd, sk, steady, burst, M = T.channelized_scan(x, nchan, nfft, Sf, fc=fc, decim=decim, taps=taps, p_false=1e-3, ctx=ctx)
    assert M == 48 and centres.shape == (nchan,) and offsets.shape == (nfft,)
    assert psd.shape == sk.shape == steady.shape == burst.shape == (nchan, nfft)
    assert psd.dtype == sk.dtype == np.float32 and steady.dtype == burst.dtype == np.bool_
    assert np.allclose(centres, fc + (np.arange(nchan) - nchan // 2) * Sf / nchan, rtol=0, atol=1e-6)
    assert np.allclose(offsets, (np.arange(nfft) - nfft // 2) * (Sf / decim) / nfft, rtol=0, atol=1e-6)
    lower, upper = T.sk_limits(48, 1e-3)
    assert np.array_equal(steady, sk < lower) and np.array_equal(burst, sk > upper)
    row = lambda k: (k + nchan // 2) % nchan      # natural channel k in the fftshifted order
    assert centres[row(10)] == pytest.approx(fc + 10 * Sf / nchan) and centres[row(40)] == pytest.approx(fc - 24 * Sf / nchan)
    quiet = np.ones(nchan, bool)
    quiet[[row(k) for k in (9, 10, 11, 39, 40, 41)]] = False
    flagged = int(np.sum((steady | burst)[quiet]))
    print('channelized_scan: min SK of channel 10 %.4f, max SK of channel 40 %.2f, %d of %d quiet cells flagged (limits %.3f, %.3f)' %
          (sk[row(10)].min(), sk[row(40)].max(), flagged, int(quiet.sum()) * nfft, lower, upper))
    assert sk[row(10)].min() < 0.05
    assert sk[row(40)].max() > 5.0
    assert int(quiet.sum()) * nfft == 3712 and flagged <= 18
    # the rows are the SK and the PSD of the library's own channel rows
    chan = ctx.channelizer(nchan, decim, taps)
    rows = chan.push(x)
    assert rows.shape == (nchan, 48 * 64)
    worst = (0.0, 0.0)
    for k in range(nchan):
        ref = SO.sk(rows[k], nfft, nfft, 0, 'hann', True)
        e = check_rows(sk[row(k)], psd[row(k)], ref, SO.psd(ref, 'hann', nfft, 'density', Sf / decim, nfft), fftshift=True)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    print('channelized_scan against the SK oracle of the channel rows: PSD %.2e, R %.2e' % worst)
    chan.close()
