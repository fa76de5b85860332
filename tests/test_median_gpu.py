"""GPU tests of the median average (oth_plan_set_average(OTH_AVERAGE_MEDIAN)) and of the per-segment rows
(oth_welch_segments_dev): rows against the float64 oracle, the selection against a sort of the GPU's own rows, end to
end against scipy's estimator, the full C2 shape, a busy stream, the schedules and the refusals."""
import numpy as np
import pytest

import median_oracle as M
from oracle import ref_cpu as R
from test_hip_parity import RTOL, check_single_rows, ctx, hip  # noqa: F401 - ctx / hip are fixtures

pytestmark = pytest.mark.gpu


def window(name, n):
    from ofdm_tools import windows
    return windows.get_window(name, n)


def noise_tones(n, seed, tones=((3.0, 0.123), (0.5, -0.31))):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    for a, f in tones:
        x = x + a * np.exp(2j * np.pi * f * t)
    return (x + 0.3 - 0.1j).astype(np.complex64)


SCALINGS = {'density': 1, 'spectrum': 3, 'raw': 0, 'over_n2': 2}


def make_plan(ctx, hip, nfft, nperseg, noverlap, win='hann', detrend=True, scaling='density', fftshift=False, trim=0,
              db=False, average='median'):
    return ctx.welch_plan(nfft, nperseg=nperseg, noverlap=noverlap, window=window(win, nperseg),
                          detrend=hip.DETREND_CONSTANT if detrend else hip.DETREND_NONE, scaling=SCALINGS[scaling],
                          fs=1.0, fftshift=fftshift, trim_bins=trim, db=db, average=average)


def within_ulps(a, b, n):
    """|a - b| <= n ulp(b) elementwise (b float32 values, a any precision)."""
    b32 = np.asarray(b, np.float32)
    return np.abs(np.asarray(a, np.float64) - b32.astype(np.float64)) <= n * np.spacing(np.abs(b32)).astype(np.float64)


# ---- 1. rows --------------------------------------------------------------------------------------------------------

ROW_CASES = [  # nfft, nperseg, overlap %, detrend, scaling, fftshift, trim, db
    (256, 256, 50, True, 'density', False, 0, False),
    (1024, 1024, 75, True, 'spectrum', True, 16, False),
    (4096, 4096, 50, True, 'density', True, 0, True),
    (4096, 4096, 0, False, 'raw', False, 0, False),
    (64, 64, 50, True, 'over_n2', True, 4, False),
    (1000, 1000, 50, True, 'density', False, 0, False),
    (4099, 4099, 75, False, 'spectrum', True, 0, False),
    (8192, 8192, 50, True, 'density', True, 32, True),
    (16384, 16384, 0, True, 'raw', False, 0, False),
    (32768, 32768, 50, True, 'density', False, 0, False),
    (2048, 1024, 50, True, 'density', False, 0, False),       # zero padding (any_run rows)
    (1000, 600, 0, False, 'spectrum', False, 0, False),
]


@pytest.mark.parametrize('nfft,nperseg,ov,detrend,scaling,fftshift,trim,db', ROW_CASES)
def test_segments_rows_match_the_oracle(ctx, hip, nfft, nperseg, ov, detrend, scaling, fftshift, trim, db):
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    x = noise_tones(noverlap + 9 * step + step // 3, nfft + ov)
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend=detrend, scaling=scaling, fftshift=fftshift, trim=trim, db=db)
    rows = plan.segments(x)
    ref = M.welch_rows(x, 1.0, 'hann', nperseg, noverlap, nfft, 'constant' if detrend else False, scaling)
    ref = M.shift_trim_db(ref, fftshift, trim)
    assert rows.shape == (9, nfft - 2 * trim)
    got = 10.0 ** (rows.astype(np.float64) / 10.0) if db else rows
    bluestein = nfft == 4099      # (prime: a Bluestein transform, ulps=8 as tests/test_anylen_gpu.py)
    check_single_rows(got, ref, ulps=8 if (bluestein or db) else 4)
    plan.close()


# ---- 2. the selection is exact ------------------------------------------------------------------------------------

def raw_rows_and_psd(ctx, hip, plan, x, nstreams=1):
    """-> (GPU raw rows [nstreams][nseg][nfft] from segments_dev, exec_dev PSD [nstreams][nfft])"""
    nseg = plan.nseg(len(x) // nstreams)
    n = len(x) // nstreams
    d = ctx.alloc(x.nbytes)
    rows = ctx.alloc(4 * nseg * plan.out_len)
    out = ctx.alloc(4 * nstreams * plan.out_len)
    try:
        ctx.h2d(d, x)
        all_rows = []
        for s in range(nstreams):
            assert plan.segments_dev(d + 8 * n * s, n, rows, nseg) == nseg
            all_rows.append(ctx.d2h(rows, (nseg, plan.out_len), np.float32))
        assert plan.exec_dev(d, n, out, nstreams=nstreams) == nseg
        psd = ctx.d2h(out, (nstreams, plan.out_len), np.float32)
    finally:
        for p in (d, rows, out):
            ctx.free(p)
    return np.array(all_rows), psd


@pytest.mark.parametrize('nfft,nseg,nstreams', [(4096, 9, 1), (4096, 10, 1), (256, 1, 1), (1024, 2, 1), (1000, 7, 1),
                                                (2048, 40, 2), (512, 33, 2)])
def test_selection_is_exact(ctx, hip, nfft, nseg, nstreams):
    noverlap = nfft // 2
    n = noverlap + nseg * (nfft - noverlap)
    x = np.concatenate([noise_tones(n, 7 + s) for s in range(nstreams)])
    plan = make_plan(ctx, hip, nfft, nfft, noverlap, scaling='raw')
    rows, psd = raw_rows_and_psd(ctx, hip, plan, x, nstreams)
    assert rows.shape[1] == nseg
    want = np.median(rows, axis=1)                      # float32, numpy's mean of the two middle values
    assert np.all(within_ulps(psd.astype(np.float64) * M.median_bias(nseg), want, 2))
    plan.close()


def test_selection_of_ties_and_zeros(ctx, hip):
    nfft, step = 1024, 512
    base = noise_tones(step, 3)
    x = np.tile(base, 42)                              # every segment holds the same samples: 41 identical rows
    plan = make_plan(ctx, hip, nfft, nfft, nfft - step, scaling='raw')
    rows, psd = raw_rows_and_psd(ctx, hip, plan, x)
    assert rows.shape[1] == 41 and np.all(rows[0] == rows[0, :1])      # bit-identical rows
    assert np.all(within_ulps(psd[0].astype(np.float64) * M.median_bias(41), rows[0, 0], 2))
    rows, psd = raw_rows_and_psd(ctx, hip, plan, np.zeros(41 * step, np.complex64))
    assert np.all(rows == 0) and np.all(psd == 0)
    rows, psd = raw_rows_and_psd(ctx, hip, plan, np.tile(base, 41))      # 40 rows: the mean of two equal values
    assert rows.shape[1] == 40 and np.all(rows[0] == rows[0, :1])
    assert np.all(within_ulps(psd[0].astype(np.float64) * M.median_bias(40), rows[0, 0], 2))
    plan.close()


def test_nan_sample_gives_nan_bins(ctx, hip):
    x = noise_tones(512 * 20, 4)
    x[3000] = np.nan
    plan = make_plan(ctx, hip, 1024, 1024, 512)
    psd = plan.exec(x)
    ref = M.welch_median(x, nperseg=1024, noverlap=512)
    assert np.array_equal(np.isnan(psd), np.isnan(ref)) and np.isnan(psd).all()
    plan.close()


# ---- 3. end to end -------------------------------------------------------------------------------------------------

def bursty(n, seg, seed, every=30, gain_db=30.0):
    """noise + tones; a burst 30 dB up over one segment length every `every` half-segment blocks (10 % of the 50 %-overlap
    segments touched)"""
    x = noise_tones(n, seed).astype(np.complex128)
    clean = x.copy()
    rng = np.random.default_rng(seed + 1)
    amp = 10.0 ** (gain_db / 20.0)
    step = seg // 2
    for b in range(1, n // step - 2, every):
        x[b * step:b * step + seg] += amp * (rng.standard_normal(seg) + 1j * rng.standard_normal(seg)) / np.sqrt(2.0)
    return x.astype(np.complex64), clean.astype(np.complex64)


@pytest.mark.parametrize('nfft', [4096, 1024, 1000])
def test_end_to_end_against_the_oracle(ctx, hip, nfft):
    step = nfft // 2
    x, clean = bursty(step * 601, nfft, 11)
    plan = make_plan(ctx, hip, nfft, nfft, step)
    psd = plan.exec(x).astype(np.float64)
    nseg = plan.last_nseg
    g = plan.segments(x).astype(np.float64)
    r = M.welch_rows(x, nperseg=nfft, noverlap=step)
    assert g.shape == r.shape == (nseg, nfft)
    bias = M.median_bias(nseg)
    ref = np.median(r, axis=0) / bias
    bound = np.max(np.abs(g - r), axis=0) / bias + np.spacing(np.abs(psd).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(psd - ref) <= bound)
    upper = ref >= np.median(ref)
    assert np.max(np.abs(psd - ref)[upper] / ref[upper]) < RTOL
    if nfft == 4096:
        # what the median is for: the noise floor of the bursty input stays within 1 dB of the burst-free PSD; the mean
        # goes 15 dB and more above it
        _, base = R.welch_np(clean, nperseg=nfft, noverlap=step)
        noise = base < 3.0 * np.median(base)
        mean_plan = make_plan(ctx, hip, nfft, nfft, step, average='mean')
        mean = mean_plan.exec(x).astype(np.float64)
        db = lambda v: 10.0 * np.log10(np.mean(v[noise]))
        assert abs(db(psd) - db(base)) < 1.0, (db(psd), db(base))
        assert db(mean) - db(base) >= 15.0, (db(mean), db(base))
        mean_plan.close()
    plan.close()


# ---- 4. the full C2 shape --------------------------------------------------------------------------------------------

def test_full_c2_shape_matches_a_sort(ctx, hip):
    import torch
    n, nfft = 1 << 28, 4096
    dev = torch.device('cuda', 0)
    x = torch.empty(2 * n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.synth_iq(x.data_ptr(), n, 2024, R.TONES, R.DC)
    raw = make_plan(ctx, hip, nfft, nfft, nfft // 2, scaling='raw')
    dens = make_plan(ctx, hip, nfft, nfft, nfft // 2, scaling='density')
    nseg = raw.nseg(n)
    rows = torch.empty((nseg, nfft), dtype=torch.float32, device=dev)
    out = torch.empty((2, nfft), dtype=torch.float32, device=dev)
    assert raw.segments_dev(x.data_ptr(), n, rows.data_ptr(), nseg) == nseg
    assert raw.exec_dev(x.data_ptr(), n, out[0].data_ptr()) == nseg
    assert dens.exec_dev(x.data_ptr(), n, out[1].data_ptr()) == nseg
    ctx.sync()
    k = (nseg - 1) // 2
    want = torch.empty(nfft, dtype=torch.float32, device=dev)
    for b0 in range(0, nfft, 256):
        srt, _ = torch.sort(rows[:, b0:b0 + 256].contiguous(), dim=0)
        want[b0:b0 + 256] = srt[k] if nseg % 2 else (srt[k] + srt[k + 1]) * 0.5
        del srt
    want = want.cpu().numpy()
    psd_raw, psd_dens = out.cpu().numpy()
    del rows
    assert np.all(within_ulps(psd_raw.astype(np.float64) * M.median_bias(nseg), want, 2))
    win = window('hann', nfft)
    scale = 1.0 / np.sum(np.float32(win).astype(np.float64) ** 2)
    assert np.all(within_ulps(psd_raw.astype(np.float64) * scale, psd_dens, 2))
    raw.close()
    dens.close()


# ---- 5. busy stream, schedules ------------------------------------------------------------------------------------

def test_exec_async_behind_a_busy_stream_and_every_schedule(ctx, hip):
    from test_chain_async_gpu import Hog
    hog = Hog(ctx, hip)
    try:
        xs = [noise_tones(2048 * (8 + 13 * i), 30 + i) for i in range(4)]

        def run(busy):
            # growing nsamples: each ticket may grow the rows workspace (ensure() drains the stream before it frees the
            # old one, so no queued ticket reads freed memory); then the same sequence again - no workspace or pinned
            # ring slot grows now - with all four tickets queued behind the hog
            plan = make_plan(ctx, hip, 4096, 4096, 2048, fftshift=True)
            probe = hog.start() if busy else None
            if busy:
                assert hog.busy(probe), 'the hog is too short'
            tickets = [plan.exec_async(x) for x in xs]
            got = [plan.wait(t) for t in tickets]
            if busy:
                hog.finish(probe)
                probe = hog.start()
            tickets = [plan.exec_async(x) for x in xs]
            if busy:
                assert hog.busy(probe), 'the stream drained before the tickets were enqueued'
            got += [plan.wait(t) for t in tickets]
            if busy:
                hog.finish(probe)
            plan.close()
            return got
        idle, busy = run(False), run(True)
        for a, b in zip(idle, busy):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for i, x in enumerate(xs):
            assert np.array_equal(idle[i].view(np.uint32), idle[4 + i].view(np.uint32))
            ref = np.fft.fftshift(M.welch_median(x, nperseg=4096, noverlap=2048))
            upper = ref >= np.median(ref)
            assert np.max(np.abs(idle[i] - ref)[upper] / ref[upper]) < RTOL
    finally:
        hog.close()
    x = noise_tones(1 << 20, 5)
    outs = []
    for sched in (hip.SCHED_CONTIGUOUS, hip.SCHED_INTERLEAVED, hip.SCHED_DYNAMIC):
        plan = make_plan(ctx, hip, 4096, 4096, 2048)
        plan.set_schedule(sched)
        outs.append(plan.exec(x))
        plan.close()
    assert all(np.array_equal(outs[0].view(np.uint32), o.view(np.uint32)) for o in outs[1:])


# ---- 6. refusals, defaults -----------------------------------------------------------------------------------------

def test_refusals_and_the_default_is_the_mean(ctx, hip):
    x = noise_tones(1 << 16, 9)
    plan = make_plan(ctx, hip, 4096, 4096, 2048)
    d = ctx.alloc(x.nbytes)
    out = ctx.alloc(4 * 4 * 4096)
    try:
        ctx.h2d(d, x)
        for call in (lambda: plan.partial_dev(d, len(x), out), lambda: plan.scale_dev(out, 10, out),
                     lambda: plan.accumulate(x), lambda: plan.finalize(), lambda: plan.csd(x, x),
                     lambda: plan.ctx.check(plan.ctx.lib.oth_csd_partial_dev(plan.h, hip.C.c_void_p(d), hip.C.c_void_p(d),
                                                                              len(x), hip.C.c_void_p(out), None), 'csd_partial'),
                     lambda: plan.ctx.check(plan.ctx.lib.oth_csd_scale_dev(plan.h, hip.C.c_void_p(out), 10, None, None, None,
                                                                            None), 'csd_scale'),
                     lambda: plan.ctx.check(plan.ctx.lib.oth_csd_exec_dev(plan.h, hip.C.c_void_p(d), hip.C.c_void_p(d),
                                                                           len(x), hip.C.c_void_p(out), None, None, None,
                                                                           None), 'csd_exec_dev')):
            with pytest.raises(hip.HipError) as ei:
                call()
            assert ei.value.code == -3 and 'MEDIAN' in str(ei.value)
        with pytest.raises(hip.HipError) as ei:
            plan.segments_dev(d, len(x), out, plan.nseg(len(x)) - 1)
        assert ei.value.code == -1
        mean = make_plan(ctx, hip, 4096, 4096, 2048, average='mean')
        mean.accumulate(x[:5000])
        with pytest.raises(hip.HipError) as ei:
            mean.set_average('median')
        assert ei.value.code == -5
        mean.reset()
        mean.set_average('median')
        mean.set_average('mean')
        a = make_plan(ctx, hip, 4096, 4096, 2048, average='mean')
        psd_a, psd_b = a.exec(x), mean.exec(x)
        assert np.array_equal(psd_a.view(np.uint32), psd_b.view(np.uint32)) and a.last_recipe() == mean.last_recipe()
        a.close()
        mean.close()
    finally:
        ctx.free(d)
        ctx.free(out)
    plan.close()
