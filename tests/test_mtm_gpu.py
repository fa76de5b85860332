"""GPU tests of the multitaper plans (oth_mtm_plan, csrc/mtm.hip): every bin of every case within RTOL = 1e-4 of the
float64 oracle (tests/mtm_oracle.py), the DC-offset cases that tell a kernel with a pilot from one without, every exec
form, the refusals, and the helpers / scan method / legacy sensor on top.  A float32 emulation of the parity cases on the
CPU (pocketfft on complex64, tree sums) read at most 7.2e-6, of the DC-offset cases 1.1e-5 with the pilot and 2.8e-4
without."""
import os

import numpy as np
import pytest

import median_oracle as M
import mtm_oracle as O
from oracle import ref_cpu as R
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import SCALINGS, noise_tones, window

pytestmark = pytest.mark.gpu


def relerr(got, ref):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / ref))


def capture(nperseg, ov, nseg, seed, offset=0.0):
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    x = noise_tones(noverlap + nseg * step + step // 3, seed)
    return (x + np.complex64(offset)).astype(np.complex64), noverlap


# ---- 1. parity ------------------------------------------------------------------------------------------------------

PARITY_CASES = [  # nfft, nperseg, overlap %, segments, NW, K, scaling, fftshift, trim, db
    (64, 64, 0, 1, 2, 3, 'density', False, 0, False),
    (256, 256, 50, 1, 2.5, 4, 'raw', True, 0, False),
    (1024, 1024, 0, 1, 4, 7, 'density', True, 16, False),
    (4096, 4096, 0, 1, 4, 7, 'density', False, 0, True),
    (4096, 4096, 50, 9, 2.5, 4, 'over_n2', False, 0, False),
    (4096, 1024, 0, 1, 3, 5, 'density', True, 0, False),          # zero-padded
    (4096, 1000, 0, 3, 3, 5, 'raw', False, 100, False),
    (8192, 8192, 0, 1, 4, 7, 'density', True, 32, True),
    (16384, 16384, 0, 1, 4, 7, 'density', False, 0, False),
    (16384, 16384, 50, 3, 8, 15, 'over_n2', True, 0, False),
    (2048, 2048, 75, 20, 2, 3, 'density', False, 0, False),
]


@pytest.mark.parametrize('weights', ['unity', 'eigen'])
@pytest.mark.parametrize('nfft,nperseg,ov,nseg,nw,K,scaling,fftshift,trim,db', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, nperseg, ov, nseg, nw, K, scaling, fftshift, trim, db, weights):
    x, noverlap = capture(nperseg, ov, nseg, nfft + ov + K)
    plan = ctx.mtm_plan(nfft, nperseg=nperseg, noverlap=noverlap, nw=nw, ntapers=K, weights=weights,
                        scaling=SCALINGS[scaling], fftshift=fftshift, trim_bins=trim, db=db)
    got = plan.exec(x)
    assert plan.last_nseg == nseg and got.shape == (nfft - 2 * trim,)
    assert plan.last_recipe().startswith('kernel=mtm nfft=%d ntapers=%d W=' % (nfft, K))
    ref = M.shift_trim_db(O.mtm_psd(x, nfft, nperseg, noverlap, nw, K, weights, True, scaling), fftshift, trim)
    lin = 10.0 ** (got.astype(np.float64) / 10.0) if db else got
    err = relerr(lin, ref)
    print('mtm parity %s %s: worst bin %.2e' % ((nfft, nperseg, ov, nseg, nw, K), weights, err))
    assert err < RTOL
    plan.close()


def test_default_taper_count_and_no_detrend(ctx, hip):
    x, _ = capture(1024, 0, 2, 5)
    plan = ctx.mtm_plan(1024, nw=3.0, detrend=hip.DETREND_NONE)      # ntapers = int(2 nw) - 1 = 5
    assert plan.ntapers == 5 and plan.tapers.shape == (5, 1024) and plan.ratios.shape == (5,)
    got = plan.exec(x)
    ref = O.mtm_psd(x, 1024, nw=3.0, K=5, detrend=False)
    assert relerr(got, ref) < RTOL
    plan.close()


# ---- 2. one taper is the Welch plan of that window ----------------------------------------------------------------------

@pytest.mark.parametrize('nfft', [1024, 4096])
def test_one_taper_equals_the_welch_plan_of_that_window(ctx, hip, nfft):
    """20 segments: a single segment at K = 1 has deep nulls that read 3e-5 in float32 alone and is not gated per bin."""
    x, noverlap = capture(nfft, 50, 20, 77)
    w = window('hann', nfft)
    plan = ctx.mtm_plan(nfft, noverlap=noverlap, tapers=w[None, :], weights='unity')
    welch = ctx.welch_plan(nfft, noverlap=noverlap, window=w, kernel=hip.KERNEL_GENERIC)
    got, ref_plan = plan.exec(x), welch.exec(x)
    assert plan.last_nseg == welch.last_nseg == 20
    _, ref = R.welch_np(x, nperseg=nfft, noverlap=noverlap)
    assert relerr(got, ref) < RTOL and relerr(got, ref_plan.astype(np.float64)) < RTOL
    plan.close()
    welch.close()


# ---- 3. DC offset: the pilot ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('offset', [35.0 + 0.0j, 25.0 - 25.0j])
@pytest.mark.parametrize('nfft,nw,K', [(1024, 4, 7), (4096, 4, 7), (4096, 2, 3), (16384, 4, 7)])
def test_every_bin_under_a_dc_offset_of_35_sigma(ctx, hip, nfft, nw, K, offset):
    """Single segments.  The float32 mean of such a segment taken directly leaves up to 2.8e-4 on a bin ((4096, 2, 3));
    with the pilot off first the emulation read at most 1.1e-5."""
    x, _ = capture(nfft, 0, 1, 900 + nfft + K, offset)
    plan = ctx.mtm_plan(nfft, nw=nw, ntapers=K)
    got = plan.exec(x)
    ref = O.mtm_psd(x, nfft, nw=nw, K=K)
    err = relerr(got, ref)
    print('mtm dc offset %s %s: worst bin %.2e' % ((nfft, nw, K), offset, err))
    assert plan.last_nseg == 1 and err < RTOL
    plan.close()


# ---- 4. exec forms ------------------------------------------------------------------------------------------------------

def test_exec_dev_64_streams_of_16384_points(ctx, hip):
    nfft, K, nstreams, sentinel = 16384, 7, 64, np.float32(-7.0)
    x = np.concatenate([noise_tones(nfft, 200 + s) for s in range(nstreams)])
    plan = ctx.mtm_plan(nfft, nw=4.0, ntapers=K)
    d = ctx.alloc(x.nbytes)
    out = ctx.alloc(4 * (nstreams + 1) * nfft)
    try:
        ctx.h2d(d, x)
        ctx.h2d(out, np.full((nstreams + 1) * nfft, sentinel, np.float32))
        assert plan.exec_dev(d, nfft, out, nstreams=nstreams) == 1
        rows = ctx.d2h(out, (nstreams + 1, nfft), np.float32)
    finally:
        ctx.free(d)
        ctx.free(out)
    assert np.all(rows[nstreams] == sentinel) and np.all(rows[:nstreams] > 0)      # every row written, nothing behind them
    assert 'ntapers=7 W=7 ' in plan.last_recipe()                                  # a single segment: one workgroup per taper
    worst = max(relerr(rows[s], O.mtm_psd(x[s * nfft:(s + 1) * nfft], nfft, nw=4.0, K=K)) for s in range(nstreams))
    print('mtm exec_dev 64 x 16384: worst bin %.2e' % worst)
    assert worst < RTOL
    plan.close()


def test_exec_async_tickets(ctx, hip):
    plan = ctx.mtm_plan(4096, nw=4.0)
    xs = [noise_tones(4096 * (1 + i), 300 + i) for i in range(4)]
    tickets = [plan.exec_async(x) for x in xs]
    assert plan.outstanding == 4
    got = [plan.wait(t) for t in tickets]
    assert plan.outstanding == 0
    for i, x in enumerate(xs):
        assert np.array_equal(got[i].view(np.uint32), plan.exec(x).view(np.uint32)) and plan.last_nseg == 1 + i
        assert relerr(got[i], O.mtm_psd(x, 4096, nw=4.0)) < RTOL
    import time
    t = plan.exec_async(xs[0])
    deadline = time.monotonic() + 20.0
    polled = plan.poll(t)
    while polled is None and time.monotonic() < deadline:
        polled = plan.poll(t)
    assert polled is not None and np.array_equal(polled.view(np.uint32), got[0].view(np.uint32))
    plan.close()


def test_partials_accumulate_and_repeat_runs(ctx, hip):
    nfft, K = 4096, 4
    x, noverlap = capture(nfft, 50, 9, 31)
    step = nfft - noverlap
    plan = ctx.mtm_plan(nfft, noverlap=noverlap, nw=2.5, ntapers=K, fftshift=True, trim_bins=8)
    one = plan.exec(x)
    assert np.array_equal(one.view(np.uint32), plan.exec(x).view(np.uint32))      # bit-identical run to run
    # two halves that share the overlap halo: segments 0 ... 4 and 5 ... 8
    a, b = x[:5 * step + noverlap], x[5 * step:]
    d = ctx.alloc(x.nbytes)
    sums = ctx.alloc(4 * 2 * nfft)
    out = ctx.alloc(4 * plan.out_len)
    try:
        ctx.h2d(d, a)
        assert plan.partial_dev(d, len(a), sums) == 5
        ctx.h2d(d, b)
        assert plan.partial_dev(d, len(b), sums + 4 * nfft) == 4
        both = ctx.d2h(sums, (2, nfft), np.float32)
        ctx.h2d(sums, both[0] + both[1])
        plan.scale_dev(sums, 9, out)
        sharded = ctx.d2h(out, (plan.out_len,), np.float32)
    finally:
        for p in (d, sums, out):
            ctx.free(p)
    assert relerr(sharded, one.astype(np.float64)) < 2e-6
    prev = 0
    for cut in (1000, 5000, 5001, 12000, len(x)):                                  # uneven chunks
        plan.accumulate(x[prev:cut])
        prev = cut
    streamed = plan.finalize()
    assert plan.last_nseg == 9 and relerr(streamed, one.astype(np.float64)) < 2e-6
    plan.set_schedule(hip.SCHED_INTERLEAVED)                                       # accepted, no effect
    assert np.array_equal(one.view(np.uint32), plan.exec(x).view(np.uint32))
    plan.close()


def test_one_long_launch(ctx, hip):
    import torch
    n, nfft, K = 1 << 24, 4096, 4
    dev = torch.device('cuda', 0)
    x = torch.empty(2 * n, dtype=torch.float32, device=dev)
    out = torch.empty(nfft, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.synth_iq(x.data_ptr(), n, 2025, R.TONES, R.DC)
    plan = ctx.mtm_plan(nfft, nw=2.5, ntapers=K)
    assert plan.exec_dev(x.data_ptr(), n, out.data_ptr()) == n // nfft
    ctx.sync()
    host = x.cpu().numpy().view(np.complex64)
    got = out.cpu().numpy()
    W = int(plan.last_recipe().split(' W=')[1].split()[0])
    assert 256 <= W <= 16384                                                       # about what the device holds at once
    ref = np.zeros(nfft)
    for c0 in range(0, n, 1 << 21):                                                # (the oracle in slices of 512 segments)
        ref += O.mtm_psd(host[c0:c0 + (1 << 21)], nfft, nw=2.5, K=K) * ((1 << 21) / n)
    err = relerr(got, ref)
    print('mtm long launch 2^24 at 4096, K 4 (W %d): worst bin %.2e' % (W, err))
    assert err < RTOL
    plan.close()


def test_fused_step_is_no_slower_than_the_generic_composition(tmp_path):
    """tools/mtm_time.py in a child process: whole steps between HIP events, fused plan and the K-launch compositions
    alternating, at the three shapes of DESIGN.md 4.9.  Its gate - fused <= 1.05 x the OTH_KERNEL_GENERIC composition (the same
    butterflies with K - 1 fewer reads and launches; 5 % for box noise) at every shape - is its exit status."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / 'mtm_shapes.txt')
    p = subprocess.run([sys.executable, os.path.join(root, 'tools', 'mtm_time.py'), '15', '--out', out, '--no-host'],
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.count('gate: fused') == 3 and 'FAILED' not in p.stdout and os.path.exists(out)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------

def test_refusals(ctx, hip):
    UNSUPPORTED, INVALID = -3, -1
    x, _ = capture(4096, 0, 2, 9)
    plan = ctx.mtm_plan(4096, nw=4.0)
    d = ctx.alloc(x.nbytes)
    out = ctx.alloc(4 * 5 * 4096)
    lib, vp = ctx.lib, hip.C.c_void_p
    try:
        ctx.h2d(d, x)
        for call in (lambda: plan.set_average('median'),
                     lambda: plan.segments_dev(d, len(x), out, 2),
                     lambda: plan.csd(x, x),
                     lambda: plan.csd_exec_dev(d, d, len(x), out),
                     lambda: plan.csd_partial_dev(d, d, len(x), out),
                     lambda: plan.csd_scale_dev(out, 2, out),
                     lambda: plan.set_kernel(hip.KERNEL_TUNED),
                     lambda: plan.set_tuning('pipe'),
                     lambda: plan.set_tuning('seg3')):
            with pytest.raises(hip.HipError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED and 'multitaper' in str(ei.value), str(ei.value)
        plan.set_kernel(hip.KERNEL_GENERIC)
        plan.set_kernel(hip.KERNEL_AUTO)
        plan.set_tuning(None, sched=1, chunk=4)                                    # no variant: accepted
        plan.set_tuning('')
        for sched in (hip.SCHED_CONTIGUOUS, hip.SCHED_INTERLEAVED, hip.SCHED_DYNAMIC):
            plan.set_schedule(sched)
        got = plan.exec(x)                                                         # ... and the plan still works
        assert relerr(got, O.mtm_psd(x, 4096, nw=4.0)) < RTOL and plan.last_recipe().startswith('kernel=mtm')
    finally:
        ctx.free(d)
        ctx.free(out)
    plan.close()
    for nfft in (1000, 32768, 32, 65536, 12288):
        with pytest.raises(hip.HipError) as ei:
            ctx.mtm_plan(nfft, nw=4.0)
        assert ei.value.code == UNSUPPORTED and 'power of two' in str(ei.value)
    with pytest.raises(hip.HipError) as ei:
        ctx.mtm_plan(1024, nw=4.0, scaling=hip.SCALE_SPECTRUM)
    assert ei.value.code == UNSUPPORTED and 'odd taper' in str(ei.value)
    # the C entry's own argument checks (the Python surface raises ValueError for most of these before it is called)
    t = np.ascontiguousarray(plan.tapers)
    h = vp()

    def c_plan(nfft=4096, nperseg=4096, noverlap=0, ntapers=7, tapers=t, weights=None, detrend=1, scaling=1, fs=1.0):
        w = None if weights is None else np.asarray(weights, np.float32)
        return lib.oth_mtm_plan(ctx.h, nfft, nperseg, noverlap, ntapers, hip._fptr(tapers) if tapers is not None else None,
                                hip._fptr(w) if w is not None else None, detrend, scaling, fs, 0, 0, hip.C.byref(h))
    for kw in (dict(ntapers=0), dict(ntapers=65), dict(tapers=None), dict(nperseg=0), dict(nperseg=4097), dict(noverlap=4096),
               dict(noverlap=-1), dict(weights=[1, 1, 1, -1, 1, 1, 1]), dict(weights=[0] * 7),
               dict(weights=[1, 1, float('nan'), 1, 1, 1, 1]), dict(detrend=9), dict(scaling=7), dict(fs=0.0), dict(nfft=0)):
        assert c_plan(**kw) == INVALID and not h.value, kw


# ---- 6. helpers, the scan method, the legacy sensor ------------------------------------------------------------------------

def test_helpers_and_scan_method(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    Sf, N = 1000000, 1024
    x = R.synth_iq(20000, 41)[:8192]
    short = x[:700]                                                                # shorter than nFFT: one zero-padded segment
    for v, NW, K in ((x, 4.0, None), (short, 4.0, None), (x, 2.5, 4)):
        ref = O.scan_psd(v, N, Sf, NW, K)
        assert np.isclose(T.mtm_power_estimate(v, N, Sf, NW, K, ctx=ctx), ref.sum(), rtol=1e-5)
        axis, db = T.mtm_plot_dB(v, Sf, 433e6, N, NW, K, ctx=ctx)
        assert np.allclose(axis, np.fft.fftshift(np.fft.fftfreq(N, 1.0 / Sf)) + 433e6)
        assert np.max(np.abs(np.asarray(db) - 10 * np.log10(ref + 1e-20))) < 10 * np.log10(1 + RTOL)
        Fr = float(Sf) / N
        bb = R.frange(-Sf // 2, Sf // 2, 50e3)
        psd, ax, plc = T.src_power_mtm(v, len(v), N, Fr, Sf, bb, 25e3 / Fr, NW, K, ctx=ctx)
        rpsd, rax, rplc = O.src_power_mtm(v, len(v), N, Fr, Sf, bb, 25e3 / Fr, NW, K)
        assert relerr(psd, rpsd) < RTOL and np.allclose(ax, rax) and np.allclose(plc, rplc, rtol=1e-4)
    for v, n_fft in ((x, N), (short, 0)):
        thr, plc, noise, cons = O.fast_spectrum_scan_mtm(v, 0, 50e3, 25e3, n_fft, Sf, 5, 1e-11, 1)
        scan = T.SpectrumScan(v, 0, 50e3, 25e3, n_fft, Sf, 'mtm', 5, 1, ctx=ctx)
        g_thr, g_plc, g_noise, g_cons = scan.wait(1e-11)
        assert np.isclose(g_thr, thr, rtol=1e-4) and np.isclose(g_noise, noise, rtol=1e-4)
        assert np.allclose(g_plc, plc, rtol=1e-4) and g_cons == cons and len(cons) > 0
        assert T.fast_spectrum_scan(v, 0, 50e3, 25e3, n_fft, Sf, 'mtm', 5, 1e-11, 1, ctx=ctx)[3] == cons
    with pytest.raises(ValueError):
        T.SpectrumScan(x, 0, 50e3, 25e3, N, Sf, 'thomson', 5, 1, ctx=ctx)


def test_legacy_spectrum_sensor_answers_sc_with_the_mtm_method(ctx, tmp_path):
    import ofdm_tools
    Sf, N = 1000000, 1024
    blk = ofdm_tools.spectrum_sensor(8192, sample_rate=Sf, fft_len=N, channel_space=50e3, search_bw=25e3, method='mtm',
                                     thr_leveler=5, tune_freq=0, alpha_avg=1, ctx=ctx, log=True, log_dir=str(tmp_path))
    out = []
    blk.msg_connect('PDU spect_msg', out.append)
    x = R.synth_iq(20000, 41)
    assert blk.work([x], []) == 8192
    blk.post('PDU from_cogeng', ({}, 'SC'))
    thr, plc, noise, cons = O.fast_spectrum_scan_mtm(x[:8192], 0, 50e3, 25e3, N, Sf, 5, 1e-11, 1)
    got = dict(out)
    assert np.isclose(got['thre'], thr, rtol=1e-4) and np.isclose(got['nois'], noise, rtol=1e-4)
    assert got['cons'] == cons and len(cons) > 0
    assert np.allclose(blk.get_power_level_ch(), plc, rtol=1e-4)
    assert os.path.exists(blk.log_file.path)
