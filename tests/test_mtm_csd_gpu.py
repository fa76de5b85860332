"""GPU tests of the two-channel multitaper plans (oth_mtm_csd_plan, csrc/mtmcsd.hip, coherence_estimator(method='mtm')):
Pxx, Pyy, Pxy and Cxy against the float64 oracle (tests/mtm_csd_oracle.py) on test_csd_gpu's inputs - y = 0.7 x delayed
by five samples plus independent noise, both with a DC term - and its five gates, each on every bin, all RTOL = 1e-4:
relerr(Pxx), relerr(Pyy), |dPxy| / sqrt(Pxx Pyy), |d Im Pxy| / sqrt(Pxx Pyy) on its own, |dCxy|.

  1. parity at the smallest shapes where the kernel can still go wrong (every size, zero padding, an nperseg that is no
     multiple of the thread count), unity and eigen weights - one item per workgroup in all of them - and 1b. launches
     with more items than resident workgroups at each kernel form: runs of several items that cut through segments;
  2. the three finalize routes, read back from the recipe's W;
  3. a DC offset of 35 sigma on both channels: a kernel with a pilot per channel against one without;
  4. every entry point, NULL outputs, the time-sharded form, the dB refusal, repeat runs, the one-channel exec;
  5. degenerate inputs: a silent channel, identical channels, one NaN sample, gains of 2^+-40;
  6. coherence_estimator(method='mtm') -> coherence_detector.

A float32 emulation on the CPU (pocketfft on complex64, float32 accumulators, pilot + residual mean; sizes 64 ... 16384,
K 3 ... 15, 1 ... 9 segments, a 35-sigma offset) read at most 5.5e-6 (Pxx, Pyy) / 5.2e-6 (Pxy) / 3.1e-6 (Cxy).
Worst readings on an MI355X (Pxx or Pyy / Pxy / Im Pxy / Cxy):
  1. 6.1e-6 / 3.5e-6 / 3.0e-6 / 2.7e-6 (16384 points, one segment, K 7; every other shape below 3.8e-6);
  2. 1.7e-6 / 1.0e-6 / 8.0e-7 / 9.0e-7;
  3. 8.1e-6 / 4.7e-6 / 4.2e-6 / 2.7e-6;
  4. 7.8e-7 / 4.2e-7 / 2.6e-7 / 5.1e-7 (raw sums 4 + 2 and the scale stage included); Pxx of csd against the one-channel
     exec 7.6e-7;
  5. gains 4.9e-7 / 4.9e-7 / 3.3e-7 / 5.5e-7, Cxy bit-identical; identical channels |Cxy - 1| = 0 and Im Pxy = 0;
  6. 1.5e-6 / 7.0e-7 / 5.1e-7 / 5.7e-7."""
import numpy as np
import pytest

import mtm_csd_oracle as MC
import mtm_oracle as MO
from oracle import ref_cpu as R
from test_csd_gpu import SENTINEL, UNSUPPORTED, DeviceOutputs, NAMES, _pair, errors, finalize_route, pair, recipe_W
from test_hip_parity import RTOL, ctx, hip, relerr  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import SCALINGS

pytestmark = pytest.mark.gpu

WORST = {}


def gate(section, label, got, ref):
    e = errors(got, ref)
    w = WORST.setdefault(section, [0.0] * 4)
    for i, v in enumerate((max(e[0], e[1]), e[2], e[3], e[4])):
        w[i] = max(w[i], v)
    print('mtm csd %s | %s | Pxx %.2e Pyy %.2e Pxy %.2e ImPxy %.2e Cxy %.2e' % ((section, label) + e))
    print('mtm csd %s | worst so far: Pxx or Pyy %.2e Pxy %.2e ImPxy %.2e Cxy %.2e' % ((section,) + tuple(w)))
    assert max(e) < RTOL, (section, label, e)


def make(ctx, nfft, nperseg=None, ov=0, nw=4.0, K=None, weights='unity', scaling='density', fs=1.0, fftshift=False, trim=0,
         db=False):
    nperseg = nfft if nperseg is None else nperseg
    return ctx.mtm_csd_plan(nfft, nperseg=nperseg, noverlap=nperseg * ov // 100, nw=nw, ntapers=K, weights=weights,
                            scaling=SCALINGS[scaling], fs=fs, fftshift=fftshift, trim_bins=trim, db=db)


# ---- 1. parity ------------------------------------------------------------------------------------------------------

PARITY_CASES = [  # nfft, nperseg, overlap %, segments, NW, K, scaling, fftshift, trim
    (64, 64, 0, 1, 2, 3, 'density', False, 0),
    (256, 256, 50, 2, 2.5, 4, 'raw', True, 0),
    (1024, 1024, 0, 1, 4, 7, 'density', True, 16),
    (4096, 1000, 0, 3, 3, 5, 'raw', False, 100),                  # zero-padded, nperseg no multiple of the thread count
    (4096, 4096, 50, 9, 2.5, 4, 'over_n2', False, 0),
    (8192, 8192, 0, 1, 4, 7, 'density', True, 32),
    (16384, 16384, 0, 1, 4, 7, 'density', False, 0),
    (16384, 16384, 50, 3, 8, 15, 'over_n2', True, 0),             # three segments: neighbouring workgroups in different ones
]
ONCE = [(n, n, 0, 1, 2, 3, 'density', False, 0) for n in (128, 512, 2048)]      # every other power of two


@pytest.mark.parametrize('nfft,nperseg,ov,nseg,nw,K,scaling,fftshift,trim,weights',
                         [c + (w,) for c in PARITY_CASES for w in ('unity', 'eigen')] + [c + ('unity',) for c in ONCE])
def test_parity_with_the_float64_oracle(ctx, hip, nfft, nperseg, ov, nseg, nw, K, scaling, fftshift, trim, weights):
    noverlap = nperseg * ov // 100
    x, y = pair(nperseg, noverlap, nseg, nfft + ov + K)
    plan = make(ctx, nfft, nperseg, ov, nw, K, weights, scaling, 1.0, fftshift, trim)
    got = plan.csd(x, y)
    rec = plan.last_recipe()
    assert plan.last_nseg == nseg and all(len(v) == nfft - 2 * trim for v in got)
    assert rec.startswith('kernel=mtmcsd nfft=%d ntapers=%d W=' % (nfft, K)), rec
    ref = MC.mtm_csd(x, y, nfft, nperseg, noverlap, nw, K, weights, True, scaling, 1.0, None, fftshift, trim)
    gate('parity', '%s %s' % ((nfft, nperseg, ov, nseg, nw, K), weights), got, ref)
    plan.close()


# ---- 1b. runs of several items ------------------------------------------------------------------------------------------

LONG_RUNS = [  # nfft, overlap %, segments, NW, K: more (segment, taper) items than the device holds workgroups of the build
    (512, 50, 1200, 4, 7),        # 64 threads, samples kept, sums in registers: 8400 items on 16 workgroups per CU
    (4096, 0, 300, 2.5, 4),       # 512 threads, samples kept, two LDS buffers: 1200 items on two workgroups per CU
    (8192, 50, 300, 2.5, 4),      # 1024 threads, samples read again per taper: 1200 items on one workgroup per CU
    (16384, 50, 110, 4, 7),       # one buffer, X through the workspace, sums read, added and stored in the partial rows: 770
]


@pytest.mark.parametrize('nfft,ov,nseg,nw,K', LONG_RUNS)
def test_runs_of_several_items_per_workgroup(ctx, hip, nfft, ov, nseg, nw, K):
    """Every case above this one gives each workgroup ONE item (W = items below what the device holds).  Here W < items:
    a run adds several items into its sums, wraps the taper index, enters a new segment in the middle (`cuts`) and, at 16384 points, reads its sum rows back from the partial buffer."""
    noverlap = nfft * ov // 100
    x, y = pair(nfft, noverlap, nseg, 7 + nfft)
    plan = make(ctx, nfft, ov=ov, nw=nw, K=K, weights='eigen')
    got = plan.csd(x, y)
    rec = plan.last_recipe()
    W, items = recipe_W(rec), nseg * K
    print('mtm csd long | %s' % rec)
    assert plan.last_nseg == nseg and rec.startswith('kernel=mtmcsd nfft=%d ' % nfft)
    cuts = [items * wg // W for wg in range(1, W)]                              # first item of every run but the first
    assert 2 * W <= items and any(c % K for c in cuts), rec                    # runs of two items and more that cut segments
    gate('long', '%s W %d, %.1f items per run' % ((nfft, ov, nseg, nw, K), W, items / W), got,
         MC.mtm_csd(x, y, nfft, noverlap=noverlap, nw=nw, K=K, weights='eigen'))
    again = plan.csd(x, y)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, got))
    plan.close()


# ---- 2. the three finalize routes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('K,nseg,W,route', [(3, 1, 3, 'one-stage'), (5, 8, 40, 'two-stage'), (7, 12, 84, 'wide')])
def test_every_finalize_route_at_1024_points(ctx, hip, K, nseg, W, route):
    nfft = 1024
    x, y = pair(nfft, 0, nseg, 50 + K)
    plan = make(ctx, nfft, nw=4.0, K=K)
    got = plan.csd(x, y)
    rec = plan.last_recipe()
    assert plan.last_nseg == nseg and rec.startswith('kernel=mtmcsd ') and recipe_W(rec) == W, rec
    assert finalize_route(W, nfft) == route
    gate('routes', 'K %d nseg %d W %d %s' % (K, nseg, W, route), got, MC.mtm_csd(x, y, nfft, nw=4.0, K=K))
    plan.close()


# ---- 3. DC offset: a pilot per channel --------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,nw,K', [(1024, 4, 7), (4096, 2, 3), (16384, 4, 7)])
def test_every_bin_under_a_dc_offset_of_35_sigma_on_both_channels(ctx, hip, nfft, nw, K):
    """Single segments, different complex offsets on the channels: a kernel that took x's pilot (or none) off y leaves
    y's float32 mean behind, up to 2.8e-4 on a bin (tests/test_mtm_gpu.py)."""
    x, y = pair(nfft, 0, 1, 900 + nfft + K)
    x, y = (x + np.complex64(35.0 + 0.0j)).astype(np.complex64), (y + np.complex64(-25.0 + 25.0j)).astype(np.complex64)
    plan = make(ctx, nfft, nw=nw, K=K)
    got = plan.csd(x, y)
    assert plan.last_nseg == 1
    gate('dc', '%s' % ((nfft, nw, K),), got, MC.mtm_csd(x, y, nfft, nw=nw, K=K))
    plan.close()


# ---- 4. entry points ----------------------------------------------------------------------------------------------------------

def test_every_entry_point_null_outputs_and_the_time_sharded_form(ctx, hip):
    nfft, K, nw, nseg, fs, trim = 1024, 4, 2.5, 6, 2.5e6, 37
    x, y = pair(nfft, 0, nseg, 40 + nfft)
    plan = make(ctx, nfft, nw=nw, K=K, fs=fs, fftshift=True, trim=trim)
    m = plan.out_len
    assert m == nfft - 2 * trim
    ref = MC.mtm_csd(x, y, nfft, nw=nw, K=K, fs=fs, fftshift=True, trim=trim)
    host = dict(zip(NAMES, plan.csd(x, y)))
    assert plan.last_nseg == nseg
    gate('entry', 'csd', [host[k] for k in NAMES], ref)
    again = plan.csd(x, y)                                                         # bit-identical run to run
    assert all(np.array_equal(a.view(np.uint32), host[k].view(np.uint32)) for a, k in zip(again, NAMES))
    dx, dy, sums = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes), ctx.alloc(4 * 2 * 4 * nfft)
    out = DeviceOutputs(ctx, m)
    try:
        ctx.h2d(dx, x)
        ctx.h2d(dy, y)

        def exec_dev(**ptrs):
            assert plan.csd_exec_dev(dx, dy, len(x), **ptrs) == nseg
        dev = out.run(NAMES, exec_dev)
        for k in NAMES:
            assert np.array_equal(dev[k].view(np.uint32), host[k].view(np.uint32)), k
        for k in NAMES:                                                            # three NULLs: no fault, no stray store
            one = out.run((k,), exec_dev)
            assert np.array_equal(one[k].view(np.uint32), dev[k].view(np.uint32)), k
        # time-sharded: segments 0 ... 3 and 4, 5, raw sums added on the host, then the scale stage
        assert plan.csd_partial_dev(dx, dy, 4 * nfft, sums) == 4
        assert plan.csd_partial_dev(dx + 8 * 4 * nfft, dy + 8 * 4 * nfft, len(x) - 4 * nfft, sums + 16 * nfft) == 2
        both = ctx.d2h(sums, (2, 4 * nfft), np.float32).astype(np.float64)
        tot = both[0] + both[1]
        sxx, syy, sxy, n_ref = MC.mtm_csd_sums(x, y, nfft, nw=nw, K=K)
        assert n_ref == nseg
        gxy = tot[2 * nfft::2] + 1j * tot[2 * nfft + 1::2]
        raw = [tot[:nfft], tot[nfft:2 * nfft], gxy, np.abs(gxy) ** 2 / (tot[:nfft] * tot[nfft:2 * nfft])]
        gate('entry', 'raw sums 4 + 2', raw, [sxx, syy, sxy, np.abs(sxy) ** 2 / (sxx * syy)])
        ctx.h2d(sums, tot.astype(np.float32))
        sharded = out.run(NAMES, lambda **ptrs: plan.csd_scale_dev(sums, nseg, **ptrs))
        gate('entry', 'csd_scale_dev', [sharded[k] for k in NAMES], ref)
        one = out.run(('cxy',), lambda **ptrs: plan.csd_scale_dev(sums, nseg, **ptrs))
        assert np.array_equal(one['cxy'].view(np.uint32), sharded['cxy'].view(np.uint32))
    finally:
        out.free()
        for p in (dx, dy, sums):
            ctx.free(p)
    plan.close()


def test_db_output_is_refused_and_the_plan_goes_on(ctx, hip):
    nfft = 1024
    x, y = pair(nfft, 0, 2, 77)
    plan = make(ctx, nfft, nw=4.0, db=True)
    dx, dy, out = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes), ctx.alloc(4 * 5 * nfft)
    try:
        ctx.h2d(dx, x)
        ctx.h2d(dy, y)
        ctx.h2d(out, np.full(5 * nfft, SENTINEL, np.float32))
        for call in (lambda: plan.csd(x, y),
                     lambda: plan.csd_exec_dev(dx, dy, len(x), out, out + 4 * nfft, out + 8 * nfft, out + 16 * nfft),
                     lambda: plan.csd_partial_dev(dx, dy, len(x), out),
                     lambda: plan.csd_scale_dev(out, 2, out, out + 4 * nfft, out + 8 * nfft, out + 16 * nfft)):
            with pytest.raises(hip.HipError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED and 'not defined for the cross spectrum' in str(ei.value), str(ei.value)
        assert np.all(ctx.d2h(out, (5 * nfft,), np.float32) == SENTINEL)              # nothing was launched
    finally:
        for p in (dx, dy, out):
            ctx.free(p)
    got = plan.exec(x)                                                             # the plan still serves its own output
    assert relerr(10.0 ** (got.astype(np.float64) / 10.0), MO.mtm_psd(x, nfft, nw=4.0)) < RTOL
    plan.close()


def test_the_one_channel_exec_is_the_mtm_plan_and_mtm_plans_still_refuse(ctx, hip):
    nfft, nw, K = 4096, 2.5, 4
    x, y = pair(nfft, nfft // 2, 3, 5)
    two = make(ctx, nfft, ov=50, nw=nw, K=K)
    one = ctx.mtm_plan(nfft, noverlap=nfft // 2, nw=nw, ntapers=K)
    a, b = two.exec(x), one.exec(x)
    assert two.last_recipe().startswith('kernel=mtm nfft=') and two.last_nseg == one.last_nseg == 3
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pxx = two.csd(x, y)[0]
    assert two.last_recipe().startswith('kernel=mtmcsd nfft=')
    e = relerr(pxx, b.astype(np.float64))
    print('mtm csd entry | Pxx of csd against the one-channel exec: %.2e' % e)
    assert e < RTOL
    with pytest.raises(hip.HipError) as ei:
        one.csd(x, y)
    assert ei.value.code == UNSUPPORTED and 'multitaper' in str(ei.value), str(ei.value)
    for call in (lambda: two.set_average('median'), lambda: two.set_kernel(hip.KERNEL_TUNED), lambda: two.set_tuning('seg3')):
        with pytest.raises(hip.HipError) as ei:
            call()
        assert ei.value.code == UNSUPPORTED and 'multitaper' in str(ei.value), str(ei.value)
    with pytest.raises(hip.HipError) as ei:
        ctx.mtm_csd_plan(1000, nw=4.0)
    assert ei.value.code == UNSUPPORTED and 'power of two' in str(ei.value)
    with pytest.raises(hip.HipError) as ei:
        ctx.mtm_csd_plan(1024, nw=4.0, scaling=hip.SCALE_SPECTRUM)
    assert ei.value.code == UNSUPPORTED and 'odd taper' in str(ei.value)
    two.close()
    one.close()


# ---- 5. degenerate inputs ---------------------------------------------------------------------------------------------------------

DEG = dict(nfft=256, nw=2.0, K=3, nseg=2)


def degenerate(ctx, x, y):
    plan = make(ctx, DEG['nfft'], nw=DEG['nw'], K=DEG['K'])
    got = plan.csd(x, y)
    assert plan.last_nseg == DEG['nseg'] and plan.last_recipe().startswith('kernel=mtmcsd ')
    plan.close()
    return got


def degenerate_pair():
    return pair(DEG['nfft'], 0, DEG['nseg'], 70 + DEG['nfft'])


def test_a_silent_channel_gives_zero_power_and_nan_coherence(ctx, hip):
    x, _ = degenerate_pair()
    gxx, gyy, gxy, gc = degenerate(ctx, x, np.zeros_like(x))
    assert np.all(gyy == 0) and np.all(gxy.real == 0) and np.all(gxy.imag == 0) and np.all(np.isnan(gc))
    assert relerr(gxx, MO.mtm_psd(x, DEG['nfft'], nw=DEG['nw'], K=DEG['K'])) < RTOL


def test_identical_channels_give_coherence_one_and_no_imaginary_part(ctx, hip):
    x, _ = degenerate_pair()
    gxx, gyy, gxy, gc = degenerate(ctx, x, x)
    assert np.all(gxy.imag == 0) and np.all(gc == 1.0), (float(np.max(np.abs(gxy.imag))), float(np.max(np.abs(gc - 1.0))))
    assert np.array_equal(gxx, gyy) and np.array_equal(gxy.real, gxx)


def test_one_nan_sample_stays_in_its_channel(ctx, hip):
    x, y = degenerate_pair()
    bad = x.copy()
    bad[len(x) // 2 + 1] = np.complex64(complex(float('nan'), 0.0))
    gxx, gyy, gxy, gc = degenerate(ctx, bad, y)
    assert np.all(np.isnan(gxx)) and np.all(np.isnan(gxy.real)) and np.all(np.isnan(gxy.imag)) and np.all(np.isnan(gc))
    assert np.all(np.isfinite(gyy)) and relerr(gyy, MO.mtm_psd(y, DEG['nfft'], nw=DEG['nw'], K=DEG['K'])) < RTOL


def test_gains_of_2_to_the_40_leave_the_coherence_bit_identical(ctx, hip):
    x, y = degenerate_pair()
    base = degenerate(ctx, x, y)
    xs, ys = (x * np.float32(2.0 ** 40)).astype(np.complex64), (y * np.float32(2.0 ** -40)).astype(np.complex64)
    got = degenerate(ctx, xs, ys)
    assert np.array_equal(got[3].view(np.uint32), base[3].view(np.uint32))
    gate('degenerate', 'gains', got, MC.mtm_csd(xs, ys, DEG['nfft'], nw=DEG['nw'], K=DEG['K']))


# ---- 6. the block on top ----------------------------------------------------------------------------------------------------------------

def test_coherence_estimator_block_with_the_mtm_method(ctx, hip):
    import ofdm_tools
    N, Sf, tune = 1024, 2000000, 433000000
    x, y = _pair(2 * N, 31 + N)
    est = ofdm_tools.coherence_estimator(N, Sf, ctx=ctx, method='mtm')
    assert est.block_len == N and est._plan.ntapers == 7
    msgs = []
    est.msg_connect('coherence', msgs.append)
    # ragged work() calls: 700 + 700 + 648 samples; the second completes vector 0, the third vector 1
    for lo, hi, want in ((0, 700, 0), (700, 1400, 1), (1400, 2048, 2)):
        assert est.work([x[lo:hi], y[lo:hi]], []) == hi - lo
        assert len(msgs) == want
        if want:
            seg = slice((want - 1) * N, want * N)
            ref = MC.mtm_csd(x[seg], y[seg], N, fs=float(Sf), fftshift=True)
            gate('block', 'vector %d' % (want - 1), (est.pxx, est.pyy, est.pxy, est.cxy), ref)
            assert msgs[-1][0] == 'coherence' and np.array_equal(np.asarray(msgs[-1][1]), est.cxy)
    assert est._plan.last_recipe().startswith('kernel=mtmcsd nfft=1024 ntapers=7 W=7 ')
    # the detector on the estimator's three rows against the detector's decision on the oracle's rows; thresholds in the
    # widest gaps of the oracle's pair sums, so that no rounding of a row can change a decision
    chans = [tune + f * Sf for f in (0.123, -0.31, 0.25, -0.4, 0.05, 0.33, -0.2, 0.45)]
    probe = ofdm_tools.coherence_detector(N, Sf, tune_freq=tune, subject_channels=chans)
    idx = probe.idx_subject_channels
    sums = [np.array([v[i - 1] + v[i] for i in idx]) for v in (ref[3], ref[0], ref[1])]

    def widest_gap(values):
        v = np.sort(values)
        i = int(np.argmax(np.diff(v) / v[1:]))
        assert (v[i + 1] - v[i]) / v[i + 1] > 1000 * RTOL
        return 0.5 * (v[i] + v[i + 1])
    thr, thr_mtm = widest_gap(sums[0]), widest_gap(np.maximum(sums[1], sums[2]))
    calls = []
    det = ofdm_tools.coherence_detector(N, Sf, threshold=thr, threshold_mtm=thr_mtm, tune_freq=tune, subject_channels=chans,
                                        valve_callback=calls.append)
    det.work([est.cxy.reshape(1, N), est.pxx.reshape(1, N), est.pyy.reshape(1, N)], [])
    coh, outcome, valve = R.coherence_scanner(ref[3], ref[0], ref[1], idx, thr, thr_mtm)
    print('mtm csd block | thresholds %.3g / %.3g, outcome %s' % (thr, thr_mtm, outcome))
    assert det.get_subject_channels_outcome() == outcome and calls == valve and len(set(outcome)) == 2
    assert np.allclose(det.subject_channels_coherence, coh, atol=2 * RTOL)


def test_the_welch_method_is_todays_estimator_bit_for_bit(ctx, hip):
    import ofdm_tools
    from ofdm_tools import windows
    N, Sf, block_len = 1024, 2000000, 4 * 1024
    x, y = _pair(block_len, 32 + N)
    plan = ctx.welch_plan(N, window=windows.get_window('hann', N), fs=float(Sf), fftshift=True)
    want = plan.csd(x, y)
    for kw in ({}, {'method': 'welch'}, {'method': 'welch', 'NW': 2.0, 'K': 3}):
        est = ofdm_tools.coherence_estimator(N, Sf, block_len=block_len, ctx=ctx, **kw)
        assert est.work([x, y], []) == block_len
        assert est._plan.last_recipe() == plan.last_recipe()
        for a, b in zip((est.pxx, est.pyy, est.pxy, est.cxy), want):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert ofdm_tools.coherence_estimator(N, Sf, ctx=ctx).block_len == 16 * N
    plan.close()
