"""GPU tests of Thomson's harmonic F-test (oth_mtm_ftest / _dev, csrc/mtmftest.hip) against the float64 oracle by the
definition (tests/mtm_ftest_oracle.py).  Parity is asked of quantities that stay well conditioned: with num' = line S and
den' = resid (K - 1) / scale (the per-segment means of the two sums the kernel forms),
    |num' - num / nseg|, |den' - den / nseg| <= RTOL (num + den) / nseg        in every bin, and
    |F - F_ref| / F_ref <= RTOL (1 / rho + 1 / (1 - rho)),  rho = num / (num + den)   in every bin, none excluded
- F is a ratio of the two, and a bin that is nearly all line (rho -> 1) or holds none (rho -> 0) divides by the small one.
A float32 emulation on the CPU (pocketfft on complex64, the subtracted form) read at most 4.8e-6 of num + den, a line 40 dB
over the noise and a 35-sigma offset included.  Measured on an MI355X, worst case of this file: 3.7e-5 of num + den (the
sums; a line of amplitude 100 on unit noise - 5.0e-6 over the parity cases) and 0.13 of the F bound."""
import numpy as np
import pytest

import median_oracle as M
import mtm_ftest_oracle as FO
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import SCALINGS, noise_tones

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
FS = 2.5


def on_off_tones(nfft):
    """one tone on a bin of the transform, one between bins"""
    return ((3.0, round(0.123 * nfft) / float(nfft)), (0.5, -0.31))


def tone_capture(nfft, nperseg, ov, nseg, seed, offset=0.0):
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    x = noise_tones(noverlap + nseg * step + step // 3, seed, on_off_tones(nfft))
    return (x + np.complex64(offset)).astype(np.complex64), noverlap


def check_rows(got, ref, scale, fftshift=False, trim=0, what=''):
    """got: (F, line, resid) of one stream; ref: the oracle's dict.  Asserts the three bounds of the file header and
    -> (worst sum error / (num + den), worst F error / its bound)."""
    F, line, resid = (np.asarray(g, np.float64) for g in got)
    nseg, K, S = ref['nseg'], ref['K'], ref['S']
    num, den, Fr = (M.shift_trim_db(ref[q], fftshift, trim) for q in ('num', 'den', 'F'))
    assert F.shape == num.shape and np.all(np.isfinite(F)) and np.all(np.isfinite(line)) and np.all(np.isfinite(resid))
    tot = (num + den) / nseg
    e_num = np.abs(line * S - num / nseg) / tot
    e_den = np.abs(resid * (K - 1) / scale - den / nseg) / tot
    rho = num / (num + den)
    e_f = np.abs(F - Fr) / Fr / (1.0 / rho + 1.0 / (1.0 - rho))
    worst = (float(max(e_num.max(), e_den.max())), float(e_f.max() / RTOL))
    if what:
        print('ftest parity %s: sums %.2e of num + den, F %.3f of its bound (F up to %.3g)' % ((what,) + worst + (Fr.max(),)))
    assert e_num.max() <= RTOL and e_den.max() <= RTOL and e_f.max() <= RTOL, (what, worst)
    return worst


def plan_scale(scaling, nfft):
    return {'density': 1.0 / FS, 'raw': 1.0, 'over_n2': 1.0 / float(nfft) ** 2}[scaling]


def run_dev(ctx, plan, x, nsamples, nstreams):
    """ftest_dev on nstreams captures back to back -> (F, line, resid) as [nstreams][out_len], and a sentinel row check"""
    m, sentinel = plan.out_len, np.float32(-7.0)
    d = ctx.alloc(x.nbytes)
    out = ctx.alloc(4 * 3 * (nstreams + 1) * m)
    try:
        ctx.h2d(d, x)
        ctx.h2d(out, np.full(3 * (nstreams + 1) * m, sentinel, np.float32))
        rows = 4 * (nstreams + 1) * m
        assert plan.ftest_dev(d, nsamples, nstreams, nsamples, out, out + rows, out + 2 * rows) == plan.last_nseg
        got = ctx.d2h(out, (3, nstreams + 1, m), np.float32)
    finally:
        ctx.free(d)
        ctx.free(out)
    assert np.all(got[:, nstreams] == sentinel)      # nothing behind the rows
    return got[0, :nstreams], got[1, :nstreams], got[2, :nstreams]


# ---- 1. parity ------------------------------------------------------------------------------------------------------

PARITY_CASES = [  # nfft, nperseg, overlap %, segments, NW, K, scaling, fftshift, trim, offset
    (64, 64, 0, 5, 2, 3, 'density', False, 0, 0.0),
    (512, 512, 50, 3, 2.5, 4, 'raw', True, 0, 0.0),
    (1024, 1024, 0, 1, 4, 7, 'density', False, 0, 0.0),
    (4096, 4096, 50, 9, 2.5, 4, 'over_n2', False, 0, 0.0),
    (4096, 1000, 0, 3, 3, 5, 'density', True, 100, 0.0),          # zero-padded
    (8192, 8192, 0, 1, 4, 7, 'density', False, 0, 0.0),
    (16384, 16384, 0, 1, 4, 7, 'raw', False, 0, 0.0),
    (16384, 16384, 50, 3, 8, 15, 'density', True, 0, 0.0),
    (256, 200, 0, 3, 2.5, 4, 'density', False, 0, 35.0),          # 35-sigma offset
]


@pytest.mark.parametrize('nfft,nperseg,ov,nseg,nw,K,scaling,fftshift,trim,offset', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, nperseg, ov, nseg, nw, K, scaling, fftshift, trim, offset):
    x, noverlap = tone_capture(nfft, nperseg, ov, nseg, 7 * nfft + ov + K, offset)
    plan = ctx.mtm_plan(nfft, nperseg=nperseg, noverlap=noverlap, nw=nw, ntapers=K, scaling=SCALINGS[scaling], fs=FS,
                        fftshift=fftshift, trim_bins=trim, db=True)      # (dB does not apply to these rows)
    got = plan.ftest(x, return_rows=True)
    assert plan.last_nseg == nseg and plan.dof == (2 * nseg, 2 * nseg * (K - 1)) and got[0].shape == (nfft - 2 * trim,)
    assert plan.last_recipe().startswith('kernel=mtmftest nfft=%d ntapers=%d W=%d nseg=%d nstreams=1 ' % (nfft, K, nseg, nseg))
    ref = FO.ftest(x, nfft, nperseg, noverlap, nw, K, True, scaling, FS)
    check_rows(got, ref, plan_scale(scaling, nfft), fftshift, trim, what=str((nfft, nperseg, ov, nseg, nw, K)))
    assert np.array_equal(plan.ftest(x).view(np.uint32), got[0].view(np.uint32))      # F alone: the other rows are optional
    plan.close()


def test_700_streams_of_256_points(ctx, hip):
    nfft, nseg, K, nstreams = 256, 5, 3, 700
    n = nfft * nseg
    x = np.concatenate([noise_tones(n, 1000 + s, on_off_tones(nfft)) for s in range(nstreams)])
    plan = ctx.mtm_plan(nfft, nw=2.0, ntapers=K, fs=FS)
    F, line, resid = run_dev(ctx, plan, x, n, nstreams)
    assert plan.last_nseg == nseg and 'nstreams=700 ' in plan.last_recipe()
    worst = np.max([check_rows((F[s], line[s], resid[s]), r, 1.0 / FS)
                    for s, r in enumerate(FO.ftest_streams(x, nstreams, nfft=nfft, nw=2.0, K=K, fs=FS))], axis=0)
    print('ftest 700 x 256 (%s): sums %.2e, F %.3f of its bound' % (plan.last_recipe(), worst[0], worst[1]))
    plan.close()


_shared = {}


def long_noise():
    """4 259 840 samples with the two tones, cut into the captures of the test below"""
    if 'x' not in _shared:
        _shared['x'] = noise_tones(130 * 32768, 4242, on_off_tones(4096))
        _shared['x'].setflags(write=False)
    return _shared['x']


@pytest.mark.parametrize('nfft,nseg,nstreams,nw,K', [(64, 9, 1200, 2, 3), (2048, 3, 690, 2, 3), (4096, 2, 520, 2, 3),
                                                     (8192, 2, 260, 2, 3), (16384, 2, 130, 2, 3)])
def test_a_workgroup_walks_several_segments(ctx, hip, nfft, nseg, nstreams, nw, K):
    """More streams than the device holds workgroups for, so that W < nseg: the running sums carry from one segment of a
    run to the next - in registers up to 2048 points, in the workgroup's own partial rows from 4096 on (and sy / p through
    the workspace at 16384).  W = max(1, resident / nstreams) with at most 32 / 8 / 4 / 2 / 1 resident workgroups on each
    of 256 CUs at these sizes (eight waves per SIMD; 160 KiB of LDS from 4096 points on)."""
    n = nfft * nseg
    x = long_noise()[:n * nstreams]
    plan = ctx.mtm_plan(nfft, nw=nw, ntapers=K, scaling=hip.SCALE_RAW)
    F, line, resid = run_dev(ctx, plan, x, n, nstreams)
    W = int(plan.last_recipe().split(' W=')[1].split()[0])
    assert plan.last_nseg == nseg and 1 <= W < nseg, plan.last_recipe()
    refs = FO.ftest_streams(x, nstreams, nfft=nfft, nw=nw, K=K, scaling='raw')
    worst = np.max([check_rows((F[s], line[s], resid[s]), r, 1.0) for s, r in enumerate(refs)], axis=0)
    print('ftest %d x %d segments of %d (%s): sums %.2e, F %.3f of its bound' % (nstreams, nseg, nfft, plan.last_recipe(),
                                                                               worst[0], worst[1]))
    plan.close()


def test_a_line_40_db_over_the_noise(ctx, hip):
    """amplitude 100 on unit-variance noise: the float32 rounding of the line's own transform is what the other bins see"""
    nfft, K = 1024, 7
    x = noise_tones(nfft, 77, ((100.0, 128.0 / nfft), (0.5, -0.31)))
    plan = ctx.mtm_plan(nfft, nw=4.0, ntapers=K)
    got = plan.ftest(x, return_rows=True)
    ref = FO.ftest(x, nfft, nw=4.0, K=K)
    assert ref['F'][128] > 1e4 and abs(float(got[1][128]) - 1e4) < 0.05e4      # the line's power: amplitude 100 squared
    check_rows(got, ref, 1.0, what='a line of amplitude 100 on unit noise')
    plan.close()


# ---- 2. ties to the rest of the library -------------------------------------------------------------------------------------

def test_sums_add_up_to_the_psd_of_the_same_plan(ctx, hip):
    """unity weights, OTH_SCALE_RAW: exec is the mean over segments of sum_k |y_k|^2 / K = (num + den) / (K nseg)"""
    for nfft, ov, nseg, nw, K in ((1024, 50, 4, 4, 7), (16384, 0, 2, 2.5, 4)):
        x, noverlap = tone_capture(nfft, nfft, ov, nseg, 300 + nfft)
        plan = ctx.mtm_plan(nfft, noverlap=noverlap, nw=nw, ntapers=K, scaling=hip.SCALE_RAW)
        psd = plan.exec(x).astype(np.float64)
        F, line, resid = (r.astype(np.float64) for r in plan.ftest(x, return_rows=True))
        S = float(np.sum(plan.tapers.astype(np.float64).sum(axis=1) ** 2))
        err = float(np.max(np.abs((line * S + resid * (K - 1)) / K - psd) / psd))
        print('ftest sums against exec at %d: %.2e' % (nfft, err))
        assert err < RTOL and plan.exec(x).tobytes() == psd.astype(np.float32).tobytes()      # and exec is untouched by it
        plan.close()


def test_two_calls_are_bit_identical_and_sources_agree(ctx, hip):
    for nfft, ov, nseg in ((4096, 50, 5), (16384, 0, 2)):
        x, noverlap = tone_capture(nfft, nfft, ov, nseg, 11 + nfft)
        plan = ctx.mtm_plan(nfft, noverlap=noverlap, nw=4.0)
        a = plan.ftest(x, return_rows=True)
        b = plan.ftest(x, return_rows=True)
        d = ctx.alloc(x.nbytes)
        try:
            ctx.h2d(d, x)
            c = plan.ftest(d, return_rows=True, nsamples=len(x))
        finally:
            ctx.free(d)
        assert plan.last_nseg == nseg
        for i in range(3):
            assert a[i].tobytes() == b[i].tobytes() == c[i].tobytes()
        plan.close()


def test_degenerate_input_gives_three_zero_rows(ctx, hip):
    for nfft in (256, 4096, 16384):
        plan = ctx.mtm_plan(nfft, nw=4.0, fftshift=True)
        raw = ctx.mtm_plan(nfft, nw=4.0, detrend=hip.DETREND_NONE)
        for p, x in ((plan, np.zeros(2 * nfft, np.complex64)), (raw, np.zeros(2 * nfft, np.complex64)),
                     (plan, np.full(2 * nfft, 3.0 - 2.0j, np.complex64))):
            for row in p.ftest(x, return_rows=True):
                assert row.shape == (nfft,) and not row.any()
        # ... and a constant WITHOUT detrend is a line at bin 0: finite everywhere, nothing but line there
        F, line, resid = raw.ftest(np.full(nfft, 3.0 - 2.0j, np.complex64), return_rows=True)
        assert not np.isnan(F).any() and np.isfinite(line).all() and np.isfinite(resid).all() and (resid >= 0).all()
        assert F[0] > 1e4 and abs(float(line[0]) - 13.0) < 13.0 * RTOL
        plan.close()
        raw.close()


def test_custom_tapers(ctx, hip):
    """sine tapers (Riedel and Sidorenko): sqrt(2 / (n + 1)) sin(pi (k + 1) (i + 1) / (n + 1)) - not Slepian's"""
    nfft, nperseg, K = 1024, 900, 5
    i = np.arange(nperseg)
    tapers = np.array([np.sqrt(2.0 / (nperseg + 1)) * np.sin(np.pi * (k + 1) * (i + 1) / (nperseg + 1)) for k in range(K)])
    x, _ = tone_capture(nfft, nperseg, 0, 2, 55)
    plan = ctx.mtm_plan(nfft, nperseg=nperseg, tapers=tapers, weights=[5, 4, 3, 2, 1])      # (the weights take no part)
    got = plan.ftest(x, return_rows=True)
    assert plan.last_nseg == 2
    check_rows(got, FO.ftest(x, nfft, nperseg, 0, tapers=tapers.astype(np.float32)), 1.0, what='sine tapers')
    plan.close()


def test_on_a_two_channel_plan(ctx, hip):
    nfft, K = 2048, 4
    x, _ = tone_capture(nfft, nfft, 0, 3, 66)
    plan = ctx.mtm_csd_plan(nfft, nw=2.5, ntapers=K)
    got = plan.ftest(x, return_rows=True)
    check_rows(got, FO.ftest(x, nfft, nw=2.5, K=K), 1.0, what='MtmCsdPlan')
    pxx, pyy, pxy, cxy = plan.csd(x, x)                                            # ... and the plan still does its own work
    assert np.array_equal(pxx, pyy) and np.all(cxy == 1.0)
    plan.close()


def test_refusals(ctx, hip):
    x, _ = tone_capture(1024, 1024, 0, 2, 9)
    one = ctx.mtm_plan(1024, nw=4.0, ntapers=1)
    with pytest.raises(hip.HipError) as ei:
        one.ftest(x)
    assert ei.value.code == UNSUPPORTED and 'two tapers' in str(ei.value)
    assert one.exec(x).shape == (1024,)
    one.close()
    odd = ctx.mtm_plan(1024, tapers=np.array([[1.0, -1.0] * 512, [1.0, 1.0, -1.0, -1.0] * 256]))      # every U_k is zero
    with pytest.raises(hip.HipError) as ei:
        odd.ftest(x)
    assert ei.value.code == UNSUPPORTED and 'non-zero sum' in str(ei.value)
    odd.close()
    welch = ctx.welch_plan(1024, noverlap=0)
    with pytest.raises(hip.HipError) as ei:
        hip.MtmPlan.ftest(welch, x)
    assert ei.value.code == UNSUPPORTED and 'multitaper' in str(ei.value)
    d = ctx.alloc(x.nbytes)
    try:
        with pytest.raises(hip.HipError) as ei:
            hip.MtmPlan.ftest_dev(welch, d, len(x), 1, len(x), d)
        assert ei.value.code == UNSUPPORTED
        plan = ctx.mtm_plan(1024, nw=4.0)
        for call in (lambda: plan.ftest(x[:1000]), lambda: plan.ftest_dev(d, 1000, 1, 1000, d),
                     lambda: plan.ftest_dev(d, 1024, 2, 1000, d), lambda: plan.ftest_dev(d, 1024, 0, 1024, d)):
            with pytest.raises(hip.HipError) as ei:
                call()
            assert ei.value.code == -1
        with pytest.raises(hip.HipError) as ei:
            plan.ftest_dev(d, 1024, 65536, 1024, d)
        assert ei.value.code == UNSUPPORTED and '65535' in str(ei.value)
        assert plan.ftest(x).shape == (1024,)                                      # ... and the plan still works
        plan.close()
    finally:
        ctx.free(d)
    welch.close()


# ---- 3. the helper: what the feature exists for ------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 3])
def test_line_scan_finds_the_line_on_the_hump(ctx, hip, seed):
    from ofdm_tools import ofdm_cr_tools as T
    n = 1024
    x = FO.hump_capture(seed, n)
    F, axis, lines = T.mtm_line_scan(x, n, float(n), ctx=ctx)                      # fs = n: the axis reads in bins
    assert F.shape == (n,) and np.array_equal(axis, np.arange(-n // 2, n // 2))
    assert sorted(lines) == [-300.0, 200.0], lines
    thr = T.ftest_threshold(1e-3 / n, 1, 7)
    far = (np.abs(axis - 200) > 4) & (np.abs(axis + 300) > 4)
    assert F[axis == 200][0] > thr and F[axis == -300][0] > thr and np.all(F[far] < thr)
    # the PSD of the same capture: its maximum is the hump (with the strong line's lobe on top), and at the weak line the
    # PSD does not stand out of its surroundings at all
    ax, db = T.mtm_plot_dB(x, float(n), 0.0, n, ctx=ctx)
    db = np.asarray(db)
    assert abs(ax[int(np.argmax(db))] - 200) <= 60
    assert T.mtm_line_scan(x, n, float(n), fc=1000.0, ctx=ctx)[2] == [f + 1000.0 for f in lines]
    assert T.mtm_line_scan(x, n, float(n), p_false=1e-30, ctx=ctx)[2] == []


def test_live_resources_return_to_their_value(ctx, hip):
    x, _ = tone_capture(16384, 16384, 0, 2, 5)

    def once():
        plan = ctx.mtm_plan(16384, nw=4.0)
        plan.ftest(x, return_rows=True)
        plan.close()
    once()                                      # (the context keeps the twiddles of a length it has seen)
    before = hip.live_resources()
    once()
    assert hip.live_resources() == before
