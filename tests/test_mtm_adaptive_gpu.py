"""GPU tests of Thomson's adaptive-weight multitaper PSD (oth_mtm_set_ratios, oth_mtm_adaptive / _dev, csrc/mtmadapt.hip)
against the float64 oracle by the definition (tests/mtm_adaptive_oracle.py).  Parity is asked in the conditioned form of the
oracle module, with S = psd / scale and Pbar the mean of the eigenspectra over segments, tapers and bins:
    |S - S_ref|   <= 1e-4 S_ref + G_S sqrt(S_ref Pbar)
    |nu - nu_ref| <= G_NU nu_ref (1 + sqrt(Pbar / S_ref))          in every bin, none excluded,
G_S = 6.7e-6 and G_NU = 1.51e-6 being 3 x what a float32 emulation on the CPU reads on this file's parity inputs
(tests/test_mtm_adaptive_cpu.py::test_float32_emulation_sets_the_gpu_gate).  Measured on an MI355X, worst case of this file as a
share of the bounds: S 0.16 and nu 0.31 over the parity cases (4096 points, 1000-sample segments, K 5, 4 iterations), S 0.38
(130 streams x 2 segments of 16384 points) and nu 0.21 (520 x 2 of 4096) where a workgroup walks several segments; with unit
ratios the row is exec_dev's to 1.6e-7 and dof is 2 K exactly."""
import numpy as np
import pytest

import median_oracle as M
import mtm_adaptive_oracle as AO
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import SCALINGS
from test_mtm_adaptive_cpu import leakage_db, test_every_mtm_adaptive_kernel_build_has_no_scratch  # noqa: F401 - collected here too

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
FS = 2.5


def plan_scale(scaling, nfft):
    return {'density': 1.0 / FS, 'raw': 1.0, 'over_n2': 1.0 / float(nfft) ** 2}[scaling]


def check_rows(psd, dof, ref, scale, fftshift=False, trim=0, db=False, what=''):
    """psd, dof: one stream's rows; ref: the oracle's dict.  Asserts the two bounds of the file header and -> (worst S share
    of its bound, worst nu share of its bound)."""
    psd, dof = np.asarray(psd, np.float64), np.asarray(dof, np.float64)
    assert np.all(np.isfinite(psd)) and np.all(np.isfinite(dof))
    if db:
        psd = 10.0 ** (psd / 10.0)
    Sr, nr = M.shift_trim_db(ref['Sm'], fftshift, trim), M.shift_trim_db(ref['dof'], fftshift, trim)
    assert psd.shape == Sr.shape == dof.shape
    Pbar = ref['Pbar']
    e_s = np.abs(psd / scale - Sr) / (AO.REL_S * Sr + AO.G_S * np.sqrt(Sr * Pbar))
    e_nu = np.abs(dof - nr) / (AO.G_NU * nr * (1.0 + np.sqrt(Pbar / Sr)))
    worst = (float(e_s.max()), float(e_nu.max()))
    if what:
        print('adaptive parity %s: S %.3f of its bound, nu %.3f of its bound (nu %.2f ... %.2f)' % ((what,) + worst + (nr.min(), nr.max())))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (what, worst)
    return worst


def run_dev(ctx, plan, x, nsamples, nstreams, iters=4, want_dof=True):
    """adaptive_dev on nstreams captures back to back -> (psd, dof) as [nstreams][out_len], and a sentinel row check"""
    m, sentinel = plan.out_len, np.float32(-7.0)
    d = ctx.alloc(x.nbytes)
    out = ctx.alloc(4 * 2 * (nstreams + 1) * m)
    try:
        ctx.h2d(d, x)
        ctx.h2d(out, np.full(2 * (nstreams + 1) * m, sentinel, np.float32))
        rows = 4 * (nstreams + 1) * m
        assert plan.adaptive_dev(d, nsamples, nstreams, nsamples, out, out + rows if want_dof else None, iters=iters) == plan.last_nseg
        got = ctx.d2h(out, (2, nstreams + 1, m), np.float32)
    finally:
        ctx.free(d)
        ctx.free(out)
    assert np.all(got[:, nstreams] == sentinel)      # nothing behind the rows
    if not want_dof:
        assert np.all(got[1] == sentinel)
    return got[0, :nstreams], got[1, :nstreams]


# ---- 1. parity ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', AO.PARITY_CASES + AO.EXTRA_CASES, ids=lambda c: '-'.join(str(v) for v in c[:6]))
def test_parity_with_the_float64_oracle(ctx, hip, case):
    nfft, nperseg, ov, nseg, nw, K, scaling, fftshift, trim, offset = case
    x, noverlap = AO.parity_capture(case)
    db = nfft == 512 and K == 4      # the dB output of the psd row on one case
    plan = ctx.mtm_plan(nfft, nperseg=nperseg, noverlap=noverlap, nw=nw, ntapers=K, scaling=SCALINGS[scaling], fs=FS,
                        fftshift=fftshift, trim_bins=trim, db=db, weights='eigen')      # (the weights take no part)
    for iters in AO.PARITY_ITERS:
        psd, dof = plan.adaptive(x, iters=iters, return_dof=True)
        assert plan.last_nseg == nseg and psd.shape == dof.shape == (nfft - 2 * trim,)
        assert plan.last_recipe().startswith('kernel=mtmadapt nfft=%d ntapers=%d iters=%d W=%d nseg=%d nstreams=1 '
                                             % (nfft, K, iters, nseg, nseg))
        ref = AO.adaptive(x, nfft, nperseg, noverlap, nw, K, iters)
        check_rows(psd, dof, ref, plan_scale(scaling, nfft), fftshift, trim, db, what=str(case[:6] + (iters,)))
        assert np.all(dof >= 2.0 * (1.0 - 1e-5)) and np.all(dof <= 2.0 * K * (1.0 + 1e-5))
        # dof_out NULL, and the other entry point: the same bits
        assert plan.adaptive(x, iters=iters).tobytes() == psd.tobytes()
        p2, d2 = run_dev(ctx, plan, x, len(x), 1, iters)
        assert p2[0].tobytes() == psd.tobytes() and d2[0].tobytes() == dof.tobytes()
    p3, _ = run_dev(ctx, plan, x, len(x), 1, AO.PARITY_ITERS[-1], want_dof=False)
    assert p3[0].tobytes() == psd.tobytes()
    plan.close()


# ---- 2. several segments per workgroup ---------------------------------------------------------------------------------------

_shared = {}
BASE = 1 << 18


def tiled_capture(total):
    """the band capture (D = 40, the tones of the 4096-point grid) of 2^18 samples, repeated: streams whose length divides
    2^18 repeat with it, so the oracle runs once per distinct stream"""
    if 'x' not in _shared:
        _shared['x'] = AO.band_capture(BASE, 4242, 40.0, 4096)
        _shared['x'].setflags(write=False)
    return np.tile(_shared['x'], -(-total // BASE))[:total]


@pytest.mark.parametrize('nfft,nseg,nstreams,nw,K', [(64, 8, 1200, 2, 3), (512, 4, 1000, 2, 3), (2048, 4, 690, 2, 3),
                                                     (4096, 2, 520, 2, 3), (16384, 2, 130, 2, 3)])
def test_a_workgroup_walks_several_segments(ctx, hip, nfft, nseg, nstreams, nw, K):
    """More streams than the device holds workgroups for, so that W < nseg and the two running sums carry from one segment
    of a run to the next through the workgroup's partial rows - one launch per form of the kernel: the eigenspectra in LDS
    (64 threads, one and eight bins a thread), in the workspace with the samples in registers (2048), read again per taper
    (4096), and the 1024-thread build.  W = max(1, resident / nstreams) with at most 32 / 15 / 5 / 4 / 1 resident workgroups
    on each of 256 CUs at these sizes."""
    n = nfft * nseg
    assert BASE % n == 0
    x = tiled_capture(n * nstreams)
    plan = ctx.mtm_plan(nfft, nw=nw, ntapers=K, scaling=hip.SCALE_RAW)
    psd, dof = run_dev(ctx, plan, x, n, nstreams)
    W = int(plan.last_recipe().split(' W=')[1].split()[0])
    assert plan.last_nseg == nseg and 1 <= W < nseg, plan.last_recipe()
    distinct = min(nstreams, BASE // n)
    refs = AO.adaptive_streams(x[:distinct * n], distinct, nfft=nfft, nw=nw, K=K, scaling='raw')
    worst = np.max([check_rows(psd[s], dof[s], refs[s % distinct], 1.0) for s in range(nstreams)], axis=0)
    print('adaptive %d x %d segments of %d (%s): S %.3f, nu %.3f of their bounds' % (nstreams, nseg, nfft, plan.last_recipe(),
                                                                                   worst[0], worst[1]))
    plan.close()


# ---- 3. ties to the rest of the library -------------------------------------------------------------------------------------

def test_unit_ratios_give_the_psd_of_the_same_plan(ctx, hip):
    """lambda_k = 1: b_k = 1 and every weight is 1, so S is the mean of the eigenspectra - exec_dev of the same unity-weight
    plan - and nu = 2 K.  Measured on an MI355X: 1.2e-7 ... 1.6e-7 of the row, dof exactly 2 K."""
    for nfft, ov, nseg, nw, K in ((256, 0, 5, 2.5, 4), (1024, 50, 4, 4, 7), (16384, 0, 2, 2.5, 4)):
        x, noverlap = AO.parity_capture((nfft, nfft, ov, nseg, nw, K, 'density', False, 0, 0.0), seed=300 + nfft)
        plan = ctx.mtm_plan(nfft, noverlap=noverlap, nw=nw, ntapers=K, fs=FS)
        before = plan.exec(x)
        plan.set_ratios(np.ones(K))
        d = ctx.alloc(x.nbytes)
        out = ctx.alloc(4 * 3 * nfft)
        try:
            ctx.h2d(d, x)
            for iters in (1, 4):
                plan.adaptive_dev(d, len(x), 1, len(x), out, out + 4 * nfft, iters=iters)
                plan.exec_dev(d, len(x), out + 8 * nfft)
                psd, dof, fixed = (r.astype(np.float64) for r in ctx.d2h(out, (3, nfft), np.float32))
                err, derr = float(np.max(np.abs(psd - fixed) / fixed)), float(np.max(np.abs(dof - 2.0 * K)) / (2.0 * K))
                print('adaptive with unit ratios against exec_dev at %d, %d iterations: %.2e, dof %.2e' % (nfft, iters, err, derr))
                assert err < RTOL and derr <= 1e-5
        finally:
            ctx.free(d)
            ctx.free(out)
        assert plan.exec(x).tobytes() == before.tobytes()      # and exec is untouched by it
        plan.close()


def test_adaptive_weights_see_the_floor_next_to_a_band(ctx, hip):
    """The point of the feature, on the GPU: the case of the CPU file's test of the same name through MtmPlan.adaptive and
    exec - the floor to 1.5 dB against at least 4 dB over it."""
    n, nw, K, D = 1024, 4.0, 7, 40.0
    x = AO.band_capture(n, 1, D)
    plan = ctx.mtm_plan(n, nw=nw, ntapers=K)
    a = leakage_db(plan.adaptive(x, iters=4).astype(np.float64), n, nw, D)
    u = leakage_db(plan.exec(x).astype(np.float64), n, nw, D)
    print('floor at -40 dB on the GPU: adaptive %+.2f dB, unity %+.2f dB' % (a, u))
    assert abs(a) <= 1.5 and u >= 4.0
    plan.close()


def test_helpers(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    n = 1024
    x = AO.band_capture(n, 1, 40.0)
    psd, dof = T.mtm_adaptive_estimate(x, n, FS, ctx=ctx)
    ref = AO.adaptive(x, n, nw=4.0, K=7, iters=4)
    check_rows(psd, dof, ref, 1.0 / FS, fftshift=True, what='mtm_adaptive_estimate')
    lo, hi = T.mtm_adaptive_interval(psd, dof, 1)
    assert np.all(lo < psd) and np.all(psd < hi)


def test_custom_tapers_and_a_two_channel_plan(ctx, hip):
    """sine tapers (Riedel and Sidorenko) with ratios of the caller's; and the call on an MtmCsdPlan"""
    nfft, nperseg, K = 1024, 900, 5
    i = np.arange(nperseg)
    tapers = np.array([np.sqrt(2.0 / (nperseg + 1)) * np.sin(np.pi * (k + 1) * (i + 1) / (nperseg + 1)) for k in range(K)])
    ratios = np.array([0.999, 0.99, 0.97, 0.9, 0.8])
    x, _ = AO.parity_capture((nfft, nperseg, 0, 2, 0, K, 'density', False, 0, 0.0), seed=55)
    plan = ctx.mtm_plan(nfft, nperseg=nperseg, tapers=tapers, weights=[5, 4, 3, 2, 1])      # (the weights take no part)
    with pytest.raises(hip.HipError) as ei:
        plan.adaptive(x)
    assert ei.value.code == UNSUPPORTED and 'oth_mtm_set_ratios' in str(ei.value)
    plan.set_ratios(ratios)
    psd, dof = plan.adaptive(x, return_dof=True)
    assert plan.last_nseg == 2
    check_rows(psd, dof, AO.adaptive(x, nfft, nperseg, 0, iters=4, tapers=tapers.astype(np.float32), ratios=ratios), 1.0, what='sine tapers')
    plan.close()
    nfft, K = 2048, 4
    x, _ = AO.parity_capture((nfft, nfft, 0, 3, 2.5, K, 'density', False, 0, 0.0), seed=66)
    plan = ctx.mtm_csd_plan(nfft, nw=2.5, ntapers=K)
    psd, dof = plan.adaptive(x, return_dof=True)
    check_rows(psd, dof, AO.adaptive(x, nfft, nw=2.5, K=K, iters=4), 1.0, what='MtmCsdPlan')
    pxx, pyy, pxy, cxy = plan.csd(x, x)                                            # ... and the plan still does its own work
    assert np.array_equal(pxx, pyy) and np.all(cxy == 1.0)
    plan.close()


# ---- 4. degenerate input, determinism, refusals -------------------------------------------------------------------------------

def test_degenerate_input(ctx, hip):
    for nfft in (256, 4096, 16384):
        plan = ctx.mtm_plan(nfft, nw=4.0, fftshift=True)
        raw = ctx.mtm_plan(nfft, nw=4.0, detrend=hip.DETREND_NONE)
        for p, x in ((plan, np.zeros(2 * nfft, np.complex64)), (raw, np.zeros(2 * nfft, np.complex64)),
                     (plan, np.full(2 * nfft, 3.0 - 2.0j, np.complex64))):
            for row in p.adaptive(x, return_dof=True):
                assert row.shape == (nfft,) and not row.any()
        # ... and a constant WITHOUT detrend is all in bin 0: finite everywhere
        psd, dof = raw.adaptive(np.full(nfft, 3.0 - 2.0j, np.complex64), return_dof=True)
        assert np.isfinite(psd).all() and np.isfinite(dof).all() and (psd >= 0).all() and (dof >= 0).all() and psd[0] > 0
        assert dof.max() <= 14.0 * (1.0 + 1e-5)
        plan.close()
        raw.close()


def test_two_calls_are_bit_identical_and_sources_agree(ctx, hip):
    for nfft, ov, nseg in ((512, 50, 5), (4096, 50, 5), (16384, 0, 2)):
        x, noverlap = AO.parity_capture((nfft, nfft, ov, nseg, 4.0, 7, 'density', False, 0, 0.0), seed=11 + nfft)
        plan = ctx.mtm_plan(nfft, noverlap=noverlap, nw=4.0)
        a = plan.adaptive(x, return_dof=True)
        b = plan.adaptive(x, return_dof=True)
        d = ctx.alloc(x.nbytes)
        try:
            ctx.h2d(d, x)
            c = plan.adaptive(d, return_dof=True, nsamples=len(x))
        finally:
            ctx.free(d)
        assert plan.last_nseg == nseg
        for i in range(2):
            assert a[i].tobytes() == b[i].tobytes() == c[i].tobytes()
        plan.close()


def test_refusals(ctx, hip):
    x, _ = AO.parity_capture((1024, 1024, 0, 2, 4.0, 7, 'density', False, 0, 0.0), seed=9)
    one = ctx.mtm_plan(1024, nw=4.0, ntapers=1)
    with pytest.raises(hip.HipError) as ei:
        one.adaptive(x)
    assert ei.value.code == UNSUPPORTED and 'two tapers' in str(ei.value)
    assert one.exec(x).shape == (1024,)
    one.close()
    welch = ctx.welch_plan(1024, noverlap=0)
    with pytest.raises(hip.HipError) as ei:
        hip.MtmPlan.adaptive(welch, x)
    assert ei.value.code == UNSUPPORTED and 'multitaper' in str(ei.value)
    with pytest.raises(hip.HipError) as ei:
        ctx.check(ctx.lib.oth_mtm_set_ratios(welch.h, np.ones(7).ctypes.data_as(hip.C.POINTER(hip.C.c_double))), 'oth_mtm_set_ratios')
    assert ei.value.code == UNSUPPORTED
    d = ctx.alloc(x.nbytes)
    try:
        with pytest.raises(hip.HipError) as ei:
            hip.MtmPlan.adaptive_dev(welch, d, len(x), 1, len(x), d)
        assert ei.value.code == UNSUPPORTED
        assert welch.exec(x).shape == (1024,)
        # no ratios set: user tapers
        bare = ctx.mtm_plan(1024, tapers=np.array([[1.0, -1.0] * 512, [1.0, 1.0, -1.0, -1.0] * 256]) / 32.0)
        with pytest.raises(hip.HipError) as ei:
            bare.adaptive_dev(d, 1024, 1, 1024, d)
        assert ei.value.code == UNSUPPORTED and 'ratios' in str(ei.value)
        for bad in ([0.5, 0.0], [0.5, 1.0 + 1e-12], [-0.1, 0.5], [float('nan'), 0.5]):      # outside (0, 1]
            with pytest.raises(hip.HipError) as ei:
                bare.set_ratios(bad)
            assert ei.value.code == INVALID
        with pytest.raises(ValueError):
            bare.set_ratios([0.5, 0.5, 0.5])
        with pytest.raises(hip.HipError) as ei:      # a refused set leaves the plan without ratios
            bare.adaptive(x)
        assert ei.value.code == UNSUPPORTED
        bare.set_ratios([1.0, 0.5])
        assert bare.adaptive(x).shape == (1024,) and bare.exec(x).shape == (1024,)
        bare.close()
        plan = ctx.mtm_plan(1024, nw=4.0)
        want = plan.exec(x)
        null = lambda: ctx.check(ctx.lib.oth_mtm_adaptive_dev(plan.h, None, 1024, 1, 1024, 4, hip.C.c_void_p(d), None, None), 'null')  # noqa: E731
        for call in (lambda: plan.adaptive(x[:1000]), lambda: plan.adaptive_dev(d, 1000, 1, 1000, d),
                     lambda: plan.adaptive_dev(d, 1024, 2, 1000, d), lambda: plan.adaptive_dev(d, 1024, 0, 1024, d),
                     lambda: plan.adaptive(x, iters=0), lambda: plan.adaptive(x, iters=65),
                     lambda: plan.adaptive_dev(d, 1024, 1, 1024, d, iters=0), lambda: plan.adaptive_dev(d, 1024, 1, 1024, d, iters=65),
                     lambda: plan.adaptive_dev(d, 1024, 1, 1024, None), null):
            with pytest.raises(hip.HipError) as ei:
                call()
            assert ei.value.code == INVALID
        with pytest.raises(hip.HipError) as ei:
            plan.adaptive_dev(d, 1024, 65536, 1024, d)
        assert ei.value.code == UNSUPPORTED and '65535' in str(ei.value)
        assert plan.adaptive(x, iters=64).shape == (1024,) and plan.exec(x).tobytes() == want.tobytes()      # ... and the plan still works
        plan.close()
    finally:
        ctx.free(d)
    welch.close()


def test_live_resources_return_to_their_value(ctx, hip):
    x, _ = AO.parity_capture((16384, 16384, 0, 2, 4.0, 7, 'density', False, 0, 0.0), seed=5)

    def once():
        plan = ctx.mtm_plan(16384, nw=4.0)
        plan.adaptive(x, return_dof=True)
        plan.close()
    once()                                      # (the context keeps the twiddles of a length it has seen)
    before = hip.live_resources()
    once()
    assert hip.live_resources() == before
