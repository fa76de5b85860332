"""GPU tests of the multitaper jackknife (oth_mtm_jackknife / _dev, oth_mtm_csd_jackknife / _dev, csrc/mtmjack.hip) against
the float64 oracle by the definitions (tests/mtm_jackknife_oracle.py).  Parity is asked of every bin, none excluded:
    |lnsd - ref| <= RTOL ref / (1 - tmax),   tmax = max_i t_i        (each channel of a pair alike)
    |zsd  - ref| <= RTOL ref / (1 - cmax),   cmax = max(C, max_i C_i)
- both statistics divide by what is left after a deletion, and the factor is their condition number (as the F-test's file
does for rho).  So that the conditioning cannot hide a failure, every parity case also asserts that at most 15 % of its bins
have cmax > 0.99 and at most 6 % tmax > 0.9.  A float32 emulation on the CPU (pocketfft on complex64) read at most 3.4e-6
and 2.2e-6 of those bounds without RTOL on shapes 64 ... 4096.  Measured on an MI355X, worst case of this file as a share
of the bound (RTOL included): lnsd 0.064 over the parity cases and 0.30 where a workgroup walks several items (130 streams x 2
segments of 16384 points); zsd 0.090 over the parity cases and 0.72 at 64 points x 3000 segments x K 3, where d_i, of the
size of 1 / M, is the difference of two float32 atanh of the size of 1."""
import numpy as np
import pytest

import mtm_jackknife_oracle as JO
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import SCALINGS, noise_tones
from test_mtm_ftest_gpu import long_noise, on_off_tones

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
FS = 2.5
CMAX_CAP, TMAX_CAP = 0.15, 0.06      # shares of bins with cmax > 0.99, tmax > 0.9


def captures(nfft, nperseg, ov, nseg, seed, offset=0.0):
    """x: noise and the two tones (+ offset); y = 0.7 x delayed by five samples + independent unit noise (+ offset)"""
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    n = noverlap + nseg * step + step // 3
    x0 = noise_tones(n, seed, on_off_tones(nfft)).astype(np.complex128)
    rng = np.random.default_rng(seed + 100000)
    w = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    y = 0.7 * np.roll(x0, 5) + w + offset
    return (x0 + offset).astype(np.complex64), y.astype(np.complex64), noverlap


def check_lnsd(got, ref_lnsd, tmax, fftshift=False, trim=0, what='', caps=True):
    """-> worst |lnsd - ref| as a share of RTOL ref / (1 - tmax)"""
    got = np.asarray(got, np.float64)
    ref, tm = JO.shift_trim(ref_lnsd, fftshift, trim), JO.shift_trim(tmax, fftshift, trim)
    assert got.shape == ref.shape and np.all(np.isfinite(got)) and np.all(got >= 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        bound = RTOL * ref / (1.0 - tm)
        share = np.where(np.abs(got - ref) > 0.0, np.abs(got - ref) / bound, 0.0)
    worst = float(share.max())
    ill = float(np.mean(tm > 0.9))
    if what:
        print('jackknife parity %s: lnsd %.4f of its bound, tmax > 0.9 in %.1f %% of the bins' % (what, worst, 100 * ill))
    assert worst <= 1.0, (what, worst)
    if caps:
        assert ill <= TMAX_CAP, (what, ill)
    return worst


def check_zsd(got, ref, fftshift=False, trim=0, what='', caps=True):
    """got: zsd; ref: the oracle's dict -> worst |zsd - ref| as a share of RTOL ref / (1 - cmax)"""
    got = np.asarray(got, np.float64)
    zr, cm = JO.shift_trim(ref['zsd'], fftshift, trim), JO.shift_trim(ref['cmax'], fftshift, trim)
    assert got.shape == zr.shape and np.all(np.isfinite(got)) and np.all(got >= 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        bound = RTOL * zr / (1.0 - cm)
        share = np.where(np.abs(got - zr) > 0.0, np.abs(got - zr) / bound, 0.0)
    worst = float(share.max())
    ill = float(np.mean(cm > 0.99))
    if what:
        print('jackknife parity %s: zsd %.4f of its bound, cmax > 0.99 in %.1f %% of the bins' % (what, worst, 100 * ill))
    assert worst <= 1.0, (what, worst)
    if caps:
        assert ill <= CMAX_CAP, (what, ill)
    return worst


def recipe_w(plan):
    return int(plan.last_recipe().split(' W=')[1].split()[0])


# ---- 1. parity ------------------------------------------------------------------------------------------------------

PARITY_CASES = [  # nfft, nperseg, overlap %, segments, NW, K, scaling, fftshift, trim, offset
    (64, 64, 0, 1, 2, 3, 'density', False, 0, 0.0),
    (64, 64, 0, 5, 2, 3, 'density', False, 0, 0.0),
    (256, 200, 0, 3, 2.5, 4, 'density', False, 0, 35.0),          # 35-sigma offset, zero-padded
    (1024, 1024, 0, 1, 4, 7, 'density', False, 0, 0.0),
    (4096, 4096, 50, 9, 2.5, 4, 'over_n2', False, 0, 0.0),
    (4096, 1000, 0, 3, 3, 5, 'density', True, 100, 0.0),          # zero-padded, fftshift, trim
    (8192, 8192, 0, 1, 4, 7, 'density', False, 0, 0.0),
    (16384, 16384, 0, 1, 4, 7, 'raw', False, 0, 0.0),
    (16384, 16384, 50, 3, 8, 15, 'density', False, 0, 0.0),
]


@pytest.mark.parametrize('nfft,nperseg,ov,nseg,nw,K,scaling,fftshift,trim,offset', PARITY_CASES)
def test_parity_one_channel(ctx, hip, nfft, nperseg, ov, nseg, nw, K, scaling, fftshift, trim, offset):
    x, _, noverlap = captures(nfft, nperseg, ov, nseg, 7 * nfft + ov + K, offset)
    plan = ctx.mtm_plan(nfft, nperseg=nperseg, noverlap=noverlap, nw=nw, ntapers=K, scaling=SCALINGS[scaling], fs=FS,
                        fftshift=fftshift, trim_bins=trim, db=True)      # (dB applies to the PSD row alone)
    lnsd, psd = plan.jackknife(x, return_psd=True)
    assert plan.last_nseg == nseg and lnsd.shape == (nfft - 2 * trim,)
    assert plan.last_recipe().startswith('kernel=mtmjack nfft=%d ntapers=%d W=%d nseg=%d nstreams=1 bpc=' % (nfft, K, K * nseg, nseg))
    ref = JO.jackknife(x, nfft, nperseg=nperseg, noverlap=noverlap, nw=nw, K=K, scaling=scaling)
    check_lnsd(lnsd, ref['lnsd'], ref['tmax'], fftshift, trim, what=str((nfft, nperseg, ov, nseg, nw, K)))
    assert psd.tobytes() == plan.exec(x).tobytes()                           # the row exec gives, dB included
    assert plan.jackknife(x).tobytes() == lnsd.tobytes()                     # the PSD row is optional
    plan.close()


@pytest.mark.parametrize('nfft,nperseg,ov,nseg,nw,K,scaling,fftshift,trim,offset', PARITY_CASES)
def test_parity_two_channels(ctx, hip, nfft, nperseg, ov, nseg, nw, K, scaling, fftshift, trim, offset):
    x, y, noverlap = captures(nfft, nperseg, ov, nseg, 7 * nfft + ov + K, offset)
    plan = ctx.mtm_csd_plan(nfft, nperseg=nperseg, noverlap=noverlap, nw=nw, ntapers=K, scaling=SCALINGS[scaling], fs=FS,
                            fftshift=fftshift, trim_bins=trim)
    cxy, zsd, lx, ly = plan.csd_jackknife(x, y)
    assert plan.last_nseg == nseg and zsd.shape == (nfft - 2 * trim,)
    assert plan.last_recipe().startswith('kernel=mtmcsdjack nfft=%d ntapers=%d W=%d nseg=%d nstreams=1 bpc=' % (nfft, K, K * nseg, nseg))
    ref = JO.csd_jackknife(x, y, nfft, nperseg=nperseg, noverlap=noverlap, nw=nw, K=K, scaling=scaling)
    what = str((nfft, nperseg, ov, nseg, nw, K))
    check_zsd(zsd, ref, fftshift, trim, what=what)
    check_lnsd(lx, ref['lnsd_x'], ref['tmax_x'], fftshift, trim, what=what + ' x')
    check_lnsd(ly, ref['lnsd_y'], ref['tmax_y'], fftshift, trim, what=what + ' y')
    assert cxy.tobytes() == plan.csd(x, y)[3].tobytes()                      # the coherence the plan gives
    one = plan.jackknife(x).astype(np.float64)                               # the one-channel call on the same plan
    tm = JO.shift_trim(ref['tmax_x'], fftshift, trim)
    assert np.all(np.abs(one - lx) <= RTOL * one / (1.0 - tm))
    plan.close()


# ---- 2. a workgroup walks several items ---------------------------------------------------------------------------------------

def run_dev(ctx, plan, x, nsamples, nstreams):
    """jackknife_dev on nstreams captures back to back -> (lnsd, psd) as [nstreams][out_len], and a sentinel row check"""
    m, sentinel = plan.out_len, np.float32(-7.0)
    d = ctx.alloc(x.nbytes)
    out = ctx.alloc(4 * 2 * (nstreams + 1) * m)
    try:
        ctx.h2d(d, x)
        ctx.h2d(out, np.full(2 * (nstreams + 1) * m, sentinel, np.float32))
        rows = 4 * (nstreams + 1) * m
        assert plan.jackknife_dev(d, nsamples, nstreams, nsamples, out, out + rows) == plan.last_nseg
        recipe = plan.last_recipe()
        got = ctx.d2h(out, (2, nstreams + 1, m), np.float32)
        ctx.h2d(out, np.full(nstreams * m, sentinel, np.float32))
        plan.exec_dev(d, nsamples, out, nstreams)
        psd = ctx.d2h(out, (nstreams, m), np.float32)
    finally:
        ctx.free(d)
        ctx.free(out)
    assert np.all(got[:, nstreams] == sentinel)      # nothing behind the rows
    assert got[1, :nstreams].tobytes() == psd.tobytes()      # the rows exec_dev gives
    return got[0, :nstreams], recipe


@pytest.mark.parametrize('nfft,nseg,nstreams,nw,K', [(64, 9, 1200, 2, 3), (2048, 3, 690, 2, 3), (4096, 2, 520, 2, 3),
                                                     (8192, 2, 260, 2, 3), (16384, 2, 130, 2, 3)])
def test_a_workgroup_walks_several_items_one_channel(ctx, hip, nfft, nseg, nstreams, nw, K):
    """More streams than the device holds workgroups for, so that W < K nseg: the running sums carry from one item of a run
    to the next and across its segments - in registers up to 8192 points, in the workgroup's own partial rows at 16384."""
    n = nfft * nseg
    x = long_noise()[:n * nstreams]
    plan = ctx.mtm_plan(nfft, nw=nw, ntapers=K, scaling=hip.SCALE_RAW)
    lnsd, recipe = run_dev(ctx, plan, x, n, nstreams)
    W = int(recipe.split(' W=')[1].split()[0])
    assert recipe.startswith('kernel=mtmjack ') and plan.last_nseg == nseg and K <= W < K * nseg, recipe
    worst = 0.0
    for s in range(nstreams):
        ref = JO.jackknife(x[s * n:(s + 1) * n], nfft, nw=nw, K=K, scaling='raw')
        worst = max(worst, check_lnsd(lnsd[s], ref['lnsd'], ref['tmax'], caps=False))
    print('jackknife %d x %d segments of %d (%s): lnsd %.4f of its bound' % (nstreams, nseg, nfft, recipe, worst))
    plan.close()


@pytest.mark.parametrize('nfft,nseg,nw,K', [(64, 3000, 2, 3), (16384, 40, 4, 7)])
def test_a_workgroup_walks_several_items_two_channels(ctx, hip, nfft, nseg, nw, K):
    """More items than the device holds workgroups for: the six running sums carry in registers (64 points), in the partial
    rows with X's spectrum through the workspace (16384 points)."""
    x, y, _ = captures(nfft, nfft, 0, nseg, 4000 + nfft)
    plan = ctx.mtm_csd_plan(nfft, nw=nw, ntapers=K)
    cxy, zsd, lx, ly = plan.csd_jackknife(x, y)
    W = recipe_w(plan)
    assert plan.last_recipe().startswith('kernel=mtmcsdjack ') and plan.last_nseg == nseg and K <= W < K * nseg, plan.last_recipe()
    ref = JO.csd_jackknife(x, y, nfft, nw=nw, K=K)
    what = '%d x %d segments, K %d (%s)' % (nfft, nseg, K, plan.last_recipe())
    check_zsd(zsd, ref, what=what)
    check_lnsd(lx, ref['lnsd_x'], ref['tmax_x'], what=what + ' x')
    check_lnsd(ly, ref['lnsd_y'], ref['tmax_y'], what=what + ' y')
    assert cxy.tobytes() == plan.csd(x, y)[3].tobytes()
    plan.close()


# ---- 3. ties to the rest of the library -------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,nseg,K', [(256, 2, 3), (4096, 3, 4), (16384, 1, 7)])
def test_a_channel_against_itself(ctx, hip, nfft, nseg, K):
    x, _, _ = captures(nfft, nfft, 0, nseg, 21 + nfft)
    plan = ctx.mtm_csd_plan(nfft, nw=0.5 * (K + 1), ntapers=K)
    cxy, zsd, lx, ly = plan.csd_jackknife(x, x)
    assert np.all(cxy == 1.0) and not zsd.any() and lx.tobytes() == ly.tobytes() and lx.any()
    plan.close()


def test_two_calls_are_bit_identical_and_sources_agree(ctx, hip):
    for nfft, ov, nseg in ((4096, 50, 5), (16384, 0, 2)):
        x, y, noverlap = captures(nfft, nfft, ov, nseg, 11 + nfft)
        plan = ctx.mtm_csd_plan(nfft, noverlap=noverlap, nw=4.0)
        a, b = plan.csd_jackknife(x, y), plan.csd_jackknife(x, y)
        a1, b1 = plan.jackknife(x, return_psd=True), plan.jackknife(x, return_psd=True)
        d = ctx.alloc(2 * x.nbytes)
        try:
            ctx.h2d(d, np.concatenate((x, y)))
            c = plan.csd_jackknife(d, d + x.nbytes, nsamples=len(x))
            c1 = plan.jackknife(d, return_psd=True, nsamples=len(x))
        finally:
            ctx.free(d)
        assert plan.last_nseg == nseg
        for i in range(4):
            assert a[i].tobytes() == b[i].tobytes() == c[i].tobytes()
        for i in range(2):
            assert a1[i].tobytes() == b1[i].tobytes() == c1[i].tobytes()
        plan.close()


def test_device_form_two_channels_and_optional_rows(ctx, hip):
    nfft, nseg = 2048, 2
    x, y, _ = captures(nfft, nfft, 0, nseg, 99)
    plan = ctx.mtm_csd_plan(nfft, nw=3.0, fftshift=True, trim_bins=10)
    m, sentinel = plan.out_len, np.float32(-7.0)
    host = plan.csd_jackknife(x, y)
    d = ctx.alloc(2 * x.nbytes)
    out = ctx.alloc(4 * 5 * m)
    try:
        ctx.h2d(d, np.concatenate((x, y)))
        ctx.h2d(out, np.full(5 * m, sentinel, np.float32))
        assert plan.csd_jackknife_dev(d, d + x.nbytes, len(x), out + 4 * m, out, out + 8 * m, out + 12 * m) == nseg
        got = ctx.d2h(out, (5, m), np.float32)
        for i in range(4):
            assert got[i].tobytes() == host[i].tobytes()
        assert np.all(got[4] == sentinel)
        ctx.h2d(out, np.full(5 * m, sentinel, np.float32))
        plan.csd_jackknife_dev(d, d + x.nbytes, len(x), out + 4 * m)             # zsd alone
        got = ctx.d2h(out, (5, m), np.float32)
        assert got[1].tobytes() == host[1].tobytes() and np.all(got[[0, 2, 3, 4]] == sentinel)
    finally:
        ctx.free(d)
        ctx.free(out)
    plan.close()


def test_custom_tapers(ctx, hip):
    """sine tapers (Riedel and Sidorenko): sqrt(2 / (n + 1)) sin(pi (k + 1) (i + 1) / (n + 1)) - not Slepian's"""
    nfft, nperseg, K = 1024, 900, 5
    i = np.arange(nperseg)
    tapers = np.array([np.sqrt(2.0 / (nperseg + 1)) * np.sin(np.pi * (k + 1) * (i + 1) / (nperseg + 1)) for k in range(K)])
    x, y, _ = captures(nfft, nperseg, 0, 2, 55)
    plan = ctx.mtm_csd_plan(nfft, nperseg=nperseg, tapers=tapers)
    cxy, zsd, lx, ly = plan.csd_jackknife(x, y)
    assert plan.last_nseg == 2
    t32 = tapers.astype(np.float32)
    ref = JO.csd_jackknife(x, y, nfft, nperseg=nperseg, tapers=t32)
    check_zsd(zsd, ref, what='sine tapers')
    check_lnsd(lx, ref['lnsd_x'], ref['tmax_x'], what='sine tapers x')
    check_lnsd(plan.jackknife(y), ref['lnsd_y'], ref['tmax_y'], what='sine tapers y, one channel')
    plan.close()


# ---- 4. degenerate input, refusals ----------------------------------------------------------------------------------------

def test_degenerate_input(ctx, hip):
    for nfft in (256, 4096, 16384):
        plan = ctx.mtm_csd_plan(nfft, nw=4.0, fftshift=True)
        raw = ctx.mtm_csd_plan(nfft, nw=4.0, detrend=hip.DETREND_NONE)
        zeros, const = np.zeros(2 * nfft, np.complex64), np.full(2 * nfft, 3.0 - 2.0j, np.complex64)
        for p, x in ((plan, zeros), (raw, zeros), (plan, const)):
            cxy, zsd, lx, ly = p.csd_jackknife(x, x)
            for row in (zsd, lx, ly, p.jackknife(x)):
                assert row.shape == (nfft,) and not row.any()
            assert np.all(np.isfinite(p.jackknife(x, return_psd=True)[1]))
        # ... and a constant WITHOUT detrend, against noise: finite and non-negative everywhere
        x, y, _ = captures(nfft, nfft, 0, 2, 3)
        for a, b in ((const, const), (const, y[:2 * nfft]), (x[:2 * nfft], const)):
            cxy, zsd, lx, ly = raw.csd_jackknife(a, b)
            for row in (zsd, lx, ly, raw.jackknife(a)):
                assert np.all(np.isfinite(row)) and np.all(row >= 0.0)
        plan.close()
        raw.close()


def refused(hip, call, code, fragment):
    with pytest.raises(hip.HipError) as ei:
        call()
    assert ei.value.code == code and fragment in str(ei.value), (ei.value.code, str(ei.value))


def test_refusals(ctx, hip):
    x, y, _ = captures(1024, 1024, 0, 2, 9)
    d = ctx.alloc(2 * x.nbytes)
    try:
        welch = ctx.welch_plan(1024, noverlap=0)      # a plan without tapers
        refused(hip, lambda: hip.MtmPlan.jackknife(welch, x), UNSUPPORTED, 'no tapers')
        refused(hip, lambda: hip.MtmPlan.jackknife_dev(welch, d, len(x), 1, len(x), d), UNSUPPORTED, 'no tapers')
        refused(hip, lambda: hip.MtmCsdPlan.csd_jackknife(welch, x, y), UNSUPPORTED, 'no tapers')
        refused(hip, lambda: hip.MtmCsdPlan.csd_jackknife_dev(welch, d, d, len(x), d), UNSUPPORTED, 'no tapers')
        assert welch.exec(x).shape == (1024,)
        welch.close()
        eigen = ctx.mtm_csd_plan(1024, nw=4.0, weights='eigen')      # non-uniform weights
        refused(hip, lambda: eigen.jackknife(x), UNSUPPORTED, 'not all equal')
        refused(hip, lambda: eigen.csd_jackknife(x, y), UNSUPPORTED, 'not all equal')
        assert eigen.csd(x, y)[3].shape == (1024,)
        eigen.close()
        same = ctx.mtm_plan(1024, nw=2.0, ntapers=3, weights=[2.0, 2.0, 2.0])      # equal weights of any size are uniform
        assert same.jackknife(x).shape == (1024,)
        refused(hip, lambda: hip.MtmCsdPlan.csd_jackknife(same, x, y), UNSUPPORTED, 'one channel')      # mtm_csd_gate
        same.close()
        plan = ctx.mtm_csd_plan(1024, nw=4.0)
        refused(hip, lambda: plan.jackknife_dev(d, 1024, 65536, 1024, d), UNSUPPORTED, '65535')
        one = ctx.mtm_csd_plan(1024, nw=1.0, ntapers=1)
        refused(hip, lambda: one.jackknife(x[:1024]), INVALID, 'at least 2')      # M = 1
        refused(hip, lambda: one.csd_jackknife(x, y), INVALID, 'at least 3')      # M = 2
        assert one.jackknife(x).shape == (1024,)                                  # M = 2 is enough for ln PSD
        one.close()
        for call in (lambda: plan.jackknife_dev(d, 1024, 1, 1024, 0), lambda: plan.jackknife_dev(0, 1024, 1, 1024, d),
                     lambda: plan.csd_jackknife_dev(d, 0, 1024, d), lambda: plan.csd_jackknife_dev(d, d, 1024, 0),
                     lambda: plan.jackknife_dev(d, 1024, 0, 1024, d)):
            refused(hip, call, INVALID, 'bad argument')
        refused(hip, lambda: plan.jackknife_dev(d, 1024, 2, 1000, d), INVALID, 'stream_stride')
        for call in (lambda: plan.jackknife(x[:1000]), lambda: plan.jackknife_dev(d, 1000, 1, 1000, d),
                     lambda: plan.csd_jackknife(x[:1000], y[:1000]), lambda: plan.csd_jackknife_dev(d, d, 1000, d)):
            refused(hip, call, INVALID, 'shorter than nperseg')
        assert plan.jackknife(x).shape == (1024,) and plan.csd_jackknife(x, y)[1].shape == (1024,)      # the plan still works
        plan.close()
    finally:
        ctx.free(d)


# ---- 5. the helpers: what the feature exists for ------------------------------------------------------------------------------

def white(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)


def test_psd_interval_helper(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    n = 1024
    x = white(n, 0).astype(np.complex64)
    axis, lo, psd, hi = T.mtm_psd_interval(x, n, float(n), fc=1000.0, ctx=ctx)      # fs = n: the true density is 1 / n
    assert lo.shape == psd.shape == hi.shape == (n,) and np.array_equal(axis, np.arange(-n // 2, n // 2) + 1000.0)
    assert np.all(lo <= psd) and np.all(psd <= hi)
    assert np.allclose(psd, np.asarray(T.mtm_plot_dB(x, float(n), 0.0, n, ctx=ctx)[1]), atol=1e-9)
    truth = 10.0 * np.log10(1.0 / n)
    nondc = axis != 1000.0
    cover = float(np.mean((lo[nondc] <= truth) & (truth <= hi[nondc])))
    wide = T.mtm_psd_interval(x, n, float(n), confidence=0.999, ctx=ctx)
    print('mtm_psd_interval: coverage %.3f' % cover)
    assert 0.88 <= cover <= 0.99 and np.all(wide[1] <= lo) and np.all(hi <= wide[3])
    with pytest.raises(ValueError):
        T.mtm_psd_interval(x, n, float(n), confidence=1.0, ctx=ctx)


def test_coherence_interval_helper(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    n = 1024
    x = white(n, 0)
    y = (x + white(n, 1000)).astype(np.complex64)      # true MSC 0.5
    x = x.astype(np.complex64)
    axis, lo, cxy, hi = T.mtm_coherence_interval(x, y, n, float(n), ctx=ctx)
    assert lo.shape == cxy.shape == hi.shape == (n,) and np.array_equal(axis, np.arange(-n // 2, n // 2))
    assert np.all(0.0 <= lo) and np.all(lo <= cxy) and np.all(cxy <= hi) and np.all(hi <= 1.0)
    cover = float(np.mean((lo <= 0.5) & (0.5 <= hi)))
    print('mtm_coherence_interval: coverage %.3f' % cover)
    assert 0.88 <= cover <= 0.99


def test_coherence_estimator_confidence(ctx, hip):
    import ofdm_tools
    N, Sf = 1024, 2000000
    x, y, _ = captures(N, N, 0, 2, 77)
    x, y = x[:2 * N], y[:2 * N]
    plain, conf = (ofdm_tools.coherence_estimator(N, Sf, ctx=ctx, method='mtm', **kw) for kw in ({}, {'confidence': 0.95}))
    msgs = [[], []]
    for est, m in zip((plain, conf), msgs):
        est.msg_connect('coherence', m.append)
        assert est.work([x, y], []) == 2 * N
    assert len(msgs[0]) == len(msgs[1]) == 2
    for a, b in zip(*msgs):
        assert a[0] == b[0] == 'coherence' and np.asarray(a[1]).tobytes() == np.asarray(b[1]).tobytes()
    for name in ('pxx', 'pyy', 'pxy', 'cxy'):
        assert getattr(plain, name).tobytes() == getattr(conf, name).tobytes()
    assert plain.cxy_sd is None and plain.cxy_lo is None
    assert conf.cxy_sd.shape == conf.cxy_lo.shape == (N,) and np.all(conf.cxy_sd >= 0.0)
    assert np.all(conf.cxy_lo <= conf.cxy) and np.all(conf.cxy_lo >= 0.0) and np.any(conf.cxy_lo < conf.cxy)
    with pytest.raises(ValueError):
        ofdm_tools.coherence_estimator(N, Sf, ctx=ctx, confidence=0.95)      # Welch: no items to delete


def test_live_resources_return_to_their_value(ctx, hip):
    x, y, _ = captures(16384, 16384, 0, 2, 5)

    def once():
        plan = ctx.mtm_csd_plan(16384, nw=4.0)
        plan.jackknife(x, return_psd=True)
        plan.csd_jackknife(x, y)
        plan.close()
    once()                                      # (the context keeps the twiddles of a length it has seen)
    before = hip.live_resources()
    once()
    assert hip.live_resources() == before
