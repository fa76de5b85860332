"""GPU tests of the cyclic spectrum and cyclic coherence of Welch plans (oth_welch_set_cycles, oth_welch_cyclic / _dev,
csrc/welchcyc.hip) against the float64 oracle by the definition (tests/welch_cyclic_oracle.py).  Gates on every bin, from the
project's RTOL = 1e-4: the PSD row within RTOL relative; |scf - oracle| <= RTOL scale sqrt(Suu Sxx) / M (the size of a fully
coherent bin); |coh - oracle| <= 4 RTOL, since d coh <= 2 e_sux + e_suu + e_sxx.  Input is unit noise plus tones whose
amplitude test_welch_sk_gpu's amp_for sets (the largest at which float32 holds a per-bin relative gate with a margin of
four).  Measured on an MI355X, worst bin of this file (PSD, scf, coh against gates 1e-4, 1e-4, 4e-4): the twelve parity
cases 2.1e-5, 2.1e-5, 9.7e-6 (4096 points and above; up to 2048 points at most 7.8e-6); the long runs (5000 segments of 64
points, 1200 of 4096) 1.0e-5, 6.6e-6, 3.7e-7; 64 streams x 8 segments of 4096 and 100 x 5 of 16384 with W < nseg 4.4e-5, 2.3e-5,
1.3e-5.  Rows of the A = 5 call against A = 1 calls: bit-identical on each of the three builds at every size tried.  cyclic_scan on the
CP-OFDM case: profile 0.150 at +-1/80 against 0.015 / 0.018 off the cycle frequency and 0.016 ... 0.018 on noise alone
(null 1 / M = 0.0167), the oracle's figures to four digits."""
import numpy as np
import pytest

import median_oracle as MO
import welch_cyclic_oracle as CO
from stat_support import FS, forced_env, recipe_field, welch_plan
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import noise_tones
from test_welch_cyclic_cpu import M as OFDM_M, NFFT as OFDM_NFFT, OFF, ON, check_detection, cp_ofdm
from test_welch_sk_gpu import amp_for, tones_for

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
ALPHAS = (0.0, 0.0123456789, -0.37, 1.0 / 80.0, 0.5)      # A = 5: a full and a partial group of the grouped build


def forced_group(g):
    """plans created inside run the build of welchcyc.hip with g cycle frequencies per workgroup (None: the library's choice)"""
    return forced_env('OTH_CYC_GROUP', g)


def make_plan(ctx, hip, nfft, *args, alphas=ALPHAS, group=None, **kw):
    with forced_group(group):
        plan = welch_plan(ctx, hip, nfft, *args, **kw)
    if alphas is not None:
        plan.set_cycles(alphas)
    return plan


def check_rows(scf, coh, psd, ref, fftshift=False, trim=0, db=False, what=''):
    """the rows of one stream against the oracle's dict at the three gates of the file header -> the worst readings"""
    st = lambda r: MO.shift_trim_db(r, fftshift, trim)      # noqa: E731
    P, S, Cxy = st(ref['psd']), st(ref['scf']), st(ref['coh'])
    size = st(ref['scale'] * np.sqrt(ref['Suu'] * ref['Sxx'][None, :]) / ref['M'])
    scf, coh, psd = np.asarray(scf, np.complex128), np.asarray(coh, np.float64), np.asarray(psd, np.float64)
    assert scf.shape == S.shape and coh.shape == Cxy.shape and psd.shape == P.shape
    assert np.all(np.isfinite(scf)) and np.all(np.isfinite(coh)) and np.all(np.isfinite(psd))
    assert coh.min() >= 0.0 and coh.max() <= 1.0
    lin = 10.0 ** (psd / 10.0) if db else psd
    e_p = float(np.max(np.abs(lin - P) / P))
    e_s = float(np.max(np.abs(scf - S) / size))
    e_c = float(np.max(np.abs(coh - Cxy)))
    if what:
        print('cyclic parity %s: PSD %.2e, scf %.2e, coh %.2e' % (what, e_p, e_s, e_c))
    assert e_p <= RTOL and e_s <= RTOL and e_c <= 4 * RTOL, (what, e_p, e_s, e_c)
    return e_p, e_s, e_c


# ---- 1. parity at every size, 2. the alpha = 0 row ----------------------------------------------------------------------------

PARITY_CASES = [  # nfft, nperseg, overlap %, M, detrend, scaling, fftshift, trim, db, offset
    (64, 64, 0, 9, True, 'density', False, 0, False, 0.0),
    (128, 100, 0, 7, True, 'raw', True, 10, False, 0.0),                      # nperseg < nfft, fftshift with trim
    (256, 256, 50, 9, True, 'density', False, 0, True, 0.0),                  # 50 % overlap, dB on the psd row
    (512, 512, 0, 1, False, 'over_n2', False, 0, False, 0.0),                 # one segment, detrend off
    (1024, 1024, 50, 5, True, 'density', True, 100, False, 35.0 - 20.0j),     # a 35-sigma complex offset under detrend
    (2048, 1500, 0, 3, True, 'spectrum', False, 0, False, 0.0),
    (4096, 4096, 50, 9, True, 'over_n2', False, 0, False, 0.0),
    (4096, 4096, 0, 4, False, 'density', True, 0, True, 0.0),
    (8192, 8192, 0, 2, False, 'raw', False, 0, False, 0.0),
    (8192, 5000, 50, 6, True, 'density', True, 1000, False, 35.0 - 20.0j),
    (16384, 16384, 0, 3, True, 'density', False, 0, False, 0.0),
    (16384, 10000, 50, 5, True, 'over_n2', True, 0, True, 35.0 - 20.0j),
]


@pytest.mark.parametrize('nfft,nperseg,ov,M,detrend,scaling,fftshift,trim,db,offset', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, nperseg, ov, M, detrend, scaling, fftshift, trim, db, offset):
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    x = (noise_tones(noverlap + M * step + step // 3, 7 * nfft + ov + M, tones_for(nfft, amp_for(M, nfft))) + np.complex64(offset)).astype(np.complex64)
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, db)
    scf, coh, psd = plan.cyclic(x, return_psd=True)
    A, m = len(ALPHAS), nfft - 2 * trim
    assert plan.last_nseg == M and scf.shape == coh.shape == (A, m) and psd.shape == (m,)
    assert scf.dtype == np.complex64 and coh.dtype == np.float32
    recipe = plan.last_recipe()
    assert recipe.startswith('kernel=welchcyc nfft=%d W=%d nseg=%d nstreams=1 ncyc=%d group=' % (nfft, M, M, A)), recipe
    assert ' bpc=' in recipe
    ref = CO.cyclic(x, nfft, ALPHAS, nperseg, noverlap, 'hann', detrend, scaling, FS)
    check_rows(scf, coh, psd, ref, fftshift, trim, db, what=str((nfft, nperseg, ov, M, detrend, scaling)) + ' ' + recipe)
    # the alpha = 0 row: three identical sums, an exactly zero imaginary part
    lin = psd.astype(np.float64)
    if db:      # the linear row of the same plan without dB
        twin = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, False)
        lin = twin.cyclic(x, return_psd=True)[2].astype(np.float64)
        twin.close()
    assert np.max(np.abs(coh[0].astype(np.float64) - 1.0)) <= 1e-6
    assert not scf[0].imag.any()
    assert np.max(np.abs(scf[0].real.astype(np.float64) - lin) / lin) <= 1e-6
    if M == 1:
        assert np.max(np.abs(coh.astype(np.float64) - 1.0)) <= 4 * RTOL      # one segment: coherence 1 everywhere
    # without the psd row: it is optional, and takes no part in the others
    only = plan.cyclic(x)
    assert len(only) == 2 and only[1].tobytes() == coh.tobytes() and only[0].tobytes() == scf.tobytes()
    plan.close()


# ---- 3. group independence: both builds, every layout of the state ----------------------------------------------------------------

@pytest.mark.parametrize('nfft,M', [(64, 7), (1024, 5), (4096, 6), (8192, 4), (16384, 3)])
def test_a_row_does_not_depend_on_its_group(ctx, hip, nfft, M):
    """Row a of the A = 5 call - on the library's choice of build and on each build forced - against an A = 1 call with the
    same alpha (one cycle frequency per workgroup, whatever the choice): scf within 1e-6 of sqrt(Suu Sxx), coh within 4e-6."""
    x = noise_tones(nfft * M + 11, 50 + nfft, tones_for(nfft, amp_for(M, nfft)))
    ref = CO.cyclic(x, nfft, ALPHAS, scaling='raw', fs=FS)
    size = ref['scale'] * np.sqrt(ref['Suu'] * ref['Sxx'][None, :]) / ref['M']
    singles = []
    for alpha in ALPHAS:
        one = make_plan(ctx, hip, nfft, scaling='raw', alphas=[alpha])
        scf1, coh1 = one.cyclic(x)
        assert ' ncyc=1 group=1 ' in one.last_recipe(), one.last_recipe()
        singles.append((scf1[0], coh1[0]))
        one.close()
    seen = set()
    for group in (None, 1, 2, 4):
        plan = make_plan(ctx, hip, nfft, scaling='raw', group=group)
        scf, coh, psd = plan.cyclic(x, return_psd=True)
        recipe = plan.last_recipe()
        seen.add(recipe_field(recipe, 'group'))
        assert group is None or recipe_field(recipe, 'group') == group
        check_rows(scf, coh, psd, ref)
        worst = 0.0
        for a in range(len(ALPHAS)):
            e_s = float(np.max(np.abs(scf[a].astype(np.complex128) - singles[a][0]) / size[a]))
            e_c = float(np.max(np.abs(coh[a].astype(np.float64) - singles[a][1])))
            worst = max(worst, e_s, e_c / 4.0)
            assert e_s <= 1e-6 and e_c <= 4e-6, (recipe, a, e_s, e_c)
        print('cyclic rows against single-alpha calls [%s]: %.1e' % (recipe, worst))
        plan.close()
    assert seen == {1, 2, 4}


# ---- 4. runs longer than one segment, large phases -------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,ov,M,group', [(64, 0, 5000, 1), (4096, 50, 1200, None), (4096, 50, 1200, 1), (4096, 50, 1200, 2), (4096, 50, 1200, 4)])
def test_long_runs_and_large_segment_phases(ctx, hip, nfft, ov, M, group):
    """W < nseg, so a workgroup carries its sums across the segments of its run, and alpha s step reaches 3 10^4 turns: the
    segment's phase has to come from the fraction of a double product.  (64 points: the grouped build holds 5000 single
    segments of one group at once on 256 CUs, so that case runs the other build.)"""
    noverlap = nfft * ov // 100
    step = nfft - noverlap
    alphas = (1.0 / 80.0, 0.0123456789)
    x = noise_tones(noverlap + M * step, 77 + nfft, tones_for(nfft, amp_for(M, nfft)))
    plan = make_plan(ctx, hip, nfft, noverlap=noverlap, alphas=alphas, group=group)
    scf, coh, psd = plan.cyclic(x, return_psd=True)
    recipe = plan.last_recipe()
    plan.close()
    W = recipe_field(recipe, 'W')
    if not W < recipe_field(recipe, 'nseg'):
        pytest.skip('this device holds a workgroup per segment: %s' % recipe)
    ref = CO.cyclic(x, nfft, alphas, noverlap=noverlap, fs=FS)
    check_rows(scf, coh, psd, ref, what='long run [%s]' % recipe)


# ---- 5. streams ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,M', [(1024, 6), (16384, 3)])
def test_streams_are_the_one_stream_calls(ctx, hip, nfft, M):
    nstreams, n = 7, nfft * M
    stride = n + 37
    A, m = len(ALPHAS), nfft
    x = noise_tones(stride * nstreams, 300 + nfft, tones_for(nfft, amp_for(M, nfft)))
    plan = make_plan(ctx, hip, nfft, fftshift=True)
    sentinel = np.float32(-7.0)
    words = (3 * A + 1) * m
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * words * (nstreams + 1))
    try:
        ctx.h2d(d, x)
        ctx.h2d(out, np.full(words * (nstreams + 1), sentinel, np.float32))
        # coh [S + 1][A][m], scf [S + 1][A][m][2], psd [S + 1][m]: a spare stream's worth behind each
        coh_d, scf_d, psd_d = out, out + 4 * (nstreams + 1) * A * m, out + 4 * (nstreams + 1) * 3 * A * m
        assert plan.cyclic_dev(d, n, nstreams, stride, coh_d, scf_d, psd_d) == M == plan.last_nseg
        recipe = plan.last_recipe()
        got = ctx.d2h(out, (words * (nstreams + 1),), np.float32)
        coh = got[:(nstreams + 1) * A * m].reshape(nstreams + 1, A, m)
        scf = got[(nstreams + 1) * A * m:(nstreams + 1) * 3 * A * m].reshape(nstreams + 1, A, m, 2)
        psd = got[(nstreams + 1) * 3 * A * m:].reshape(nstreams + 1, m)
        assert np.all(coh[nstreams] == sentinel) and np.all(scf[nstreams] == sentinel) and np.all(psd[nstreams] == sentinel)
        assert 'nstreams=%d ' % nstreams in recipe
        W = recipe_field(recipe, 'W')
        for s in range(nstreams):
            xs = x[s * stride:s * stride + n]
            scf1, coh1, psd1 = plan.cyclic(xs, return_psd=True)
            got_scf = scf[s, ..., 0] + 1j * scf[s, ..., 1]
            if recipe_field(plan.last_recipe(), 'W') == W:
                assert coh[s].tobytes() == coh1.tobytes() and psd[s].tobytes() == psd1.tobytes()
                assert np.array_equal(got_scf.astype(np.complex64).view(np.uint32), scf1.view(np.uint32))
            else:
                ref = CO.cyclic(xs, nfft, ALPHAS, fs=FS)
                size = np.fft.fftshift(ref['scale'] * np.sqrt(ref['Suu'] * ref['Sxx'][None, :]) / ref['M'], axes=-1)
                assert np.max(np.abs(got_scf - scf1) / size) <= 1e-6 and np.max(np.abs(coh[s] - coh1)) <= 4e-6
                assert np.max(np.abs(psd[s] - psd1) / psd1) <= 1e-6
        # coh alone on the device form: no other row is touched
        ctx.h2d(out, np.full(words * (nstreams + 1), sentinel, np.float32))
        plan.cyclic_dev(d, n, nstreams, stride, coh_d)
        again = ctx.d2h(out, (words * (nstreams + 1),), np.float32)
        assert again[:nstreams * A * m].tobytes() == coh[:nstreams].tobytes() and np.all(again[nstreams * A * m:] == sentinel)
    finally:
        ctx.free(d)
        ctx.free(out)
    plan.close()


@pytest.mark.parametrize('nfft,M,nstreams', [(4096, 8, 64), (16384, 5, 100)])
def test_streams_whose_workgroups_walk_several_segments(ctx, hip, nfft, M, nstreams):
    """more streams than the device holds a workgroup per segment for: W < nseg with stream_stride > nsamples, every stream
    against the oracle (sums in registers at 4096 points, in the partial rows and with the workspace row at 16384)"""
    alphas = (1.0 / 80.0, 0.0123456789, -0.37)
    n = nfft * M
    stride = n + 64
    A, m = len(alphas), nfft
    x = noise_tones(stride * nstreams, 700 + nfft, tones_for(nfft, amp_for(M, nfft * nstreams)))
    plan = make_plan(ctx, hip, nfft, alphas=alphas)
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * (3 * A + 1) * m * nstreams)
    try:
        ctx.h2d(d, x)
        coh_d, scf_d, psd_d = out, out + 4 * nstreams * A * m, out + 4 * nstreams * 3 * A * m
        assert plan.cyclic_dev(d, n, nstreams, stride, coh_d, scf_d, psd_d) == M
        got = ctx.d2h(out, ((3 * A + 1) * m * nstreams,), np.float32)
    finally:
        ctx.free(d)
        ctx.free(out)
    recipe = plan.last_recipe()
    plan.close()
    assert 1 <= recipe_field(recipe, 'W') < M, recipe
    coh = got[:nstreams * A * m].reshape(nstreams, A, m)
    scf = got[nstreams * A * m:nstreams * 3 * A * m].reshape(nstreams, A, m, 2)
    psd = got[nstreams * 3 * A * m:].reshape(nstreams, m)
    worst = np.zeros(3)
    for s in range(nstreams):
        ref = CO.cyclic(x[s * stride:s * stride + n], nfft, alphas, fs=FS)
        worst = np.maximum(worst, check_rows(scf[s, ..., 0] + 1j * scf[s, ..., 1], coh[s], psd[s], ref))
    print('cyclic %d streams x %d segments of %d [%s]: PSD %.2e, scf %.2e, coh %.2e' % (nstreams, M, nfft, recipe, worst[0], worst[1], worst[2]))


# ---- 6. run-to-run identity ------------------------------------------------------------------------------------------------------

def test_two_calls_are_bit_identical_and_sources_agree(ctx, hip):
    for nfft, ov, M in ((2048, 50, 21), (8192, 0, 5), (16384, 0, 5)):
        noverlap = nfft * ov // 100
        x = noise_tones(noverlap + M * (nfft - noverlap), 13 + nfft, tones_for(nfft))
        plan = make_plan(ctx, hip, nfft, noverlap=noverlap)
        a = plan.cyclic(x, return_psd=True)
        b = plan.cyclic(x, return_psd=True)
        d = ctx.alloc(x.nbytes)
        try:
            ctx.h2d(d, x)
            c = plan.cyclic(d, return_psd=True, nsamples=len(x))
        finally:
            ctx.free(d)
        assert plan.last_nseg == M
        for i in range(3):
            assert a[i].tobytes() == b[i].tobytes() == c[i].tobytes()
        plan.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_plan_usable(ctx, hip):
    x = noise_tones(4096, 9)
    d = ctx.alloc(x.nbytes)

    def refused(call, code, word):
        with pytest.raises(hip.HipError) as ei:
            call()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    try:
        ctx.h2d(d, x)
        mtm = ctx.mtm_plan(1024, nw=4.0)
        refused(lambda: mtm.set_cycles([0.0125]), UNSUPPORTED, 'multitaper')
        refused(lambda: mtm.cyclic(x), UNSUPPORTED, 'multitaper')
        refused(lambda: mtm.cyclic_dev(d, len(x), 1, len(x), d), UNSUPPORTED, 'multitaper')
        assert mtm.exec(x).shape == (1024,)
        mtm.close()
        med = make_plan(ctx, hip, 1024)                                            # (the cycles go in before the median)
        med.set_average('median')
        refused(lambda: med.cyclic(x), UNSUPPORTED, 'MEDIAN')
        refused(lambda: med.cyclic_dev(d, len(x), 1, len(x), d), UNSUPPORTED, 'MEDIAN')
        refused(lambda: med.set_cycles([0.1]), UNSUPPORTED, 'MEDIAN')
        assert med.exec(x).shape == (1024,)
        med.set_average('mean')
        assert med.cyclic(x)[1].shape == (len(ALPHAS), 1024)                       # ... and the mean is served
        med.close()
        for nfft in (100, 32, 32768):
            odd = make_plan(ctx, hip, nfft, alphas=None)
            big = noise_tones(4 * nfft, 3)
            refused(lambda: odd.set_cycles([0.0125]), UNSUPPORTED, 'power of two')
            refused(lambda: odd.cyclic(big), UNSUPPORTED, 'power of two')
            assert odd.exec(big).shape == (nfft,)
            odd.close()
        plan = make_plan(ctx, hip, 1024, alphas=None)
        refused(lambda: plan.cyclic(x), UNSUPPORTED, 'oth_welch_set_cycles')       # no cycles yet
        refused(lambda: plan.cyclic_dev(d, 2048, 1, 2048, d), UNSUPPORTED, 'oth_welch_set_cycles')
        refused(lambda: plan.set_cycles([]), INVALID, 'ncycles')
        refused(lambda: plan.set_cycles(np.zeros(65)), INVALID, 'ncycles')
        for bad in ([0.1, 0.51], [-0.5000001], [float('nan')], [0.0, float('inf')]):
            refused(lambda: plan.set_cycles(bad), INVALID, 'alpha')
        refused(lambda: ctx.check(ctx.lib.oth_welch_set_cycles(plan.h, 2, None), 'oth_welch_set_cycles'), INVALID, 'NULL')
        refused(lambda: plan.cyclic(x), UNSUPPORTED, 'oth_welch_set_cycles')       # a refused set leaves none
        plan.set_cycles([0.25])
        assert plan.cyclic(x)[1].shape == (1, 1024)
        plan.set_cycles(np.linspace(-0.5, 0.5, 64))                                # the bounds are in; 64 is served
        assert plan.cyclic(x)[1].shape == (64, 1024)
        plan.set_cycles(ALPHAS)                                                    # a second call replaces the set
        refused(lambda: plan.set_cycles([0.7]), INVALID, 'alpha')                  # ... and a refused one keeps it
        refused(lambda: plan.cyclic(x[:1000]), INVALID, 'nperseg')
        refused(lambda: plan.cyclic_dev(d, 2048, 2, 2000, d), INVALID, 'stream_stride')
        refused(lambda: plan.cyclic_dev(d, 2048, 0, 2048, d), INVALID, 'bad argument')
        refused(lambda: plan.cyclic_dev(0, 2048, 1, 2048, d), INVALID, 'bad argument')
        refused(lambda: plan.cyclic_dev(d, 2048, 1, 2048, 0), INVALID, 'bad argument')
        refused(lambda: plan.cyclic_dev(d, 2048, 65536, 2048, d), UNSUPPORTED, '65535')
        ref = CO.cyclic(x, 1024, ALPHAS, fs=FS)
        scf, coh, psd = plan.cyclic(x, return_psd=True)                            # ... and the plan still works
        check_rows(scf, coh, psd, ref)
        exec_row = plan.exec(x)                                                    # no other call of the plan is affected
        assert np.max(np.abs(exec_row - ref['psd']) / ref['psd']) <= RTOL
        plan.close()
    finally:
        ctx.free(d)


# ---- 8. degenerate input ---------------------------------------------------------------------------------------------------------

def test_silence_and_a_constant_give_zero_rows(ctx, hip):
    for nfft in (256, 4096, 16384):
        plan = make_plan(ctx, hip, nfft, fftshift=True)
        raw = make_plan(ctx, hip, nfft, detrend=False)
        for p, x in ((plan, np.zeros(3 * nfft, np.complex64)), (raw, np.zeros(3 * nfft, np.complex64)),
                     (plan, np.full(3 * nfft, 3.0 - 2.0j, np.complex64))):
            scf, coh, psd = p.cyclic(x, return_psd=True)
            assert scf.shape == coh.shape == (len(ALPHAS), nfft) and psd.shape == (nfft,)
            assert not scf.any() and not coh.any() and not psd.any()
        plan.close()
        raw.close()


def test_a_strong_tone_on_a_bin_stays_finite(ctx, hip):
    """noise plus one tone on a bin, its amplitude from amp_for, and the same tone with nothing else: every row finite,
    the coherence inside [0, 1]"""
    for nfft, M in ((512, 5), (16384, 4)):
        k = nfft // 8
        t = np.arange(nfft * M)
        amp = amp_for(M, nfft)
        tone = (amp * np.exp(2j * np.pi * k / float(nfft) * t)).astype(np.complex64)
        plan = make_plan(ctx, hip, nfft)
        for x in (noise_tones(nfft * M, 31, ((amp, k / float(nfft)),)), tone):
            scf, coh, psd = plan.cyclic(x, return_psd=True)
            assert np.all(np.isfinite(scf)) and np.all(np.isfinite(coh)) and np.all(np.isfinite(psd))
            assert coh.min() >= 0.0 and coh.max() <= 1.0 and np.all(psd >= 0)
        plan.close()


# ---- 9. detection: what the feature exists for --------------------------------------------------------------------------------------

def test_cyclic_scan_detects_cp_ofdm_and_reads_the_null_on_noise(ctx, hip):
    """the CP-OFDM case of the CPU file, seed 0 (Tu 64, Tcp 16, 20 dB, 256 points, M = 60) through cyclic_scan: the profile
    within 1e-3 of the oracle's, at least 5 x the off-cycle entries at +-1/80, those and the noise-only profile <= 2.5 / M"""
    from ofdm_tools import ofdm_cr_tools as T
    Sf = 20e6
    alphas = np.array(ON + OFF)
    x = cp_ofdm(0)
    prof, coh, axis, null = T.cyclic_scan(x, OFDM_NFFT, Sf, alphas * Sf, ctx=ctx)
    assert prof.shape == (4,) and coh.shape == (4, OFDM_NFFT) and null == 1.0 / OFDM_M
    assert np.array_equal(axis, np.fft.fftshift(np.fft.fftfreq(OFDM_NFFT, 1.0 / Sf)))
    ref = CO.cyclic(x, OFDM_NFFT, alphas)
    assert np.max(np.abs(prof - ref['coh'].mean(axis=1))) <= 1e-3
    assert np.max(np.abs(coh - np.fft.fftshift(ref['coh'], axes=-1))) <= 4 * RTOL
    check_detection(prof[:2], prof[2:], 'GPU, seed 0')
    assert np.allclose(T.ofdm_cycle_frequencies(64, 16, Sf, harmonics=1), alphas[:2] * Sf, rtol=1e-12)
    noise = T.cyclic_scan(cp_ofdm(0, signal=False), OFDM_NFFT, Sf, alphas * Sf, fc=1e9, ctx=ctx)
    print('noise alone: %s' % np.round(noise[0], 4))
    assert max(noise[0]) <= 2.5 / OFDM_M and np.array_equal(noise[2], axis + 1e9)
