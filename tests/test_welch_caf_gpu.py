"""GPU tests of the cyclic autocorrelation of Welch plans (oth_welch_set_lags, oth_welch_caf / _dev, csrc/welchlag.hip)
against the float64 oracle by the definition (tests/welch_caf_oracle.py).  Gates from the project's RTOL = 1e-4: every bin of
caf within RTOL relative of the oracle, |r - oracle| <= RTOL mean|z|.  A float32 emulation of the definition (complex64
products, a float32 transform) against float64, on unit noise with a 3-sigma tone or a 35 - 20j offset, stayed at or below
3.5e-6 per bin on caf and 5e-8 on r for M >= 3; with one segment it reached 4e-5 per bin, so the one-segment case is gated at
RTOL of the row's mean, not per bin.  Input is test_median_gpu's noise_tones: unit noise, a 3-sigma and a 0.5-sigma tone, a
small offset.
Measured on an MI355X, worst readings of this file (caf per bin, r; gates 1e-4, 1e-4): the ten parity cases with M >= 3
8.3e-6, 5.9e-8 (the worst at 8192 points under the 35 - 20j offset; 64 ... 256 points at most 4.0e-7); the one-segment case
1.5e-5 of the row's mean, 6.8e-8; lag 65535 3.4e-6, 4.8e-8; three padded streams with NaN gaps 5.0e-6, 4.7e-8; 64 streams x 8
segments of 4096 2.9e-6, 4.5e-8 and 100 x 5 of 16384 with W < nseg 8.3e-6, 4.4e-8.  Rows of the L = 5 call against L = 1 calls:
bit-identical on both builds at every size tried.  Against the torch product + exec_dev: 1.5e-6.  ofdm_blind_parameters on
CP-OFDM at 0 dB: statistic 23.2 for (64, 16) and for (256, 64) against a threshold of 1.57, 1.24 on noise alone - the
oracle's figures to seven digits."""
import numpy as np
import pytest

import median_oracle as MO
import welch_caf_oracle as LO
import welch_cyclic_oracle as CO
from stat_support import FS, forced_env, recipe_field, welch_plan
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import noise_tones
from test_welch_caf_cpu import BLIND_LENS, BLIND_M, BLIND_NFFT, blind_capture, blind_oracle
from test_welch_cyclic_cpu import check_detection

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
LAGS = (0, 1, 37, 64, 5000)      # L = 5: full groups and a partial one of the grouped build
GROUPS = (1, 2)                  # the shipped builds of welchlag.hip


def forced_group(g):
    """plans created inside run the build of welchlag.hip with g lags per workgroup (None: the library's choice)"""
    return forced_env('OTH_LAG_GROUP', g)


def make_plan(ctx, hip, nfft, *args, lags=LAGS, group=None, **kw):
    with forced_group(group):
        plan = welch_plan(ctx, hip, nfft, *args, **kw)
    if lags is not None:
        plan.set_lags(lags)
    return plan


def check_rows(caf, r, ref, fftshift=False, trim=0, db=False, one_segment=False, what=''):
    """the rows of one stream against the oracle's dict at the gates of the file header -> the worst readings (caf, r)"""
    want = MO.shift_trim_db(ref['caf'], fftshift, trim)
    caf = np.asarray(caf, np.float64)
    assert caf.shape == want.shape
    assert np.all(np.isfinite(caf))
    lin = 10.0 ** (caf / 10.0) if db else caf
    if one_segment:
        e_c = float(np.max(np.abs(lin - want) / want.mean(axis=-1, keepdims=True)))
    else:
        e_c = float(np.max(np.abs(lin - want) / want))
    e_r = 0.0
    if r is not None:
        r = np.asarray(r, np.complex128)
        assert r.shape == ref['r'].shape and np.all(np.isfinite(r))
        e_r = float(np.max(np.abs(r - ref['r']) / ref['zabs']))
    if what:
        print('caf parity %s: caf %.2e, r %.2e' % (what, e_c, e_r))
    assert e_c <= RTOL and e_r <= RTOL, (what, e_c, e_r)
    return e_c, e_r


def run_dev(ctx, plan, x, nsamples, nstreams, stride, L, want_r=True):
    """caf_dev on nstreams captures -> (caf [nstreams, L, out_len], r [nstreams, L] complex, M)"""
    m = plan.out_len
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * nstreams * L * (m + 2))
    try:
        ctx.h2d(d, x)
        M = plan.caf_dev(d, nsamples, nstreams, stride, out, out + 4 * nstreams * L * m if want_r else None)
        got = ctx.d2h(out, (nstreams * L * (m + 2),), np.float32)
    finally:
        ctx.free(d)
        ctx.free(out)
    rr = got[nstreams * L * m:].reshape(nstreams, L, 2)
    return got[:nstreams * L * m].reshape(nstreams, L, m), rr[..., 0] + 1j * rr[..., 1], M


# ---- 1. parity at every size ---------------------------------------------------------------------------------------------------

PARITY_CASES = [  # nfft, nperseg, overlap %, M, detrend, scaling, fftshift, trim, db, offset
    (64, 64, 0, 9, True, 'density', False, 0, False, 0.0),
    (128, 100, 0, 7, True, 'raw', True, 10, False, 0.0),                      # nperseg < nfft, fftshift with trim
    (256, 256, 50, 9, True, 'density', False, 0, True, 0.0),                  # 50 % overlap, dB
    (512, 512, 0, 1, False, 'density', False, 0, False, 0.0),                 # one segment, detrend off: the one-segment gate
    (1024, 1024, 50, 5, True, 'density', False, 0, False, 35.0 - 20.0j),      # a 35-sigma complex offset under detrend
    (2048, 1500, 0, 3, True, 'spectrum', False, 0, False, 0.0),
    (4096, 4096, 50, 9, True, 'density', False, 0, False, 0.0),
    (4096, 4096, 0, 4, False, 'density', False, 0, False, 0.0),
    (8192, 5000, 50, 6, True, 'density', False, 0, False, 35.0 - 20.0j),
    (16384, 16384, 0, 3, True, 'density', False, 0, False, 0.0),
    (16384, 10000, 50, 5, True, 'density', False, 0, False, 0.0),
]


@pytest.mark.parametrize('nfft,nperseg,ov,M,detrend,scaling,fftshift,trim,db,offset', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, nperseg, ov, M, detrend, scaling, fftshift, trim, db, offset):
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    x = (noise_tones(max(LAGS) + noverlap + M * step + step // 3, 7 * nfft + ov + M) + np.complex64(offset)).astype(np.complex64)
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, db)
    caf, r = plan.caf(x, return_r=True)
    L, m = len(LAGS), nfft - 2 * trim
    assert plan.last_nseg == M and caf.shape == (L, m) and r.shape == (L,)
    assert caf.dtype == np.float32 and r.dtype == np.complex64
    recipe = plan.last_recipe()
    assert recipe.startswith('kernel=welchlag nfft=%d W=%d nseg=%d nstreams=1 nlags=%d group=' % (nfft, M, M, L)), recipe
    assert ' bpc=' in recipe
    ref = LO.caf(x, nfft, LAGS, nperseg, noverlap, 'hann', detrend, scaling, FS)
    assert ref['M'] == M
    check_rows(caf, r, ref, fftshift, trim, db, one_segment=M == 1, what=str((nfft, nperseg, ov, M, detrend, scaling)) + ' ' + recipe)
    assert r[0].imag == 0.0 and r[0].real > 0.0      # lag 0: the mean power, an exactly zero imaginary part
    only = plan.caf(x)                               # without r: it is optional, and takes no part in the rows
    assert only.tobytes() == caf.tobytes()
    plan.close()


# ---- 2. the largest lag ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft', [64, 4096])
def test_the_largest_lag_reads_up_to_the_last_sample(ctx, hip, nfft):
    M, lags = 3, (65535, 0)
    x = noise_tones(65535 + M * nfft, 40 + nfft)
    plan = make_plan(ctx, hip, nfft, lags=lags)
    caf, r = plan.caf(x, return_r=True)
    assert plan.last_nseg == M
    check_rows(caf, r, LO.caf(x, nfft, lags, fs=FS), what='lag 65535 at %d points' % nfft)
    plan.close()


# ---- 3. no read outside a stream -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft', [64, 4096, 16384])
def test_no_read_leaves_the_stream(ctx, hip, nfft):
    """three streams with a gap of NaN behind each: the furthest lagged sample of a stream's last segment is its last sample"""
    M, lags, nstreams = 3, (0, 999), 3
    n = 999 + M * nfft
    stride = n + 100
    x = noise_tones(stride * nstreams, 90 + nfft)
    for s in range(nstreams):
        x[s * stride + n:(s + 1) * stride] = np.nan
    plan = make_plan(ctx, hip, nfft, lags=lags)
    caf, r, got_m = run_dev(ctx, plan, x, n, nstreams, stride, len(lags))
    assert got_m == M == plan.last_nseg
    for s in range(nstreams):
        check_rows(caf[s], r[s], LO.caf(x[s * stride:s * stride + n], nfft, lags, fs=FS), what='stream %d of %d points' % (s, nfft))
    plan.close()


# ---- 4. group independence: both builds, every layout of the state ---------------------------------------------------------------

@pytest.mark.parametrize('nfft,M', [(64, 7), (1024, 5), (4096, 6), (8192, 4), (16384, 3)])
def test_a_row_does_not_depend_on_its_group(ctx, hip, nfft, M):
    """Row l of the L = 5 call - on the library's choice of build and on each build forced - against an L = 1 call with the same
    lag and the same capture length: within 1e-6 of the row's mean.  (The L = 1 plan sees the capture cut to its own lag's
    reach, so that both count the same segments.)"""
    x = noise_tones(nfft * M + max(LAGS) + 11, 50 + nfft)
    ref = LO.caf(x, nfft, LAGS, scaling='raw', fs=FS)
    singles = []
    for tau in LAGS:
        one = make_plan(ctx, hip, nfft, scaling='raw', lags=[tau])
        row, r1 = one.caf(x[:nfft * M + tau + 11], return_r=True)
        assert one.last_nseg == M and ' nlags=1 group=1 ' in one.last_recipe(), one.last_recipe()
        singles.append((row[0].astype(np.float64), r1[0]))
        one.close()
    seen = set()
    for group in (None,) + GROUPS:
        plan = make_plan(ctx, hip, nfft, scaling='raw', group=group)
        caf, r = plan.caf(x, return_r=True)
        recipe = plan.last_recipe()
        seen.add(recipe_field(recipe, 'group'))
        assert group is None or recipe_field(recipe, 'group') == group
        check_rows(caf, r, ref)
        worst = 0.0
        for l in range(len(LAGS)):
            e = float(np.max(np.abs(caf[l].astype(np.float64) - singles[l][0])) / singles[l][0].mean())
            worst = max(worst, e)
            assert e <= 1e-6 and abs(r[l] - singles[l][1]) <= 1e-6 * ref['zabs'][l], (recipe, l, e)
        print('caf rows against single-lag calls [%s]: %.1e' % (recipe, worst))
        plan.close()
    assert seen == set(GROUPS)


# ---- 5. many streams ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,M,nstreams', [(4096, 8, 64), (16384, 5, 100)])
def test_many_streams_against_the_oracle_and_bit_identical(ctx, hip, nfft, M, nstreams):
    lags = (0, 64, 700)
    n = nfft * M + max(lags)
    stride = n + 64
    x = noise_tones(stride * nstreams, 700 + nfft)
    plan = make_plan(ctx, hip, nfft, lags=lags)
    caf, r, got_m = run_dev(ctx, plan, x, n, nstreams, stride, len(lags))
    recipe = plan.last_recipe()
    again = run_dev(ctx, plan, x, n, nstreams, stride, len(lags))
    plan.close()
    assert got_m == M and 'nstreams=%d ' % nstreams in recipe
    assert again[0].tobytes() == caf.tobytes() and again[1].tobytes() == r.tobytes()
    if nfft == 16384:
        assert 1 <= recipe_field(recipe, 'W') < M, recipe      # a workgroup carries its sums across the segments of its run
    worst = np.zeros(2)
    for s in range(nstreams):
        worst = np.maximum(worst, check_rows(caf[s], r[s], LO.caf(x[s * stride:s * stride + n], nfft, lags, fs=FS)))
    print('caf %d streams x %d segments of %d [%s]: caf %.2e, r %.2e' % (nstreams, M, nfft, recipe, worst[0], worst[1]))


# ---- 6. against the composition on the GPU -----------------------------------------------------------------------------------------

def test_the_composition_gives_the_same_rows(ctx, hip):
    """what a user had before: one torch product per lag, then exec_dev of the same plan with the products as streams"""
    import torch
    nfft, M, lags = 4096, 6, (0, 64)
    n = nfft * M
    x = noise_tones(n + max(lags), 123)
    plan = make_plan(ctx, hip, nfft, lags=lags)
    caf = plan.caf(x)
    dev = torch.device('cuda', 0)
    xt = torch.from_numpy(x).to(dev)
    z = torch.stack([xt[tau:tau + n] * torch.conj(xt[:n]) for tau in lags]).contiguous()
    out = torch.empty((len(lags), nfft), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    assert plan.exec_dev(z.data_ptr(), n, out.data_ptr(), nstreams=len(lags), stream_stride=n) == M == plan.last_nseg
    ctx.sync()
    comp = out.cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(caf.astype(np.float64) - comp) / comp))
    print('caf against torch product + exec_dev: %.2e [%s]' % (err, plan.last_recipe()))
    assert err <= 2 * RTOL
    plan.close()


# ---- 7. degenerate input -------------------------------------------------------------------------------------------------------------

def test_silence_and_a_constant_give_zero_rows(ctx, hip):
    for nfft in (256, 4096, 16384):
        n = 3 * nfft + max(LAGS)
        plan = make_plan(ctx, hip, nfft, fftshift=True)
        raw = make_plan(ctx, hip, nfft, detrend=False)
        dbp = make_plan(ctx, hip, nfft, db=True)
        for p in (plan, raw):
            caf, r = p.caf(np.zeros(n, np.complex64), return_r=True)
            assert caf.shape == (len(LAGS), nfft) and not caf.any() and not r.any()
        const = np.full(n, 3.0 - 2.0j, np.complex64)
        caf, r = plan.caf(const, return_r=True)
        assert not caf.any() and np.all(r == np.complex64(13.0))
        assert np.all(np.isneginf(dbp.caf(const)))
        for p in (plan, raw, dbp):
            p.close()


@pytest.mark.parametrize('nfft', [256, 4096, 16384])
def test_a_nan_stays_in_its_stream_and_its_rows(ctx, hip, nfft):
    """a NaN in the last segment's reach of lag 5000 only: that row of that stream is NaN in every bin, the stream's other
    rows and the other streams are the clean launch's bit for bit; then a clean call on the same plan"""
    M, nstreams = 3, 3
    n = nfft * M + max(LAGS)
    x = noise_tones(n * nstreams, 5 + nfft)
    plan = make_plan(ctx, hip, nfft, db=True)
    clean, r_clean, _ = run_dev(ctx, plan, x, n, nstreams, n, len(LAGS))
    bad = x.copy()
    bad[n + n - 1] = np.complex64(complex(np.nan, 0.0))      # stream 1's last sample: lag 5000 alone reaches it
    caf, r, _ = run_dev(ctx, plan, bad, n, nstreams, n, len(LAGS))
    assert np.all(np.isnan(caf[1, 4])) and np.isnan(r[1, 4])
    assert caf[1, :4].tobytes() == clean[1, :4].tobytes() and caf[0].tobytes() == clean[0].tobytes() and caf[2].tobytes() == clean[2].tobytes()
    assert r[0].tobytes() == r_clean[0].tobytes() and r[2].tobytes() == r_clean[2].tobytes()
    bad[n + nfft] = np.complex64(complex(0.0, np.inf))       # ... and an inf every lag's products hold: NaN, never inf
    caf, r, _ = run_dev(ctx, plan, bad, n, nstreams, n, len(LAGS))
    assert np.all(np.isnan(caf[1])) and caf[0].tobytes() == clean[0].tobytes() and caf[2].tobytes() == clean[2].tobytes()
    after, r_after, _ = run_dev(ctx, plan, x, n, nstreams, n, len(LAGS))
    assert after.tobytes() == clean.tobytes() and r_after.tobytes() == r_clean.tobytes()
    plan.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_plan_usable(ctx, hip):
    x = noise_tones(4096 + 5000, 9)
    d = ctx.alloc(x.nbytes)

    def refused(call, code, word):
        with pytest.raises(hip.HipError) as ei:
            call()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    try:
        ctx.h2d(d, x)
        mtm = ctx.mtm_plan(1024, nw=4.0)
        refused(lambda: mtm.set_lags([64]), UNSUPPORTED, 'multitaper')
        refused(lambda: mtm.caf(x), UNSUPPORTED, 'multitaper')
        refused(lambda: mtm.caf_dev(d, len(x), 1, len(x), d), UNSUPPORTED, 'multitaper')
        assert mtm.exec(x).shape == (1024,)
        mtm.close()
        med = make_plan(ctx, hip, 1024)                                            # (the lags go in before the median)
        med.set_average('median')
        refused(lambda: med.caf(x), UNSUPPORTED, 'MEDIAN')
        refused(lambda: med.caf_dev(d, len(x), 1, len(x), d), UNSUPPORTED, 'MEDIAN')
        refused(lambda: med.set_lags([1]), UNSUPPORTED, 'MEDIAN')
        assert med.exec(x).shape == (1024,)
        med.set_average('mean')
        assert med.caf(x).shape == (len(LAGS), 1024)                               # ... and the mean is served
        med.close()
        for nfft in (100, 32, 32768):
            odd = make_plan(ctx, hip, nfft, lags=None)
            big = noise_tones(4 * nfft, 3)
            refused(lambda: odd.set_lags([1]), UNSUPPORTED, 'power of two')
            refused(lambda: odd.caf(big), UNSUPPORTED, 'power of two')
            assert odd.exec(big).shape == (nfft,)
            odd.close()
        plan = make_plan(ctx, hip, 1024, lags=None)
        refused(lambda: plan.caf(x), UNSUPPORTED, 'oth_welch_set_lags')            # no lags yet
        refused(lambda: plan.caf_dev(d, 2048, 1, 2048, d), UNSUPPORTED, 'oth_welch_set_lags')
        refused(lambda: plan.set_lags([]), INVALID, 'nlags')
        refused(lambda: plan.set_lags(np.zeros(65, np.int64)), INVALID, 'nlags')
        for bad in ([1, -1], [65536], [0, 1 << 40]):
            refused(lambda: plan.set_lags(bad), INVALID, '65535')
        refused(lambda: ctx.check(ctx.lib.oth_welch_set_lags(plan.h, 2, None), 'oth_welch_set_lags'), INVALID, 'NULL')
        refused(lambda: plan.caf(x), UNSUPPORTED, 'oth_welch_set_lags')            # a refused set leaves none
        plan.set_lags([7])
        assert plan.caf(x).shape == (1, 1024)
        plan.set_lags(np.arange(64) * 70)                                          # 64 is served
        assert plan.caf(x).shape == (64, 1024)
        plan.set_lags([0, 65535])                                                  # the bounds are in
        refused(lambda: plan.caf(x), INVALID, 'nperseg')                           # ... and the capture is too short for them
        plan.set_lags(LAGS)                                                        # a second call replaces the set
        refused(lambda: plan.set_lags([70000]), INVALID, '65535')                  # ... and a refused one keeps it
        refused(lambda: plan.caf(x[:5000 + 1023]), INVALID, 'nperseg')
        assert plan.caf(x[:5000 + 1024]).shape == (len(LAGS), 1024) and plan.last_nseg == 1
        refused(lambda: plan.caf_dev(d, 7000, 2, 6999, d), INVALID, 'stream_stride')
        refused(lambda: plan.caf_dev(d, 7000, 0, 7000, d), INVALID, 'bad argument')
        refused(lambda: plan.caf_dev(0, 7000, 1, 7000, d), INVALID, 'bad argument')
        refused(lambda: plan.caf_dev(d, 7000, 1, 7000, 0), INVALID, 'bad argument')
        refused(lambda: plan.caf_dev(d, 7000, 65536, 7000, d), UNSUPPORTED, '65535')
        ref = LO.caf(x, 1024, LAGS, fs=FS)
        caf, r = plan.caf(x, return_r=True)                                        # ... and the plan still works
        check_rows(caf, r, ref)
        psd = plan.exec(x)                                                         # no other call of the plan is affected
        want = CO.cyclic(x, 1024, [0.0], fs=FS)['psd']
        assert np.max(np.abs(psd - want) / want) <= RTOL
        plan.close()
    finally:
        ctx.free(d)


# ---- 9. end to end: what the feature exists for ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('tu,tcp', [(64, 16), (256, 64)])
def test_blind_parameters_find_cp_ofdm_and_feed_cyclic_scan(ctx, hip, tu, tcp):
    """CP-OFDM at 0 dB, 4096 points, 32 segments, candidates (32, 64, 128, 256): the right pair, detected, the statistic
    within 1e-3 relative of the oracle's.  Its cycles_hz then go through cyclic_scan on the same capture (4 Tu points) next to
    two cycle frequencies of other symbol periods: the profile is the float64 oracle's, and for (64, 16) it passes the on / off
    condition of the cyclic tests.  For (256, 64) at 0 dB the float64 oracle itself reads on / off = 1.1 ... 2.0 at every
    transform length from 64 to 16384 - 131072 samples hold 410 symbols - so there the condition is not the code's to meet."""
    from ofdm_tools import ofdm_cr_tools as T
    Sf = 20e6
    x = blind_capture(0, tu, tcp, 0.0)
    got = T.ofdm_blind_parameters(x, Sf, fft_lens=BLIND_LENS, nFFT=BLIND_NFFT, ctx=ctx)
    want = blind_oracle(x, Sf)
    print('blind parameters: %s' % {k: got[k] for k in ('detected', 'fft_len', 'cp_len', 'stat', 'threshold', 'rho', 'nseg')})
    assert got['detected'] and (got['fft_len'], got['cp_len']) == (tu, tcp) and got['nseg'] == BLIND_M
    assert abs(got['stat'] - want['stat']) <= 1e-3 * want['stat'] and got['threshold'] == want['threshold']
    assert abs(got['rho'] - want['rho']) <= 1e-3 * want['rho']
    assert np.array_equal(got['cycles_hz'], T.ofdm_cycle_frequencies(tu, tcp, Sf))
    ts = tu + tcp
    cycles = np.concatenate([got['cycles_hz'][:2], [Sf / (ts - 3.0), -Sf / (ts + 7.0)]])
    prof = T.cyclic_scan(x, 4 * tu, Sf, cycles, ctx=ctx)[0]
    ref = CO.profile(x, 4 * tu, cycles / Sf)
    print('cyclic_scan on the blind cycle frequencies (%d, %d): on %s, off %s (oracle %s)' % (tu, tcp, np.round(prof[:2], 4), np.round(prof[2:], 4), np.round(ref, 4)))
    assert np.max(np.abs(prof - ref)) <= 1e-3
    if (tu, tcp) == (64, 16):
        check_detection(prof[:2], prof[2:], 'GPU, blind (%d, %d)' % (tu, tcp))
    else:
        assert min(prof[:2]) > max(prof[2:])


def test_blind_parameters_on_noise_alone(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    x = blind_capture(0, signal=False)
    got = T.ofdm_blind_parameters(x, 20e6, fft_lens=BLIND_LENS, nFFT=BLIND_NFFT, ctx=ctx)
    want = blind_oracle(x, 20e6)
    print('blind parameters on noise alone: stat %.3f (oracle %.3f), threshold %.3f' % (got['stat'], want['stat'], got['threshold']))
    assert not got['detected'] and got['nseg'] == BLIND_M
    assert abs(got['stat'] - want['stat']) <= 1e-3 * want['stat']
