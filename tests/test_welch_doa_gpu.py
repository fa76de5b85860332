"""GPU tests of the Bartlett, Capon and MUSIC direction spectra of the spectral matrix of Welch plans (oth_welch_set_steering,
oth_welch_matrix_doa / _dev, csrc/matdoa.hip and the basis build of csrc/mateig.hip) against the float64 oracle
(tests/welch_doa_oracle.py: numpy.linalg.eigh per bin and the header's definitions).  The gates follow from the eigenvalue gate
g of tests/test_welch_eig_gpu.py (gate_of: RTOL trace(S) of S, 2 C RTOL of G - a bound on the 2-norm of the matrix's error E):
  Bartlett   |B - oracle| <= g / C:  |w^H E w| / C^2 <= ||E|| |w|^2 / C^2 = g / C;
  Capon      with loading = 1e-2, relative error <= 2 (1 + loading) g / (l_C + delta): the loaded matrix's smallest eigenvalue is
             l_C + delta, its inverse moves by ||E|| / (l_C + delta) relative to first order, the loading's own trace moves with
             E, and the factor 2 pays for the higher orders while g / (l_C + delta) <= 0.25, which is asserted (the oracle
             keeps it at or below 0.16: g / delta = C RTOL / loading of S, 2 C RTOL / loading of G);
  MUSIC      the null spectrum 1 / P = sum_{i > nsrc} p_i / C absolutely <= 2 g / (l_nsrc - l_nsrc+1) (Davis-Kahan on the noise
             projector) on the bins where the oracle's gap is at least 0.1 l_1, which at least 75 % of a parity case's bins
             must be; nsrc = 1 on test_welch_matrix_gpu's captures, nsrc = 2 on the two-source line-array captures.
The degenerate cases (a silent channel, M < C) meet the same three gates; the share of bins under the gap condition is a
property of the parity captures and is asserted there only.
Measured on an MI355X, worst bin of this file as a fraction of its gate: the 12 parity cases under both matrices Bartlett
0.078, Capon 0.011, MUSIC 0.020 (all three at 16384 points of S), g / (l_C + delta) at most 0.160, at most 3.1 % of a case's
bins outside the gap condition; the degenerate cases 0.029, below 0.001 and 0.014; doa_scan 0.001, below 0.001 and below
0.001 with 0.4 % of the bins outside, its band-combined spectra within 6.4e-8 relative of the oracle's.  All-zero delays:
Bartlett against sum_ab S_ab / C^2 at most 0.081 of C^2 2^-23 trace / C."""
import ctypes as C
import gc

import numpy as np
import pytest

import welch_doa_oracle as DO
import welch_matrix_oracle as XO
from stat_support import FS, welch_plan as make_plan
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_welch_doa_cpu import GRID, RES, check_resolution
from test_welch_eig_gpu import gate_of
from test_welch_matrix_gpu import OPTIONS, capture

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
METHODS = ('bartlett', 'capon', 'music')
LOADING = 1e-2


def table(D, C_, seed):
    """D directions of fractional delays of either sign, a few samples at most"""
    return np.random.default_rng(seed).uniform(-3.0, 3.0, (D, C_))


def check_doa(rows, ref, delays, fc, of, nsrc, loading, fftshift=False, trim=0, what='', min_share=0.75):
    """rows: dict method -> [D, m] of the device against the oracle at the gates of the file header -> the worst readings as
    fractions of their gates (bartlett, capon, music), the worst g / (l_C + delta) and the share of bins outside the gap
    condition"""
    nfft, C_ = ref['T'].shape[2], ref['T'].shape[0]
    want = DO.doa(None, nfft, delays, fc, of=of, nsrc=nsrc, loading=loading, ref=ref)
    st = lambda r: XO.shape_out(r, fftshift, trim)      # noqa: E731
    gate = gate_of(ref, of, fftshift, trim)
    lam, delta = st(want['lam']), st(want['delta'])
    e_b = e_c = e_m = cond = share = 0.0
    for m, r in rows.items():
        assert r.dtype == np.float32 and r.shape == st(want[m]).shape and np.all(np.isfinite(r)) and r.min() >= 0.0, m
    if 'bartlett' in rows:
        e_b = float(np.max(np.abs(rows['bartlett'].astype(np.float64) - st(want['bartlett'])) / (gate / C_)))
    if 'capon' in rows:
        floor = lam[C_ - 1] + delta
        cond = float(np.max(gate / floor))
        assert loading > 0 and cond <= 0.25, (what, cond)
        rel = np.abs(rows['capon'].astype(np.float64) / st(want['capon']) - 1.0)
        e_c = float(np.max(rel / (2.0 * (1.0 + loading) * gate / floor)))
    if 'music' in rows:
        gap = lam[nsrc - 1] - lam[nsrc]
        wide = gap >= 0.1 * lam[0]
        share = float(np.mean(~wide))
        null = np.abs(1.0 / rows['music'].astype(np.float64) - 1.0 / st(want['music']))
        e_m = float(np.max((null * gap / (2.0 * gate))[:, wide])) if wide.any() else 0.0
    if what:
        print('doa parity %s of %s: bartlett %.3f, capon %.3f, music %.3f of their gates; g / (l_C + delta) at most %.3f (gate 0.25), '
              '%.1f %% of the bins outside the gap condition' % (what, of, e_b, e_c, e_m, cond, 100 * share))
    assert e_b <= 1.0 and e_c <= 1.0 and e_m <= 1.0 and share <= 1.0 - min_share, (what, of, e_b, e_c, e_m, share)
    return e_b, e_c, e_m, cond, share


def line_capture(C_, n, nfft, angles, seed, fc, offset=0.0):
    """DO.doa_capture cut to n samples: sources of 10 dB each on a half-wavelength line array"""
    x = DO.doa_capture(C_, nfft, -(-n // nfft), angles, (10,) * len(angles), seed, fc)[:, :n]
    return (x + offset).astype(np.complex64)


# ---- 1. parity with the oracle ---------------------------------------------------------------------------------------------------

PARITY = [  # nfft, C, M, D, option of test_welch_matrix_gpu (nperseg, overlap, detrend, scaling, fftshift, trim, dB, offset), fc, sources
    (64, 2, 6, 1, 0, 0.0, None),
    (64, 3, 11, 7, 1, 1000.25, None),              # nperseg < nfft, fftshift with trim; a carrier of many cycles per sample
    (64, 4, 9, 65, 2, 0.0, None),                  # 50 % overlap, dB on the plan; a direction tile is crossed
    (64, 5, 12, 7, 3, 1000.25, None),
    (64, 8, 10, 65, 4, 2.0, (5, 14)),              # two sources on the line array: nsrc = 2
    (256, 2, 5, 65, 5, 1000.25, None),
    (256, 3, 10, 1, 6, 0.0, None),
    (256, 4, 8, 7, 0, 0.37, None),
    (256, 5, 12, 65, 1, 2.0, (-30, 20)),           # capacity 8 part-filled, nsrc = 2
    (256, 8, 7, 7, 2, 1000.25, None),              # M < C
    (4096, 8, 9, 65, 1, 1000.25, None),
    (16384, 3, 5, 7, 4, 0.0, None),
]


def parity_input(nfft, C_, M, D, option, fc, sources):
    frac, ov, detrend, scaling, fftshift, trim64, db, offset = OPTIONS[option]
    nperseg = nfft * frac // 16
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    n = noverlap + M * step + step // 3
    seed = 7 * nfft + 13 * C_ + M
    if sources:
        x, delays, nsrc = line_capture(C_, n, nfft, sources, seed, fc, offset), DO.ula_delays(C_, np.linspace(-60.0, 60.0, D), fc), 2
    else:
        x, delays, nsrc = capture(C_, n, seed, nfft, M, offset), table(D, C_, seed), 1
    return x, delays, nsrc, (nperseg, noverlap, detrend, scaling, fftshift, trim64 * nfft // 64, db)


@pytest.mark.parametrize('nfft,C_,M,D,option,fc,sources', PARITY)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, C_, M, D, option, fc, sources):
    x, delays, nsrc, (nperseg, noverlap, detrend, scaling, fftshift, trim, db) = parity_input(nfft, C_, M, D, option, fc, sources)
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, db)
    plan.set_steering(delays, fc)
    ref = XO.matrix(x, nfft, nperseg, noverlap, 'hann', detrend, scaling, FS)
    for of in 'SG':
        rows = plan.matrix_doa(x, of=of, nsrc=nsrc, loading=LOADING)
        assert plan.last_nseg == M and set(rows) == set(METHODS)
        recipe = plan.last_recipe()
        assert recipe.startswith('kernel=welchmat nfft=%d W=%d nseg=%d nstreams=1 nchan=%d ' % (nfft, M, M, C_)), recipe
        assert recipe.endswith(' doa=%s ndir=%d' % (of, D)), recipe
        check_doa(rows, ref, delays, fc, of, nsrc, LOADING, fftshift, trim, what=str((nfft, C_, M, D, option, fc, sources)))
        if db:      # always linear: the linear twin's rows, bit for bit
            twin = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, False)
            twin.set_steering(delays, fc)
            other = twin.matrix_doa(x, of=of, nsrc=nsrc, loading=LOADING)
            assert all(other[m].tobytes() == rows[m].tobytes() for m in METHODS)
            twin.close()
    plan.close()


# ---- 2. identities on the device's own rows --------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,C_,M', [(64, 2, 3), (256, 5, 7), (4096, 8, 4)])
def test_zero_delays_sum_the_matrix(ctx, hip, nfft, C_, M):
    x = capture(C_, nfft * M + 5, 3 * nfft + C_, nfft, M)
    plan = make_plan(ctx, hip, nfft, fftshift=True, trim=nfft // 32)
    plan.set_steering(np.zeros((1, C_)), 0.0)
    S = plan.matrix(x, return_gcoh=False).astype(np.complex128)
    bart = plan.matrix_doa(x, of='S', methods='bartlett')['bartlett']
    assert bart.shape == (1, plan.out_len)
    total, trace = S.sum(axis=(0, 1)).real / C_ ** 2, np.einsum('aaj->j', S).real
    err = float(np.max(np.abs(bart[0] - total) / (C_ ** 2 * 2.0 ** -23 * trace / C_)))
    print('zero delays, %d points C = %d: bartlett against sum_ab S_ab / C^2 %.3f of the gate C^2 2^-23 trace / C' % (nfft, C_, err))
    assert err <= 1.0
    plan.close()


@pytest.mark.parametrize('nfft,C_,M,db', [(64, 3, 4, False), (256, 8, 9, True), (4096, 4, 3, False)])
def test_bit_equal_forms(ctx, hip, nfft, C_, M, db):
    n, stride, D, fc, nsrc = nfft * M + 5, nfft * M + 5 + 77, 65, 1000.25, C_ - 1
    x = capture(C_, n, 5 * nfft + C_, nfft, M)
    delays = table(D, C_, nfft + C_)
    plan = make_plan(ctx, hip, nfft, fftshift=True, trim=nfft // 32, db=db)
    twin = make_plan(ctx, hip, nfft, fftshift=True, trim=nfft // 32, db=not db)
    m = plan.out_len
    plan.set_steering(delays, fc)
    twin.set_steering(delays, fc)
    padded = np.full((C_, stride), np.nan + 1j * np.nan, np.complex64)      # what lies between the channels is never read
    padded[:, :n] = x
    dx, dout = ctx.alloc(padded.nbytes), [ctx.alloc(4 * D * m) for _ in METHODS]
    try:
        ctx.h2d(dx, padded)
        for of in 'SG':
            rows = plan.matrix_doa(x, of=of, nsrc=nsrc, loading=LOADING)
            again = plan.matrix_doa(x, of=of, nsrc=nsrc, loading=LOADING)                       # two runs
            other = twin.matrix_doa(x, of=of, nsrc=nsrc, loading=LOADING)                       # dB plan against linear plan
            assert all(again[k].tobytes() == rows[k].tobytes() == other[k].tobytes() for k in METHODS)
            for asked in (METHODS, ('bartlett',), ('capon',), ('music',), ('bartlett', 'music')):
                # each output alone is the output asked with the others (host form) ...
                part = plan.matrix_doa(x, of=of, nsrc=nsrc, loading=LOADING, methods=asked)
                assert set(part) == set(asked) and all(part[k].tobytes() == rows[k].tobytes() for k in asked)
                # ... the _dev form gives the same bits, and a row that is not asked for is left untouched
                for d in dout:
                    ctx.h2d(d, np.full(D * m, -7.0, np.float32))
                assert plan.matrix_doa_dev(dx, n, C_, stride, of, nsrc, LOADING, *[d if k in asked else None for k, d in zip(METHODS, dout)]) == M
                for k, d in zip(METHODS, dout):
                    got = ctx.d2h(d, (D, m), np.float32)
                    assert got.tobytes() == rows[k].tobytes() if k in asked else np.all(got == -7.0), (of, asked, k)
            for d in (0, 31, 32, 64):      # a direction alone and inside the 65-direction table: the same bits
                plan.set_steering(delays[d:d + 1], fc)
                alone = plan.matrix_doa(x, of=of, nsrc=nsrc, loading=LOADING)
                assert all(alone[k].shape == (1, m) and alone[k][0].tobytes() == rows[k][d].tobytes() for k in METHODS), (of, d)
            plan.set_steering(delays, fc)
    finally:
        for d in [dx] + dout:
            ctx.free(d)
    twin.close()
    plan.close()


# ---- 3. degenerate input ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft', [64, 4096])
def test_degenerate_input(ctx, hip, nfft):
    C_, M, D, fc = 3, 5, 7, 0.37
    x = capture(C_, nfft * M, nfft + 1, nfft, M)
    delays = table(D, C_, nfft)
    plan = make_plan(ctx, hip, nfft)
    plan.set_steering(delays, fc)
    clean = {of: plan.matrix_doa(x, of=of, nsrc=1, loading=LOADING) for of in 'SG'}
    for bad in (np.nan, np.inf):
        for of in 'SG':
            y = x.copy()
            y[2, nfft + 17] = bad
            rows = plan.matrix_doa(y, of=of, nsrc=1, loading=LOADING)
            assert all(np.isnan(rows[k]).all() for k in METHODS), (bad, of)
            rows = plan.matrix_doa(x, of=of, nsrc=1, loading=LOADING)      # the next call on clean input: the one before, bit for bit
            assert all(rows[k].tobytes() == clean[of][k].tobytes() for k in METHODS)
    y = x.copy()
    y[1] = 0.0      # a silent channel
    ref = XO.matrix(y, nfft, fs=FS)
    for of in 'SG':
        check_doa(plan.matrix_doa(y, of=of, nsrc=1, loading=LOADING), ref, delays, fc, of, 1, LOADING, what='silent channel, %d points' % nfft,
                  min_share=0.0)
    rows = plan.matrix_doa(y, of='S', nsrc=1, loading=0.0)      # no loading: the matrix is singular in every bin
    assert not rows['capon'].any() and np.all(np.isfinite(rows['bartlett'])) and np.all(rows['bartlett'] > 0) and np.all(rows['music'] > 0)
    plan.close()
    for C2, M2 in ((4, 1), (8, 3)):      # M < C: rank one, singular
        y = capture(C2, nfft * M2, nfft + 7 + C2, nfft, M2)
        delays = table(D, C2, nfft + C2)
        plan = make_plan(ctx, hip, nfft)
        plan.set_steering(delays, fc)
        ref = XO.matrix(y, nfft, fs=FS)
        for of in 'SG':
            rows = plan.matrix_doa(y, of=of, nsrc=1, loading=LOADING)
            assert plan.last_nseg == M2
            check_doa(rows, ref, delays, fc, of, 1, LOADING, what='M = %d < C = %d, %d points' % (M2, C2, nfft), min_share=0.0)
        plan.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------

N5, C5, D5 = 64, 3, 5
WHAT = 'the direction spectra of the spectral matrix'
TEXT_MTM = WHAT + " is not available on a multitaper plan: its segments' transforms are Welch's (oth_welch_plan)"
TEXT_MEDIAN = WHAT + ' is not available with OTH_AVERAGE_MEDIAN: its rows are means over segments (oth_plan_set_average(OTH_AVERAGE_MEAN) first)'
TEXT_SIZE = WHAT + ' takes a transform length that is a power of two from 64 to 16384, not 32'
TEXT_NCHAN = 'nchan must lie in 2 ... 8'
TEXT_OF = 'of must be OTH_EIG_OF_S or OTH_EIG_OF_G'
TEXT_INPUT = 'the input is NULL'
TEXT_ROWS = 'bartlett_out, capon_out and music_out are all NULL'
TEXT_TABLE = 'the direction spectra need a steering table: call oth_welch_set_steering on this plan'
TEXT_DIFFER = 'nchan is 4 and the steering table holds 3 channels'
TEXT_NSRC = 'nsrc must lie in 1 ... nchan - 1 for the MUSIC spectrum'
TEXT_LOADING = 'loading must be finite and >= 0'
TEXT_STRIDE = 'chan_stride < nsamples'
TEXT_SHORT = 'input shorter than nperseg'


def test_refusals_in_order_leave_the_plan_usable(ctx, hip):
    n = 4 * N5
    x = capture(4, n, 9, N5, 4)      # four channels in memory: the plan's table holds three
    delays = table(D5, C5, 1)
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * 3 * D5 * N5)
    host = [np.empty(D5 * N5, np.float32) for _ in METHODS]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    welch = make_plan(ctx, hip, N5)
    welch.set_steering(delays, 0.25)
    bare = make_plan(ctx, hip, N5)      # no table
    mtm = ctx.mtm_plan(N5, nw=2.0, ntapers=3)
    med = make_plan(ctx, hip, N5)
    med.set_steering(delays, 0.25)
    med.set_average('median')
    small = make_plan(ctx, hip, 32)
    want = welch.matrix_doa(x[:C5], of='S', nsrc=1, loading=LOADING)

    def call(dev, plan, nchan=C5, of=0, src=True, rows=(True, True, True), nsrc=1, loading=LOADING, nsamples=n, stride=n):
        nseg = C.c_uint64()
        before = hip.live_resources()
        if dev:
            rc = ctx.lib.oth_welch_matrix_doa_dev(plan.h, C.c_void_p(d) if src else None, nsamples, nchan, stride, of, nsrc, loading,
                                                  *[C.c_void_p(out + 4 * D5 * N5 * k) if on else None for k, on in enumerate(rows)],
                                                  C.byref(nseg))
        else:
            rc = ctx.lib.oth_welch_matrix_doa(plan.h, x.ctypes.data_as(C.c_void_p) if src else None, nsamples, nchan, 0, of, nsrc, loading,
                                              *[fp(h) if on else None for h, on in zip(host, rows)], C.byref(nseg))
        return rc, ctx.lib.oth_last_error(ctx.h).decode(), hip.live_resources() == before

    none, no_music = (False, False, False), (True, True, False)
    table_ = [  # the header's eleven in order, then two at once: which goes first
        (dict(plan=mtm), UNSUPPORTED, TEXT_MTM), (dict(plan=med), UNSUPPORTED, TEXT_MEDIAN), (dict(plan=small), UNSUPPORTED, TEXT_SIZE),
        (dict(nchan=1), INVALID, TEXT_NCHAN), (dict(nchan=9), INVALID, TEXT_NCHAN),
        (dict(of=2), INVALID, TEXT_OF), (dict(of=-1), INVALID, TEXT_OF),
        (dict(src=False), INVALID, TEXT_INPUT),
        (dict(rows=none), INVALID, TEXT_ROWS),
        (dict(plan=bare), UNSUPPORTED, TEXT_TABLE),
        (dict(nchan=4), INVALID, TEXT_DIFFER),
        (dict(nsrc=0), INVALID, TEXT_NSRC), (dict(nsrc=C5), INVALID, TEXT_NSRC),
        (dict(loading=-1e-3), INVALID, TEXT_LOADING), (dict(loading=float('nan')), INVALID, TEXT_LOADING),
        (dict(loading=float('inf')), INVALID, TEXT_LOADING),
        (dict(stride=n - 1), INVALID, TEXT_STRIDE),
        (dict(nsamples=N5 - 1, stride=N5 - 1), INVALID, TEXT_SHORT),
        (dict(plan=mtm, nchan=9), UNSUPPORTED, TEXT_MTM),
        (dict(nchan=9, of=2), INVALID, TEXT_NCHAN), (dict(of=2, src=False), INVALID, TEXT_OF),
        (dict(src=False, rows=none), INVALID, TEXT_INPUT), (dict(rows=none, plan=bare), INVALID, TEXT_ROWS),
        (dict(plan=bare, nchan=4), UNSUPPORTED, TEXT_TABLE), (dict(nchan=4, nsrc=0), INVALID, TEXT_DIFFER),
        (dict(nsrc=0, loading=-1.0), INVALID, TEXT_NSRC), (dict(loading=-1.0, nsamples=N5 - 1, stride=N5 - 1), INVALID, TEXT_LOADING),
    ]
    try:
        ctx.h2d(d, x)
        ctx.sync()
        gc.collect()      # once: nothing a call below makes owns a device resource, so no later collection moves the count
        for dev in (False, True):
            for kw, code, text in table_:
                if not dev and 'stride' in kw and 'nsamples' not in kw:
                    continue      # the host form has no stride of its own
                kw = dict(kw)
                plan = kw.pop('plan', welch)
                rc, said, untouched = call(dev, plan, **kw)
                print('dev' if dev else 'host', kw, rc, repr(said))
                assert (rc, said) == (code, text)
                assert untouched      # refused before anything is allocated or staged
                got = welch.matrix_doa(x[:C5], of='S', nsrc=1, loading=LOADING)      # ... and the plan goes on working
                assert all(got[k].tobytes() == want[k].tobytes() for k in METHODS)
            # nsrc is read with music_out only
            rc, said, _ = call(dev, welch, nsrc=0, rows=no_music)
            assert rc == 0, said
        assert mtm.exec(x[0]).shape == (N5,) and med.exec(x[0]).shape == (N5,) and small.exec(x[0]).shape == (32,)
        with pytest.raises(ValueError):
            welch.matrix_doa(x[0], nsrc=1)
        with pytest.raises(ValueError):
            welch.matrix_doa(x[:C5])      # music without nsrc
        with pytest.raises(ValueError):
            welch.matrix_doa(x[:C5], methods=('esprit',))
        with pytest.raises(KeyError):
            welch.matrix_doa(x[:C5], of='T', nsrc=1)
        # the table's own refusals, and clearing it
        for args, text in (((0, C5, None), None), ((1025, C5, delays), 'ndir must lie in 0 ... 1024'), ((D5, 9, delays), TEXT_NCHAN),
                           ((D5, C5, None), 'delays is NULL')):
            ptr = None if args[2] is None else args[2].ctypes.data_as(C.POINTER(C.c_double))
            rc = ctx.lib.oth_welch_set_steering(bare.h, args[0], args[1], ptr, 0.25)
            assert (rc, ctx.lib.oth_last_error(ctx.h).decode()) == (INVALID, text) if text else rc == 0
        rc = ctx.lib.oth_welch_set_steering(bare.h, D5, C5, delays.ctypes.data_as(C.POINTER(C.c_double)), float('nan'))
        assert (rc, ctx.lib.oth_last_error(ctx.h).decode()) == (INVALID, 'fc must be finite')
        assert ctx.lib.oth_welch_set_steering(mtm.h, D5, C5, delays.ctypes.data_as(C.POINTER(C.c_double)), 0.25) == UNSUPPORTED
        welch.set_steering(np.zeros((0, C5)), 0.0)      # cleared: refused again, and set again: the rows of before
        rc, said, untouched = call(False, welch)
        assert (rc, said, untouched) == (UNSUPPORTED, TEXT_TABLE, True)
        welch.set_steering(delays, 0.25)
        got = welch.matrix_doa(x[:C5], of='S', nsrc=1, loading=LOADING)
        assert all(got[k].tobytes() == want[k].tobytes() for k in METHODS)
        check_doa(want, XO.matrix(x[:C5], N5, fs=FS), delays, 0.25, 'S', 1, LOADING)
    finally:
        ctx.free(d)
        ctx.free(out)
        for p in (welch, bare, mtm, med, small):
            p.close()


# ---- 5. doa_scan ---------------------------------------------------------------------------------------------------------------

def test_doa_scan_resolves_two_sources(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    x = DO.doa_capture(RES['C'], RES['nfft'], RES['M'], RES['angles'], RES['snr'], 0, fc=RES['fc'])
    delays = T.ula_delays(RES['C'], GRID, 0.5, RES['fc'])
    axis, bartlett, capon, music, combined = T.doa_scan(x, RES['nfft'], 20e6, delays, RES['fc'], RES['nsrc'], loading=RES['loading'], ctx=ctx)
    m = RES['nfft']
    assert axis.shape == (m,) and bartlett.shape == capon.shape == music.shape == (len(GRID), m)
    assert np.isclose(axis[m // 2], RES['fc'] * 20e6, rtol=1e-12) and set(combined) == set(METHODS)
    check_resolution(combined, 'doa_scan')
    ref = XO.matrix(x, m, detrend=True, fs=20e6)
    check_doa({'bartlett': bartlett, 'capon': capon, 'music': music}, ref, delays, RES['fc'], 'S', RES['nsrc'], RES['loading'], fftshift=True,
              what='doa_scan')
    want = DO.combine(DO.doa(None, m, delays, RES['fc'], nsrc=RES['nsrc'], loading=RES['loading'], ref=ref))
    worst = max(float(np.max(np.abs(combined[k] / want[k] - 1.0))) for k in METHODS)
    print('doa_scan, band-combined spectra against the oracle: %.2e relative' % worst)
    half = T.doa_scan(x, m, 20e6, delays, RES['fc'], RES['nsrc'], loading=RES['loading'], band=(m // 4, 3 * m // 4), ctx=ctx)[4]
    assert all(np.array_equal(half[k], T.doa_band_combine({k: r}, (m // 4, 3 * m // 4))[k]) for k, r in zip(METHODS, (bartlett, capon, music)))
    eig = T.eigen_scan(x, m, 20e6, ctx=ctx)[1]      # the same cached plan serves the sibling helpers
    assert eig.shape == (RES['C'], m)
