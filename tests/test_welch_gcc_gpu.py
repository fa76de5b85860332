"""GPU tests of the generalized cross-correlation of the spectral matrix's pairs on Welch plans (oth_welch_matrix_gcc / _dev,
csrc/matgcc.hip) against the float64 oracle (tests/welch_gcc_oracle.py: the header's definitions on welch_matrix_oracle's sums,
numpy.fft.ifft, the same parabola on |R|).  The gates follow from the matrix family's contract |dT_ab| <= RTOL sqrt(T_aa T_bb)
with RTOL of tests/test_hip_parity.py, and from no measured number (welch_gcc_oracle.gates, delay_gate):
  R, absolute      g = 3 RTOL (plain), 2 RTOL (SCOT), mean over the in-band bins of min(2, 2 RTOL / |G_ab|) (PHAT), each plus the
                   float32 transform's worst case 16 2^-24 log2(NI) sum_k w_k / Z;
  |R| at the peak  g;   arg R at the peak  asin(g / |R|);
  the delay        3 g / (|den| - 4 g) / U samples (plus the float32 rounding of the stored delay), den the oracle's parabola
                   denominator - under the conditions that the oracle's top leads every other lag of the window by more than
                   2 g, so that the device picks the same lag, and that |den| > 8 g unless that lag is a window edge.  The
                   conditions are properties of the inputs: tests/test_welch_gcc_cpu.py shows on the oracle alone that every
                   pair of every parity case meets them, and they are asserted again here for every pair - none is left out.
Measured on an MI355X, worst reading of this file as a fraction of its gate: the 12 parity cases under the three weightings
R 0.0004, |R| at the peak 0.0004, arg R 0.0001, the delay 0.0003 (the same lag as the oracle in every pair); two identical
channels R 0.0004, below 0.0001 elsewhere; tdoa_scan 0.0003, 0.0001, 0.0001 and 0.0001, its pair delays within 0.0070 sample of
3.3 / -7.6 / -10.9 and channel_delays within 0.0076 of 0 / 3.3 / -7.6; the upsample identity reads exactly 0 of its gate 2 f at
64 and 1024 points (the interpolating transform's extra passes only add zeros to the same butterflies)."""
import ctypes as C
import gc

import numpy as np
import pytest

import welch_gcc_oracle as GO
import welch_matrix_oracle as XO
from stat_support import FS, welch_plan as make_plan
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_welch_gcc_cpu import RTOL as CPU_RTOL, TRUE

pytestmark = pytest.mark.gpu

assert RTOL == CPU_RTOL
UNSUPPORTED, INVALID = -3, -1
CODES = {'plain': 0, 'phat': 1, 'scot': 2}


def run(ctx, plan, x, weighting, band=None, U=1, maxlag=None, rows=True, peak=True):
    """the host form through the C ABI with either output left out -> (rows complex64 [P, 2 L + 1] or None, peak float32
    [P, 3] or None, nseg)"""
    x = np.ascontiguousarray(x, np.complex64)
    nchan, n = x.shape
    lo, hi = (-(plan.nfft // 2), plan.nfft // 2 - 1) if band is None else band
    L = U * plan.nfft // 2 - 1 if maxlag is None else maxlag
    P = nchan * (nchan - 1) // 2
    r = np.full((P, 2 * L + 1), -7.0, np.complex64) if rows else None
    pk = np.full((P, 3), -7.0, np.float32) if peak else None
    nseg = C.c_uint64()
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    rc = ctx.lib.oth_welch_matrix_gcc(plan.h, x.ctypes.data_as(C.c_void_p), n, nchan, 0, CODES[weighting], lo, hi, U, L, fp(r), fp(pk),
                                      C.byref(nseg))
    assert rc == 0, ctx.lib.oth_last_error(ctx.h).decode()
    return r, pk, nseg.value


def check_gcc(rows, peak, want, weighting, NI, U, what=''):
    """the device's rows and peaks against the oracle at the gates of the file header, every pair under the gate's conditions
    -> the worst readings as fractions of their gates (R, |R| at the peak, arg R, delay; the delay's fraction counts the
    pairs with a gate above 0: at a window edge both sides store the same lag exactly)"""
    g = GO.gates(want, weighting, NI, RTOL)
    dgate, ok = GO.delay_gate(want, g, U)
    assert ok.all(), (what, weighting, ok)      # every pair: the inputs are chosen so
    e_r = e_p = e_a = e_d = 0.0
    if rows is not None:
        assert rows.dtype == np.complex64 and rows.shape == want['R'].shape and np.all(np.isfinite(rows.view(np.float32)))
        e_r = float(np.max(np.abs(rows.astype(np.complex128) - want['R']) / g[:, None]))
    if peak is not None:
        assert peak.dtype == np.float32 and peak.shape == want['peak'].shape and np.all(np.isfinite(peak))
        pk = peak.astype(np.float64)
        top = want['peak'][:, 1]
        e_p = float(np.max(np.abs(pk[:, 1] - top) / g))
        turn = np.abs(np.angle(np.exp(1j * (pk[:, 2] - want['peak'][:, 2]))))
        e_a = float(np.max(turn / np.arcsin(np.minimum(1.0, g / top))))
        off = np.abs(pk[:, 0] - want['peak'][:, 0])
        room = dgate + 2.0 ** -23 * np.abs(want['peak'][:, 0])
        assert np.all(off[room == 0.0] == 0.0), (what, weighting)
        e_d = float(np.max(off[room > 0] / room[room > 0])) if (room > 0).any() else 0.0
    if what:
        print('gcc parity %s %s: R %.4f, peak %.4f, phase %.4f, delay %.4f of their gates (g at most %.1e, delay gate at most %.4f sample)'
              % (what, weighting, e_r, e_p, e_a, e_d, g.max(), dgate.max()))
    assert e_r <= 1.0 and e_p <= 1.0 and e_a <= 1.0 and e_d <= 1.0, (what, weighting, e_r, e_p, e_a, e_d)
    return e_r, e_p, e_a, e_d


# ---- 1. parity with the oracle ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', GO.PARITY)
def test_parity_with_the_float64_oracle(ctx, hip, case):
    nfft, U, C_, M, option, narrow, maxlag = case
    x, (nperseg, noverlap, detrend, scaling, fftshift, trim, db), band = GO.parity_input(*case)
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, db)
    twin = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling) if (fftshift or trim or db) else None
    ref = XO.matrix(x, nfft, nperseg, noverlap, 'hann', detrend, scaling, FS)
    NI = U * nfft
    L = NI // 2 - 1 if maxlag is None else maxlag
    lo, hi = (-(nfft // 2), nfft // 2 - 1) if band is None else band
    for w in GO.WEIGHTINGS:
        rows, peak, nseg = run(ctx, plan, x, w, band, U, maxlag)
        assert nseg == M
        recipe = plan.last_recipe()
        assert recipe.startswith('kernel=welchmat nfft=%d W=%d nseg=%d nstreams=1 nchan=%d ' % (nfft, M, M, C_)), recipe
        assert recipe.endswith(' gcc=%s ni=%d band=%d:%d maxlag=%d' % (w, NI, lo, hi, L)), recipe
        check_gcc(rows, peak, GO.gcc(ref['T'], w, band, U, maxlag), w, NI, U, what=str(case))
        # each output alone is the output asked with the other, byte for byte
        assert run(ctx, plan, x, w, band, U, maxlag, peak=False)[0].tobytes() == rows.tobytes()
        assert run(ctx, plan, x, w, band, U, maxlag, rows=False)[1].tobytes() == peak.tobytes()
        # the Python method unpacks the same numbers
        delays, peaks, phases, again = plan.matrix_gcc(x, weighting=w, band=band, upsample=U, maxlag=maxlag)
        assert again.tobytes() == rows.tobytes() and delays.shape == peaks.shape == phases.shape == (C_, C_)
        for p, (a, b) in enumerate(GO.pairs(C_)):
            assert (delays[a, b], peaks[a, b], phases[a, b]) == tuple(peak[p]) and (delays[b, a], peaks[b, a], phases[b, a]) == (-peak[p, 0], peak[p, 1], -peak[p, 2])
        if twin is not None:      # the plan's fftshift, trim and dB take no part: not a byte moves
            other = run(ctx, twin, x, w, band, U, maxlag)
            assert other[0].tobytes() == rows.tobytes() and other[1].tobytes() == peak.tobytes()
    if twin is not None:
        twin.close()
    plan.close()


# ---- 2. identities on the device's own rows --------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,C_,M', [(64, 3, 5), (1024, 2, 3)])
def test_upsample_identity_on_the_device(ctx, hip, nfft, C_, M):
    """R_U[U l] = R_1[l]: both rows are within the float32 transform's term f of the same float64 sum of the same float32
    phasors, so they differ by at most 2 f (f at the longer transform)"""
    x = GO.delayed_capture(GO.channel_delays(C_, 1), nfft * M, nfft + C_)
    plan = make_plan(ctx, hip, nfft)
    ref = XO.matrix(x, nfft, fs=FS)
    worst = 0.0
    for w in GO.WEIGHTINGS:
        one = run(ctx, plan, x, w)[0].astype(np.complex128)
        for U in (2, 4, 8):
            up = run(ctx, plan, x, w, U=U, maxlag=U * (nfft // 2 - 1))[0].astype(np.complex128)
            f = 16.0 * 2.0 ** -24 * np.log2(U * nfft) * GO.gcc(ref['T'], w)['wsum']
            worst = max(worst, float(np.max(np.abs(up[:, ::U] - one) / (2.0 * f[:, None]))))
    print('upsample identity on the device, %d points: at most %.2e of 2 f' % (nfft, worst))
    assert worst <= 1.0
    plan.close()


@pytest.mark.parametrize('nfft,C_,M,U', [(64, 3, 4, 2), (4096, 5, 3, 4)])
def test_bit_equal_forms(ctx, hip, nfft, C_, M, U):
    """two runs, and the _dev form on channels chan_stride > nsamples apart: the same bytes; a row that is not asked for is
    left untouched"""
    n, stride, L = nfft * M + 5, nfft * M + 5 + 77, 3 * U
    x = GO.delayed_capture(GO.channel_delays(C_, U), n, 5 * nfft + C_)
    plan = make_plan(ctx, hip, nfft, fftshift=True, trim=nfft // 32)
    P = C_ * (C_ - 1) // 2
    padded = np.full((C_, stride), np.nan + 1j * np.nan, np.complex64)      # what lies between the channels is never read
    padded[:, :n] = x
    dx, drows, dpeak = ctx.alloc(padded.nbytes), ctx.alloc(8 * P * (2 * L + 1)), ctx.alloc(4 * 3 * P)
    try:
        ctx.h2d(dx, padded)
        for w in GO.WEIGHTINGS:
            rows, peak, _ = run(ctx, plan, x, w, (-nfft // 4, nfft // 8), U, L)
            again = run(ctx, plan, x, w, (-nfft // 4, nfft // 8), U, L)
            assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == peak.tobytes()
            for asked in ((True, True), (True, False), (False, True)):
                ctx.h2d(drows, np.full(2 * P * (2 * L + 1), -7.0, np.float32))
                ctx.h2d(dpeak, np.full(3 * P, -7.0, np.float32))
                assert plan.matrix_gcc_dev(dx, n, C_, stride, w, (-nfft // 4, nfft // 8), U, L, drows if asked[0] else None,
                                           dpeak if asked[1] else None) == M
                got_r, got_p = ctx.d2h(drows, (P, 2 * L + 1), np.complex64), ctx.d2h(dpeak, (P, 3), np.float32)
                assert got_r.tobytes() == rows.tobytes() if asked[0] else np.all(got_r.view(np.float32) == -7.0), (w, asked)
                assert got_p.tobytes() == peak.tobytes() if asked[1] else np.all(got_p == -7.0), (w, asked)
    finally:
        for d in (dx, drows, dpeak):
            ctx.free(d)
    plan.close()


# ---- 3. degenerate input ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,U', [(64, 4), (4096, 1)])
def test_degenerate_input(ctx, hip, nfft, U):
    C_, M, NI = 4, 5, U * nfft
    x = GO.delayed_capture(GO.channel_delays(C_, U), nfft * M, nfft + 1)
    plan = make_plan(ctx, hip, nfft)
    for w in GO.WEIGHTINGS:
        clean = run(ctx, plan, x, w, U=U)
        for fill in (0.0, 3.0 - 1.0j):      # a silent channel, a constant under detrend: zeros in its pairs, the others as they were
            y = x.copy()
            y[1] = fill
            rows, peak, _ = run(ctx, plan, y, w, U=U)
            for p, (a, b) in enumerate(GO.pairs(C_)):
                if 1 in (a, b):
                    assert not rows[p].any() and not peak[p].any(), (w, fill, p)
                else:
                    assert rows[p].tobytes() == clean[0][p].tobytes() and peak[p].tobytes() == clean[1][p].tobytes(), (w, fill, p)
        y = x.copy()
        y[2, nfft + 17] = np.nan      # a NaN sample: NaN in its channel's pairs, never inf; the others byte for byte
        rows, peak, _ = run(ctx, plan, y, w, U=U)
        for p, (a, b) in enumerate(GO.pairs(C_)):
            if 2 in (a, b):
                assert np.isnan(rows[p].view(np.float32)).all() and np.isnan(peak[p]).all(), (w, p)
            else:
                assert rows[p].tobytes() == clean[0][p].tobytes() and peak[p].tobytes() == clean[1][p].tobytes(), (w, p)
        again = run(ctx, plan, x, w, U=U)      # the next call on clean input: the one before, bit for bit
        assert again[0].tobytes() == clean[0].tobytes() and again[1].tobytes() == clean[1].tobytes()
        # two identical channels: lag 0, |R| = 1 and phase 0 within the gates (PHAT and SCOT; plain too: the coefficient is 1)
        twins = np.stack([x[0], x[0]])
        rows, peak, _ = run(ctx, plan, twins, w, U=U)
        want = GO.gcc(XO.matrix(twins, nfft, fs=FS)['T'], w, upsample=U)
        assert want['lag'][0] == 0 and abs(want['peak'][0, 1] - 1.0) <= 1e-12 and abs(want['peak'][0, 2]) <= 1e-12
        check_gcc(rows, peak, want, w, NI, U, what='identical channels, %d points U = %d' % (nfft, U))
        g = GO.gates(want, w, NI, RTOL)[0]
        assert abs(peak[0, 1] - 1.0) <= g and abs(peak[0, 2]) <= np.arcsin(g) and abs(peak[0, 0]) <= GO.delay_gate(want, np.array([g]), U)[0][0]
    one = GO.delayed_capture(GO.channel_delays(3, U), nfft, nfft + 3)      # M = 1
    for w in GO.WEIGHTINGS:
        rows, peak, nseg = run(ctx, plan, one, w, U=U, maxlag=NI // 4)
        assert nseg == 1 and np.all(np.isfinite(rows.view(np.float32))) and np.all(np.isfinite(peak))
        want = GO.gcc(XO.matrix(one, nfft, fs=FS)['T'], w, None, U, NI // 4)
        assert np.max(np.abs(rows.astype(np.complex128) - want['R']) / GO.gates(want, w, NI, RTOL)[:, None]) <= 1.0
    plan.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------

N5, C5, BIG = 64, 3, 4096
WHAT = 'the generalized cross-correlation of the spectral matrix'
TEXT_MTM = WHAT + " is not available on a multitaper plan: its segments' transforms are Welch's (oth_welch_plan)"
TEXT_MEDIAN = WHAT + ' is not available with OTH_AVERAGE_MEDIAN: its rows are means over segments (oth_plan_set_average(OTH_AVERAGE_MEAN) first)'
TEXT_SIZE = WHAT + ' takes a transform length that is a power of two from 64 to 16384, not 32'
TEXT_NCHAN = 'nchan must lie in 2 ... 8'
TEXT_INPUT = 'the input is NULL'
TEXT_STRIDE = 'chan_stride < nsamples'
TEXT_SHORT = 'input shorter than nperseg'
TEXT_WEIGHTING = 'weighting must be OTH_GCC_PLAIN, OTH_GCC_PHAT or OTH_GCC_SCOT'
TEXT_BAND = 'band_lo <= band_hi must lie in -nfft / 2 ... nfft / 2 - 1 = -32 ... 31'
TEXT_UPSAMPLE = 'upsample must be 1, 2, 4 or 8'
TEXT_POINTS = 'upsample times the transform length is 32768: the interpolated transform takes 16384 points at most'
TEXT_MAXLAG = 'maxlag must lie in 0 ... upsample nfft / 2 - 1 = 63'
TEXT_ROWS = 'gcc_out and peak_out are both NULL'


def test_refusals_in_order_leave_the_plan_usable(ctx, hip):
    n, L = 4 * N5, 9
    x = GO.delayed_capture(GO.channel_delays(C5, 2), BIG, 9)      # the 64-point plans read its first C5 n samples as C5 channels
    P = C5 * (C5 - 1) // 2
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * (2 * P * 127 + 3 * P))
    host = [np.empty(2 * P * 127, np.float32), np.empty(3 * P, np.float32)]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    welch = make_plan(ctx, hip, N5)
    big = make_plan(ctx, hip, BIG)
    mtm = ctx.mtm_plan(N5, nw=2.0, ntapers=3)
    med = make_plan(ctx, hip, N5)
    med.set_average('median')
    small = make_plan(ctx, hip, 32)

    def call(dev, plan=welch, nchan=C5, src=True, rows=(True, True), weighting=1, lo=-20, hi=11, U=2, maxlag=L, nsamples=n, stride=n):
        nseg = C.c_uint64()
        before = hip.live_resources()
        if dev:
            rc = ctx.lib.oth_welch_matrix_gcc_dev(plan.h, C.c_void_p(d) if src else None, nsamples, nchan, stride, weighting, lo, hi, U, maxlag,
                                                  C.c_void_p(out) if rows[0] else None, C.c_void_p(out + 8 * P * 127) if rows[1] else None,
                                                  C.byref(nseg))
        else:
            rc = ctx.lib.oth_welch_matrix_gcc(plan.h, x.ctypes.data_as(C.c_void_p) if src else None, nsamples, nchan, 0, weighting, lo, hi, U,
                                              maxlag, fp(host[0]) if rows[0] else None, fp(host[1]) if rows[1] else None, C.byref(nseg))
        return rc, ctx.lib.oth_last_error(ctx.h).decode(), hip.live_resources() == before

    def working():
        rc, said, _ = call(False)
        assert rc == 0, said
        return host[0][:2 * P * (2 * L + 1)].tobytes() + host[1].tobytes()

    none = (False, False)
    table_ = [  # the header's order, then two at once: which goes first
        (dict(plan=mtm), UNSUPPORTED, TEXT_MTM), (dict(plan=med), UNSUPPORTED, TEXT_MEDIAN), (dict(plan=small), UNSUPPORTED, TEXT_SIZE),
        (dict(nchan=1), INVALID, TEXT_NCHAN), (dict(nchan=9), INVALID, TEXT_NCHAN),
        (dict(src=False), INVALID, TEXT_INPUT),
        (dict(stride=n - 1), INVALID, TEXT_STRIDE),
        (dict(nsamples=N5 - 1, stride=N5 - 1), INVALID, TEXT_SHORT),
        (dict(weighting=3), INVALID, TEXT_WEIGHTING), (dict(weighting=-1), INVALID, TEXT_WEIGHTING),
        (dict(lo=-33), INVALID, TEXT_BAND), (dict(hi=32), INVALID, TEXT_BAND), (dict(lo=5, hi=4), INVALID, TEXT_BAND),
        (dict(U=0), INVALID, TEXT_UPSAMPLE), (dict(U=3), INVALID, TEXT_UPSAMPLE), (dict(U=16), INVALID, TEXT_UPSAMPLE),
        (dict(plan=big, U=8, nchan=2, nsamples=BIG, stride=BIG), UNSUPPORTED, TEXT_POINTS),
        (dict(maxlag=-1), INVALID, TEXT_MAXLAG), (dict(maxlag=64), INVALID, TEXT_MAXLAG),
        (dict(rows=none), INVALID, TEXT_ROWS),
        (dict(plan=mtm, nchan=9), UNSUPPORTED, TEXT_MTM), (dict(nchan=9, src=False), INVALID, TEXT_NCHAN),
        (dict(src=False, nsamples=N5 - 1, stride=N5 - 1), INVALID, TEXT_INPUT),
        (dict(nsamples=N5 - 1, stride=N5 - 1, weighting=3), INVALID, TEXT_SHORT), (dict(weighting=3, lo=-33), INVALID, TEXT_WEIGHTING),
        (dict(lo=-33, U=3), INVALID, TEXT_BAND), (dict(U=3, maxlag=-1), INVALID, TEXT_UPSAMPLE),
        (dict(plan=big, U=8, nchan=2, nsamples=BIG, stride=BIG, maxlag=-1), UNSUPPORTED, TEXT_POINTS),
        (dict(maxlag=64, rows=none), INVALID, TEXT_MAXLAG),
    ]
    try:
        ctx.h2d(d, x)
        ctx.sync()
        want = working()
        gc.collect()      # once: nothing a call below makes owns a device resource, so no later collection moves the count
        for dev in (False, True):
            for kw, code, text in table_:
                if not dev and 'stride' in kw and 'nsamples' not in kw:
                    continue      # the host form has no stride of its own
                rc, said, untouched = call(dev, **kw)
                print('dev' if dev else 'host', {k: v for k, v in kw.items() if k != 'plan'}, rc, repr(said))
                assert (rc, said) == (code, text)
                assert untouched      # refused before anything is allocated or staged
                assert working() == want      # ... and the plan goes on working
            rc, said, _ = call(dev, maxlag=63, lo=-32, hi=31)      # the limits themselves pass
            assert rc == 0, said
        assert mtm.exec(x[0]).shape == (N5,) and med.exec(x[0]).shape == (N5,) and small.exec(x[0]).shape == (32,)
        assert big.matrix_gcc(x[:2], upsample=4, maxlag=5)[3].shape == (1, 11)
        with pytest.raises(ValueError):
            welch.matrix_gcc(x[0])
        with pytest.raises(KeyError):
            welch.matrix_gcc(x[:C5, :n], weighting='ml')
    finally:
        ctx.free(d)
        ctx.free(out)
        for p in (welch, big, mtm, med, small):
            p.close()


# ---- 5. tdoa_scan ---------------------------------------------------------------------------------------------------------------

def test_tdoa_scan_recovers_the_delays(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    nfft, M, Sf, U = 256, 40, 20e6, 8
    x = GO.delayed_capture(TRUE, nfft * M, 3, snr_db=10.0)      # the CPU suite's capture: the oracle is within 0.02 sample
    delays, peaks, phases, axis, rows = T.tdoa_scan(x, nfft, Sf, upsample=U, ctx=ctx)
    L = U * nfft // 2 - 1
    assert delays.shape == peaks.shape == phases.shape == (3, 3) and rows.shape == (3, 2 * L + 1) and axis.shape == (2 * L + 1,)
    assert axis[L] == 0.0 and np.isclose(axis[-1], L / (U * Sf), rtol=1e-12)
    want = GO.gcc(XO.matrix(x, nfft, fs=Sf)['T'], 'phat', upsample=U)
    peak = np.array([(delays[a, b] * Sf, peaks[a, b], phases[a, b]) for a, b in GO.pairs(3)], np.float32)
    check_gcc(rows, peak, want, 'phat', U * nfft, U, what='tdoa_scan')
    true = np.array([TRUE[b] - TRUE[a] for a, b in GO.pairs(3)])
    off = np.abs(peak[:, 0] - true).max()
    tau = T.channel_delays(delays, peaks) * Sf
    print('tdoa_scan: pair delays within %.4f sample of 3.3 / -7.6 / -10.9, channel delays within %.4f of 0 / 3.3 / -7.6' % (off, np.abs(tau - TRUE).max()))
    assert off <= 0.02 and np.abs(tau - TRUE).max() <= 0.02
    assert np.array_equal(delays, -delays.T) and np.array_equal(peaks, peaks.T) and np.array_equal(phases, -phases.T)
    band = T.tdoa_scan(x, nfft, Sf, weighting='scot', band=(-5e6, 5e6), upsample=4, maxlag=1e-6, ctx=ctx)
    assert band[4].shape == (3, 161) and np.abs(band[0][0, 1] * Sf - 3.3) <= 0.05
    assert T.multiantenna_scan(x, nfft, Sf, ctx=ctx)[2].shape == (nfft,)      # the same cached plan serves the sibling helpers
