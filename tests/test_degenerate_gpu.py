"""GPU tests of the one-channel Welch average (oth_welch_exec*, accumulate / finalize, partial_dev / scale_dev, segments) and
of the periodogram chain (oth_chain_*: raw rows, IIR + log rows, peak hold) on non-finite and extreme input, on every route
of tests/degenerate_cases.py - the contract stated beside oth_welch_exec and the chain block in include/ofdm_tools_hip.h.
What the inputs and the float64 references are is pinned without a GPU in tests/test_degenerate_cpu.py.

  a. one NaN / +inf / -inf sample (either part, middle of the stream and sample 0, every detrend mode): NaN in every bin,
     linear and dB; the Pxx of csd() and exec() agree in their NaN pattern;
  b. three streams in one launch, the bad sample in the middle one: the outer two bit-identical to a clean launch under the
     static schedules, within RTOL of the oracle under all three;
  c. a plan after a poisoned launch: exec, accumulate / reset / finalize bit-identical to a fresh plan's; a bad sample in the
     second of four ragged chunks: finalize all NaN;
  d. per-segment rows: exactly the rows that hold the sample are non-finite, the others bit-identical;
  e. silence: exact zeros (-inf in dB); a constant: exact zeros under CONSTANT, below (4 ulp)^2 of the undetrended line under
     CONSTANT_FAST, the line itself under NONE;
  f. gains of 2^+-20: out(x 2^k) = out(x) 4^k bit for bit;
  g. a gain under which float32 |X|^2 overflows in a few bins: those read NaN, never inf, the rest stay right;
  h. the chain: the bad vector's row non-finite, every other raw row bit-identical, IIR / dB rows / peak non-finite from that
     vector on and across pushes until reset(); a bad sample in a vector keep_one_in_n drops changes nothing.

The NONE case of (e) does not call check_single_rows on the whole row, as the issue words it: the oracle of a constant is a
line - exactly 0 (rectangular) or 1e-30 of the peak (Hann) outside bins 0, +-1, and sidelobes down to 1e-13 of it on a
zero-padded plan - where "1e-4 of the bin" and a mean relative error are quotients by zero that no float32 transform meets.
Every bin takes the function's first criterion (amplitude within 4 ulp of the row's peak amplitude), and the bins whose
amplitude is at least 1 % of the peak - where that criterion implies 1e-4 of the power - take check_single_rows whole.

Worst readings on an MI355X:
  b. clean and outer streams against the oracle 1.6e-5 (32768 points, one workgroup per segment); bit-identical under both
     static schedules on every route;
  e. silence and a constant under CONSTANT: exact zeros on every route (no residue to gate); CONSTANT_FAST: 4.3e-11 against
     a bound of 3.2e-8 (16384 points, 50 % overlap), 3.5e-11 / 1.6e-8 (8192 role-split), 1.2e-11 / 8.1e-9 (4096 ws), below
     1e-13 on the seg kernels, exactly 0 elsewhere; NONE: 1.31 ulp of the peak amplitude (32768 points, twolevel:r16), 0.91
     (seg_padded 1024), 0.85 (onewg), at most 0.54 elsewhere;
  f. bit-exact on every route and detrend mode, both gains;
  g. gains 2^52 (32768, 16384) ... 2^61 (mtm): the 3-9 bins that must be NaN are, 0-4 of the 3-6 that may go either way
     are too, no inf; the bins that must be right within 1.6e-5 (32768 onewg), 7.3e-6 (twolevel:r16), 5.0e-6 and below.
What the routes returned before the output stage wrote NaN for sums float32 does not hold and before the peak hold kept a
NaN - inf-bin counts per route, which peak forms dropped the NaN - is in NOTES.md section 2 ("Edge cases")."""
import numpy as np
import pytest

import degenerate_cases as D
from oracle import ref_cpu as R
from test_csd_gpu import census
from test_hip_parity import RTOL, check_single_rows, ctx, hip, relerr  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import window

pytestmark = pytest.mark.gpu

ROUTES = sorted(D.ROUTES)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_plan(ctx, hip, route, detrend=None, sched=None, **kw):
    r = D.shape(route)
    detrend = detrend or r['detrends'][0]
    det = {'constant': hip.DETREND_CONSTANT, 'fast': hip.DETREND_CONSTANT_FAST, 'none': hip.DETREND_NONE}[detrend]
    if r['mtm']:
        plan = ctx.mtm_plan(r['nfft'], noverlap=r['noverlap'], nw=4.0, ntapers=r['mtm'], detrend=det, **kw)
    else:
        kern = {'auto': hip.KERNEL_AUTO, 'generic': hip.KERNEL_GENERIC, 'tuned': hip.KERNEL_TUNED}[r['kernel']]
        plan = ctx.welch_plan(r['nfft'], nperseg=r['nperseg'], noverlap=r['noverlap'], window=window(r['window'], r['nperseg']),
                              detrend=det, kernel=kern, **kw)
        if r['tuning']:
            plan.set_tuning(r['tuning'])
    if sched is not None:
        plan.set_schedule(sched)
    return plan


def db_plan(ctx, hip, route, detrend):
    return make_plan(ctx, hip, route, detrend, db=True, fftshift=True, trim_bins=D.ROUTES[route]['nfft'] // 16)


def on_route(plan, route):
    """the finite input went the way the table says, in nine segments"""
    assert plan.last_recipe().startswith(D.ROUTES[route]['recipe']) and plan.last_nseg == D.NSEG, (route, plan.last_recipe())


def report(what, failures):
    for line in failures:
        print('degenerate %s | %s' % (what, line))
    assert not failures, '%d case(s): %s' % (len(failures), '; '.join(failures[:6]))


# ---- a. one bad sample ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', ROUTES)
def test_one_bad_sample_gives_nan_in_every_bin(ctx, hip, route):
    r = D.shape(route)
    x = D.stream(route)
    failures = []
    for detrend in r['detrends']:
        lin, db = make_plan(ctx, hip, route, detrend), db_plan(ctx, hip, route, detrend)
        assert db.out_len == r['nfft'] - 2 * (r['nfft'] // 16)
        for plan in (lin, db):
            assert np.isfinite(plan.exec(x)).all()
            on_route(plan, route)
        for pos in D.positions(len(x)):
            for name in sorted(D.BAD):
                for part in ('re', 'im'):
                    v = D.poisoned(x, pos, D.BAD[name], part)
                    for plan, form in ((lin, 'linear'), (db, 'dB')):
                        out = plan.exec(v)
                        if not np.isnan(out).all():
                            failures.append('%s %s %s %s at %d %s: %s' % (route, detrend, name, part, pos, form, census(out)))
        lin.close()
        db.close()
    report('a', failures)


@pytest.mark.parametrize('route', ['generic-256', 'w4096-ws', 'any-1021'])
def test_csd_pxx_and_exec_agree_on_a_bad_sample(ctx, hip, route):
    x, y = D.stream(route), D.stream(route, D.SEED + 1)
    plan = make_plan(ctx, hip, route)
    failures = []
    for pos in D.positions(len(x)):
        for name in sorted(D.BAD):
            v = D.poisoned(x, pos, D.BAD[name])
            pxx, one = plan.csd(v, y)[0], plan.exec(v)
            if not np.array_equal(np.isnan(pxx), np.isnan(one)) or not np.isnan(one).all():
                failures.append('%s %s at %d: csd Pxx %s; exec %s' % (route, name, pos, census(pxx), census(one)))
    plan.close()
    report('a csd', failures)


# ---- b. stream isolation ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', ROUTES)
def test_a_bad_sample_stays_in_its_stream(ctx, hip, route):
    r = D.shape(route)
    n, nfft, detrend = r['nsamples'], r['nfft'], r['detrends'][0]
    xs = [D.stream(route, D.SEED + s) for s in range(3)]
    refs = [D.clean_reference(route, detrend, D.SEED + s) for s in range(3)]
    d_in, d_out = ctx.alloc(3 * n * 8), ctx.alloc(3 * nfft * 4)
    failures = []
    try:
        for sched in (hip.SCHED_CONTIGUOUS, hip.SCHED_INTERLEAVED, hip.SCHED_DYNAMIC):
            plan = make_plan(ctx, hip, route, detrend, sched=sched)
            ctx.h2d(d_in, np.concatenate(xs))
            assert plan.exec_dev(d_in, n, d_out, nstreams=3, stream_stride=n) == D.NSEG
            clean = ctx.d2h(d_out, (3, nfft), np.float32)
            for s in range(3):
                e = relerr(clean[s], refs[s])
                print('degenerate b | %s sched %d clean stream %d | %.2e' % (route, sched, s, e))
                assert e < RTOL, (route, sched, s, e)
            for name in ('nan', '+inf'):
                ctx.h2d(d_in, np.concatenate([xs[0], D.poisoned(xs[1], n // 2 + 1, D.BAD[name]), xs[2]]))
                assert plan.exec_dev(d_in, n, d_out, nstreams=3, stream_stride=n) == D.NSEG
                got = ctx.d2h(d_out, (3, nfft), np.float32)
                if not np.isnan(got[1]).all():
                    failures.append('%s sched %d %s: the bad stream %s' % (route, sched, name, census(got[1])))
                for s in (0, 2):
                    if not np.isfinite(got[s]).all() or relerr(got[s], refs[s]) >= RTOL:
                        failures.append('%s sched %d %s: stream %d %s' % (route, sched, name, s, census(got[s])))
                    elif sched != hip.SCHED_DYNAMIC and not same_bits(got[s], clean[s]):
                        failures.append('%s sched %d %s: stream %d moved by %.2e' % (route, sched, name, s, relerr(got[s], clean[s])))
            plan.close()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    report('b', failures)


# ---- c. reuse after poison --------------------------------------------------------------------------------------------------------------

def ragged_cuts(n):
    return (0, n // 5 + 3, n // 2 + 1, (3 * n) // 4 + 7, n)


def streamed(plan, x):
    cuts = ragged_cuts(len(x))
    for a, b in zip(cuts[:-1], cuts[1:]):
        plan.accumulate(x[a:b])
    out = plan.finalize()
    assert plan.last_nseg == D.NSEG
    return out


@pytest.mark.parametrize('route', ROUTES)
def test_a_plan_is_clean_after_a_poisoned_launch(ctx, hip, route):
    """Partial rows, stage-1 scratch, the Bluestein / two-level workspaces with their zero padding, the pilot buffer, the
    running sums and the overlap tail of the streaming form: nothing of a poisoned launch reaches the next one."""
    r = D.shape(route)
    x, detrend = D.stream(route), r['detrends'][0]
    n = len(x)
    fresh = make_plan(ctx, hip, route, detrend, sched=hip.SCHED_CONTIGUOUS)
    want = fresh.exec(x)
    want_streamed = streamed(fresh, x)
    fresh.close()
    assert np.isfinite(want).all() and relerr(want, D.clean_reference(route, detrend)) < RTOL
    assert relerr(want_streamed, D.clean_reference(route, detrend)) < RTOL
    plan = make_plan(ctx, hip, route, detrend, sched=hip.SCHED_CONTIGUOUS)
    failures = []
    for name in ('nan', '+inf'):
        for pos in D.positions(n):
            bad = D.poisoned(x, pos, D.BAD[name])
            assert np.isnan(plan.exec(bad)).all()
            if not same_bits(plan.exec(x), want):
                failures.append('%s exec after %s at %d' % (route, name, pos))
            plan.accumulate(bad)
            plan.reset()
            if not same_bits(streamed(plan, x), want_streamed):
                failures.append('%s accumulate / reset / accumulate after %s at %d' % (route, name, pos))
        # the bad sample in the second of four ragged chunks
        out = streamed(plan, D.poisoned(x, ragged_cuts(n)[1] + 5, D.BAD[name]))
        if not np.isnan(out).all():
            failures.append('%s %s in the second chunk: finalize %s' % (route, name, census(out)))
        if not same_bits(streamed(plan, x), want_streamed):      # finalize() has reset the sums
            failures.append('%s streaming after a poisoned finalize (%s)' % (route, name))
    plan.close()
    report('c', failures)


def test_partial_dev_hands_back_raw_sums_and_scale_dev_applies_the_rule(ctx, hip):
    """oth_welch_partial_dev: the raw sums as they are, non-finite or not (time-sharded ranks add them);
    oth_welch_scale_dev: NaN where the sum is not finite - an inf sum, a NaN sum - and the plan's value elsewhere."""
    route = 'w4096-ws'
    nfft = 4096
    x = D.stream(route)
    plan = make_plan(ctx, hip, route)
    d_in, d_sum, d_out = ctx.alloc(x.nbytes), ctx.alloc(4 * nfft), ctx.alloc(4 * nfft)
    try:
        ctx.h2d(d_in, x)
        assert plan.partial_dev(d_in, len(x), d_sum) == D.NSEG
        sums = ctx.d2h(d_sum, (nfft,), np.float32)
        ref = D.clean_reference(route)
        w = R.get_window('hann', nfft)
        assert relerr(sums.astype(np.float64) / (D.NSEG * np.sum(w * w)), ref) < RTOL
        ctx.h2d(d_in, D.poisoned(x, len(x) // 2 + 1, float('inf')))
        assert plan.partial_dev(d_in, len(x), d_sum) == D.NSEG
        raw = ctx.d2h(d_sum, (nfft,), np.float32)
        print('degenerate c | raw sums of %s with an inf sample: %s' % (route, census(raw)))
        assert not np.isfinite(raw).any()
        spoiled = sums.copy()
        spoiled[5], spoiled[77], spoiled[4000] = np.inf, np.nan, np.float32(3.0e38)
        ctx.h2d(d_sum, spoiled)
        plan.scale_dev(d_sum, D.NSEG, d_out)
        out = ctx.d2h(d_out, (nfft,), np.float32)
        bad = np.zeros(nfft, bool)
        bad[[5, 77]] = True
        assert np.isnan(out[bad]).all() and np.isfinite(out[~bad]).all()
        keep = ~bad
        keep[4000] = False
        assert relerr(out[keep], ref[keep]) < RTOL and out[4000] > 0
    finally:
        for p in (d_in, d_sum, d_out):
            ctx.free(p)
    plan.close()


# ---- d. per-segment rows ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', ['segws-1024', 'w4096-ws'])
def test_segment_rows_only_the_segments_that_hold_the_sample(ctx, hip, route):
    x = D.stream(route)
    plan = make_plan(ctx, hip, route)
    clean = plan.segments(x)
    assert clean.shape == (D.NSEG, D.ROUTES[route]['nfft']) and np.isfinite(clean).all()
    failures = []
    for pos in D.positions(len(x)):
        held = D.segments_holding(route, pos)
        assert 1 <= len(held) <= 2
        for name in sorted(D.BAD):
            for part in ('re', 'im'):
                rows = plan.segments(D.poisoned(x, pos, D.BAD[name], part))
                for s in range(D.NSEG):
                    ok = (not np.isfinite(rows[s]).any()) if s in held else same_bits(rows[s], clean[s])
                    if not ok:
                        failures.append('%s %s %s at %d: row %d (%s) %s' % (route, name, part, pos, s, 'holds it' if s in held else 'clean',
                                                                          census(rows[s])))
    plan.close()
    report('d', failures)


# ---- e. silence and a constant ----------------------------------------------------------------------------------------------------------

def check_line_row(got, ref):
    """the row of a line spectrum against its oracle (see the file header) -> worst amplitude error in ulp of the peak"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    amp, amp_ref = np.sqrt(got), np.sqrt(ref)
    err = float(np.max(np.abs(amp - amp_ref)) / amp_ref.max())
    assert err <= D.ULP4, err * 2.0 ** 23
    strong = amp_ref >= 0.01 * amp_ref.max()
    check_single_rows(got[strong], ref[strong], ulps=4)
    return err * 2.0 ** 23


@pytest.mark.parametrize('route', ROUTES)
def test_silence_and_a_constant(ctx, hip, route):
    r = D.shape(route)
    zeros = np.zeros(r['nsamples'], np.complex64)
    const = np.full(r['nsamples'], D.CONSTANT, np.complex64)
    failures = []
    for detrend in r['detrends']:
        lin, db = make_plan(ctx, hip, route, detrend), db_plan(ctx, hip, route, detrend)
        out = lin.exec(zeros)
        if not np.all(out == 0):
            failures.append('%s %s silence: %d bins not zero, max %.2e' % (route, detrend, np.count_nonzero(out), np.nanmax(np.abs(out))))
        out = db.exec(zeros)
        if not np.isneginf(out).all():
            failures.append('%s %s silence in dB: %s' % (route, detrend, census(out)))
        out = lin.exec(const)
        assert lin.last_nseg == D.NSEG
        if detrend == 'constant':
            if not np.all(out == 0):
                failures.append('%s constant detrended: %d bins not zero, max %.2e (fast bound %.2e)'
                                % (route, np.count_nonzero(out), np.nanmax(np.abs(out)), D.constant_fast_bound(route)))
        elif detrend == 'fast':
            print('degenerate e | %s constant, fast detrend | max %.2e of a bound of %.2e' % (route, np.nanmax(out), D.constant_fast_bound(route)))
            if not (np.all(out >= 0) and np.all(out <= D.constant_fast_bound(route))):
                failures.append('%s constant, fast detrend: max %.2e above %.2e' % (route, np.nanmax(out), D.constant_fast_bound(route)))
        else:
            print('degenerate e | %s constant, no detrend | %.2f ulp of the peak amplitude' % (route, check_line_row(out, D.reference(route, const, 'none'))))
        lin.close()
        db.close()
    report('e', failures)


# ---- f. powers of two -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', ROUTES)
def test_gains_that_are_powers_of_two_scale_the_output_exactly(ctx, hip, route):
    r = D.shape(route)
    x = D.stream(route)
    failures = []
    for detrend in r['detrends']:
        plan = make_plan(ctx, hip, route, detrend, sched=hip.SCHED_CONTIGUOUS)
        base = plan.exec(x)
        on_route(plan, route)
        assert relerr(base, D.clean_reference(route, detrend)) < (RTOL if detrend != 'fast' else 2e-3)
        for k in (20, -20):
            got = plan.exec(D.gained(x, k))
            want = base * np.float32(4.0 ** k)      # exact: a power of two inside the normal range (test_degenerate_cpu.py)
            if not same_bits(got, want):
                failures.append('%s %s 2^%d: %d bins differ, by at most %.2e' % (route, detrend, k, np.count_nonzero(bits(got) != bits(want)),
                                                                            relerr(got, want)))
        plan.close()
    report('f', failures)


# ---- g. overflow ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', D.OVERFLOW_ROUTES)
def test_bins_whose_float32_sum_overflows_read_nan_never_inf(ctx, hip, route):
    detrend = D.shape(route)['detrends'][0]
    g, must_nan, must_right, either = D.overflow_case(route, detrend)
    ref = D.clean_reference(route, detrend) * 4.0 ** g
    plan = make_plan(ctx, hip, route, detrend)
    got = plan.exec(D.gained(D.stream(route), g))
    assert plan.last_nseg == D.NSEG
    plan.close()
    e = relerr(got[must_right], ref[must_right]) if np.isfinite(got[must_right]).all() else float('inf')
    print('degenerate g | %s gain 2^%d | %s; must be NaN %d (NaN %d), either %d (NaN %d), must be right %d: %.2e'
          % (route, g, census(got), must_nan.sum(), np.isnan(got[must_nan]).sum(), either.sum(), np.isnan(got[either]).sum(),
             must_right.sum(), e))
    assert not np.isinf(got).any(), census(got)
    assert np.isnan(got[must_nan]).all()
    assert np.isfinite(got[must_right]).all() and e < RTOL
    assert either.sum() <= 0.02 * len(got)


# ---- h. the chain -----------------------------------------------------------------------------------------------------------------------

def make_chain(ctx, hip, nfft, kern, form, keep=1):
    from ofdm_tools import windows
    if form == 'sensor':
        ch = ctx.chain(nfft, None, True, hip.EPI_MAG2_OVER_N2, keep)
    elif form == 'peak':
        ch = ctx.chain(nfft, windows.blackmanharris(nfft), False, hip.EPI_MAG, keep)
        ch.set_peak_hold(True)
    else:
        ch = ctx.chain(nfft, windows.blackmanharris(nfft), True, hip.EPI_MAG2, keep)
        ch.set_iir_log(D.IIR_ALPHA, -10.0 * np.log10(nfft))
    if kern == 'generic':
        ch.set_kernel(hip.KERNEL_GENERIC)
    return ch


def state_of(ch, form):
    return ch.peak() if form == 'peak' else (ch.iir() if form == 'iir' else None)


def pushes(ch, form, x, cuts, max_rows=None):
    """-> per push (rows, rows produced, state after it)"""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        rows, n = ch.push(x[a:b], max_rows=max_rows)
        out.append((rows.copy(), n, state_of(ch, form)))
    return out


def all_bad(v):
    return not np.isfinite(v).any()


def compare_runs(label, form, clean, bad, first_bad_push, bad_row, failures):
    """clean / bad: pushes() of the same cuts, every row handed back; first_bad_push: the push that holds the bad vector;
    bad_row: its row index within that push"""
    for i, ((rc, nc, sc), (rb, nb, sb)) in enumerate(zip(clean, bad)):
        assert nc == nb and rc.shape == rb.shape == (nc, rc.shape[1]), (label, i)
        for j in range(nc):
            after = i > first_bad_push or (i == first_bad_push and j >= bad_row)
            here = i == first_bad_push and j == bad_row
            if here or (form == 'iir' and after):      # dB rows carry the filter's memory
                ok = all_bad(rb[j])
            else:
                ok = same_bits(rb[j], rc[j])
            if not ok:
                failures.append('%s push %d row %d: %s' % (label, i, j, census(rb[j])))
        if sc is not None:
            ok = all_bad(sb) if i >= first_bad_push else same_bits(sb, sc)
            if not ok:
                failures.append('%s state after push %d: %s' % (label, i, census(sb)))


@pytest.mark.parametrize('form', D.CHAIN_FORMS)
@pytest.mark.parametrize('nfft,kern', D.CHAIN_SIZES)
def test_chain_one_bad_vector(ctx, hip, nfft, kern, form):
    x = D.chain_stream(nfft)
    k = D.CHAIN_BAD_VECTOR
    two = D.chain_cuts(nfft)                                               # splits inside vector 7
    three = (0, 4 * nfft + nfft // 3, 7 * nfft + nfft // 3, len(x))        # the first push ends before vector 5
    ref_rows, ref_state = D.chain_reference(form, x, nfft)
    failures = []
    clean = {}
    for name, cuts, max_rows in (('two', two, None), ('three', three, None), ('latest', three, 1)):
        ch = make_chain(ctx, hip, nfft, kern, form)
        clean[name] = pushes(ch, form, x, cuts, max_rows=max_rows)
        ch.close()
    # the clean run is the oracle's: rows in time order, the state after the last push
    rows = np.concatenate([p[0] for p in clean['two']])
    assert rows.shape == (D.CHAIN_VECTORS, nfft)
    if form == 'iir':
        check_single_rows(10.0 ** ((rows.astype(np.float64) + 10.0 * np.log10(nfft)) / 10.0), ref_state, ulps=16)      # through float32 dB
    else:
        check_single_rows(rows, ref_rows, power=form == 'sensor')
    if form != 'sensor':
        for name in clean:
            check_single_rows(clean[name][-1][2], ref_state[-1], power=form == 'iir')
    if form != 'iir':      # the latest row is the same row whether or not the others are handed back
        assert all(same_bits(a[0][-1:], b[0]) for a, b in zip(clean['three'], clean['latest']))
    for name in ('nan', '+inf'):
        v = D.poisoned(x, k * nfft + nfft // 2 + 1, D.BAD[name])
        for run, cuts, first_bad, bad_row in (('two', two, 0, k), ('three', three, 1, k - 4)):
            ch = make_chain(ctx, hip, nfft, kern, form)
            compare_runs('%d %s %s %s %s pushes' % (nfft, kern, form, name, run), form, clean[run], pushes(ch, form, v, cuts), first_bad,
                         bad_row, failures)
            # reset(), then the clean stream in ONE push (more than eight rows: the IIR rows take their own launch)
            ch.reset()
            again = pushes(ch, form, x, (0, len(x)))
            ch.close()
            ch = make_chain(ctx, hip, nfft, kern, form)
            fresh = pushes(ch, form, x, (0, len(x)))
            ch.close()
            if not (same_bits(again[0][0], fresh[0][0]) and (fresh[0][2] is None or same_bits(again[0][2], fresh[0][2]))):
                failures.append('%d %s %s: after reset() behind %s the clean stream differs from a fresh chain' % (nfft, kern, form, name))
        # the latest row only (max_rows = 1), against a clean run of the same shape: the fused IIR launch takes the rows
        # it does not hand back into its weighted sum, so its bits depend on how many rows the caller asks for
        ch = make_chain(ctx, hip, nfft, kern, form)
        one = pushes(ch, form, v, three, max_rows=1)
        ch.close()
        for i, ((rc, nc, sc), (rb, nb, sb)) in enumerate(zip(clean['latest'], one)):
            assert nb == nc and rb.shape == rc.shape == (1, nfft)
            ok = all_bad(rb[0]) if (form == 'iir' and i >= 1) else same_bits(rb[0], rc[0])
            if sc is not None:
                ok = ok and (all_bad(sb) if i >= 1 else same_bits(sb, sc))
            if not ok:
                failures.append('%d %s %s %s max_rows 1 push %d: row %s state %s' % (nfft, kern, form, name, i, census(rb[0]),
                                                                                  census(sb) if sb is not None else '-'))
    report('h', failures)


@pytest.mark.parametrize('form', D.CHAIN_FORMS)
@pytest.mark.parametrize('nfft,kern', D.CHAIN_SIZES)
def test_chain_bad_sample_in_a_dropped_vector_changes_nothing(ctx, hip, nfft, kern, form):
    x = D.chain_stream(nfft)
    cuts = D.chain_cuts(nfft)
    ch = make_chain(ctx, hip, nfft, kern, form, keep=2)      # keeps vectors 1, 3, 5, ...
    clean = pushes(ch, form, x, cuts)
    ch.close()
    assert sum(p[1] for p in clean) == D.CHAIN_VECTORS // 2
    for name in ('nan', '+inf'):
        ch = make_chain(ctx, hip, nfft, kern, form, keep=2)
        got = pushes(ch, form, D.poisoned(x, 4 * nfft + 3, D.BAD[name]), cuts)
        ch.close()
        for (rc, nc, sc), (rb, nb, sb) in zip(clean, got):
            assert nc == nb and same_bits(rb, rc) and (sc is None or same_bits(sb, sc)), (nfft, kern, form, name)


@pytest.mark.parametrize('form', ['peak', 'iir'])
@pytest.mark.parametrize('nfft', [256, 1024])
def test_chain_bad_vector_through_the_two_launch_tail(ctx, hip, nfft, form):
    """The fused launch hands W = min(resident teams, ceil(vectors / 2)) team rows to the tail (interleaved_chunks,
    abi_state.h: chunks of 2 vectors below four per resident team; 12288 / 3072 resident teams at 256 / 1024 points), and
    chain_tail_groups(W, nfft) > 0 - chain_reduce_kernel in front of chain_state_kernel - from W = 129 on: 300 vectors in one
    push are W = 150 team rows in 13 groups.  The bad vector is number 150; twenty clean vectors follow in a second push."""
    nvec, k = 320, 150
    x = D.chain_stream(nfft, nvec)
    cuts = (0, 300 * nfft, nvec * nfft)
    ch = make_chain(ctx, hip, nfft, 'auto', form)
    clean = pushes(ch, form, x, cuts, max_rows=2)
    ch.close()
    ref_rows, ref_state = D.chain_reference(form, x, nfft)
    assert [p[1] for p in clean] == [300, 20]
    assert relerr(clean[0][2], ref_state[299]) < RTOL and relerr(clean[1][2], ref_state[-1]) < RTOL
    failures = []
    for name in ('nan', '+inf'):
        ch = make_chain(ctx, hip, nfft, 'auto', form)
        got = pushes(ch, form, D.poisoned(x, k * nfft + nfft // 2 + 1, D.BAD[name]), cuts, max_rows=2)
        for i, ((rc, nc, sc), (rb, nb, sb)) in enumerate(zip(clean, got)):
            assert nc == nb and rb.shape == (2, nfft)
            rows_ok = all_bad(rb) if form == 'iir' else same_bits(rb, rc)
            if not (rows_ok and all_bad(sb)):
                failures.append('%d %s %s push %d: rows %s state %s' % (nfft, form, name, i, census(rb), census(sb)))
        ch.reset()
        again = pushes(ch, form, x, cuts, max_rows=2)
        ch.close()
        for (rc, nc, sc), (rb, nb, sb) in zip(clean, again):
            if not (same_bits(rb, rc) and same_bits(sb, sc)):
                failures.append('%d %s: after reset() behind %s the clean stream differs from a fresh chain' % (nfft, form, name))
    report('h tail', failures)
