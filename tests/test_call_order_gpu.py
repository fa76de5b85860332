"""Every entry point of a plan against its own solo result under shared use.

All of a plan's calls write through the same few holders of csrc/abi_state.h (d_partial, d_reduce, d_out, d_stage, d_rows,
the per-family workspaces, five replaceable tables, the four-slot output ring, last_recipe), and all plans of a context share
the 64 ticket words of the dynamic schedule with their queue_clean / queue_used flags ("Who writes what on a
plan").  Each family's own suite calls only its own family on a plan of its own; here one plan runs them all.

The method: a SOLO is a fresh plan, set up exactly like the shared one (call_order_cases.build: the same setters and tables,
the schedule forced to contiguous runs), that runs one op at one input size and is closed; its output bytes, last_recipe()
and segment count are kept.  Every solo is computed twice on two fresh plans and the two must agree, so that a difference
under sharing is due to sharing.  A SHARED plan then runs seeded sequences of all (op, size) pairs, and every output must
equal its solo byte for byte, recipe string for string, segment count exactly - no tolerance anywhere but in sections 4
and 5's ticketed launches, which run the dynamic schedule on purpose: their summation order is not fixed, and they are held to
the float64 oracle at the project's own gates (RTOL of test_hip_parity on linear power, 1e-4 absolute on coherence;
test_call_order_cpu.py shows that a lost or doubled segment misses those gates on these inputs).

A failure prints the order with its seed, the op before the one that differs and the first differing row.

Measured on an MI355X: 1 592 (op, size) pairs over the nine plan shapes of sections 1 and 2 and 195 behind replaced tables,
all byte-equal to their solo, every solo reproducible on two fresh plans.  The worst bin of a ticketed launch: 0.016 of RTOL
(1.6e-6 relative; 4096 points x 64 streams, welch4096:ws); by plan 0.004 of RTOL at 1024 points (segws), 0.016 at 4096, 0.010
at 8192 (welch16k1x_half); the two-channel launch 0.012 of RTOL on power and 0.004 of its 1e-4 on coherence (csd4096ws).
With the `queue_clean = false` line of run_average taken out of a scratch build, test_ticket_words_shared_by_plans_of_one_context
fails: the 64-stream launch at 4096 points reads stale ticket words and misses the oracle by 0.84 relative.
What the suite found when it first ran is kept in REGRESSIONS.
"""
import collections

import numpy as np
import pytest

import call_order_cases as C
import csd_oracle as O
from oracle import ref_cpu as R
from test_hip_parity import RTOL, ctx, hann, hip, relerr  # noqa: F401 - ctx / hip are fixtures

pytestmark = pytest.mark.gpu

Env = collections.namedtuple('Env', 'ctx hip')
Result = collections.namedtuple('Result', 'outs recipe nseg')
SEED = 20260117
STATE, UNSUPPORTED, INVALID = -5, -3, -1
CXY_ATOL = 1e-4      # the project's gate on a coherence (test_consumer_path_gpu, test_csd_gpu)
SOLOS = {}           # (shape, tables, op, M) -> Result: computed once per module, read by every order


def run(env, plan, name, shape, M, tables=C.TABLES_A):
    """one row of the op table on `plan` -> what is compared"""
    dev = C.Dev(env.ctx)
    try:
        outs, nseg = C.BY_NAME[name].run(env, plan, C.inputs(name, shape, M, tables), dev)
    finally:
        dev.close()
    return Result(tuple(np.array(o, copy=True) for o in outs), plan.last_recipe(), int(nseg))


def difference(got, want):
    """None if the two results are the same bytes, recipe and count; else the first difference in words"""
    if got.nseg != want.nseg:
        return 'segment count %d, solo %d' % (got.nseg, want.nseg)
    if got.recipe != want.recipe:
        return 'recipe %r, solo %r' % (got.recipe, want.recipe)
    if len(got.outs) != len(want.outs):
        return '%d outputs, solo %d' % (len(got.outs), len(want.outs))
    for k, (a, b) in enumerate(zip(got.outs, want.outs)):
        if a.shape != b.shape or a.dtype != b.dtype:
            return 'output %d: %s %s, solo %s %s' % (k, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            nrows = a.shape[0] if a.ndim > 1 else 1
            a2, b2 = (np.ascontiguousarray(v).reshape(nrows, -1) for v in (a, b))
            bad = a2.view(np.uint8).reshape(nrows, a2.shape[1], -1) != b2.view(np.uint8).reshape(nrows, a2.shape[1], -1)
            bad = np.any(bad, axis=2)      # [row, element]
            row = int(np.argmax(np.any(bad, axis=1)))
            at = int(np.argmax(bad[row]))
            return 'output %d differs first in row %d at element %d: %r, solo %r (%d of %d elements of the row, %d of %d rows differ)' % (
                k, row, at, a2[row, at], b2[row, at], int(bad[row].sum()), bad.shape[1], int(np.any(bad, axis=1).sum()), nrows)
    return None


def solo(env, shape, name, M, tables=C.TABLES_A):
    key = (shape, tables, name, M)
    if key not in SOLOS:
        pair = []
        for _ in range(2):
            plan = C.build(env.ctx, env.hip, shape, tables)
            try:
                pair.append(run(env, plan, name, shape, M, tables))
            finally:
                plan.close()
        diff = difference(pair[1], pair[0])
        assert diff is None, 'not reproducible on two fresh plans: %s of %d segments on %s: %s' % (name, M, C.shape_id(shape), diff)
        op = C.BY_NAME[name]
        assert pair[0].nseg == C.segments_of(op, shape, C.inputs(name, shape, M, tables), tables) == M, (name, M, pair[0].nseg)
        SOLOS[key] = pair[0]
    return SOLOS[key]


def run_order(env, plan, shape, what, seq, tables=C.TABLES_A):
    """the (op, size) pairs of `seq` on the shared plan, each against its solo -> how many were compared"""
    before = 'the plan is fresh'
    for k, (name, M) in enumerate(seq):
        want = solo(env, shape, name, M, tables)
        diff = difference(run(env, plan, name, shape, M, tables), want)
        assert diff is None, '%s, order "%s", call %d: %s of %d segments after %s: %s' % (C.shape_id(shape), what, k, name, M, before, diff)
        before = '%s of %d segments' % (name, M)
    return len(seq)


def shared_orders(env, shape):
    """sections 1 and 2: every solo twice, then the three orders, each on a plan of its own"""
    for name, M in C.pairs_for(shape):
        solo(env, shape, name, M)
    total = 0
    for what, seq in C.orders(shape, SEED):
        plan = C.build(env.ctx, env.hip, shape)
        try:
            total += run_order(env, plan, shape, what, seq)
        finally:
            plan.close()
    print('%s: %d solos reproducible on two fresh plans; %d (op, size) pairs compared over three orders, all byte-equal to their solo'
          % (C.shape_id(shape), len(C.pairs_for(shape)), total))
    return total


# ---- 1. Welch plans -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', C.WELCH_SHAPES, ids=C.shape_id)
def test_welch_plan_every_op_equals_its_solo_in_three_orders(ctx, hip, shape):
    env = Env(ctx, hip)
    assert shared_orders(env, shape) == 4 * len(C.pairs_for(shape))
    # the routes the sizes stand for: the test must not pass on a fallback
    route = {64: 'kernel=welch_generic ', 1024: 'kernel=segws ', 4096: 'kernel=welch4096:', 16384: 'kernel=welch16k'}[shape.nfft]
    for M in C.SIZES:
        for name in ('exec', 'exec_dev', 'exec_async'):
            r = solo(env, shape, name, M).recipe
            assert r.startswith(route) and ' sched=contiguous ' in r, (name, M, r)
    if shape.nfft == 4096:
        assert solo(env, shape, 'exec', C.LARGE).recipe.startswith('kernel=welch4096:ws ') and ' pilot=inline ' in solo(env, shape, 'exec', C.LARGE).recipe
    assert solo(env, shape, 'matrix', C.LARGE).recipe.startswith('kernel=welchmat nfft=%d ' % shape.nfft)


# Orders that once differed, by name, next to the seeded ones.
REGRESSIONS = [
    # oth_welch_segments_dev launched kernels of its own but did not write last_recipe: the string named the call before it
    # (large-first, call 7: '' on the solo's fresh plan, the last accumulate's launch on the shared one)
    ('segments behind accumulate named the accumulate in last_recipe', C.welch_shape(64), [('accumulate', C.LARGE), ('segments', C.LARGE)]),
    ('segments behind exec_dev named the exec_dev in last_recipe', C.welch_shape(4096), [('exec_dev', C.SMALL), ('segments', C.LARGE), ('median', C.SMALL)]),
]


@pytest.mark.parametrize('what,shape,seq', REGRESSIONS, ids=['segments_behind_accumulate', 'segments_behind_exec_dev'])
def test_orders_that_once_differed(ctx, hip, what, shape, seq):
    env = Env(ctx, hip)
    plan = C.build(ctx, hip, shape)
    try:
        run_order(env, plan, shape, what, seq)
    finally:
        plan.close()
    assert solo(env, shape, 'segments', C.LARGE).recipe.startswith('kernel=segments rows=')


# ---- 2. multitaper plans ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', C.MTM_SHAPES, ids=C.shape_id)
def test_multitaper_plan_every_op_equals_its_solo_in_three_orders(ctx, hip, shape):
    assert shared_orders(Env(ctx, hip), shape) == 4 * len(C.pairs_for(shape))


# ---- 3. tables replaced between calls -------------------------------------------------------------------------------------

FIELD = dict(set_cycles='cycles', set_lags='lags', set_prototype='ntaps', set_steering='steer', set_ratios='ratio_pow')


@pytest.mark.parametrize('setter', sorted(C.SETTERS))
def test_a_replaced_table_serves_its_family_and_disturbs_no_other(ctx, hip, setter):
    """Table A, the family; table B of another length (the steering table: another channel count too, and 24 -> 40 -> 24
    directions across one tile of 32), the family again; back to A.  Each result equals the solo of a plan that was built with
    that table.  Then every other op of the plan, each run right after the setter was called once more (B and A in turn),
    still equals its solo.  (The filter bank's own suite pins the A / B pair of the prototype; it costs nothing to keep.)"""
    env = Env(ctx, hip)
    apply, kinds, readers = C.SETTERS[setter]
    shape = C.welch_shape(1024) if 'welch' in kinds else C.MTM_SHAPES[0]
    a = C.TABLES_A
    b = a._replace(name='A with %s of B' % FIELD[setter], **{FIELD[setter]: getattr(C.TABLES_B, FIELD[setter])})
    plan = C.build(ctx, hip, shape, a)
    compared = 0
    try:
        for k, t in enumerate((a, b, a, b)):
            if k:
                apply(plan, shape, t)
            compared += run_order(env, plan, shape, '%s: table %s (round %d)' % (setter, t.name, k), [(r, M) for r in readers for M in C.SIZES], t)
        others = [op.name for op in C.ops_for(shape) if op.name not in readers]
        for k, name in enumerate(others):
            t = (a, b)[k % 2]
            apply(plan, shape, t)
            compared += run_order(env, plan, shape, '%s(%s) in front of every call' % (setter, t.name), [(name, C.SMALL)])
    finally:
        plan.close()
    print('%s on %s: %d (op, size) pairs compared, all byte-equal to their solo' % (setter, C.shape_id(shape), compared))


# ---- 4. the ticket words: several plans on one context -------------------------------------------------------------------

def forced_dynamic(ctx, hip, nfft, **kw):
    plan = ctx.welch_plan(nfft, window=hann(nfft), detrend=hip.DETREND_CONSTANT, **kw)
    plan.set_tuning(None, sched=hip.SCHED_DYNAMIC, chunk=2)
    return plan


class Streams(object):
    """65 streams of the nfft-point plan on the device (stream k is call_order_cases.ticket_stream(nfft, k % 3)), the oracle
    of the three, and an output row per stream"""

    def __init__(self, ctx, nfft, count=65):
        xs = [C.ticket_stream(nfft, k) for k in range(3)]
        self.ctx, self.nfft, self.n, self.count = ctx, nfft, len(xs[0]), count
        self.refs = [R.welch_np(x, fs=1.0, nperseg=nfft, nfft=nfft)[1] for x in xs]
        self.d_in = ctx.alloc(8 * self.n * count)
        for k in range(count):
            ctx.h2d(self.d_in + 8 * self.n * k, xs[k % 3])
        self.d_out = ctx.alloc(4 * nfft * count)

    def launch(self, plan, ns, sched):
        """a ticketed exec_dev over the first ns streams -> the worst bin as a fraction of RTOL"""
        self.ctx.h2d(self.d_out, np.full(ns * self.nfft, C.SENTINEL, np.uint32))
        nseg = plan.exec_dev(self.d_in, self.n, self.d_out, nstreams=ns, stream_stride=self.n)
        recipe = plan.last_recipe()
        assert nseg == C.TICKET_M[self.nfft] and ' sched=%s ' % sched in recipe, recipe
        rows = self.ctx.d2h(self.d_out, (ns, self.nfft), np.float32)
        worst = float(np.max([relerr(rows[k], self.refs[k % 3]) for k in range(ns)]))      # (np.max: a NaN row shows)
        print('ticketed exec_dev %5d points x %2d streams (%s): worst bin %.3f of RTOL' % (self.nfft, ns, recipe.split(' nfft=')[0], worst / RTOL))
        assert worst < RTOL, (self.nfft, ns, worst, recipe)
        return worst / RTOL

    def close(self):
        self.ctx.free(self.d_in)
        self.ctx.free(self.d_out)


def csd_launch(plan):
    """the ticketed two-channel call -> the worst reading as a fraction of its gate"""
    x, y = C.ticket_pair()
    pxx, pyy, pxy, cxy = O.csd(x, y, 1.0, 'hann', 4096, 2048, 4096, 'constant', 'density')
    gxx, gyy, gxy, gc = plan.csd(x, y)
    recipe = plan.last_recipe()
    assert plan.last_nseg == C.TICKET_CSD_M and recipe.startswith('kernel=csd4096') and ' sched=dynamic ' in recipe, recipe
    power = max(relerr(gxx, pxx), relerr(gyy, pyy), float(np.max(np.abs(np.asarray(gxy, np.complex128) - pxy) / np.sqrt(pxx * pyy))))
    coh = float(np.max(np.abs(np.asarray(gc, np.float64) - cxy)))
    print('ticketed csd 4096 points (%s): worst bin %.3f of RTOL on power, %.3f of 1e-4 on coherence' % (recipe.split(' nfft=')[0], power / RTOL, coh / CXY_ATOL))
    assert power < RTOL and coh < CXY_ATOL, (power, coh, recipe)
    return max(power / RTOL, coh / CXY_ATOL)


def fillers(env, plans):
    """The calls that go between two ticketed launches: they draw no ticket, pass through no finalize_and_rearm of a ticketed
    launch, or end early -> [(name, call -> bytes that must not change from one call to the next)]"""
    ctx, hip = env
    w1024, mtm = C.welch_shape(1024), C.MTM_SHAPES[0]
    x = C.inputs('exec', w1024, C.LARGE)['x']
    rows = np.abs(x[:4 * 1024].reshape(4, 1024)).astype(np.float32) ** 2
    d_rows = ctx.alloc(rows.nbytes)
    ctx.h2d(d_rows, rows)
    plans['free'] = lambda: ctx.free(d_rows)

    def median():
        return run(env, plans['other'], 'median', w1024, C.LARGE)

    def stat(name, plan, shape):
        return lambda: run(env, plans[plan], name, shape, C.LARGE)

    def push():
        plans['chain'].reset()
        got, n = plans['chain'].push(x[:4096])
        assert n == 4
        return Result((got,), '', n)

    def xcorr():
        got = ctx.xcorr(x[:200], x[50:250], 256)
        ref = R.xcorr(x[:200], x[50:250], 256)
        assert np.max(np.abs(got - ref)) / np.max(ref) < 1e-5
        return Result((got,), '', 0)

    def decide(nch):
        def call():
            lo = np.arange(nch) * 100
            _, noise, power = ctx.scan_decide_dev(d_rows, 4, 1024, 16, 2.0, lo, lo + 64)
            assert np.all(noise > 0) and power.shape == (4, nch)
            return Result((noise, power), '', 0)
        return call

    def refused(call, code, text):
        def go():
            with pytest.raises(hip.HipError) as ei:
                call()
            assert ei.value.code == code and text in str(ei.value), str(ei.value)
            return Result((), '', 0)
        return go

    pair = C.inputs('csd', w1024, C.SMALL)
    short = C.ticket_stream(4096, 0)[:4095]      # one sample shorter than nperseg
    return [('median exec', median), ('sk', stat('sk', 'other', w1024)), ('matrix', stat('matrix', 'other', w1024)),
            ('ftest', stat('ftest', 'mtm', mtm)), ('chain.push', push), ('xcorr', xcorr), ('scan_decide_dev, 4 channels', decide(4)),
            ('scan_decide_dev, 9 channels', decide(9)),
            ('csd refused on a dB plan', refused(lambda: plans['db'].csd(pair['x'], pair['y']), UNSUPPORTED, 'dB output is not defined')),
            ('exec refused on a short input', refused(lambda: plans[4096].exec(short), INVALID, 'input shorter than nperseg'))]


def test_ticket_words_shared_by_plans_of_one_context(ctx, hip):
    """Three plans with the dynamic schedule forced (4096 tuned, 1024 seg, 8192) and a 4096-point two-channel plan alternate
    on one context in a seeded order, exec_dev at 1, 3 and 64 streams, and between two ticketed launches goes one of the
    calls that leave the ticket words alone or end early.  Every ticketed result meets the float64 oracle at the project's
    gates; every filler repeats its first answer bit for bit (the solo's, where the op table has one).  65 streams do not fit
    the 64 ticket words: the recipe says interleaved."""
    env = Env(ctx, hip)
    w1024, mtm = C.welch_shape(1024), C.MTM_SHAPES[0]
    plans = {n: forced_dynamic(ctx, hip, n, **({'kernel': hip.KERNEL_TUNED} if n == 4096 else {})) for n in sorted(C.TICKET_M)}
    plans['csd'] = forced_dynamic(ctx, hip, 4096, kernel=hip.KERNEL_TUNED)
    plans['other'], plans['mtm'] = C.build(ctx, hip, w1024), C.build(ctx, hip, mtm)
    plans['db'] = C.build(ctx, hip, C.WELCH_SHAPES[4])
    plans['chain'] = ctx.chain(1024, None, True, hip.EPI_MAG2, 1)
    streams = {n: Streams(ctx, n) for n in sorted(C.TICKET_M)}
    try:
        fill = fillers(env, plans)
        first = {name: call() for name, call in fill}      # before any ticket is drawn
        for name, shape, plan in (('median', w1024, 'other'), ('sk', w1024, 'other'), ('matrix', w1024, 'other'), ('ftest', mtm, 'mtm')):
            key = 'median exec' if name == 'median' else name
            assert difference(first[key], solo(env, shape, name, C.LARGE)) is None, name
        ticketed = [(n, ns) for n in sorted(C.TICKET_M) for ns in C.TICKET_STREAMS] + [('csd', 1), ('csd', 1)]
        rng = np.random.default_rng(SEED)
        ticketed = [ticketed[k] for k in rng.permutation(len(ticketed))]
        order = rng.permutation(len(fill))
        worst, before = 0.0, 'nothing'
        for k, (n, ns) in enumerate(ticketed):
            worst = max(worst, csd_launch(plans['csd']) if n == 'csd' else streams[n].launch(plans[n], ns, 'dynamic'))
            name, call = fill[order[k % len(fill)]]
            diff = difference(call(), first[name])
            assert diff is None, 'seed %d, call %d: %s after the ticketed launch %s x %d (before it: %s): %s' % (SEED, k, name, n, ns, before, diff)
            before = name
        assert len(ticketed) >= len(fill)      # every filler went in
        for n in sorted(C.TICKET_M):
            streams[n].launch(plans[n], 65, 'interleaved')
        worst = max(worst, streams[4096].launch(plans[4096], 64, 'dynamic'), csd_launch(plans['csd']))
        print('%d ticketed launches on one context, worst bin %.3f of its gate' % (len(ticketed) + 2, worst))
    finally:
        for s in streams.values():
            s.close()
        for p in plans.values():
            p() if callable(p) else p.close()


# ---- 5. tickets outstanding across other work ------------------------------------------------------------------------------

def solo_exec(env, shape, x):
    plan = C.build(env.ctx, env.hip, shape)
    try:
        return plan.exec(x), plan.last_nseg
    finally:
        plan.close()


@pytest.mark.parametrize('shape,middle', [(C.welch_shape(4096), 'matrix_eig'), (C.MTM_SHAPES[0], 'jackknife')], ids=['welch4096', 'mtm256'])
def test_tickets_outstanding_across_other_work(ctx, hip, shape, middle):
    """Three exec_async tickets of three different inputs; then, on the same plan, a statistic whose input makes the staging
    buffer, the partial rows and the device output rows regrow (DevBuf::ensure drains the stream and frees: a ticket's rows
    must be out of them by then); then a ticketed exec_dev on a second plan; then the three tickets are collected in reverse
    order and each equals the solo exec of its input.
    By construction from the sizes: the tickets staged at most 7 segments of one channel and left at most 7 partial rows;
    matrix_eig stages 5 channels of 11 segments, asks for W x 25 partial rows and for 15 nfft floats of d_out (above the floor of
    5 nfft floats); jackknife stages 11 segments and asks for two partial rows per workgroup."""
    env = Env(ctx, hip)
    xs = [R.synth_iq(C.nsamples(shape, M), 9000 + M) for M in (3, 7, 5)]
    want = [solo_exec(env, shape, x) for x in xs]
    assert [w[1] for w in want] == [3, 7, 5]
    plan = C.build(ctx, hip, shape)
    second = forced_dynamic(ctx, hip, 4096, kernel=hip.KERNEL_TUNED)
    streams = Streams(ctx, 4096, count=3)
    try:
        tickets = [plan.exec_async(x) for x in xs]
        diff = difference(run(env, plan, middle, shape, C.LARGE), solo(env, shape, middle, C.LARGE))
        assert diff is None, '%s behind three outstanding tickets: %s' % (middle, diff)
        streams.launch(second, 3, 'dynamic')
        for k in (2, 1, 0):
            got = plan.wait(tickets[k])
            assert plan.last_nseg == want[k][1]
            assert got.tobytes() == want[k][0].tobytes(), 'ticket %d, collected behind %s and in reverse order, is not the solo exec of its input' % (k, middle)
        assert plan.outstanding == 0
    finally:
        streams.close()
        second.close()
        plan.close()


def test_the_output_ring_keeps_four_tickets(ctx, hip):
    """The documented limit (ofdm_tools_hip.h: "The plan keeps the last 4 launches: an older ticket reports OTH_ERR_STATE"): a
    fifth exec_async takes the first ticket's slot; the first answers OTH_ERR_STATE, the other four are intact."""
    env = Env(ctx, hip)
    shape = C.welch_shape(4096)
    xs = [R.synth_iq(C.nsamples(shape, M), 9100 + M) for M in (3, 4, 5, 6, 7)]
    want = [solo_exec(env, shape, x) for x in xs]
    plan = C.build(ctx, hip, shape)
    try:
        tickets = [plan.exec_async(x) for x in xs]
        assert hip.OUT_RING == 4 and len(set(tickets)) == 5
        with pytest.raises(hip.HipError) as ei:
            plan.wait(tickets[0])
        assert ei.value.code == STATE and 'ticket unknown or overwritten (the ring keeps the last 4 launches)' in str(ei.value)
        for k in (4, 2, 3, 1):
            assert plan.wait(tickets[k]).tobytes() == want[k][0].tobytes() and plan.last_nseg == want[k][1], k
    finally:
        plan.close()


# ---- 6. streaming across other calls -------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft', (1024, 4096))
def test_streaming_across_other_calls(ctx, hip, nfft):
    """accumulate(chunk 1), every non-streaming op at the large size, accumulate(chunk 2), an exec_async, accumulate(chunk 3),
    finalize: the sum and the carried tail survive everything in between.  Chunk 1 holds one segment and a quarter: it
    consumes one step and keeps three quarters of a segment, keep > consumed - the carry that bounces through d_stage, which
    the host forms that follow restage.  The median average is the one call an unfinished accumulation refuses (the header
    says so); it is asserted as that refusal."""
    env = Env(ctx, hip)
    shape = C.welch_shape(nfft)
    x = C.inputs('accumulate', shape, C.LARGE)['x']
    cuts = (0, nfft + nfft // 4, nfft + nfft // 4 + 3 * nfft + 11, len(x))
    assert (cuts[1] - shape.noverlap) // C.step(shape) == 1 and cuts[1] - C.step(shape) > C.step(shape)      # keep > consumed
    chunks = [x[lo:hi] for lo, hi in zip(cuts, cuts[1:])]

    def stream(plan, between=(None, None)):
        for k, chunk in enumerate(chunks):
            plan.accumulate(chunk)
            if k < 2 and between[k]:
                between[k]()
        return plan.finalize(), plan.last_nseg

    alone = C.build(ctx, hip, shape)
    try:
        want = stream(alone)
        recipe = alone.last_recipe()
    finally:
        alone.close()
    assert want[1] == C.LARGE
    plan = C.build(ctx, hip, shape)
    ticket, compared = [], [0]

    def everything_else():
        for op in C.ops_for(shape, streaming=False):
            if op.name == 'median':
                with pytest.raises(hip.HipError) as ei:
                    plan.set_average('median')
                assert ei.value.code == STATE and 'an accumulation is in progress' in str(ei.value)
                continue
            compared[0] += run_order(env, plan, shape, 'inside an accumulation', [(op.name, C.LARGE)])

    try:
        got = stream(plan, (everything_else, lambda: ticket.append(plan.exec_async(chunks[1]))))
        assert got[1] == want[1] == C.LARGE and plan.last_recipe() == recipe
        assert got[0].tobytes() == want[0].tobytes(), 'the streamed sum changed under the calls in between'
        late = plan.wait(ticket[0])
        assert late.tobytes() == solo_exec(env, shape, chunks[1])[0].tobytes()
    finally:
        plan.close()
    print('%d points: the stream of %d segments equals its solo across %d other calls, an exec_async and a refused set_average' % (nfft, want[1], compared[0]))
