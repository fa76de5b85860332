"""The asynchronous work() path (oth_chain_push_async / poll / wait, oth_welch_exec_async) against the float64 oracle
while the GPU is BEHIND: the context's own stream is kept busy by ordinary Welch launches queued ahead of the pushes, so
a push that reuses a pinned slot whose copy is still pending, a vector lost to keep_one_in_n's set_n, or a ticket pushed
out of a shared plan's output ring shows up as a wrong or missing result.

Every push pattern runs twice - behind the hog and on an idle stream - and the two final states must be bit-identical.
A busy-stream run checks that it really reached the hazard: right before the first push that enqueues work into a slot an
earlier such push of the run has used, the probe launch queued behind the hog must still be running.  (Where real pushes
follow each other closely - keep_one_in_n = 5 with 2.5 N pushes, or the random chunks at 16384 points, which spread one
vector over several pushes - that first reuse comes with a real push in the slot's previous ticket, and the ring's
back-pressure legitimately drains the stream there.  keep_one_in_n = 3 with one-vector pushes reaches the hazard at every
length, 16384 points included.)"""
import math
import time

import numpy as np
import pytest

from oracle import ref_cpu as R
from test_hip_parity import RTOL, check_single_rows, ctx, hip, relerr  # noqa: F401 - ctx / hip are fixtures

pytestmark = pytest.mark.gpu

KRING = 4                     # oth_chain::kRing: pinned input slots of the asynchronous form
STAGE_MAX = 1 << 17           # kPinnedStageMax / sizeof(complex64): work()-sized chunks go through the pinned ring
HOG_SECONDS = 0.25            # GPU time queued ahead of the pushes
SF = 1.0e6
ALPHA = 0.3


class Hog(object):
    """4096-point Welch launches over 2^27 device-resident samples (WelchPlan.exec_dev, asynchronous), ended by one
    exec_async launch on a plan of its own whose ticket is the probe: poll() is None while the stream is still busy."""

    def __init__(self, ctx, hip):
        from ofdm_tools import windows
        self.ctx = ctx
        self.n = 1 << 27
        self.d = ctx.alloc(self.n * 8)
        self.out = ctx.alloc(4096 * 4)
        ctx.synth_iq(self.d, self.n, 77, R.TONES, R.DC)
        w = windows.get_window('hann', 4096)
        self.plan = ctx.welch_plan(4096, window=w, detrend=hip.DETREND_NONE)
        self.probe_plan = ctx.welch_plan(4096, window=w, detrend=hip.DETREND_NONE)
        self.plan.exec_dev(self.d, self.n, self.out)
        self.probe_plan.wait(self.probe_plan.exec_async(self.d, self.n))
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(4):
            self.plan.exec_dev(self.d, self.n, self.out)
        ctx.sync()
        self.per_launch = (time.perf_counter() - t0) / 4
        self.launches = int(min(4000, max(8, math.ceil(HOG_SECONDS / self.per_launch))))
        print('hog: %.3f ms per 2^27-sample launch, %d launches' % (self.per_launch * 1e3, self.launches))

    def start(self):
        for _ in range(self.launches):
            self.plan.exec_dev(self.d, self.n, self.out)
        return self.probe_plan.exec_async(self.d, self.n)

    def busy(self, probe):
        return self.probe_plan.poll(probe) is None

    def finish(self, probe):
        self.probe_plan.wait(probe)

    def close(self):
        self.ctx.sync()
        self.plan.close()
        self.probe_plan.close()
        self.ctx.free(self.d)
        self.ctx.free(self.out)


@pytest.fixture(scope='module')
def hog(ctx, hip):
    h = Hog(ctx, hip)
    yield h
    h.close()


# ---- the chains and their oracles -----------------------------------------------------------------------------

def make_chain(ctx, hip, form, N, decim):
    from ofdm_tools import windows
    if form == 'psd_logger':           # psd_logger.py: BH window, no shift, |X|, peak hold
        ch = ctx.chain(N, windows.blackmanharris(N), False, hip.EPI_MAG, decim)
        ch.set_peak_hold(True)
    elif form == 'local_worker':       # local_worker.py: BH window, shifted |X|^2, IIR + 10 log10 + k
        ch = ctx.chain(N, windows.blackmanharris(N), True, hip.EPI_MAG2, decim)
        ch.set_iir_log(ALPHA, log_k(N))
    else:                              # spectrum_sensor_v2.py: rectangular, shifted |X|^2 / N^2
        ch = ctx.chain(N, None, True, hip.EPI_MAG2_OVER_N2, decim)
    return ch


def log_k(N):
    return -10 * math.log10(N) - 10 * math.log10(SF)


def oracle_rows(form, x, N, decim, schedule=None):
    """-> (per kept vector: the row the chain hands back, the chain's state after it or None)."""
    if form == 'psd_logger':
        return R.chain_psd_logger(x, N, decim, schedule)
    if form == 'local_worker':
        lin, _ = R.chain_local_worker(x, N, SF, ALPHA, decim, schedule)
        return lin, lin
    return R.chain_sensor_v2(x, N, decim, schedule), None


def kept_per_push(bounds, N, kept):
    """Rows each push [a, b) produces (kept vectors completing inside it) and the index of its last one."""
    ends = (np.asarray(kept, np.int64) + 1) * N
    out = []
    for a, b in bounds:
        lo, hi = np.searchsorted(ends, a, 'right'), np.searchsorted(ends, b, 'right')
        out.append((int(hi - lo), int(hi) - 1))
    return out


def touches_kept(a, b, N, kept):
    kept = np.asarray(kept, np.int64)
    return bool(np.any((kept * N < b) & ((kept + 1) * N > a)))


def check_row(form, row, ref):
    if form == 'psd_logger':
        check_single_rows(row, ref, power=False)
    elif form == 'local_worker':      # the IIR's linear value behind the dB row (an averaged quantity: RTOL on every bin)
        assert relerr(10 ** ((row.astype(np.float64) - log_k(len(row))) / 10), ref) < RTOL
    else:
        check_single_rows(row, ref)


# ---- push patterns -------------------------------------------------------------------------------------------

def pattern(name, N):
    """-> (samples, chunk sizes, keep_one_in_n)."""
    if name == 'keep3_N':              # (a) the minimal case: real pushes every third ticket, slots 3, 2, 1, 0, 3, ...
        decim, chunks = 3, [N] * (3 * 9)
    elif name == 'keep5_2.5N':         # (b)
        decim, chunks = 5, [N * 5 // 2] * 40
    elif name == 'random_decim100':    # (c) as the sensor runs: 1 - 9000 items per work(), decimation 100
        decim, rng, chunks, total = 100, np.random.default_rng(N + 5), [], 100 * N * 6 + N // 3
        while sum(chunks) < total:
            chunks.append(int(rng.integers(1, 9001)))
    else:                              # (d) the control: every push enqueues work
        decim, chunks = 1, [N + N // 2] * 12
    assert max(chunks) <= STAGE_MAX
    return R.synth_iq(sum(chunks), 300 + N), chunks, decim


PATTERNS = ['keep3_N', 'keep5_2.5N', 'random_decim100', 'keep1_control']
_data = {}


def data(name, N):
    if (name, N) not in _data:
        _data.clear()
        _data[(name, N)] = pattern(name, N)
    return _data[(name, N)]


def warm(ch, N, decim, biggest):
    """Size every buffer the pushes will use (pinned slots, staging, rows) before the timed part, so that no allocation
    in the middle of the run waits for the stream; then restart the chain's stream state."""
    ch.set_keep_one_in_n(1)
    z = np.zeros(biggest + N, np.complex64)
    ts = [ch.push_async(z) for _ in range(KRING)]
    ch.wait(ts[-1])
    ch.set_keep_one_in_n(decim)
    ch.reset()
    return ts[-1]


def run_pushes(ctx, hip, hog, form, N, name, busy, kernel=None):
    x, chunks, decim = data(name, N)
    ch = make_chain(ctx, hip, form, N, decim)
    if kernel is not None:
        ch.set_kernel(kernel)
    last = warm(ch, N, decim, max(chunks))
    probe = hog.start() if busy else None
    kept = R.gr_kept_indices(len(x) // N, N, decim)
    tickets, bounds, used, checked = [], [], set(), False
    pos = 0
    try:
        for m in chunks:
            real = touches_kept(pos, pos + m, N, kept)
            if busy and real and not checked and (last + 1) % KRING in used:
                # the first reuse of a pinned slot: every real push so far must have returned with its copy pending
                assert hog.busy(probe), ('the stream drained before the hazard: the hog (%d x %.3f ms) is too short'
                                         % (hog.launches, hog.per_launch * 1e3))
                checked = True
            t = ch.push_async(x[pos:pos + m])
            ops = ch.last_push_ops()
            assert t == last + 1
            last = t
            tickets.append(t)
            bounds.append((pos, pos + m))
            # a push enqueues nothing exactly when none of its samples belongs to a kept vector
            assert (ops == 0) == (not real), (len(tickets), pos, m, ops)
            if real:
                used.add(t % KRING)
            pos += m
        assert checked or not busy
        ch.wait(tickets[-1])
        per_push = kept_per_push(bounds, N, kept)
        rows, state = oracle_rows(form, x, N, decim)
        assert len(kept) == len(rows)
        got = {}
        for i in range(len(tickets) - KRING, len(tickets)):      # every ticket still in the ring
            n, last = per_push[i]
            assert ch.ticket_rows(tickets[i]) == n, (i, n)
            row, k = ch.wait(tickets[i])
            assert k == n
            if n:
                check_row(form, row, rows[last])
                got[i] = row.copy()
            else:
                assert row is None
        if form == 'psd_logger':
            final = ch.peak()
            assert relerr(final, state[-1]) < RTOL
        elif form == 'local_worker':
            final = ch.iir()
            assert relerr(final, state[-1]) < RTOL
        else:
            final = None
        return got, final
    finally:
        if busy:
            hog.finish(probe)
        ch.close()


def same_state(a, b):
    (ra, fa), (rb, fb) = a, b
    assert sorted(ra) == sorted(rb)
    for i in ra:
        assert np.array_equal(ra[i], rb[i]), i
    assert (fa is None) == (fb is None)
    if fa is not None:
        assert np.array_equal(fa, fb)


@pytest.mark.parametrize('name', PATTERNS)
@pytest.mark.parametrize('N', [1024, 4096, 16384, 1000])
@pytest.mark.parametrize('form', ['psd_logger', 'local_worker', 'spectrum_sensor_v2'])
def test_push_async_behind_a_busy_stream(ctx, hip, hog, form, N, name):
    idle = run_pushes(ctx, hip, hog, form, N, name, False)
    busy = run_pushes(ctx, hip, hog, form, N, name, True)
    same_state(busy, idle)


@pytest.mark.parametrize('name', PATTERNS)
def test_push_async_behind_a_busy_stream_coverage_kernel(ctx, hip, hog, name):
    idle = run_pushes(ctx, hip, hog, 'psd_logger', 4096, name, False, hip.KERNEL_GENERIC)
    busy = run_pushes(ctx, hip, hog, 'psd_logger', 4096, name, True, hip.KERNEL_GENERIC)
    same_state(busy, idle)


# ---- set_keep_one_in_n in mid-stream, row by row -------------------------------------------------------------

SET_N_CASES = {
    # keep 7, 700-item pushes, set_n(2) once 4900 items are in (the case of the old loose check)
    'set_n2_at_4900': (7, 700, [(4900, 2)]),
    # keep 7: vector 2 (items 2048-3071) is partial after the push ending at 2100 and, under n = 7, a dropped one - its
    # first samples were skipped; set_n(1) makes it a kept vector
    'set_n1_stale_partial': (7, 700, [(2100, 1)]),
    # keep 4: two partial pushes of vector 1 (items 1024-2047) with set_n(1) between them, then set_n(3) between two
    # partial pushes of vector 5 (items 5120-6143)
    'set_n_between_partials': (4, 700, [(1400, 1), (5600, 3)]),
}


@pytest.mark.parametrize('form', ['spectrum_sensor_v2', 'psd_logger'])
@pytest.mark.parametrize('how', ['push_async', 'push', 'push_dev', 'mixed', 'mixed_dev'])
@pytest.mark.parametrize('case', sorted(SET_N_CASES))
def test_set_keep_one_in_n_mid_stream_row_by_row(ctx, hip, case, how, form):
    """'mixed': push_async up to the first set_n call, push after it - the blocking form then uploads the samples the
    dropped asynchronous pushes kept on the host.  'mixed_dev': push_async up to the first set_n call, then push_dev and
    push_async in turn - push_dev uploads those samples without waiting, and a dropped push_async after it waits for
    that copy before it reuses the host buffer."""
    N = 1024
    decim, step, schedule = SET_N_CASES[case]
    x = R.synth_iq(20 * N, 61)
    at = dict(schedule)
    kept = R.gr_kept_indices(len(x) // N, N, decim, schedule)
    rows, state = oracle_rows(form, x, N, decim, schedule)
    ch = make_chain(ctx, hip, form, N, decim)
    cap = step // N + 2
    d_rows = ctx.alloc(cap * N * 4) if how in ('push_dev', 'mixed_dev') else None
    d_x = ctx.alloc(len(x) * 8) if how in ('push_dev', 'mixed_dev') else None
    try:
        if d_x:
            ctx.h2d(d_x, x)
        got, nrows = [], 0
        for pos in range(0, len(x), step):
            if pos in at:
                ch.set_keep_one_in_n(at[pos])
            end = min(pos + step, len(x))
            n_want, last = kept_per_push([(pos, end)], N, kept)[0]
            mode = how
            if how in ('mixed', 'mixed_dev'):
                after = ('push_dev', 'push_async')[(pos // step) % 2] if how == 'mixed_dev' else 'push'
                mode = 'push_async' if pos < schedule[0][0] else after
            if mode == 'push_async':
                t = ch.push_async(x[pos:end])
                assert ch.ticket_rows(t) == n_want, pos
                row, k = ch.wait(t)
                assert k == n_want, pos
                if k:
                    check_row(form, row, rows[last])
                    got.append(last)
            elif mode == 'push':
                r, k = ch.push(x[pos:end])
                assert k == n_want and len(r) == k, pos
                for j, row in enumerate(r):
                    check_row(form, row, rows[last - k + 1 + j])
                    got.append(last - k + 1 + j)
            else:
                k = ch.push_dev(d_x + pos * 8, end - pos, d_rows, cap)
                assert k == n_want, pos
                if k:
                    r = ctx.d2h(d_rows, (k, N), np.float32)
                    for j, row in enumerate(r):
                        check_row(form, row, rows[last - k + 1 + j])
                        got.append(last - k + 1 + j)
            nrows += k
        assert nrows == len(kept)
        assert got == list(range(len(kept)))      # (step < N: a push completes one vector at most)
        if form == 'psd_logger':
            assert relerr(ch.peak(), state[-1]) < RTOL
    finally:
        ch.close()
        if d_x:
            ctx.free(d_x)
            ctx.free(d_rows)


def test_local_worker_set_rate_mid_stream(ctx):
    """local_worker.set_rate at run time (local_worker.py set_rate / set_sample_rate -> set_keep_one_in_n): the rows the
    block emits and its IIR state against the scheduled oracle, including a vector that was partial - and dropped under
    the old rate - when the rate changed."""
    import ofdm_tools
    N, Sf = 1024, 1024 * 1000
    blk = ofdm_tools.local_worker(N, Sf, ALPHA, 125, 1472, True, ctx=ctx, threaded=False)
    assert blk._decimation() == 8
    seen = []
    blk._on_vector = lambda r: seen.append(r.copy())
    x = R.synth_iq(40 * N, 62)
    step, at = 1500, {3000: 1000, 19500: 250}       # -> keep 1 (vector 2 is partial and was a dropped one), then keep 4
    schedule = []
    for pos in range(0, len(x), step):
        if pos in at:
            blk.set_rate(at[pos])
            schedule.append((pos, blk._decimation()))
        assert blk.work([x[pos:pos + step]], []) == len(x[pos:pos + step])
    assert [n for _, n in schedule] == [1, 4]
    kept = R.gr_kept_indices(len(x) // N, N, 8, schedule)
    lin, _ = R.chain_local_worker(x, N, Sf, ALPHA, 8, schedule)
    k = -10 * math.log10(N) - 10 * math.log10(Sf)
    want = [last for n, last in kept_per_push([(p, min(p + step, len(x))) for p in range(0, len(x), step)], N, kept) if n]
    assert blk.rows_total == len(kept) and len(seen) == len(want)
    for row, i in zip(seen, want):
        assert relerr(10 ** ((row.astype(np.float64) - k) / 10), lin[i]) < RTOL, i
    assert relerr(blk._chain.iir(), lin[-1]) < RTOL
    blk.stop()


# ---- SpectrumScan: many scans of one shape in flight ---------------------------------------------------------

@pytest.mark.parametrize('method', ['welch', 'fft'])
def test_ten_spectrum_scans_of_one_shape_in_flight(ctx, hog, method):
    """Ten SpectrumScans of one shape created back to back behind the hog (what ten legacy sensors on the default
    context do): each collects its own vector's result - half with wait() in reverse order, half by polling - equal to
    a blocking fast_spectrum_scan of the same vector."""
    from ofdm_tools import ofdm_cr_tools as T
    Sf, N = 1000000, 1024
    vecs = [R.synth_iq(8192, 500 + i) for i in range(10)]
    args = (0, 50e3, 25e3, N, Sf, method, 5)
    want = [T.fast_spectrum_scan(v, *(args + (1e-11, 0.5)), ctx=ctx) for v in vecs]      # (builds the shape's plan)
    probe = hog.start()
    try:
        scans = []
        for i, v in enumerate(vecs):
            if i == KRING:
                assert hog.busy(probe), 'the stream drained before the fifth scan was enqueued: the hog is too short'
            scans.append(T.SpectrumScan(v, *(args + (0.5,)), ctx=ctx))
        got = {}
        for i in reversed(range(5)):
            got[i] = scans[i].wait(1e-11)
        end = time.monotonic() + 30.0
        while len(got) < 10 and time.monotonic() < end:
            for i in range(5, 10):
                if i not in got:
                    r = scans[i].poll(1e-11)
                    if r is not None:
                        got[i] = r
            time.sleep(0.0005)
        assert len(got) == 10
    finally:
        hog.finish(probe)
    for i in range(10):
        assert got[i][0] == want[i][0] and got[i][2] == want[i][2], (method, i)
        assert list(got[i][1]) == list(want[i][1]) and got[i][3] == want[i][3], (method, i)
