"""The op table of the call-order suites (test_call_order_cpu.py / test_call_order_gpu.py) - a plain module, no fixtures.

A plan has about thirty entry points that all write through the same few holders of csrc/abi_state.h ("Who
writes what on a plan").  A row of OPS is one way to call a plan: which plan kinds take it, the entry points it goes
through, a function (env, plan, inputs, dev) -> (tuple of arrays, segment count), and its inputs at two sizes - SMALL = 3
and LARGE = 11 segments, so that in a small-first order every workspace regrows at least once.  The GPU suite runs every
row alone on a fresh plan (the solo) and in seeded orders on one shared plan, and asks for the same bytes.

Plans are described by a Shape and made by build(): the Welch plans through stat_support.welch_plan (Hann, constant
detrend, density), the multitaper ones through ctx.mtm_plan / ctx.mtm_csd_plan, each with every table of its Tables set
and the schedule forced to contiguous runs - a static schedule sums in one order, so a solo repeats bit for bit."""
import collections
import functools

import numpy as np

from oracle import ref_cpu as R
from stat_support import FS, welch_plan

SMALL, LARGE = 3, 11
SIZES = (SMALL, LARGE)
SENTINEL = 0x7fc5a5a5      # a quiet NaN with a payload no kernel writes: what the test's own device rows hold before a call
GUARD = 64                 # floats behind every device row of the test's own: still the sentinel after the call

Shape = collections.namedtuple('Shape', 'kind nfft noverlap fftshift trim db nw ntapers')
# the tables a plan carries: cycle frequencies, lags, taps per branch of the prototype, (directions, channels, seed, fc) of the
# steering table, and the exponent applied to a multitaper plan's own concentration ratios (1: as the plan computed them)
Tables = collections.namedtuple('Tables', 'name cycles lags ntaps steer ratio_pow')

TABLES_A = Tables('A', (0.0, 0.0123456789, -0.37), (0, 3, 37), 4, (24, 4, 11, 0.0), 1.0)
# another length each; the steering table also another channel count and, 24 -> 40 -> 24, a direction count that crosses one
# direction tile of 32 both ways
TABLES_B = Tables('B', (0.25, -0.0123456789, 0.0, 1.0 / 80.0, 0.5), (5, 0, 64, 1, 100), 8, (40, 3, 12, 0.125), 2.0)


def welch_shape(nfft, fftshift=False, trim=0, db=False):
    return Shape('welch', nfft, nfft // 2, fftshift, trim, db, 0.0, 0)


WELCH_SHAPES = tuple(welch_shape(n) for n in (64, 1024, 4096, 16384)) + (welch_shape(1024, True, 100, True),)
MTM_SHAPES = (Shape('mtm', 256, 0, False, 0, False, 4.0, 7), Shape('mtm', 16384, 0, False, 0, False, 2.5, 4),
              Shape('mtmcsd', 1024, 0, False, 0, False, 3.0, 5), Shape('mtmcsd', 16384, 0, False, 0, False, 2.5, 4))


def shape_id(s):
    return '%s%d%s' % (s.kind, s.nfft, '-shift-trim-db' if s.db else '')


def step(shape):
    return shape.nfft - shape.noverlap


def steering(tables):
    D, C, seed, _ = tables.steer
    return np.random.default_rng(seed).uniform(-3.0, 3.0, (D, C))


def ratios_for(plan, tables):
    """the plan's own concentration ratios (as its constructor clips them) to the power of the table set"""
    return np.clip(np.asarray(plan_ratios(plan), np.float64), np.finfo(np.float64).tiny, 1.0) ** tables.ratio_pow


def plan_ratios(plan):
    if not hasattr(plan, '_own_ratios'):
        plan._own_ratios = np.array(plan.ratios, np.float64)
    return plan._own_ratios


# table setter -> (how to apply it to a plan, the plan kinds that take it, the ops that read the table)
SETTERS = {
    'set_cycles': (lambda plan, shape, t: plan.set_cycles(t.cycles), ('welch',), ('cyclic', 'cyclic_dev')),
    'set_lags': (lambda plan, shape, t: plan.set_lags(list(t.lags)), ('welch',), ('caf', 'caf_dev')),
    'set_prototype': (lambda plan, shape, t: plan.set_prototype(prototype(shape.nfft, t.ntaps)), ('welch',), ('pfb', 'pfb_dev')),
    'set_steering': (lambda plan, shape, t: plan.set_steering(steering(t), t.steer[3]), ('welch',), ('matrix_doa', 'matrix_doa_dev')),
    'set_ratios': (lambda plan, shape, t: plan.set_ratios(ratios_for(plan, t)), ('mtm', 'mtmcsd'), ('adaptive', 'adaptive_dev')),
}


@functools.lru_cache(maxsize=None)
def prototype(nfft, ntaps):
    from ofdm_tools import windows
    h = windows.pfb_prototype(nfft, ntaps)
    h.setflags(write=False)
    return h


def build(ctx, hip, shape, tables=TABLES_A, contiguous=True):
    """A fresh plan of `shape` with every table of `tables` set and - unless the caller sets a schedule of its own - the
    schedule forced to contiguous runs.  The shared plan and every solo come from here, so they are set up alike."""
    if shape.kind == 'welch':
        plan = welch_plan(ctx, hip, shape.nfft, shape.nfft, shape.noverlap, True, 'density', shape.fftshift, shape.trim, shape.db)
    else:
        make = ctx.mtm_plan if shape.kind == 'mtm' else ctx.mtm_csd_plan
        plan = make(shape.nfft, noverlap=shape.noverlap, nw=shape.nw, ntapers=shape.ntapers, fs=FS, fftshift=shape.fftshift,
                    trim_bins=shape.trim, db=shape.db)
    for name in sorted(SETTERS):
        apply, kinds, _ = SETTERS[name]
        if shape.kind in kinds:
            apply(plan, shape, tables)
    if contiguous:
        plan.set_schedule(hip.SCHED_CONTIGUOUS)
        plan.set_tuning(None, sched=hip.SCHED_CONTIGUOUS)
    return plan


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def nsamples(shape, M, extra=0):
    """M segments and a third of a step more (a ragged end), `extra` samples in front of the count"""
    return shape.noverlap + M * step(shape) + step(shape) // 3 + extra


def seed(shape, M, k=0):
    return 1000003 * k + 31 * shape.nfft + M + (7 if shape.db else 0)


def _ro(a):
    a.setflags(write=False)
    return a


def in_stream(shape, M, tables):
    return dict(x=_ro(R.synth_iq(nsamples(shape, M), seed(shape, M))))


def in_pair(shape, M, tables):
    n = nsamples(shape, M)
    x = R.synth_iq(n, seed(shape, M, 1), dc=2 - 1j)
    y = (0.7 * np.roll(x, 5) + 0.5 * R.synth_iq(n, seed(shape, M, 2), tones=(), dc=0.5 + 0.25j)).astype(np.complex64)
    return dict(x=_ro(x), y=_ro(y))


def in_streams(count):
    def make(shape, M, tables):
        n = nsamples(shape, M)
        stride = n + 37      # a padded stride
        buf = np.zeros(count * stride, np.complex64)
        for i in range(count):
            buf[i * stride:i * stride + n] = R.synth_iq(n, seed(shape, M, 3 + i), dc=(0.0, 3 - 2j, -1 + 4j)[i % 3])
        return dict(buf=_ro(buf), n=n, stride=stride, count=count)
    return make


def in_caf(shape, M, tables):
    return dict(x=_ro(R.synth_iq(nsamples(shape, M, max(tables.lags)), seed(shape, M, 7))))


def in_pfb(shape, M, tables):
    """M frames: a frame spans ntaps * nfft samples, one every step"""
    return dict(x=_ro(R.synth_iq(tables.ntaps * shape.nfft + (M - 1) * step(shape) + step(shape) // 3, seed(shape, M, 8))))


def in_channels(count):
    def make(shape, M, tables):
        from test_welch_matrix_gpu import capture
        C = tables.steer[1] if count is None else count
        return dict(x=_ro(capture(C, nsamples(shape, M), seed(shape, M, 9 + C), shape.nfft, M)))
    return make


def segments_of(op, shape, inp, tables):
    """The segment count the library is to report for the row's inputs, from the lengths alone."""
    if 'buf' in inp:
        n = inp['n']
    else:
        n = inp['x'].shape[-1]
    if op.make is in_caf:
        n -= max(tables.lags)
    if op.make is in_pfb:
        return (n - tables.ntaps * shape.nfft) // step(shape) + 1
    return (n - shape.noverlap) // step(shape)


@functools.lru_cache(maxsize=None)
def inputs(op_name, shape, M, tables=TABLES_A):
    return BY_NAME[op_name].make(shape, M, tables)


# ---- device rows of the test's own ------------------------------------------------------------------------------------------

class Dev(object):
    """Device buffers of one call: inputs uploaded, output rows pre-filled with SENTINEL and followed by GUARD floats of it.
    get() reads a row back and asserts that the call wrote all of it and nothing behind it."""

    def __init__(self, ctx):
        self.ctx, self.ptrs, self.sizes = ctx, [], {}

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.alloc(arr.nbytes)
        self.ptrs.append(p)
        self.ctx.h2d(p, arr)
        return p

    def out(self, nfloats):
        p = self.put(np.full(nfloats + GUARD, SENTINEL, np.uint32))
        self.sizes[p] = nfloats
        return p

    def get(self, p, shape, dtype=np.float32):
        words = self.ctx.d2h(p, (self.sizes[p] + GUARD,), np.uint32)
        row, guard = words[:self.sizes[p]], words[self.sizes[p]:]
        assert np.all(guard == SENTINEL), 'the call wrote behind its row'
        assert not np.any(row == SENTINEL), 'the call left %d words of its row unwritten' % int(np.sum(row == SENTINEL))
        return row.view(dtype).reshape(shape)

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


# ---- the ops --------------------------------------------------------------------------------------------------------------------

def op_exec(env, plan, i, dev):
    return (plan.exec(i['x']),), plan.last_nseg


def op_exec_device_src(env, plan, i, dev):
    return (plan.exec_device_src(dev.put(i['x']), len(i['x'])),), plan.last_nseg


def op_exec_dev(env, plan, i, dev):
    o = dev.out(i['count'] * plan.out_len)
    nseg = plan.exec_dev(dev.put(i['buf']), i['n'], o, nstreams=i['count'], stream_stride=i['stride'])
    return (dev.get(o, (i['count'], plan.out_len)),), nseg


def op_exec_async(env, plan, i, dev):
    return (plan.wait(plan.exec_async(i['x'])),), plan.last_nseg


def op_exec_async_poll(env, plan, i, dev):
    t = plan.exec_async(i['x'])
    env.ctx.sync()      # the stream has drained: one look finds the row
    out = plan.poll(t)
    assert out is not None
    return (out,), plan.last_nseg


def halves(plan, n, M):
    """(first sample, samples) of two time chunks that share M segments: M // 2 and the rest"""
    k = M // 2
    return (0, plan.noverlap + k * plan.step), (k * plan.step, n - k * plan.step)


def op_partial_scale(env, plan, i, dev):
    x = i['x']
    d_in, nfft = dev.put(x), plan.nfft
    total, nseg = np.zeros(nfft, np.float32), 0
    for first, count in halves(plan, len(x), plan.nseg(len(x))):
        d_sum = dev.out(nfft)
        nseg += plan.partial_dev(d_in + 8 * first, count, d_sum)
        total += dev.get(d_sum, (nfft,))      # (float32 + float32: one rounding, the same in every run)
    o = dev.out(plan.out_len)
    plan.scale_dev(dev.put(total), nseg, o)
    return (dev.get(o, (plan.out_len,)),), nseg


def ragged_chunks(plan, n):
    """three chunks, the first shorter than a segment, none on a segment boundary"""
    a = plan.nperseg // 3
    b = a + plan.nperseg + 5
    assert 0 < a < plan.nperseg and b < n
    return (0, a), (a, b), (b, n)


def op_accumulate(env, plan, i, dev):
    plan.reset()
    for lo, hi in ragged_chunks(plan, len(i['x'])):
        plan.accumulate(i['x'][lo:hi])
    return (plan.finalize(),), plan.last_nseg


def op_segments(env, plan, i, dev):
    rows = plan.segments(i['x'])
    return (rows,), rows.shape[0]


def op_median(env, plan, i, dev):
    plan.set_average('median')
    try:
        return (plan.exec(i['x']),), plan.last_nseg
    finally:
        plan.set_average('mean')


def op_csd(env, plan, i, dev):
    return plan.csd(i['x'], i['y']), plan.last_nseg


def op_csd_dev(env, plan, i, dev):
    m = plan.out_len
    rows = [dev.out(k * m) for k in (1, 1, 2, 1)]
    nseg = plan.csd_exec_dev(dev.put(i['x']), dev.put(i['y']), len(i['x']), *rows)
    return tuple(dev.get(p, (k * m,)) for p, k in zip(rows, (1, 1, 2, 1))), nseg


def op_csd_partial_scale(env, plan, i, dev):
    x, m, nfft = i['x'], plan.out_len, plan.nfft
    dx, dy = dev.put(x), dev.put(i['y'])
    total, nseg = np.zeros(4 * nfft, np.float32), 0
    for first, count in halves(plan, len(x), plan.nseg(len(x))):
        d_sum = dev.out(4 * nfft)
        nseg += plan.csd_partial_dev(dx + 8 * first, dy + 8 * first, count, d_sum)
        total += dev.get(d_sum, (4 * nfft,))
    rows = [dev.out(k * m) for k in (1, 1, 2, 1)]
    plan.csd_scale_dev(dev.put(total), nseg, *rows)
    return tuple(dev.get(p, (k * m,)) for p, k in zip(rows, (1, 1, 2, 1))), nseg


def op_sk(env, plan, i, dev):
    return plan.sk(i['x'], return_psd=True), plan.last_nseg


def _rows_dev(call, dev, i, plan, widths):
    """a _dev form over the streams of i: call(d_in, n, count, stride, *rows) -> the rows [count, width]"""
    rows = [dev.out(i['count'] * w) for w in widths]
    nseg = call(dev.put(i['buf']), i['n'], i['count'], i['stride'], *rows)
    return tuple(dev.get(p, (i['count'], w)) for p, w in zip(rows, widths)), nseg


def op_sk_dev(env, plan, i, dev):
    return _rows_dev(plan.sk_dev, dev, i, plan, (plan.out_len, plan.out_len))


def op_cyclic(env, plan, i, dev):
    return plan.cyclic(i['x'], return_psd=True), plan.last_nseg


def op_cyclic_dev(env, plan, i, dev):
    A, m = plan.ncycles, plan.out_len
    call = lambda d, n, ns, stride, coh, scf, psd: plan.cyclic_dev(d, n, ns, stride, coh, scf_dev=scf, psd_dev=psd)      # noqa: E731
    return _rows_dev(call, dev, i, plan, (A * m, 2 * A * m, m))


def op_caf(env, plan, i, dev):
    return plan.caf(i['x'], return_r=True), plan.last_nseg


def op_caf_dev(env, plan, i, dev):
    x, L, m = i['x'], plan.nlags, plan.out_len
    caf, r = dev.out(L * m), dev.out(2 * L)
    nseg = plan.caf_dev(dev.put(x), len(x), 1, len(x), caf, r)
    return (dev.get(caf, (L, m)), dev.get(r, (2 * L,))), nseg


def op_pfb(env, plan, i, dev):
    return (plan.pfb(i['x']),), plan.last_nseg


def op_pfb_dev(env, plan, i, dev):
    x, o = i['x'], dev.out(plan.out_len)
    nseg = plan.pfb_dev(dev.put(x), len(x), 1, len(x), o)
    return (dev.get(o, (plan.out_len,)),), nseg


def op_matrix(env, plan, i, dev):
    return plan.matrix(i['x']), plan.last_nseg


def op_matrix_dev(env, plan, i, dev):
    (C, n), m = i['x'].shape, plan.out_len
    s, g = dev.out(C * (C + 1) * m), dev.out(m)
    nseg = plan.matrix_dev(dev.put(i['x']), n, C, n, s, g)
    return (dev.get(s, (C * (C + 1) // 2, 2 * m)), dev.get(g, (m,))), nseg


def op_matrix_eig(env, plan, i, dev):
    return plan.matrix_eig(i['x'], of='G', return_vector=True), plan.last_nseg


def op_matrix_eig_dev(env, plan, i, dev):
    (C, n), m = i['x'].shape, plan.out_len
    e, v = dev.out(C * m), dev.out(2 * C * m)
    nseg = plan.matrix_eig_dev(dev.put(i['x']), n, C, n, 'G', e, v)
    return (dev.get(e, (C, m)), dev.get(v, (C, 2 * m))), nseg


DOA = dict(of='S', nsrc=1, loading=1e-2)


def op_matrix_doa(env, plan, i, dev):
    rows = plan.matrix_doa(i['x'], **DOA)
    return tuple(rows[k] for k in plan.DOA_METHODS), plan.last_nseg


def op_matrix_doa_dev(env, plan, i, dev):
    (C, n), D, m = i['x'].shape, plan.ndir, plan.out_len
    rows = [dev.out(D * m) for _ in range(3)]
    nseg = plan.matrix_doa_dev(dev.put(i['x']), n, C, n, DOA['of'], DOA['nsrc'], DOA['loading'], *rows)
    return tuple(dev.get(p, (D, m)) for p in rows), nseg


GCC_MAXLAG = 31


def gcc_args(hip, plan):
    """upsample=2 wherever the interpolated transform fits (upsample * nfft <= GCC_POINTS_MAX: not at 16384 points)"""
    return dict(weighting='phat', upsample=2 if 2 * plan.nfft <= hip.GCC_POINTS_MAX else 1, maxlag=GCC_MAXLAG)


def op_matrix_gcc(env, plan, i, dev):
    return plan.matrix_gcc(i['x'], return_rows=True, **gcc_args(env.hip, plan)), plan.last_nseg


def op_matrix_gcc_dev(env, plan, i, dev):
    C, n = i['x'].shape
    pairs, width = C * (C - 1) // 2, 2 * GCC_MAXLAG + 1
    g, pk = dev.out(2 * pairs * width), dev.out(3 * pairs)
    nseg = plan.matrix_gcc_dev(dev.put(i['x']), n, C, n, gcc_dev=g, peak_dev=pk, **gcc_args(env.hip, plan))
    return (dev.get(g, (pairs, 2 * width)), dev.get(pk, (pairs, 3))), nseg


def op_adaptive(env, plan, i, dev):
    return plan.adaptive(i['x'], return_dof=True), plan.last_nseg


def op_adaptive_dev(env, plan, i, dev):
    return _rows_dev(plan.adaptive_dev, dev, i, plan, (plan.out_len, plan.out_len))


def op_ftest(env, plan, i, dev):
    return plan.ftest(i['x'], return_rows=True), plan.last_nseg


def op_ftest_dev(env, plan, i, dev):
    return _rows_dev(plan.ftest_dev, dev, i, plan, (plan.out_len,) * 3)


def op_jackknife(env, plan, i, dev):
    return plan.jackknife(i['x'], return_psd=True), plan.last_nseg


def op_jackknife_dev(env, plan, i, dev):
    return _rows_dev(plan.jackknife_dev, dev, i, plan, (plan.out_len, plan.out_len))


def op_csd_jackknife(env, plan, i, dev):
    return plan.csd_jackknife(i['x'], i['y']), plan.last_nseg


def op_csd_jackknife_dev(env, plan, i, dev):
    rows = [dev.out(plan.out_len) for _ in range(4)]      # zsd, cxy, lnsd x, lnsd y
    nseg = plan.csd_jackknife_dev(dev.put(i['x']), dev.put(i['y']), len(i['x']), *rows)
    return tuple(dev.get(p, (plan.out_len,)) for p in rows), nseg


# name, the plan kinds that take it, the entry points it goes through, the call, its inputs; linear: refused on a dB plan (the
# cross spectrum has no dB); streaming: it is the accumulate / finalize form itself
Op = collections.namedtuple('Op', 'name kinds entries run make linear streaming')
ALL, WELCH, MTM, MTMCSD, TWO = ('welch', 'mtm', 'mtmcsd'), ('welch',), ('mtm', 'mtmcsd'), ('mtmcsd',), ('welch', 'mtmcsd')


def _op(name, kinds, entries, run, make, linear=False, streaming=False):
    return Op(name, kinds, tuple(entries.split()), run, make, linear, streaming)


OPS = (
    _op('exec', ALL, 'oth_welch_exec', op_exec, in_stream),
    _op('exec_device_src', ALL, 'oth_welch_exec', op_exec_device_src, in_stream),
    _op('exec_dev', ALL, 'oth_welch_exec_dev', op_exec_dev, in_streams(3)),
    _op('exec_async', ALL, 'oth_welch_exec_async oth_welch_wait', op_exec_async, in_stream),
    _op('exec_async_poll', ALL, 'oth_welch_exec_async oth_welch_poll', op_exec_async_poll, in_stream),
    _op('partial_scale', ALL, 'oth_welch_partial_dev oth_welch_scale_dev', op_partial_scale, in_stream),
    _op('accumulate', ALL, 'oth_welch_reset oth_welch_accumulate oth_welch_finalize', op_accumulate, in_stream, streaming=True),
    _op('segments', WELCH, 'oth_welch_segments_dev', op_segments, in_stream),
    _op('median', WELCH, 'oth_plan_set_average oth_welch_exec', op_median, in_stream),
    _op('csd', TWO, 'oth_csd_exec', op_csd, in_pair, linear=True),
    _op('csd_dev', TWO, 'oth_csd_exec_dev', op_csd_dev, in_pair, linear=True),
    _op('csd_partial_scale', TWO, 'oth_csd_partial_dev oth_csd_scale_dev', op_csd_partial_scale, in_pair, linear=True),
    _op('sk', WELCH, 'oth_welch_sk', op_sk, in_stream),
    _op('sk_dev', WELCH, 'oth_welch_sk_dev', op_sk_dev, in_streams(2)),
    _op('cyclic', WELCH, 'oth_welch_cyclic', op_cyclic, in_stream),
    _op('cyclic_dev', WELCH, 'oth_welch_cyclic_dev', op_cyclic_dev, in_streams(2)),
    _op('caf', WELCH, 'oth_welch_caf', op_caf, in_caf),
    _op('caf_dev', WELCH, 'oth_welch_caf_dev', op_caf_dev, in_caf),
    _op('pfb', WELCH, 'oth_welch_pfb', op_pfb, in_pfb),
    _op('pfb_dev', WELCH, 'oth_welch_pfb_dev', op_pfb_dev, in_pfb),
    _op('matrix', WELCH, 'oth_welch_matrix', op_matrix, in_channels(3)),
    _op('matrix_dev', WELCH, 'oth_welch_matrix_dev', op_matrix_dev, in_channels(3)),
    _op('matrix_eig', WELCH, 'oth_welch_matrix_eig', op_matrix_eig, in_channels(5)),
    _op('matrix_eig_dev', WELCH, 'oth_welch_matrix_eig_dev', op_matrix_eig_dev, in_channels(5)),
    _op('matrix_doa', WELCH, 'oth_welch_matrix_doa', op_matrix_doa, in_channels(None)),
    _op('matrix_doa_dev', WELCH, 'oth_welch_matrix_doa_dev', op_matrix_doa_dev, in_channels(None)),
    _op('matrix_gcc', WELCH, 'oth_welch_matrix_gcc', op_matrix_gcc, in_channels(3)),
    _op('matrix_gcc_dev', WELCH, 'oth_welch_matrix_gcc_dev', op_matrix_gcc_dev, in_channels(3)),
    _op('adaptive', MTM, 'oth_mtm_adaptive', op_adaptive, in_stream),
    _op('adaptive_dev', MTM, 'oth_mtm_adaptive_dev', op_adaptive_dev, in_streams(2)),
    _op('ftest', MTM, 'oth_mtm_ftest', op_ftest, in_stream),
    _op('ftest_dev', MTM, 'oth_mtm_ftest_dev', op_ftest_dev, in_streams(2)),
    _op('jackknife', MTM, 'oth_mtm_jackknife', op_jackknife, in_stream),
    _op('jackknife_dev', MTM, 'oth_mtm_jackknife_dev', op_jackknife_dev, in_streams(2)),
    _op('csd_jackknife', MTMCSD, 'oth_mtm_csd_jackknife', op_csd_jackknife, in_pair),
    _op('csd_jackknife_dev', MTMCSD, 'oth_mtm_csd_jackknife_dev', op_csd_jackknife_dev, in_pair),
)
BY_NAME = {op.name: op for op in OPS}
assert len(BY_NAME) == len(OPS)

# Entry points that take a plan and are no row of the table: they compute nothing.
NOT_OPS = (
    'oth_plan_destroy',                # the destructor: every solo ends with it
    'oth_plan_out_len',                # read once by the binding's constructor
    'oth_plan_set_output_db', 'oth_plan_set_kernel', 'oth_plan_set_schedule', 'oth_plan_set_hostwait', 'oth_plan_set_tuning',
    # the table setters: build() calls each on every plan, test_a_replaced_table_* replaces them between calls
    'oth_welch_set_cycles', 'oth_welch_set_lags', 'oth_welch_set_prototype', 'oth_welch_set_steering', 'oth_mtm_set_ratios',
    'oth__debug_last_recipe',          # read after every op: the recipe string is part of what is compared
)


def ops_for(shape, streaming=True):
    """the rows a plan of `shape` takes, in the table's order"""
    return tuple(op for op in OPS if shape.kind in op.kinds and not (op.linear and shape.db) and (streaming or not op.streaming))


def pairs_for(shape):
    return [(op.name, M) for op in ops_for(shape) for M in SIZES]


def orders(shape, seed_):
    """the three orders of the issue: large-first, small-first, and one seeded shuffle of all (op, size) pairs run twice back
    to back -> [(name of the order, [(op, M), ...])]"""
    names = [op.name for op in ops_for(shape)]
    shuffled = pairs_for(shape)
    np.random.default_rng(seed_).shuffle(shuffled)
    shuffled = [tuple(p) for p in shuffled]
    return [('large-first', [(n, LARGE) for n in names] + [(n, SMALL) for n in names]),
            ('small-first', [(n, SMALL) for n in names] + [(n, LARGE) for n in names]),
            ('shuffle seed %d, twice' % seed_, [(n, int(M)) for n, M in shuffled] * 2)]


# ---- section 4: the inputs of the ticketed launches -------------------------------------------------------------------------

TICKET_M = {4096: 40, 1024: 100, 8192: 56}      # segments per stream, by the plan's length: 40 ... 200, and few enough that one shows (test_call_order_cpu)
TICKET_STREAMS = (1, 3, 64)
TICKET_CSD_M = 40      # ... and of the two-channel launch; its channels share a third of their power (coherence near 1 / 3: where a segment moves it most)


@functools.lru_cache(maxsize=None)
def ticket_stream(nfft, k):
    """stream k of the ticketed launches of the nfft-point plan (50 % overlap): unit noise, R.synth_iq's tones, an offset"""
    n = nfft // 2 + TICKET_M[nfft] * (nfft // 2)
    return _ro(R.synth_iq(n, 5000 + 17 * nfft + k, dc=(0.0, 2 - 1j, -3 + 0.5j)[k % 3]))


@functools.lru_cache(maxsize=None)
def ticket_pair():
    n = 2048 + TICKET_CSD_M * 2048 + 700
    x = R.synth_iq(n, 6001, dc=2 - 1j)
    y = (0.5 * np.roll(x, 5) + 0.7 * R.synth_iq(n, 6002, tones=(), dc=0.5 + 0.25j)).astype(np.complex64)
    return _ro(x), _ro(y)
