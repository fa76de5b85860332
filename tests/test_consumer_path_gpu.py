"""The consumer loop of the role-split 4096-point kernels (welch4096ws, csd4096ws) on the edges its control flow has:
segment -> segment (the data path: pass 2 at the end of the loop body), segment -> idle step -> segment (pass 2 on the
idle exit), segment -> idle step -> stop, and segment -> stop.  The producer idles in one place only: under the dynamic
schedule (tickets) behind a one-segment chunk.

The schedule is FORCED through set_tuning(variant, sched=..., chunk=...): set_schedule() alone leaves the choice to the
library, which runs launches this short as contiguous runs.  The grid is min(resident workgroups, segments), so a workgroup
sees more than one segment - and the ticket queue more than one chunk per workgroup - only when the launch has several
times as many segments as there are resident workgroups (512 per stream on MI355X; 256 for csd4096ws): 3001 segments here
(1031 segment pairs), where the dynamic schedule with one-segment chunks makes every workgroup alternate segment and idle
step and end on idle step -> stop, and with two-segment chunks (one-segment tail chunks) mixes all four edges.  Every
case reads the launch's recipe back and asserts the kernel, the schedule and the chunk size that really ran, and for the
large counts that every workgroup had more than two chunks to draw.  The issue's small counts (1 ... 33 segments: one
segment per workgroup, segment -> stop only) stay alongside.

4096-point periodic Hann, constant detrend, the forced complementary ('ws') and general ('wsgen') builds; one stream (DC
offset 0 and 40 sigma) and three streams in one launch (0, 40 and 40 sigma at another phase).  Every output is compared with
the float64 oracle: from eight segments on at the project's gate, 1e-4 relative on every bin; below that - where the plan
would not pick these builds - at the few-segment gate of test_compl_window_gpu.py (5e-5 against max(bin, median / 10)).
The static schedules are run twice and must repeat bit for bit.

The two-channel kernel runs the same chunk and schedule set on two different channels, 1e-4 on Pxx, Pyy, Pxy, Im Pxy
(relative to sqrt(Pxx Pyy)) and Cxy.
"""
import functools

import numpy as np
import pytest

import csd_oracle as O
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

RTOL = 1e-4
FEW = 5e-5
NSEG = (1, 2, 3, 8, 9, 33, 3001)
SCHED_NAME = {0: 'contiguous', 1: 'interleaved', 2: 'dynamic'}
DCS = (0.0, 40.0 * np.exp(0.54j), 40.0 * np.exp(-2.1j))      # in units of the noise's sigma (= 1)


@pytest.fixture(scope='module')
def hip():
    from ofdm_tools import _hip
    return _hip


@pytest.fixture(scope='module')
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


def window():
    from ofdm_tools import windows
    return windows.get_window('hann', 4096)


def schedules(hip):
    """(schedule, segments per chunk; 0: the route's own)"""
    return ((hip.SCHED_DYNAMIC, 1), (hip.SCHED_DYNAMIC, 2), (hip.SCHED_INTERLEAVED, 1), (hip.SCHED_CONTIGUOUS, 0))


def recipe(plan):
    return dict(kv.split('=', 1) for kv in plan.last_recipe().split())


def check_recipe(rec, kernel, sched, chunk, nseg):
    """what really ran: kernel, schedule, chunk; a launch larger than the grid gives every workgroup several chunks"""
    assert rec['kernel'].startswith(kernel) and rec['sched'] == SCHED_NAME[sched], (rec, kernel, sched)
    W = int(rec['W'])
    if chunk:
        assert int(rec['chunk']) == chunk, (rec, chunk)
    if sched == 2:
        assert int(rec['tail']) == 1, rec      # one-segment chunks at least in the tail: idle steps
    if nseg > 1000:
        assert W < nseg and nseg > 2 * W * max(chunk, 1), (rec, nseg)
    else:
        assert W == nseg, (rec, nseg)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def floored(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(b, 0.1 * np.median(b))))


@functools.lru_cache(maxsize=None)
def signals(nseg):
    """-> ([three complex64 streams], [their float64 Welch spectra]); computed once, read-only"""
    n = 4096 + 2048 * (nseg - 1)
    rng = np.random.default_rng(4096 + nseg)
    xs, refs = [], []
    for dc in DCS:
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
        x += 0.5 * np.exp(2j * np.pi * 0.1234 * np.arange(n))
        x = (x + dc).astype(np.complex64)
        x.setflags(write=False)
        ref = R.welch_np(x, fs=1.0, window=window(), nperseg=4096, noverlap=2048, nfft=4096)[1]
        ref.setflags(write=False)
        xs.append(x)
        refs.append(ref)
    return xs, refs


def run_streams(ctx, plan, xs):
    n, ns = len(xs[0]), len(xs)
    buf = np.concatenate(xs).astype(np.complex64)
    d_in, d_out = ctx.alloc(buf.nbytes), ctx.alloc(ns * 4096 * 4)
    try:
        ctx.h2d(d_in, buf)
        nseg = plan.exec_dev(d_in, n, d_out, nstreams=ns, stream_stride=n)
        return nseg, ctx.d2h(d_out, (ns, 4096), np.float32)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


@pytest.mark.parametrize('nseg', NSEG)
@pytest.mark.parametrize('build', ['ws', 'wsgen'])
def test_every_schedule_and_chunk_against_the_oracle(ctx, hip, build, nseg):
    xs, refs = signals(nseg)
    plan = ctx.welch_plan(4096, window=window(), detrend=hip.DETREND_CONSTANT, kernel=hip.KERNEL_TUNED)
    try:
        for sched, chunk in schedules(hip):
            plan.set_tuning(build, sched=sched, chunk=chunk)
            for pick in ((0,), (1,), (0, 1, 2)):
                k, got = run_streams(ctx, plan, [xs[i] for i in pick])
                assert k == nseg
                rec = recipe(plan)
                check_recipe(rec, 'welch4096:ws', sched, chunk, nseg)
                for row, i in zip(got, pick):
                    err, few = relerr(row, refs[i]), floored(row, refs[i])
                    print('%s sched %s chunk %s tail %s W %s nseg %d streams %s stream %d: rel %.2e floored %.2e'
                          % (build, rec['sched'], rec['chunk'], rec['tail'], rec['W'], nseg, pick, i, err, few))
                    if nseg >= 8:
                        assert err < RTOL, (build, sched, chunk, nseg, pick, i, err)
                    else:
                        assert few < FEW, (build, sched, chunk, nseg, pick, i, few)
                if sched != hip.SCHED_DYNAMIC:      # static: the same sums in the same order
                    _, again = run_streams(ctx, plan, [xs[i] for i in pick])
                    assert np.array_equal(got, again), (build, sched, chunk, nseg, pick)
    finally:
        plan.close()


@pytest.mark.parametrize('nseg', [9, 33, 1031])
def test_two_channel_kernel_every_schedule_and_chunk(ctx, hip, nseg):
    n = 4096 + 2048 * (nseg - 1) + 700
    x = R.synth_iq(n, 500 + nseg, dc=2 - 1j)
    y = (0.7 * np.roll(x, 5) + 0.5 * R.synth_iq(n, 1500 + nseg, tones=(), dc=0.5 + 0.25j)).astype(np.complex64)
    pxx, pyy, pxy, cxy = O.csd(x, y, 1.0, 'hann', 4096, 2048, 4096, 'constant', 'density')
    norm = np.sqrt(pxx * pyy)
    plan = ctx.welch_plan(4096, noverlap=2048, window=window(), detrend=hip.DETREND_CONSTANT, kernel=hip.KERNEL_TUNED)
    try:
        for sched, chunk in schedules(hip):
            plan.set_tuning(None, sched=sched, chunk=chunk)
            gxx, gyy, gxy, gc = plan.csd(x, y)
            rec = recipe(plan)
            assert plan.last_nseg == nseg
            check_recipe(rec, 'csd4096ws', sched, chunk, nseg)
            d = np.asarray(gxy).astype(np.complex128) - pxy
            e = (relerr(gxx, pxx), relerr(gyy, pyy), float(np.max(np.abs(d) / norm)), float(np.max(np.abs(d.imag) / norm)),
                 float(np.max(np.abs(np.asarray(gc, np.float64) - cxy))))
            print('csd sched %s chunk %s tail %s W %s nseg %d: Pxx %.2e Pyy %.2e Pxy %.2e ImPxy %.2e Cxy %.2e'
                  % ((rec['sched'], rec['chunk'], rec['tail'], rec['W'], nseg) + e))
            assert max(e) < RTOL, (sched, chunk, nseg, e)
    finally:
        plan.close()
