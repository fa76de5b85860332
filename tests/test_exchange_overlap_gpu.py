"""welch4096ws's complementary-window build with the exchange stores issued inside the last butterfly layer of passes 1 and
2 (dft16_layer2_scatter_sym, fft4096.hip.h): the flagship route, forced role-split, on the smallest launches that reach
every flavour of the producer's item() and every edge of the consumer's loop - which now writes exchange 2 from pass 2,
before it has looked at the item word, in idle steps and in the last step too.

  * one stream of 1 ... 7 segments (2048 (nseg + 1) samples), which the library runs as contiguous runs.  The grid is
    min(resident workgroups, segments), so these are one segment per workgroup: first + none, segment -> stop;
  * 3001 segments (512 workgroups), forced through set_tuning as tests/test_consumer_path_gpu.py does, kernel, schedule
    and chunk asserted from the recipe: under the dynamic schedule with two-segment chunks and one-segment tail chunks
    - the head flavour (prefetch across a chunk boundary), one-segment chunks and the idle step behind them - and, for
    what the short launches cannot reach, under the two static schedules: interleaved two-segment chunks, and
    contiguous runs of five or six segments per workgroup - first + mid, the two-per-trip loop, its remainder, the last.

Input: seeded unit-variance complex noise plus two weak tones and a DC offset of 3 sigma; once, under the pilot detrend,
of 300 sigma.  Detrend constant (the pilot flavour), constant-fast and none: the three flavours of the kernel.

Every case three ways:
  * against oracle.ref_cpu.welch_np in float64: the suite's 1e-4 relative on every bin;
  * against the general build ('wsgen') on the same samples: both builds are held to the oracle - 1e-4 on every bin of
    an average, a one-segment row to tests/test_symtw_gpu.py's check_single_rows (4 ulp of the row's peak amplitude on
    every bin, mean 2e-6) - so they lie within twice that of each other: 2e-4 on every bin; for a one-segment row
    8 ulp of the peak amplitude and 4e-6 in the mean;
  * under a static schedule a second call returns the same bits.
"""
import functools

import numpy as np
import pytest

from oracle import ref_cpu as R
from test_consumer_path_gpu import check_recipe, recipe, relerr

pytestmark = pytest.mark.gpu

RTOL = 1e-4
SHORT = (1, 2, 3, 4, 5, 6, 7)
LONG = 3001
# (detrend, DC offset in units of the noise's sigma)
CASES = (('constant', 3.0), ('constant', 300.0), ('fast', 3.0), ('none', 3.0))


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


@functools.lru_cache(maxsize=None)
def signal(nseg, dc):
    """-> (complex64 samples, {detrends: float64 Welch spectrum}); computed once, read-only"""
    n = 2048 * (nseg + 1)
    x = R.synth_iq(n, 7100 + 16 * nseg + int(dc), tones=((0.5, 0.1234), (0.25, -0.3071)), dc=dc * np.exp(0.54j))
    x.setflags(write=False)
    with_mean = R.welch_np(x, fs=1.0, window=window(), nperseg=4096, noverlap=2048, nfft=4096)[1]
    without = R.welch_np(x, fs=1.0, window=window(), nperseg=4096, noverlap=2048, nfft=4096, detrend=False)[1]
    for r in (with_mean, without):
        r.setflags(write=False)
    return x, {'constant': with_mean, 'fast': with_mean, 'none': without}


def run(ctx, plan, x):
    d_in, d_out = ctx.alloc(x.nbytes), ctx.alloc(4096 * 4)
    try:
        ctx.h2d(d_in, x)
        nseg = plan.exec_dev(d_in, len(x), d_out)
        return nseg, ctx.d2h(d_out, (4096,), np.float32)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


def plans(ctx, hip, detrend):
    det = {'constant': hip.DETREND_CONSTANT, 'fast': hip.DETREND_CONSTANT_FAST, 'none': hip.DETREND_NONE}[detrend]
    return (ctx.welch_plan(4096, window=window(), detrend=det, kernel=hip.KERNEL_TUNED),
            ctx.welch_plan(4096, window=window(), detrend=det, kernel=hip.KERNEL_TUNED))


def against_general_build(row, gen, nseg):
    row, gen = np.asarray(row, np.float64), np.asarray(gen, np.float64)
    if nseg > 1:
        assert relerr(row, gen) < 2 * RTOL, relerr(row, gen)
        return
    amp = np.abs(np.sqrt(row) - np.sqrt(gen)) / np.sqrt(gen).max()
    assert amp.max() <= 8 * 2.0 ** -23, amp.max() * 2.0 ** 23
    assert np.mean(np.abs(row - gen) / gen) < 4e-6


@pytest.mark.parametrize('nseg', SHORT)
@pytest.mark.parametrize('detrend,dc', CASES)
def test_short_launches_every_flavour(ctx, hip, detrend, dc, nseg):
    x, refs = signal(nseg, dc)
    plan, gen = plans(ctx, hip, detrend)
    try:
        plan.set_tuning('ws')
        gen.set_tuning('wsgen')
        k, got = run(ctx, plan, x)
        rec = recipe(plan)
        assert k == nseg
        check_recipe(rec, 'welch4096:ws', hip.SCHED_CONTIGUOUS, 0, nseg)
        _, other = run(ctx, gen, x)
        err, dev = relerr(got, refs[detrend]), relerr(got, other)
        print('%s dc %g nseg %d W %s: oracle %.2e, against the general build %.2e' % (detrend, dc, nseg, rec['W'], err, dev))
        assert err < RTOL, (detrend, dc, nseg, err)
        against_general_build(got, other, nseg)
        _, again = run(ctx, plan, x)
        assert np.array_equal(got, again), (detrend, dc, nseg)
    finally:
        plan.close()
        gen.close()


@pytest.mark.parametrize('detrend', ['constant', 'fast', 'none'])
def test_dynamic_schedule_head_flavour_and_idle_step(ctx, hip, detrend):
    x, refs = signal(LONG, 3.0)
    plan, gen = plans(ctx, hip, detrend)
    try:
        plan.set_tuning('ws', sched=hip.SCHED_DYNAMIC, chunk=2)
        gen.set_tuning('wsgen', sched=hip.SCHED_DYNAMIC, chunk=2)
        k, got = run(ctx, plan, x)
        rec = recipe(plan)
        assert k == LONG
        check_recipe(rec, 'welch4096:ws', hip.SCHED_DYNAMIC, 2, LONG)
        _, other = run(ctx, gen, x)
        err, dev = relerr(got, refs[detrend]), relerr(got, other)
        print('%s nseg %d sched %s chunk %s tail %s W %s: oracle %.2e, against the general build %.2e'
              % (detrend, LONG, rec['sched'], rec['chunk'], rec['tail'], rec['W'], err, dev))
        assert err < RTOL, (detrend, err)
        against_general_build(got, other, LONG)
        # the static schedules over the same samples, the same sums in the same order: two-segment chunks, and contiguous
        # runs of five or six segments per workgroup (first + mid, the two-per-trip loop, its remainder, the last)
        for sched, chunk in ((hip.SCHED_INTERLEAVED, 2), (hip.SCHED_CONTIGUOUS, 0)):
            plan.set_tuning('ws', sched=sched, chunk=chunk)
            _, first = run(ctx, plan, x)
            rec = recipe(plan)
            check_recipe(rec, 'welch4096:ws', sched, chunk, LONG)
            _, again = run(ctx, plan, x)
            err = relerr(first, refs[detrend])
            print('%s nseg %d sched %s chunk %s W %s: oracle %.2e' % (detrend, LONG, rec['sched'], rec['chunk'], rec['W'], err))
            assert err < RTOL, (detrend, sched, err)
            against_general_build(first, other, LONG)
            assert np.array_equal(first, again), (detrend, sched)
    finally:
        plan.close()
        gen.close()
