"""welch4096ws's complementary-window producer (WelchArgs.compl_win: w[n] + w[n + 2048] = 1, SciPy's periodic Hann) against
the general-window producer of the same kernel, the float64 oracle and the coverage kernel.

set_tuning('ws') forces the role-split route with the producer the plan's window admits (the complementary one for Hann),
set_tuning('wsgen') the same route with the general producer; without a tuning word the plan takes the role-split route
from eight segments per stream on and the time-domain builds below that.
"""
import numpy as np
import pytest

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

RTOL = 1e-4          # the project's gate: relative, linear power, every bin
FEW = 5e-5           # few-segment launches (test_tuned_vs_generic_on_awkward_segment_counts): near-empty bins are judged
                     # against a tenth of the spectrum's median level


@pytest.fixture(scope='module')
def hip():
    from ofdm_tools import _hip
    return _hip


@pytest.fixture(scope='module')
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


def window(name, n=4096):
    from ofdm_tools import windows
    return windows.get_window(name, n)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def floored(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(b, 0.1 * np.median(b))))


def run_streams(ctx, plan, xs, n):
    """one launch over len(xs) device-resident streams -> float64 [stream][bin]"""
    ns = len(xs)
    buf = np.concatenate(xs).astype(np.complex64)
    d_in, d_out = ctx.alloc(buf.nbytes), ctx.alloc(ns * 4096 * 4)
    try:
        ctx.h2d(d_in, buf)
        nseg = plan.exec_dev(d_in, n, d_out, nstreams=ns, stream_stride=n)
        return nseg, ctx.d2h(d_out, (ns, 4096), np.float32).astype(np.float64)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


def test_complementary_and_general_producer_against_the_oracle(ctx, hip):
    """Hann at 4096 points; 1, 2, 7, 8, 9 and 2047 segments; three streams with DC offsets of 0.1, 30 and 300 sigma in one
    launch.  The default plan, the forced complementary build ('ws') and the forced general build ('wsgen') run the same
    samples.  Gates, none of them new: the default plan holds 1e-4 on every bin against the float64 oracle at every count
    (test_detrend_forms_few_segments_and_large_dc, 'auto'); the forced role-split builds hold the same from eight segments
    on, and below that - where the plan would not pick them - the few-segment gate of
    test_tuned_vs_generic_on_awkward_segment_counts against the oracle.  The deviation between the two producers is printed,
    not gated (a CPU emulation of the two window forms alone gives 1e-8 over 511 segments; the builds also differ in their
    pass-1 twiddles - thirteen table values against six and nine products of them).

    Measured on MI355X (max over the three streams; against the float64 oracle, all bins / build against build, all bins):
        nseg    default    complementary   general     complementary vs general
           1    2.4e-05    3.1e-05         3.4e-05     2.6e-05  (3.2e-06 against max(bin, median / 10))
           2    4.2e-06    1.8e-06         1.8e-06     2.0e-06
           7    1.4e-06    1.1e-06         7.7e-07     1.0e-06
           8    5.9e-07    5.9e-07         1.4e-06     1.1e-06
           9    7.5e-07    7.5e-07         7.4e-07     6.8e-07
        2047    2.0e-07    2.0e-07         2.0e-07     1.2e-07"""
    rng = np.random.default_rng(2025)
    w = window('hann')
    lines = []
    for nseg in (1, 2, 7, 8, 9, 2047):
        n = 4096 + 2048 * (nseg - 1)
        xs = []
        for dc in (0.1 + 0.05j, 30.0 - 18.0j, 300.0 * np.exp(0.54j)):
            x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
            x += 0.5 * np.exp(2j * np.pi * 0.1234 * np.arange(n))
            xs.append((x + dc).astype(np.complex64))
        refs = [R.welch_np(x, fs=1.0, window=w, nperseg=4096, noverlap=2048, nfft=4096)[1] for x in xs]
        got = {}
        for force in (None, 'ws', 'wsgen'):
            plan = ctx.welch_plan(4096, window=w, kernel=hip.KERNEL_TUNED)
            plan.set_tuning(force)
            k, got[force] = run_streams(ctx, plan, xs, n)
            plan.close()
            assert k == nseg
        errs = {f: max(relerr(got[f][i], refs[i]) for i in range(3)) for f in got}
        few = {f: max(floored(got[f][i], refs[i]) for i in range(3)) for f in got}
        dev = max(relerr(got['ws'][i], got['wsgen'][i]) for i in range(3))
        dev_few = max(floored(got['ws'][i], got['wsgen'][i]) for i in range(3))
        lines.append('nseg=%4d  oracle: default %.2e  compl %.2e (floored %.2e)  general %.2e (floored %.2e)   compl vs general %.2e '
                     '(floored %.2e)' % (nseg, errs[None], errs['ws'], few['ws'], errs['wsgen'], few['wsgen'], dev, dev_few))
        print(lines[-1])
        assert errs[None] < RTOL, lines[-1]
        for f in ('ws', 'wsgen'):
            if nseg >= 8:
                assert errs[f] < RTOL, lines[-1]
            else:
                assert few[f] < FEW, lines[-1]


@pytest.mark.parametrize('name', ['hann_off', 'flattop', 'boxcar', 'blackmanharris'])
def test_windows_that_are_not_complementary_run_the_general_build_bit_for_bit(ctx, hip, name):
    """The plan-time check refuses a Hann window with one value moved by 2^-20 (|w[n] + w[n + 2048] - 1| = 9.5e-7 > 2^-23),
    flattop, boxcar and Blackman-Harris: with or without the tuning word that forces the general build, such a plan runs
    the same code on the same static schedule, so the outputs are equal bit for bit.  The true Hann window is the
    control: its default run differs from its forced-general run in some bit (the complementary build did run) and
    agrees with it to rounding."""
    x = R.synth_iq(4096 + 2048 * 700, 77)
    ws = {'hann_off': window('hann').copy()} if name == 'hann_off' else {name: window(name)}
    if name == 'hann_off':
        ws['hann_off'][1000] += np.float32(2.0 ** -20)
        ws['hann'] = window('hann')
    for wname, w in ws.items():
        outs = []
        for force in (None, 'wsgen'):
            plan = ctx.welch_plan(4096, window=w, kernel=hip.KERNEL_TUNED)
            plan.set_tuning(force)
            plan.set_schedule(hip.SCHED_INTERLEAVED)      # static: bit-reproducible
            outs.append(plan.exec(x))
            assert plan.last_nseg == 701
            plan.close()
        _, ref = R.welch_np(x, fs=1.0, window=w, nperseg=4096, noverlap=2048, nfft=4096)
        # (floored: a detrended boxcar's bin 0 is exactly zero in the oracle)
        assert floored(outs[0], ref) < RTOL and floored(outs[1], ref) < RTOL
        if wname == 'hann':
            assert not np.array_equal(outs[0], outs[1])
            assert relerr(outs[0], outs[1]) < 2e-5
        else:
            assert np.array_equal(outs[0], outs[1]), (wname, relerr(outs[0], outs[1]))


def test_complementary_build_schedules_and_short_chunks_against_the_coverage_kernel(ctx, hip):
    """All three schedules at the default chunk size, then one- and two-segment chunks (their own paths in the producer:
    first-of-chunk with nothing to prefetch, and first + last) under both chunked schedules, one to three streams, with
    and without the detrend (the pilot and the plain flavours) - the complementary build against the independent
    generic kernel on device-resident data, at the gate of test_tuned_vs_generic_on_awkward_segment_counts."""
    nmax = 4096 + 2048 * 1500
    d_in = ctx.alloc(3 * nmax * 8)
    d_a, d_b = ctx.alloc(3 * 4096 * 4), ctx.alloc(3 * 4096 * 4)
    try:
        ctx.synth_iq(d_in, 3 * nmax, 31, R.TONES, R.DC)
        for det in (hip.DETREND_CONSTANT, hip.DETREND_CONSTANT_FAST, hip.DETREND_NONE):
            tuned = ctx.welch_plan(4096, window=window('hann'), detrend=det, kernel=hip.KERNEL_TUNED)
            gen = ctx.welch_plan(4096, window=window('hann'), detrend=det, kernel=hip.KERNEL_GENERIC)
            cases = [(s, 0, nseg, ns) for s in (hip.SCHED_CONTIGUOUS, hip.SCHED_INTERLEAVED, hip.SCHED_DYNAMIC)
                     for nseg, ns in ((1463, 1), (700, 3))]
            cases += [(s, chunk, nseg, ns) for s in (hip.SCHED_INTERLEAVED, hip.SCHED_DYNAMIC) for chunk in (1, 2)
                      for nseg, ns in ((1500, 2), (9, 3), (8, 1))]
            for sched, chunk, nseg, ns in cases:
                n = 4096 + 2048 * (nseg - 1) + 11
                tuned.set_tuning('ws', chunk=chunk)
                tuned.set_schedule(sched)
                assert tuned.exec_dev(d_in, n, d_a, nstreams=ns, stream_stride=nmax) == nseg
                assert gen.exec_dev(d_in, n, d_b, nstreams=ns, stream_stride=nmax) == nseg
                a = ctx.d2h(d_a, (ns, 4096), np.float32)
                b = ctx.d2h(d_b, (ns, 4096), np.float32)
                err = floored(a, b)
                assert err < FEW, (det, sched, chunk, nseg, ns, err)
            tuned.close()
            gen.close()
    finally:
        for ptr in (d_in, d_a, d_b):
            ctx.free(ptr)
