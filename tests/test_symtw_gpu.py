"""welch4096ws's complementary-window build on signed digits (time origin n - 136, three-shear twiddles, one detrended
bin per consumer thread; tests/test_symtw_model_cpu.py is its NumPy model) against the float64 oracle.

Input: unit-variance complex noise plus 24 tones that sit exactly on bins - the digit edges of the new bin map (0, 1, 7,
8, 15, 16, 119, 120, 121, 135, 136, 137, 255, 256, 3839, 3840, 3959, 3960, 4095), the middle (2047, 2048) and three more
(128, 2176, 3967) - with amplitudes in geometric steps from 0.04 to 1, so every tone has its own power, 4 to 2700 times the
noise level of a bin: a register stored at another bin's place cannot hide.  Segment counts 1, 2, 3, 9, 41 (one segment per
workgroup) and 3001 under the dynamic schedule with one-segment chunks, forced through set_tuning as
tests/test_consumer_path_gpu.py does, where every workgroup alternates segment and idle step.

Detrend and DC offset.  OTH_DETREND_CONSTANT (the pilot build): three different streams with DC offsets of 0, 35 and 300
sigma in one launch at a stride, and the first of them alone.  OTH_DETREND_NONE and OTH_DETREND_CONSTANT_FAST run the
offset-free stream, alone and three times in one launch at the same stride: there the DC line itself goes through the
float32 transform, and one ulp of its amplitude (35 or 300 x 2048) is 1e-4 ... 1e-3 of a noise bin (39) for any float32
FFT - tests/test_hip_parity.py::test_detrend_forms_few_segments_and_large_dc holds those combinations to their own gates.

Criteria, all the project's: every multi-segment output within 1e-4 relative of the oracle on every bin; the one-segment
rows by check_single_rows (4 ulp of the row's peak amplitude on every bin, 1e-4 from the median up, mean 2e-6); the
static schedules repeat bit for bit over three runs; the default plan names the role-split route.  The deviation from the
general build ('wsgen') on the same samples is printed, not asserted.
"""
import functools

import numpy as np
import pytest

from oracle import ref_cpu as R
from test_consumer_path_gpu import SCHED_NAME, check_recipe, recipe, relerr
from test_hip_parity import RTOL, check_single_rows

pytestmark = pytest.mark.gpu

NSEG = (1, 2, 3, 9, 41, 3001)
TONE_BINS = (0, 1, 7, 8, 15, 16, 119, 120, 121, 135, 136, 137, 255, 256, 2047, 2048, 3839, 3840, 3959, 3960, 4095, 128, 2176, 3967)
TONE_AMPS = tuple(0.04 * (1.0 / 0.04) ** (i / (len(TONE_BINS) - 1.0)) for i in range(len(TONE_BINS)))
DCS = (0.0, 35.0 * np.exp(0.54j), 300.0 * np.exp(-2.1j))      # in units of the noise's sigma (= 1)
PAD = 777                                                      # samples between the end of one stream and the next


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
def signals(nseg):
    """-> ([three complex64 streams: DC 0 / 35 / 300 sigma], {(detrend name, stream): float64 Welch spectrum}); read-only"""
    n = 4096 + 2048 * (nseg - 1)
    tones = tuple((a, k / 4096.0) for a, k in zip(TONE_AMPS, TONE_BINS))
    xs, refs = [], {}
    for i, dc in enumerate(DCS):
        x = R.synth_iq(n, 9000 + 10 * nseg + i, tones=tones, dc=dc)
        x.setflags(write=False)
        xs.append(x)
        refs[('constant', i)] = R.welch_np(x, fs=1.0, window=window(), nperseg=4096, noverlap=2048, nfft=4096)[1]
    refs[('none', 0)] = R.welch_np(xs[0], fs=1.0, window=window(), nperseg=4096, noverlap=2048, nfft=4096, detrend=False)[1]
    refs[('fast', 0)] = refs[('constant', 0)]
    for r in refs.values():
        r.setflags(write=False)
    return xs, refs


def run_streams(ctx, plan, xs):
    n, ns = len(xs[0]), len(xs)
    buf = np.zeros(ns * (n + PAD), np.complex64)
    for i, x in enumerate(xs):
        buf[i * (n + PAD):i * (n + PAD) + n] = x
    d_in, d_out = ctx.alloc(buf.nbytes), ctx.alloc(ns * 4096 * 4)
    try:
        ctx.h2d(d_in, buf)
        nseg = plan.exec_dev(d_in, n, d_out, nstreams=ns, stream_stride=n + PAD)
        return nseg, ctx.d2h(d_out, (ns, 4096), np.float32)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


def schedules(hip, nseg):
    """(schedule, chunk): the large count on the idle-step edge, the small ones on both static schedules"""
    if nseg > 1000:
        return ((hip.SCHED_DYNAMIC, 1), (hip.SCHED_INTERLEAVED, 1))
    return ((hip.SCHED_CONTIGUOUS, 0), (hip.SCHED_INTERLEAVED, 1))


@pytest.mark.parametrize('nseg', NSEG)
@pytest.mark.parametrize('detrend', ['constant', 'none', 'fast'])
def test_signed_digit_build_against_the_oracle(ctx, hip, detrend, nseg):
    xs, refs = signals(nseg)
    det = {'constant': hip.DETREND_CONSTANT, 'none': hip.DETREND_NONE, 'fast': hip.DETREND_CONSTANT_FAST}[detrend]
    # (streams of the launch, their reference rows)
    if detrend == 'constant':
        launches = (((0,), (0,)), ((0, 1, 2), (0, 1, 2)))
    else:
        launches = (((0,), (0,)), ((0, 0, 0), (0, 0, 0)))
    plan = ctx.welch_plan(4096, window=window(), detrend=det, kernel=hip.KERNEL_TUNED)
    gen = ctx.welch_plan(4096, window=window(), detrend=det, kernel=hip.KERNEL_TUNED)
    try:
        for sched, chunk in schedules(hip, nseg):
            plan.set_tuning('ws', sched=sched, chunk=chunk)
            gen.set_tuning('wsgen', sched=sched, chunk=chunk)
            for pick, which in launches:
                k, got = run_streams(ctx, plan, [xs[i] for i in pick])
                assert k == nseg
                rec = recipe(plan)
                check_recipe(rec, 'welch4096:ws', sched, chunk, nseg)
                _, other = run_streams(ctx, gen, [xs[i] for i in pick])
                for row, orow, i in zip(got, other, which):
                    ref = refs[(detrend, i)]
                    err = relerr(row, ref)
                    print('%s sched %s chunk %s W %s nseg %d streams %s stream %d: oracle %.2e, against the general build %.2e'
                          % (detrend, rec['sched'], rec['chunk'], rec['W'], nseg, pick, i, err, relerr(row, orow)))
                    if nseg == 1:
                        check_single_rows(row, ref)
                    else:
                        assert err < RTOL, (detrend, SCHED_NAME[sched], chunk, nseg, pick, i, err)
                if sched != hip.SCHED_DYNAMIC:      # static: the same sums in the same order, three runs
                    for _ in range(2):
                        _, again = run_streams(ctx, plan, [xs[i] for i in pick])
                        assert np.array_equal(got, again), (detrend, sched, chunk, nseg, pick)
    finally:
        plan.close()
        gen.close()


def test_default_plan_takes_the_role_split_route(ctx, hip):
    xs, refs = signals(41)
    plan = ctx.welch_plan(4096, window=window(), kernel=hip.KERNEL_TUNED)
    try:
        k, got = run_streams(ctx, plan, xs)
        assert k == 41
        assert plan.last_recipe().startswith('kernel=welch4096:ws '), plan.last_recipe()
        for i in range(3):
            assert relerr(got[i], refs[('constant', i)]) < RTOL
    finally:
        plan.close()
