"""The opt-in to more than 64 KiB of dynamic LDS is remembered per kernel instantiation AND per device (csrc/launch.h).  One
process, two contexts: the smallest launch of every family whose tile needs the opt-in runs on device 0, then on device 1.
A flag keyed by the instantiation alone would leave device 1 unarmed and its first launch would come back as an error.
Device 1's results equal device 0's bit for bit, and both meet the gate of the family's own parity test (its oracle helper,
its input where that is a function, RTOL).

Inputs: averages of a few segments take noise (test_hip_parity._dc_stream: the input of
test_detrend_forms_few_segments_and_large_dc, 3.6 sigma of DC where the plan detrends, none where it does not - an
undetrended DC line of 3.6 sigma stands 50 dB over a noise bin and its float32 rounding alone is 1e-4 of that bin).  The
single 32768-point segment is a single row: check_single_rows, as in test_welch_32768_65536_inside_one_workgroup.  The
multitaper launches are ONE segment under TWO tapers: over 16384 bins the sum of two |X|^2 dips to 1e-2 of its mean, where
the rounding of a tone 50 dB over the noise is 1e-4 of the bin (check_single_rows' docstring), so they take the parity
tests' noise without its tones."""
import ctypes

import numpy as np
import pytest

import mtm_csd_oracle as MC
import mtm_oracle as MO
import test_csd_gpu as TC
from oracle import ref_cpu as R
from test_hip_parity import RTOL, _dc_stream, check_single_rows, hann, hip, relerr  # noqa: F401 - hip is a fixture
from test_median_gpu import noise_tones

pytestmark = pytest.mark.gpu


def welch_case(route, nfft, nseg, noverlap, dc, detrend=True, rect=False, kernel=None):
    """-> run(ctx, hip), ref(), err(got, ref) of a Welch plan on nseg segments of noise"""
    x = _dc_stream(nfft + (nfft - noverlap) * (nseg - 1) + 5, dc, 77 + nfft + nseg)

    def run(ctx, hip):
        plan = ctx.welch_plan(nfft, noverlap=noverlap, window=None if rect else hann(nfft),
                              detrend=hip.DETREND_CONSTANT if detrend else hip.DETREND_NONE,
                              kernel=hip.KERNEL_AUTO if kernel is None else getattr(hip, kernel))
        got = plan.exec(x)
        assert plan.last_nseg == nseg and plan.last_recipe().startswith(route), plan.last_recipe()
        plan.close()
        return (got,)

    def ref():
        return R.welch_np(x, window='boxcar' if rect else 'hann', nperseg=nfft, noverlap=noverlap, nfft=nfft,
                          detrend='constant' if detrend else False)[1]
    return run, ref, lambda got, ref: relerr(got[0], ref)


def csd4096ws_case():
    x, y = TC.pair(4096, 2048, 16, 4096 + 16)

    def run(ctx, hip):
        plan = ctx.welch_plan(4096, window=hann(4096))
        got = plan.csd(x, y)
        assert plan.last_nseg == 16 and plan.last_recipe().startswith('kernel=csd4096ws '), plan.last_recipe()
        plan.close()
        return tuple(got)
    return run, lambda: TC.oracle(x, y, 4096, 4096, 2048), lambda got, ref: max(TC.errors(got, ref))


def welch32k_case():
    n = 32768
    x = R.synth_iq(n + 17, 101, dc=30 + 20j)

    def run(ctx, hip):
        plan = ctx.welch_plan(n, noverlap=n // 2, window=hann(n))
        got = plan.exec(x)
        assert plan.last_nseg == 1 and plan.last_recipe().startswith('kernel=anyfft:onewg '), plan.last_recipe()
        plan.close()
        return (got,)

    def err(got, ref):
        check_single_rows(got[0][None, :], ref[None, :], ulps=4)      # asserts the single-row criteria itself
        return 0.0
    return run, lambda: R.welch_np(x, nperseg=n, nfft=n, noverlap=n // 2)[1], err


def anylen_case(n=12000, nseg=9):
    x = R.synth_iq(n // 2 * (nseg + 1) + 3, 600 + n % 97)      # test_welch_any_length_against_the_oracle's input

    def run(ctx, hip):
        plan = ctx.welch_plan(n, window=hann(n))
        got = plan.exec(x)
        assert plan.last_nseg == nseg and plan.last_recipe().startswith('kernel=anyfft:direct '), plan.last_recipe()
        plan.close()
        return (got,)
    return run, lambda: R.welch_np(x, nperseg=n, nfft=n)[1], lambda got, ref: relerr(got[0], ref)


def mtm_case(two, nfft=16384, nw=2.0, K=2):
    x = noise_tones(nfft + nfft // 3, nfft + K, tones=())
    y = (0.7 * np.roll(x, 5) + 0.5 * noise_tones(len(x), nfft + K + 1000, tones=())).astype(np.complex64)

    def run(ctx, hip):
        plan = (ctx.mtm_csd_plan if two else ctx.mtm_plan)(nfft, nw=nw, ntapers=K)
        got = tuple(plan.csd(x, y)) if two else (plan.exec(x),)
        want = 'kernel=%s nfft=%d ntapers=%d ' % ('mtmcsd' if two else 'mtm', nfft, K)
        assert plan.last_nseg == 1 and plan.last_recipe().startswith(want), plan.last_recipe()
        plan.close()
        return got

    if two:
        return run, lambda: MC.mtm_csd(x, y, nfft, nw=nw, K=K), lambda got, ref: max(TC.errors(got, ref))
    return run, lambda: MO.mtm_psd(x, nfft, nw=nw, K=K), lambda got, ref: relerr(got[0], ref)


def cases():
    return {
        'welch16k1x_half': welch_case('kernel=welch16k1x_half ', 16384, 3, 8192, 0.0, detrend=False),
        'welch16k1x pipe': welch_case('kernel=welch16k1x:pipe ', 16384, 2, 0, 0.0, detrend=False, rect=True),
        'welch16k': welch_case('kernel=welch16k ', 16384, 3, 8192, 3.6),      # fewer than 8 segments: the time-domain builds
        '8192 fd': welch_case('kernel=welch16k1x_half:ws ', 8192, 16, 4096, 3.6),
        'welch4096 ws': welch_case('kernel=welch4096:ws ', 4096, 16, 2048, 3.6),
        'csd4096ws': csd4096ws_case(),
        'welch32k': welch32k_case(),
        'mtm': mtm_case(False),
        'mtmcsd': mtm_case(True),
        'anyfft 12000': anylen_case(),
        'generic 16384': welch_case('kernel=welch_generic ', 16384, 3, 8192, 3.6, kernel='KERNEL_GENERIC'),
    }


def test_every_big_lds_launch_on_device_0_then_on_device_1(hip):
    count = ctypes.c_int(0)
    assert hip.load().oth_device_count(ctypes.byref(count)) == 0
    if count.value < 2:
        pytest.skip('needs two visible devices, found %d' % count.value)
    todo = cases()
    got = {}
    for dev in (0, 1):
        ctx = hip.Context(dev)
        try:
            for name, case in todo.items():
                got[dev, name] = case[0](ctx, hip)
        finally:
            ctx.close()
    for name, (_, ref, err_of) in todo.items():
        for a, b in zip(got[0, name], got[1, name]):
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), name
        want = ref()
        for dev in (0, 1):
            err = err_of(got[dev, name], want)
            print('launch arming | %-16s device %d | worst %.2e' % (name, dev, err))
            assert err < RTOL, (name, dev, err)
