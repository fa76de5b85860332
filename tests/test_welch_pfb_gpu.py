"""GPU tests of the polyphase filter-bank (WOLA) PSD of Welch plans (oth_welch_set_prototype, oth_welch_pfb / _dev,
csrc/welchpfb.hip) against the float64 oracle by the definition (tests/welch_pfb_oracle.py).  The gate is the project's
RTOL = 1e-4: every bin within RTOL relative of the oracle.  A float32 emulation of the definition (complex64 samples,
float32 taps and accumulators, the pilot then the residual mean, a complex64 transform) against float64 on the exact
inputs of the parity cases stays at or below 1.9e-5 per bin (tests/test_welch_pfb_cpu.py asserts RTOL / 2), the one-frame
case at 512 x 2 at 1.3e-5.  Input is test_median_gpu's noise_tones: unit noise, a 3-sigma and a 0.5-sigma tone, a small
offset; the 35 - 20j offset goes on detrending plans only (without detrend it is the float32 reference's own loss).
Measured on an MI355X, worst readings of this file per group (gate 1e-4 per bin): the ten parity cases with M >= 3 1.9e-5
(at 16384 x 16; 64 ... 256 points at most 8.2e-7), the one-frame case 1.2e-5; against exec of the P N-point plan 8.5e-7 at
256 x 4 and 5.2e-6 at 1024 x 16; three padded streams with NaN gaps 1.9e-5; 64 streams x 8 frames of 4096 x 4 1.3e-5 and
100 x 5 of 16384 x 2 with W = 2 < nseg 4.0e-5; P = 4 then P = 8 on one plan 2.7e-6, 3.6e-6; the helpers' rows inside RTOL.
Identical streams, repeated calls and exec around set_prototype / pfb: bit-identical.  Leakage capture: the filter bank's
bins 96 ... 98 and 112 ... 114 within -1.20 ... +0.38 dB of the row's median, the Hann plan +32.7 dB at bin 98 and +20.1 dB
at bin 112 - the float64 oracle's figures to the digits shown.  A NaN or +-inf sample: NaN in every bin of its stream's row,
linear and dB, with and without detrend."""
import ctypes as C
import gc

import numpy as np
import pytest

import median_oracle as MO
import welch_pfb_oracle as PO
from oracle import ref_cpu as R
from stat_support import FS, recipe_field, welch_plan
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import SCALINGS, noise_tones
from test_welch_pfb_cpu import PARITY_CASES, parity_input, prototype

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1


def make_plan(ctx, hip, nfft, ntaps=None, hop=None, detrend=True, scaling='density', fftshift=False, trim=0, db=False):
    """a Welch plan with nperseg = nfft at hop `hop` (Hann: the window takes no part) and, with ntaps, its prototype"""
    plan = welch_plan(ctx, hip, nfft, nfft, 0 if hop is None else nfft - hop, detrend, scaling, fftshift, trim, db)
    if ntaps is not None:
        plan.set_prototype(prototype(nfft, ntaps))
        assert plan.ntaps == ntaps
    return plan


def proto32(nfft, ntaps):
    """the taps the plan holds: the oracle runs on the same float32 values"""
    return prototype(nfft, ntaps).astype(np.float32)


def check_row(row, ref, fftshift=False, trim=0, db=False, what=''):
    """one stream's row against the oracle's dict, every bin within RTOL -> the worst reading"""
    want = MO.shift_trim_db(ref['pfb'], fftshift, trim)
    row = np.asarray(row, np.float64)
    assert row.shape == want.shape and np.all(np.isfinite(row))
    lin = 10.0 ** (row / 10.0) if db else row
    err = float(np.max(np.abs(lin - want) / want))
    if what:
        print('pfb parity %s: %.2e' % (what, err))
    assert err <= RTOL, (what, err)
    return err


def run_dev(ctx, plan, x, nsamples, nstreams, stride):
    """pfb_dev on nstreams captures -> (rows [nstreams, out_len], M)"""
    m = plan.out_len
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * nstreams * m)
    try:
        ctx.h2d(d, x)
        M = plan.pfb_dev(d, nsamples, nstreams, stride, out)
        got = ctx.d2h(out, (nstreams, m), np.float32)
    finally:
        ctx.free(d)
        ctx.free(out)
    return got, M


# ---- 1. parity at every size ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,ntaps,hop,M,detrend,scaling,fftshift,trim,db,offset', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, ntaps, hop, M, detrend, scaling, fftshift, trim, db, offset):
    x = parity_input(nfft, ntaps, hop, M, offset)
    plan = make_plan(ctx, hip, nfft, ntaps, hop, detrend, scaling, fftshift, trim, db)
    row = plan.pfb(x)
    assert plan.last_nseg == M and row.shape == (nfft - 2 * trim,) and row.dtype == np.float32
    recipe = plan.last_recipe()
    assert recipe.startswith('kernel=welchpfb nfft=%d ntaps=%d W=%d nseg=%d nstreams=1 bpc=' % (nfft, ntaps, M, M)), recipe
    ref = PO.pfb(x, nfft, ntaps, proto32(nfft, ntaps), nfft - hop, detrend, scaling, FS)
    assert ref['M'] == M
    check_row(row, ref, fftshift, trim, db, what=str((nfft, ntaps, hop, M, detrend, scaling)) + ' ' + recipe)
    plan.close()


# ---- 2. against the composition on the GPU --------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,ntaps,hop', [(256, 4, 256), (1024, 16, 512)])
def test_the_composition_gives_the_same_row(ctx, hip, nfft, ntaps, hop):
    """what a user had before: a Welch plan of P N points with the prototype as its window, every P-th bin kept"""
    L, M = nfft * ntaps, 6
    x = noise_tones(L + (M - 1) * hop, 123 + nfft)
    plan = make_plan(ctx, hip, nfft, ntaps, hop)
    row = plan.pfb(x).astype(np.float64)
    assert plan.last_nseg == M
    long = ctx.welch_plan(L, nperseg=L, noverlap=L - hop, window=proto32(nfft, ntaps), detrend=hip.DETREND_CONSTANT,
                          scaling=SCALINGS['density'], fs=FS)
    comp = long.exec(x).astype(np.float64)[::ntaps]
    assert long.last_nseg == M
    err = float(np.max(np.abs(row - comp) / comp))
    print('pfb %d x %d against exec of the %d-point plan, every %d-th bin: %.2e [%s]' % (nfft, ntaps, L, ntaps, err, plan.last_recipe()))
    assert err <= RTOL
    plan.close()
    long.close()


# ---- 3. streams ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,ntaps', [(64, 3), (4096, 4), (16384, 2)])
def test_no_read_leaves_the_stream(ctx, hip, nfft, ntaps):
    """three streams at a padded stride with NaN in the gaps: the last sample a stream's last frame reads is its last sample"""
    M, nstreams = 3, 3
    n = ntaps * nfft + (M - 1) * nfft
    stride = n + 100
    x = noise_tones(stride * nstreams, 90 + nfft)
    for s in range(nstreams):
        x[s * stride + n:(s + 1) * stride] = np.nan
    plan = make_plan(ctx, hip, nfft, ntaps)
    rows, got_m = run_dev(ctx, plan, x, n, nstreams, stride)
    assert got_m == M == plan.last_nseg
    for s in range(nstreams):
        check_row(rows[s], PO.pfb(x[s * stride:s * stride + n], nfft, ntaps, proto32(nfft, ntaps), fs=FS), what='stream %d of %d points' % (s, nfft))
    plan.close()


@pytest.mark.parametrize('nfft,ntaps,M,nstreams', [(4096, 4, 8, 64), (16384, 2, 5, 100)])
def test_many_streams_against_the_oracle_and_bit_identical(ctx, hip, nfft, ntaps, M, nstreams):
    n = ntaps * nfft + (M - 1) * nfft
    stride = n + 64
    x = noise_tones(stride * nstreams, 700 + nfft)
    x[stride:stride + n] = x[:n]      # streams 0 and 1 hold the same capture
    plan = make_plan(ctx, hip, nfft, ntaps)
    rows, got_m = run_dev(ctx, plan, x, n, nstreams, stride)
    recipe = plan.last_recipe()
    again, _ = run_dev(ctx, plan, x, n, nstreams, stride)
    plan.close()
    assert got_m == M and 'nstreams=%d ' % nstreams in recipe
    assert again.tobytes() == rows.tobytes()              # a repeated call
    assert rows[0].tobytes() == rows[1].tobytes()         # two identical streams of one launch
    if nfft == 16384:
        assert 1 <= recipe_field(recipe, 'W') < M, recipe      # a workgroup carries its row across the frames of its run
    h = proto32(nfft, ntaps)
    worst = max(check_row(rows[s], PO.pfb(x[s * stride:s * stride + n], nfft, ntaps, h, fs=FS)) for s in range(nstreams))
    print('pfb %d streams x %d frames of %d x %d [%s]: %.2e' % (nstreams, M, nfft, ntaps, recipe, worst))


# ---- 4. degenerate input -------------------------------------------------------------------------------------------------------------

def test_silence_and_a_constant_give_zero_rows(ctx, hip):
    for nfft, ntaps in ((256, 3), (4096, 8), (16384, 2)):
        n = ntaps * nfft + 2 * nfft
        plan = make_plan(ctx, hip, nfft, ntaps, fftshift=True)
        raw = make_plan(ctx, hip, nfft, ntaps, detrend=False)
        dbp = make_plan(ctx, hip, nfft, ntaps, db=True)
        for p in (plan, raw):
            row = p.pfb(np.zeros(n, np.complex64))
            assert row.shape == (nfft,) and not row.any()
        const = np.full(n, 3.0 - 2.0j, np.complex64)
        assert not plan.pfb(const).any()
        assert np.all(np.isneginf(dbp.pfb(const))) and np.all(np.isneginf(dbp.pfb(np.zeros(n, np.complex64))))
        assert raw.pfb(const).any()      # (without detrend the constant is a line)
        for p in (plan, raw, dbp):
            p.close()


@pytest.mark.parametrize('nfft,ntaps', [(256, 5), (4096, 4), (16384, 2)])
@pytest.mark.parametrize('detrend', [True, False])
def test_a_non_finite_sample_stays_in_its_stream(ctx, hip, nfft, ntaps, detrend):
    """a NaN, then an inf sample in stream 1 of three: its row reads NaN in every bin (linear and dB; never inf), the other
    streams are the clean launch's bit for bit; then a clean call on the same plan"""
    M, nstreams = 3, 3
    n = ntaps * nfft + (M - 1) * nfft
    x = noise_tones(n * nstreams, 5 + nfft)
    for db in (False, True):
        plan = make_plan(ctx, hip, nfft, ntaps, detrend=detrend, db=db)
        clean, _ = run_dev(ctx, plan, x, n, nstreams, n)
        assert np.all(np.isfinite(clean))
        for value in (complex(np.nan, 0.0), complex(0.0, np.inf), complex(-np.inf, 1.0)):
            bad = x.copy()
            bad[n + n - 1] = np.complex64(value)      # stream 1's last sample: its last frame alone holds it
            rows, _ = run_dev(ctx, plan, bad, n, nstreams, n)
            assert np.all(np.isnan(rows[1])), value
            assert rows[0].tobytes() == clean[0].tobytes() and rows[2].tobytes() == clean[2].tobytes()
        after, _ = run_dev(ctx, plan, x, n, nstreams, n)
        assert after.tobytes() == clean.tobytes()
        plan.close()


# ---- 5. leakage on the device --------------------------------------------------------------------------------------------------------

def test_a_strong_band_stays_out_of_its_neighbours(ctx, hip):
    """the CPU test's capture and conditions on the GPU's rows: the filter bank against the Hann Welch plan of the same size"""
    x = PO.leak_capture()
    plan = make_plan(ctx, hip, PO.LEAK_NFFT, PO.LEAK_TAPS)
    row = plan.pfb(x)
    assert plan.last_nseg == PO.LEAK_M
    hann = plan.exec(x)      # the plan's own window is Hann, no overlap
    PO.check_leakage(row, hann, 'GPU')
    plan.close()


# ---- 6. plan hygiene -----------------------------------------------------------------------------------------------------------------

def test_the_prototype_touches_no_other_call_and_a_second_one_takes_effect(ctx, hip):
    nfft = 1024
    x = noise_tones(nfft * 12 + 17, 77)
    plan = make_plan(ctx, hip, nfft)
    before = plan.exec(x)
    plan.set_prototype(prototype(nfft, 4))
    assert plan.exec(x).tobytes() == before.tobytes()
    four = plan.pfb(x)
    assert plan.last_nseg == 12 - 4 + 1
    assert plan.exec(x).tobytes() == before.tobytes() and plan.last_nseg == 12
    check_row(four, PO.pfb(x, nfft, 4, proto32(nfft, 4), fs=FS), what='P = 4')
    plan.set_prototype(prototype(nfft, 8), ntaps=8)      # a second prototype replaces the first, and M follows
    eight = plan.pfb(x)
    assert plan.last_nseg == 12 - 8 + 1 and ' ntaps=8 ' in plan.last_recipe()
    check_row(eight, PO.pfb(x, nfft, 8, proto32(nfft, 8), fs=FS), what='P = 8 on the same plan')
    assert plan.exec(x).tobytes() == before.tobytes()
    plan.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------

PF_MTM = "the filter-bank PSD is not available on a multitaper plan: its segments' transforms are Welch's (oth_welch_plan)"
PF_MEDIAN = ('the filter-bank PSD is not available with OTH_AVERAGE_MEDIAN: its rows are means over segments '
             '(oth_plan_set_average(OTH_AVERAGE_MEAN) first)')
PF_SIZE = 'the filter-bank PSD takes a transform length that is a power of two from 64 to 16384, not %d'
PF_NPERSEG = 'the filter-bank PSD folds whole transform lengths: it takes a plan with nperseg == nfft, not 48 and 64'
PF_NONE = 'the filter-bank PSD needs its prototype: call oth_welch_set_prototype on this plan'
PF_STREAMS = 'the filter-bank PSD takes at most 65535 streams per launch'
PF_SHORT = 'input shorter than ntaps * nfft (4 * 64 samples)'
SP_TAPS, SP_NULL = 'ntaps must lie in 2 ... 16', 'h is NULL'
SP_FINITE, SP_ZERO = 'every tap of the prototype must be finite', 'the prototype is all zero'
SP_SUM = 'OTH_SCALE_SPECTRUM needs a prototype with a non-zero sum'
BAD, STRIDE = 'bad argument', 'stream_stride < nsamples'


def test_every_refusal_with_its_code_and_text(ctx, hip):
    N, P, NS = 64, 4, 64 * 7
    x = R.synth_iq(3 * NS, 4711)
    d_in, d_out = ctx.alloc(x.nbytes), ctx.alloc(4 * 4 * N)
    host = np.zeros(N, np.float32)
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    taps = proto32(N, P)
    plans = dict(w=make_plan(ctx, hip, N, P), none=make_plan(ctx, hip, N), wmed=make_plan(ctx, hip, N),
                 w32=make_plan(ctx, hip, 32), w100=make_plan(ctx, hip, 100), w32k=make_plan(ctx, hip, 32768),
                 pad=welch_plan(ctx, hip, N, 48), spec=make_plan(ctx, hip, N, scaling='spectrum'),
                 m=ctx.mtm_plan(N, nw=2.0, ntapers=3))
    plans['wmed'].set_prototype(taps)      # (the prototype goes in before the median)
    plans['wmed'].set_average('median')

    def answer(call):
        gc.collect()
        before = hip.live_resources()
        rc = call()
        return rc, ctx.lib.oth_last_error(ctx.h).decode(), tuple(np.subtract(hip.live_resources(), before))

    def setter(key, ntaps, h):
        ptr = None if h is None else np.ascontiguousarray(h, np.float32).ctypes.data_as(fp)
        return answer(lambda: ctx.lib.oth_welch_set_prototype(plans[key].h, ntaps, ptr))

    def host_form(key, src=x, n=NS, out=host):
        return answer(lambda: ctx.lib.oth_welch_pfb(plans[key].h, None if src is None else src.ctypes.data_as(vp), n, 0,
                                                    None if out is None else out.ctypes.data_as(fp), None))

    def dev_form(key, src=d_in, n=NS, ns=1, stride=NS, out=d_out):
        return answer(lambda: ctx.lib.oth_welch_pfb_dev(plans[key].h, vp(src) if src else None, n, ns, stride, vp(out) if out else None, None))

    try:
        ctx.h2d(d_in, x)
        wavy = taps.copy()
        wavy[5] = np.nan
        odd = np.tile(np.array([1.0, -1.0], np.float32), N * P // 2)      # sums to zero
        table = [
            # the setter: the plan's kind, then its arguments
            (setter('m', P, taps), UNSUPPORTED, PF_MTM), (setter('wmed', P, taps), UNSUPPORTED, PF_MEDIAN),
            (setter('w32', P, np.ones(32 * P)), UNSUPPORTED, PF_SIZE % 32), (setter('w100', P, np.ones(100 * P)), UNSUPPORTED, PF_SIZE % 100),
            (setter('w32k', 2, np.ones(8)), UNSUPPORTED, PF_SIZE % 32768), (setter('pad', P, taps), UNSUPPORTED, PF_NPERSEG),
            (setter('w', 1, taps), INVALID, SP_TAPS), (setter('w', 17, taps), INVALID, SP_TAPS), (setter('w', 0, taps), INVALID, SP_TAPS),
            (setter('w', P, None), INVALID, SP_NULL), (setter('w', P, wavy), INVALID, SP_FINITE),
            (setter('w', P, np.where(np.arange(N * P) == 9, np.inf, taps)), INVALID, SP_FINITE),
            (setter('w', P, np.zeros(N * P)), INVALID, SP_ZERO), (setter('spec', P, odd), INVALID, SP_SUM),
            # two at once: the plan's kind goes in front of the arguments, the tap count in front of the taps
            (setter('m', 99, None), UNSUPPORTED, PF_MTM), (setter('w', 17, None), INVALID, SP_TAPS),
        ]
        for form in (host_form, dev_form):
            table += [
                (form('m'), UNSUPPORTED, PF_MTM), (form('wmed'), UNSUPPORTED, PF_MEDIAN), (form('w32'), UNSUPPORTED, PF_SIZE % 32),
                (form('pad'), UNSUPPORTED, PF_NPERSEG), (form('none'), UNSUPPORTED, PF_NONE),
                (form('w', src=None), INVALID, BAD), (form('w', out=None), INVALID, BAD), (form('w', n=P * N - 1), INVALID, PF_SHORT),
                # two at once: no prototype goes in front of a NULL input, the plan's kind in front of a short input
                (form('none', src=None), UNSUPPORTED, PF_NONE), (form('wmed', n=1), UNSUPPORTED, PF_MEDIAN),
            ]
        table += [
            (dev_form('w', ns=0), INVALID, BAD), (dev_form('w', ns=3, stride=NS - 1), INVALID, STRIDE),
            (dev_form('w', ns=70000), UNSUPPORTED, PF_STREAMS),
            # two at once: a NULL output in front of the stream limit, the stride in front of the length
            (dev_form('w', out=None, ns=70000), INVALID, BAD), (dev_form('w', n=P * N - 1, ns=3, stride=P * N - 2), INVALID, STRIDE),
        ]
        for i, ((rc, said, left), code, text) in enumerate(table):
            print(i, rc, repr(said), left)
            assert (rc, said) == (code, text), i
            assert left == (0, 0, 0), i      # refused before anything is allocated or staged
        # the refused setters left the prototype, and the plans go on working
        row = plans['w'].pfb(x[:NS])
        assert plans['w'].last_nseg == 4
        check_row(row, PO.pfb(x[:NS], N, P, taps, fs=FS), what='after the refusals')
        assert setter('spec', P, taps)[0] == 0 and plans['spec'].pfb(x[:NS]).shape == (N,)
        assert plans['w'].pfb(x[:P * N]).shape == (N,) and plans['w'].last_nseg == 1      # exactly one frame is served
        for key in ('m', 'wmed', 'pad', 'none'):
            assert plans[key].exec(x[:NS]).shape == (N,)
        plans['wmed'].set_average('mean')
        assert plans['wmed'].pfb(x[:NS]).tobytes() == row.tobytes()      # ... and the mean is served, with the prototype it kept
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
        for p in plans.values():
            p.close()


def test_set_prototype_checks_the_length_in_python(ctx, hip):
    plan = make_plan(ctx, hip, 64)
    for h, ntaps in ((np.ones(64 * 3 + 1), None), (np.ones(0), None), (np.ones(64 * 3), 4)):
        with pytest.raises(ValueError):
            plan.set_prototype(h, ntaps)
    with pytest.raises(hip.HipError) as ei:
        plan.set_prototype(np.ones(64))      # ntaps = 1 from the length: the library's refusal
    assert ei.value.code == INVALID and SP_TAPS in str(ei.value)
    plan.close()


# ---- 8. helpers ------------------------------------------------------------------------------------------------------------------------

def test_helpers_against_the_oracle(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    Sf, N = 1000000, 1024
    x = R.synth_iq(40000, 41)[:N * 20 + 300]
    for ntaps in (8, 4):
        ref = np.fft.fftshift(PO.pfb(x, N, ntaps, proto32(N, ntaps), fs=float(Sf))['pfb'])
        kw = {} if ntaps == 8 else {'ntaps': ntaps}      # 8 taps by default
        assert np.isclose(T.pfb_power_estimate(x, N, Sf, ctx=ctx, **kw), ref.sum(), rtol=1e-5)
        axis, db = T.pfb_plot_dB(x, Sf, 433e6, N, ctx=ctx, **kw)
        assert np.allclose(axis, np.fft.fftshift(np.fft.fftfreq(N, 1.0 / Sf)) + 433e6)
        assert np.max(np.abs(np.asarray(db) - 10 * np.log10(ref + 1e-20))) < 10 * np.log10(1 + RTOL)
        Fr = float(Sf) / N
        bb = R.frange(-Sf // 2, Sf // 2, 50e3)
        psd, ax, plc = T.src_power_pfb(x, len(x), N, Fr, Sf, bb, 25e3 / Fr, ctx=ctx, **kw)
        assert np.max(np.abs(psd - ref) / ref) <= RTOL and np.allclose(ax, np.fft.fftshift(np.fft.fftfreq(N, 1.0 / Sf)))
        assert np.allclose(plc, R._channel_sums(ref, Fr, Sf, bb, 25e3 / Fr), rtol=1e-4)
