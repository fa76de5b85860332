"""What ofdm_tools._hip passes to the C library, pinned without a library and without a GPU.

A recording stand-in takes the place of the loaded library: it checks every call against _hip.SIGNATURES (argument count,
every argument acceptable to the declared type), records (symbol, arguments) with the arguments normalised by meaning - a
pointer is its address, NULL is None, a byref is a marker, a number stays - writes a fixed count through every uint64_t *
that came as byref, and returns OTH_OK.  The expectations below are written out by hand, one tuple per call: argument order,
the NULL of a row left out, src_is_device, strides and the defaults the binding resolves itself.  The GPU suites check the
same things only by way of a refusal or a fault on a device."""
import contextlib
import ctypes as C
import functools
import numbers
import threading

import numpy as np
import pytest

from ofdm_tools import _hip, windows

OTH_ERR_INVALID = -1
CH, PH, NEW = 0xC0, 0xA0, 0xBEE0      # the stand-in context's handle, a plan's / chain's / channelizer's, one the library hands out
M, NFFT = 5, 8                        # out_len and nfft of the stand-in plans
COUNT = 7                             # what the library writes through a uint64_t * given as byref
UNTOUCHED = -5                        # last_nseg before a call
R = '<byref>'
BUF = '<buffer>'


class _Some(object):
    """the address of a buffer the method keeps to itself: equal to any address but NULL"""

    def __eq__(self, other):
        return isinstance(other, int) and other != 0

    def __repr__(self):
        return 'SOME'


SOME = _Some()

# arrays the binding builds itself and does not hand back are read through the pointer instead: symbol -> {argument:
# the argument that holds the element count, or a function of the arguments}
READS = {
    'oth_cp_sync': {5: 4, 6: 4},
    'oth_cp_sync_dev': {6: 5, 7: 5},
    'oth_synth_iq': {5: 4, 6: 4},
    'oth_welch_set_cycles': {2: 1},
    'oth_welch_set_lags': {2: 1},
    'oth_welch_set_prototype': {2: lambda args: args[1] * NFFT},
    'oth_mtm_plan': {6: 4},
    'oth_mtm_csd_plan': {6: 4},
    'oth_mtm_set_ratios': {1: lambda args: 3},
}
INT_BYREF = {'oth_plan_out_len': M}      # what goes through an int * given as byref (default: Lib.ready)


class Lib(object):
    """The stand-in.  rc: what every call returns, or with fail_at only the call of that index (the others OTH_OK)."""

    def __init__(self, rc=_hip.OK, fail_at=None):
        self.calls, self.keep, self.fills = [], [], {}
        self.rc, self.fail_at, self.count, self.ready = rc, fail_at, COUNT, 1

    def __getattr__(self, name):
        if name not in _hip.SIGNATURES:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _write(self, name, t, obj):
        if t is _hip._u64p:      # (and size_t *: the same ctypes type where both have 64 bits)
            obj.value = self.count
        elif t is _hip._pp:
            obj.value = NEW
        elif t is C.POINTER(C.c_int):
            obj.value = INT_BYREF.get(name, self.ready)
        elif t is C.POINTER(C.c_double):
            obj.value = 0.5
        else:
            raise AssertionError('%s: byref for %r' % (name, t))

    def _call(self, name, *args):
        res, types = _hip.SIGNATURES[name]
        if res is C.c_char_p:      # oth_last_error / oth_strerror
            return b'stand-in detail'
        assert len(args) == len(types), (name, len(args), len(types))
        norm = []
        for i, (a, t) in enumerate(zip(args, types)):
            if type(a).__name__ == 'CArgObject':
                self._write(name, t, a._obj)
                norm.append(R)
                continue
            t.from_param(a)      # raises what a real call would raise
            n = READS.get(name, {}).get(i)
            if n is not None and a is not None:
                norm.append(tuple(C.cast(a, t)[:n(args) if callable(n) else args[n]]))
            else:
                norm.append(self._norm(a, t))
        index = len(self.calls)
        self.calls.append((name, tuple(norm)))
        for i, rows in self.fills.get(name, {}).items():
            C.memmove(args[i], rows.ctypes.data, rows.nbytes)
        return self.rc if self.fail_at in (None, index) else _hip.OK

    @staticmethod
    def _norm(a, t):
        if a is None:
            return None
        if t is C.c_char_p:
            return BUF if isinstance(a, C.Array) else a
        if t is C.c_void_p or issubclass(t, C._Pointer):
            if isinstance(a, numbers.Integral):
                return int(a) or None
            return C.cast(a, C.c_void_p).value
        return a


def adr(a):
    return a.ctypes.data


def c64(n, *shape):
    return (np.arange(n * int(np.prod(shape or (1,)))) * (1 - 0.5j)).astype(np.complex64).reshape(shape + (n,))


def f32(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)


def i32(*v):
    return np.array(v, np.int32)


@contextlib.contextmanager
def loaded(lib):
    old = _hip.load
    _hip.load = lambda: lib
    try:
        yield
    finally:
        _hip.load = old


@contextlib.contextmanager
def slepian(tapers, ratios):
    """windows.dpss (a call of the library of its own) out of the way of the multitaper constructor"""
    old = windows.dpss
    windows.dpss = lambda n, nw, k, return_ratios=False: (tapers, ratios)
    try:
        yield
    finally:
        windows.dpss = old


def ctx_of(lib):
    ctx = object.__new__(_hip.Context)
    ctx.lib, ctx.h, ctx.device, ctx.stream, ctx._plans_lock = lib, C.c_void_p(CH), 0, None, threading.Lock()
    lib.keep.append(ctx)      # (alive until the stand-in goes: no destroy call from __del__ inside a trace)
    return ctx


def plan_of(lib, cls=_hip.WelchPlan, **attrs):
    p = object.__new__(cls)
    p.ctx, p.h, p.out_len, p.last_nseg = ctx_of(lib), C.c_void_p(PH), M, UNTOUCHED
    p.nfft, p.nperseg, p.noverlap, p.step, p.ntapers = NFFT, NFFT, NFFT // 2, NFFT // 2, 3
    p._tickets, p._last_ticket, p._tickets_lock = set(), 0, threading.Lock()
    p.__dict__.update(attrs)
    lib.keep.append(p)
    return p


def chain_of(lib):
    c = object.__new__(_hip.Chain)
    c.ctx, c.h, c.nfft = ctx_of(lib), C.c_void_p(PH), NFFT
    lib.keep.append(c)
    return c


def chan_of(lib):
    c = object.__new__(_hip.Channelizer)
    c.ctx, c.h, c.nchan, c.decim, c.taps = ctx_of(lib), C.c_void_p(PH), 64, 32, 8
    lib.keep.append(c)
    return c


def kept(lib, obj):
    lib.keep.append(obj)
    return obj


def rows_ok(rows, n, shape=(M,), dtype=np.float32):
    assert len(rows) == n and all(isinstance(r, np.ndarray) and r.shape == shape and r.dtype == dtype for r in rows)


CASES = []


def case(fn):
    CASES.append(fn)
    return fn


# ---- Context -----------------------------------------------------------------------------------------------------------

@case
def ctx_create(lib):
    with loaded(lib):
        ctx = kept(lib, _hip.Context(2))
    assert (ctx.h.value, ctx.device, ctx.stream, ctx.lib) == (NEW, 2, None, lib)
    return [('oth_ctx_create', (2, R))]


@case
def ctx_create_on_stream(lib):
    with loaded(lib):
        ctx = kept(lib, _hip.Context(1, stream=0x5000))
    assert (ctx.h.value, ctx.device, ctx.stream) == (NEW, 1, 0x5000)
    return [('oth_ctx_create_on_stream', (1, 0x5000, R))]


@case
def ctx_close(lib):
    ctx, plan = ctx_of(lib), plan_of(lib)
    ctx._plans = {'k': plan}
    ctx.close()
    ctx.close()
    assert ctx.h is None and plan.h is None and '_plans' not in ctx.__dict__
    return [('oth_plan_destroy', (PH,)), ('oth_ctx_destroy', (CH,))]


@case
def ctx_plumbing(lib):
    ctx = ctx_of(lib)
    ctx.sync()
    assert ctx.device_name() == ''
    ctx.set_timing(True)
    ctx.set_timing(0)
    assert ctx.get_timing() == (0.5, COUNT) and ctx.get_timing(reset=False) == (0.5, COUNT)
    assert ctx.alloc(64) == NEW
    ctx.free(0x1000)
    assert ctx.stream_read_probe(0x1000, 4096) == 0.5 and ctx.stream_read_probe(0x1000, 4096, repeats=2) == 0.5
    assert ctx.iq_power(0x1000, 100) == (0.5 + 0.5j, 0.5)
    return [('oth_ctx_sync', (CH,)), ('oth_ctx_device_name', (CH, BUF, 256)), ('oth_ctx_set_timing', (CH, 1)),
            ('oth_ctx_set_timing', (CH, 0)), ('oth_ctx_get_timing', (CH, R, R, 1)), ('oth_ctx_get_timing', (CH, R, R, 0)),
            ('oth_dev_alloc', (CH, 64, R)), ('oth_dev_free', (CH, 0x1000)),
            ('oth_stream_read_probe', (CH, 0x1000, 4096, 5, R)), ('oth_stream_read_probe', (CH, 0x1000, 4096, 2, R)),
            ('oth_iq_power', (CH, 0x1000, 100, R, R, R))]


@case
def ctx_copies(lib):
    ctx, a = ctx_of(lib), f32(2, 3)
    ctx.h2d(0x1000, a)
    out = ctx.d2h(0x2000, (2, 3), np.float32)
    assert out.shape == (2, 3) and out.dtype == np.float32
    return [('oth_memcpy_h2d', (CH, 0x1000, adr(a), 24)), ('oth_memcpy_d2h', (CH, adr(out), 0x2000, 24))]


@case
def ctx_synth_iq(lib):
    ctx = ctx_of(lib)
    ctx.synth_iq(0x1000, 100, 9)
    ctx.synth_iq(0x1000, 100, 9, tones=[(1.0, 0.25), (0.5, -0.125)], dc=1 + 2j)
    return [('oth_synth_iq', (CH, 0x1000, 100, 9, 0, None, None, 0.0, 0.0)),
            ('oth_synth_iq', (CH, 0x1000, 100, 9, 2, (1.0, 0.5), (0.25, -0.125), 1.0, 2.0))]


HYPS = [(16, 4), (32, 8)]


@case
def ctx_cp_sync_host(lib):
    ctx, x = ctx_of(lib), c64(100)
    gamma, phi, est, nsym = ctx.cp_sync(x, HYPS)
    assert [g.shape for g in gamma] == [(20,), (40,)] and all(g.dtype == np.complex64 for g in gamma)
    assert [p.shape for p in phi] == [(20,), (40,)] and all(p.dtype == np.float32 for p in phi)
    assert (est.shape, est.dtype, nsym.shape, nsym.dtype) == ((2, 4), np.float32, (2,), np.uint64)
    return [('oth_cp_sync', (CH, adr(x), 100, 0, 2, (16, 32), (4, 8), 1.0, 40, adr(gamma[0]), adr(phi[0]), adr(est), adr(nsym)))]


@case
def ctx_cp_sync_device_no_rows(lib):
    gamma, phi, est, nsym = ctx_of(lib).cp_sync(0x1000, HYPS, rho=0.5, nsamples=100, want_rows=False)
    assert gamma is None and phi is None and est.shape == (2, 4) and nsym.shape == (2,)
    return [('oth_cp_sync', (CH, 0x1000, 100, 1, 2, (16, 32), (4, 8), 0.5, 40, None, None, adr(est), adr(nsym)))]


@case
def ctx_cp_sync_dev_defaults(lib):
    nsym = ctx_of(lib).cp_sync_dev(0x1000, 100, HYPS, 0x2000)
    assert (nsym.shape, nsym.dtype) == ((2,), np.uint64)
    return [('oth_cp_sync_dev', (CH, 0x1000, 100, 1, 100, 2, (16, 32), (4, 8), 1.0, 40, None, None, 0x2000, adr(nsym)))]


@case
def ctx_cp_sync_dev_all(lib):
    nsym = ctx_of(lib).cp_sync_dev(0x1000, 100, HYPS, 0x2000, gamma_dev=0x3000, phi_dev=0x4000, row_stride=64, rho=0.25,
                                   nstreams=3, stride=128)
    return [('oth_cp_sync_dev', (CH, 0x1000, 100, 3, 128, 2, (16, 32), (4, 8), 0.25, 64, 0x3000, 0x4000, 0x2000, adr(nsym)))]


@case
def ctx_small_ops(lib):
    ctx, rows, psd, lo, hi = ctx_of(lib), f32(4, 8), f32(16), i32(1, 5), i32(3, 9)
    mean = ctx.rows_group_mean(rows, 2)
    power = ctx.channel_power(psd, 3, lo, hi)
    power2, ma = ctx.channel_power(psd, 3, lo, hi, want_movavg=True)
    mask, noise = ctx.bin_threshold(rows, 3, 1.5)
    assert (mean.shape, power.shape, power2.shape, ma.shape) == ((2, 8), (2,), (2,), (16,))
    assert (mask.shape, mask.dtype, noise.shape, noise.dtype) == ((4, 8), np.uint8, (4,), np.float32)
    return [('oth_rows_group_mean', (CH, adr(rows), 4, 8, 2, adr(mean))),
            ('oth_channel_power', (CH, adr(psd), 16, 3.0, 2, adr(lo), adr(hi), adr(power), None)),
            ('oth_channel_power', (CH, adr(psd), 16, 3.0, 2, adr(lo), adr(hi), adr(power2), adr(ma))),
            ('oth_bin_threshold', (CH, adr(rows), 4, 8, 3.0, 1.5, adr(mask), adr(noise)))]


@case
def ctx_scan_decide(lib):
    ctx, lo, hi = ctx_of(lib), i32(1, 5), i32(3, 9)
    mask, noise, power = ctx.scan_decide_dev(0x1000, 2, 8, 3, 1.5)
    mask2, noise2, power2 = ctx.scan_decide_dev(0x1000, 2, 8, 3, 1.5, lo, hi, want_mask=False)
    assert (mask.shape, mask.dtype, noise.shape, power.shape) == ((2, 8), np.uint8, (2,), (2, 0))
    assert mask2 is None and noise2.shape == (2,) and (power2.shape, power2.dtype) == ((2, 2), np.float32)
    assert ctx.scan_decide_dev_out(0x1000, 2, 8, 3, 1.5, lo, hi, 0x2000, 0x3000) is None
    ctx.scan_decide_dev_out(0x1000, 2, 8, 3, 1.5, (), (), 0x2000, 0x3000, mask_dptr=0x4000)
    return [('oth_scan_decide_dev', (CH, 0x1000, 2, 8, 3.0, 1.5, 0, None, None, adr(mask), adr(noise), None)),
            ('oth_scan_decide_dev', (CH, 0x1000, 2, 8, 3.0, 1.5, 2, adr(lo), adr(hi), None, adr(noise2), adr(power2))),
            ('oth_scan_decide_dev_out', (CH, 0x1000, 2, 8, 3.0, 1.5, 2, adr(lo), adr(hi), None, 0x2000, 0x3000)),
            ('oth_scan_decide_dev_out', (CH, 0x1000, 2, 8, 3.0, 1.5, 0, None, None, 0x4000, 0x2000, None))]


@case
def ctx_xcorr_fac(lib):
    ctx, a, b = ctx_of(lib), c64(10), c64(12)
    xc, ac = ctx.xcorr(a, b, 8), ctx.fac(a, 8)
    assert (xc.shape, xc.dtype, ac.shape, ac.dtype) == ((4,), np.float32, (4,), np.float32)
    return [('oth_xcorr', (CH, adr(a), 8, adr(b), 8, 8, adr(xc))), ('oth_fac', (CH, adr(a), 8, 8, adr(ac)))]


# ---- the constructors, through the context's factories -----------------------------------------------------------------

@case
def welch_plan_defaults(lib):
    p = kept(lib, ctx_of(lib).welch_plan(8))
    assert (p.h.value, p.out_len, p.nfft, p.nperseg, p.noverlap, p.step, p.average) == (NEW, M, 8, 8, 4, 4, _hip.AVERAGE_MEAN)
    assert p.outstanding == 0 and not hasattr(p, 'last_nseg')
    return [('oth_welch_plan', (CH, 8, 8, 4, None, 1, 1, 1.0, 0, 0, R)), ('oth_plan_out_len', (NEW, R))]


@case
def welch_plan_everything(lib):
    w = f32(6)
    p = kept(lib, ctx_of(lib).welch_plan(8, nperseg=6, noverlap=2, window=w, detrend=_hip.DETREND_NONE, scaling=_hip.SCALE_SPECTRUM,
                                         fs=2.0, fftshift=True, trim_bins=1, db=True, kernel=_hip.KERNEL_GENERIC, average='median'))
    assert (p.nperseg, p.noverlap, p.step, p.average) == (6, 2, 4, _hip.AVERAGE_MEDIAN)
    return [('oth_welch_plan', (CH, 8, 6, 2, adr(w), 0, 3, 2.0, 1, 1, R)), ('oth_plan_out_len', (NEW, R)),
            ('oth_plan_set_output_db', (NEW, 1)), ('oth_plan_set_kernel', (NEW, 1)), ('oth_plan_set_average', (NEW, 1))]


@case
def mtm_plan_own_tapers(lib):
    t = f32(2, 8)
    p = kept(lib, ctx_of(lib).mtm_plan(8, tapers=t))
    assert type(p) is _hip.MtmPlan and (p.h.value, p.out_len, p.ntapers, p.noverlap, p.ratios) == (NEW, M, 2, 0, None)
    assert adr(p.tapers) == adr(t)
    return [('oth_mtm_plan', (CH, 8, 8, 0, 2, adr(t), None, 1, 1, 1.0, 0, 0, R)), ('oth_plan_out_len', (NEW, R))]


@case
def mtm_plan_slepian_eigen(lib):
    ratios = np.array([0.75, 0.5, 0.25])
    with slepian(np.ones((3, 8)), ratios):
        p = kept(lib, ctx_of(lib).mtm_plan(8, nw=2.0, weights='eigen', db=True))
    assert p.ntapers == 3 and p.ratios is ratios and p.tapers.dtype == np.float32
    return [('oth_mtm_plan', (CH, 8, 8, 0, 3, adr(p.tapers), (0.75, 0.5, 0.25), 1, 1, 1.0, 0, 0, R)), ('oth_plan_out_len', (NEW, R)),
            ('oth_plan_set_output_db', (NEW, 1)), ('oth_mtm_set_ratios', (NEW, (0.75, 0.5, 0.25)))]


@case
def mtm_csd_plan_weights(lib):
    t = f32(3, 8)
    p = kept(lib, ctx_of(lib).mtm_csd_plan(8, noverlap=4, tapers=t, weights=[1, 2, 0], detrend=0, scaling=0, fs=4.0, fftshift=True,
                                           trim_bins=2))
    assert type(p) is _hip.MtmCsdPlan and p.ntapers == 3
    return [('oth_mtm_csd_plan', (CH, 8, 8, 4, 3, adr(t), (1.0, 2.0, 0.0), 0, 0, 4.0, 1, 2, R)), ('oth_plan_out_len', (NEW, R))]


@case
def chain_create(lib):
    ctx, w = ctx_of(lib), f32(8)
    c1 = kept(lib, ctx.chain(8))
    c2 = kept(lib, ctx.chain(8, window=w, fftshift=False, epilogue=_hip.EPI_MAG, keep_one_in_n=4))
    assert (c1.h.value, c1.nfft, c2.h.value) == (NEW, 8, NEW)
    return [('oth_chain_create', (CH, 8, None, 1, 1, 1, R)), ('oth_chain_create', (CH, 8, adr(w), 0, 0, 4, R))]


@case
def channelizer_create(lib):
    c = kept(lib, ctx_of(lib).channelizer(64, prototype=np.ones(512)))
    assert (c.h.value, c.nchan, c.decim, c.taps, c.prototype.dtype) == (NEW, 64, 32, 8, np.float32)
    c2 = kept(lib, ctx_of(lib).channelizer(64, decim=16, taps=2, prototype=np.ones(128)))
    return [('oth_channelizer_create', (CH, 64, 32, 8, adr(c.prototype), R)), ('oth_channelizer_create', (CH, 64, 16, 2, adr(c2.prototype), R))]


# ---- WelchPlan -----------------------------------------------------------------------------------------------------------

@case
def plan_setters(lib):
    p = plan_of(lib)
    p.set_kernel(_hip.KERNEL_TUNED)
    p.set_tuning()
    p.set_tuning('ws', 1, 20, 4)
    p.set_schedule(_hip.SCHED_INTERLEAVED)
    p.set_hostwait(True)
    p.set_hostwait(False)
    p.set_average('median')
    assert p.average == _hip.AVERAGE_MEDIAN and p.last_nseg == UNTOUCHED
    assert p.last_recipe() == ''
    p.reset()
    return [('oth_plan_set_kernel', (PH, 2)), ('oth_plan_set_tuning', (PH, None, -1, 0, 0)), ('oth_plan_set_tuning', (PH, b'ws', 1, 20, 4)),
            ('oth_plan_set_schedule', (PH, 1)), ('oth_plan_set_hostwait', (PH, 1)), ('oth_plan_set_hostwait', (PH, 0)),
            ('oth_plan_set_average', (PH, 1)), ('oth__debug_last_recipe', (PH, BUF, 512)), ('oth_welch_reset', (PH,))]


@case
def plan_close(lib):
    p = plan_of(lib)
    p.close()
    p.close()
    assert p.h is None
    return [('oth_plan_destroy', (PH,))]


@case
def plan_segments(lib):
    p, x = plan_of(lib), c64(16)
    rows = p.segments(x)
    assert (rows.shape, rows.dtype, p.last_nseg) == ((3, M), np.float32, UNTOUCHED)
    assert p.segments_dev(0x1000, 100, 0x2000, 9) == COUNT and p.last_nseg == UNTOUCHED
    return [('oth_dev_alloc', (CH, 128, R)), ('oth_dev_alloc', (CH, 60, R)), ('oth_memcpy_h2d', (CH, NEW, adr(x), 128)),
            ('oth_welch_segments_dev', (PH, NEW, 16, NEW, 3, R)), ('oth_memcpy_d2h', (CH, adr(rows), NEW, 60)),
            ('oth_dev_free', (CH, NEW)), ('oth_dev_free', (CH, NEW)),
            ('oth_welch_segments_dev', (PH, 0x1000, 100, 0x2000, 9, R))]


@case
def plan_sk(lib):
    p, x = plan_of(lib), c64(64)
    sk = p.sk(x)
    assert p.last_nseg == COUNT
    both = p.sk(0x1000, return_psd=True, nsamples=100)
    rows_ok([sk], 1)
    rows_ok(both, 2)
    return [('oth_welch_sk', (PH, adr(x), 64, 0, adr(sk), None, R)), ('oth_welch_sk', (PH, 0x1000, 100, 1, adr(both[0]), adr(both[1]), R))]


@case
def plan_sk_dev(lib):
    p = plan_of(lib)
    assert p.sk_dev(0x1000, 100, 2, 128, 0x2000) == COUNT and p.last_nseg == COUNT
    p.sk_dev(0x1000, 100, 2, 128, 0x2000, psd_dev=0x3000)
    return [('oth_welch_sk_dev', (PH, 0x1000, 100, 2, 128, 0x2000, None, R)), ('oth_welch_sk_dev', (PH, 0x1000, 100, 2, 128, 0x2000, 0x3000, R))]


@case
def plan_cyclic(lib):
    p, x = plan_of(lib), c64(64)
    p.set_cycles([0.25, -0.125])
    assert p.ncycles == 2 and p.last_nseg == UNTOUCHED
    scf, coh = p.cyclic(x)
    assert p.last_nseg == COUNT
    scf2, coh2, psd = p.cyclic(0x1000, return_psd=True, nsamples=100)
    assert (scf.shape, scf.dtype, coh.shape, coh.dtype, psd.shape, psd.dtype) == ((2, M), np.complex64, (2, M), np.float32, (M,), np.float32)
    return [('oth_welch_set_cycles', (PH, 2, (0.25, -0.125))), ('oth_welch_cyclic', (PH, adr(x), 64, 0, adr(scf), adr(coh), None, R)),
            ('oth_welch_cyclic', (PH, 0x1000, 100, 1, adr(scf2), adr(coh2), adr(psd), R))]


@case
def plan_cyclic_dev(lib):
    p = plan_of(lib)
    assert p.cyclic_dev(0x1000, 100, 2, 128, 0x2000) == COUNT and p.last_nseg == COUNT
    p.cyclic_dev(0x1000, 100, 2, 128, 0x2000, scf_dev=0x3000, psd_dev=0x4000)
    return [('oth_welch_cyclic_dev', (PH, 0x1000, 100, 2, 128, None, 0x2000, None, R)),
            ('oth_welch_cyclic_dev', (PH, 0x1000, 100, 2, 128, 0x3000, 0x2000, 0x4000, R))]


@case
def plan_caf(lib):
    p, x = plan_of(lib), c64(64)
    p.set_lags([0, 8])
    assert p.nlags == 2 and p.last_nseg == UNTOUCHED
    caf = p.caf(x)
    assert p.last_nseg == COUNT
    caf2, r = p.caf(0x1000, return_r=True, nsamples=100)
    assert (caf.shape, caf.dtype, r.shape, r.dtype) == ((2, M), np.float32, (2,), np.complex64)
    return [('oth_welch_set_lags', (PH, 2, (0, 8))), ('oth_welch_caf', (PH, adr(x), 64, 0, adr(caf), None, R)),
            ('oth_welch_caf', (PH, 0x1000, 100, 1, adr(caf2), adr(r), R))]


@case
def plan_caf_dev(lib):
    p = plan_of(lib)
    assert p.caf_dev(0x1000, 100, 2, 128, 0x2000) == COUNT and p.last_nseg == COUNT
    p.caf_dev(0x1000, 100, 2, 128, 0x2000, r_dev=0x3000)
    return [('oth_welch_caf_dev', (PH, 0x1000, 100, 2, 128, 0x2000, None, R)), ('oth_welch_caf_dev', (PH, 0x1000, 100, 2, 128, 0x2000, 0x3000, R))]


@case
def plan_pfb(lib):
    p, x, h = plan_of(lib), c64(64), [float(v) for v in range(16)]
    p.set_prototype(h)
    assert p.ntaps == 2
    p.set_prototype(h + h, ntaps=4)
    assert p.ntaps == 4 and p.last_nseg == UNTOUCHED
    out = p.pfb(x)
    assert p.last_nseg == COUNT
    out2 = p.pfb(0x1000, nsamples=100)
    rows_ok([out, out2], 2)
    p.last_nseg = UNTOUCHED
    assert p.pfb_dev(0x1000, 100, 2, 128, 0x2000) == COUNT and p.last_nseg == COUNT
    return [('oth_welch_set_prototype', (PH, 2, tuple(h))), ('oth_welch_set_prototype', (PH, 4, tuple(h + h))),
            ('oth_welch_pfb', (PH, adr(x), 64, 0, adr(out), R)), ('oth_welch_pfb', (PH, 0x1000, 100, 1, adr(out2), R)),
            ('oth_welch_pfb_dev', (PH, 0x1000, 100, 2, 128, 0x2000, R))]


@case
def plan_matrix(lib):
    p, x = plan_of(lib), c64(32, 2)
    packed = (np.arange(3 * M).reshape(3, M) * (1 + 2j) + 1j).astype(np.complex64)
    lib.fills['oth_welch_matrix'] = {5: packed}
    S, gcoh = p.matrix(x)
    assert p.last_nseg == COUNT and (S.shape, S.dtype, gcoh.shape, gcoh.dtype) == ((2, 2, M), np.complex64, (M,), np.float32)
    assert np.array_equal(S[0, 0], packed[0]) and np.array_equal(S[0, 1], packed[1]) and np.array_equal(S[1, 1], packed[2])
    assert np.array_equal(S[1, 0], np.conj(packed[1]))
    lib.fills.clear()
    S3 = p.matrix(0x1000, return_gcoh=False, nsamples=(3, 100))
    assert isinstance(S3, np.ndarray) and S3.shape == (3, 3, M)
    return [('oth_welch_matrix', (PH, adr(x), 32, 2, 0, SOME, adr(gcoh), R)), ('oth_welch_matrix', (PH, 0x1000, 100, 3, 1, SOME, None, R))]


@case
def plan_matrix_dev(lib):
    p = plan_of(lib)
    assert p.matrix_dev(0x1000, 100, 3, 128, s_dev=0x2000) == COUNT and p.last_nseg == COUNT
    p.matrix_dev(0x1000, 100, 3, 128, gcoh_dev=0x3000)
    p.matrix_dev(0x1000, 100, 3, 128, 0x2000, 0x3000)
    return [('oth_welch_matrix_dev', (PH, 0x1000, 100, 3, 128, 0x2000, None, R)), ('oth_welch_matrix_dev', (PH, 0x1000, 100, 3, 128, None, 0x3000, R)),
            ('oth_welch_matrix_dev', (PH, 0x1000, 100, 3, 128, 0x2000, 0x3000, R))]


@case
def plan_matrix_eig(lib):
    p, x = plan_of(lib), c64(32, 2)
    eig, vec = p.matrix_eig(x)
    assert p.last_nseg == COUNT and (eig.shape, eig.dtype, vec.shape, vec.dtype) == ((2, M), np.float32, (2, M), np.complex64)
    eig3 = p.matrix_eig(0x1000, of='G', return_vector=False, nsamples=(3, 100))
    assert isinstance(eig3, np.ndarray) and eig3.shape == (3, M)
    return [('oth_welch_matrix_eig', (PH, adr(x), 32, 2, 0, 0, adr(eig), adr(vec), R)),
            ('oth_welch_matrix_eig', (PH, 0x1000, 100, 3, 1, 1, adr(eig3), None, R))]


@case
def plan_matrix_eig_dev(lib):
    p = plan_of(lib)
    assert p.matrix_eig_dev(0x1000, 100, 3, 128, 'G', eig_dev=0x2000) == COUNT and p.last_nseg == COUNT
    p.matrix_eig_dev(0x1000, 100, 3, 128, _hip.EIG_OF_S, vec_dev=0x3000)
    p.matrix_eig_dev(0x1000, 100, 3, 128, 'S', 0x2000, 0x3000)
    return [('oth_welch_matrix_eig_dev', (PH, 0x1000, 100, 3, 128, 1, 0x2000, None, R)),
            ('oth_welch_matrix_eig_dev', (PH, 0x1000, 100, 3, 128, 0, None, 0x3000, R)),
            ('oth_welch_matrix_eig_dev', (PH, 0x1000, 100, 3, 128, 0, 0x2000, 0x3000, R))]


@case
def plan_steering(lib):
    p, d = plan_of(lib), np.arange(8.0).reshape(4, 2)
    p.set_steering(d, 0.25)
    assert p.ndir == 4
    p.set_steering([], 0)
    assert p.ndir == 0 and p.last_nseg == UNTOUCHED
    return [('oth_welch_set_steering', (PH, 4, 2, adr(d), 0.25)), ('oth_welch_set_steering', (PH, 0, 0, None, 0.0))]


@case
def plan_matrix_doa(lib):
    p, x = plan_of(lib, ndir=4), c64(32, 2)
    rows = p.matrix_doa(x, nsrc=1)
    assert p.last_nseg == COUNT and sorted(rows) == ['bartlett', 'capon', 'music']
    rows_ok(list(rows.values()), 3, (4, M))
    capon = p.matrix_doa(x, methods='capon')
    assert list(capon) == ['capon']
    some = p.matrix_doa(0x1000, of='G', nsrc=2, loading=0.5, methods=('music', 'bartlett'), nsamples=(3, 100))
    assert sorted(some) == ['bartlett', 'music']
    return [('oth_welch_matrix_doa', (PH, adr(x), 32, 2, 0, 0, 1, 0.0, adr(rows['bartlett']), adr(rows['capon']), adr(rows['music']), R)),
            ('oth_welch_matrix_doa', (PH, adr(x), 32, 2, 0, 0, 0, 0.0, None, adr(capon['capon']), None, R)),
            ('oth_welch_matrix_doa', (PH, 0x1000, 100, 3, 1, 1, 2, 0.5, adr(some['bartlett']), None, adr(some['music']), R))]


@case
def plan_matrix_doa_dev(lib):
    p = plan_of(lib)
    assert p.matrix_doa_dev(0x1000, 100, 3, 128, 'S', None, 0.0, capon_dev=0x2000) == COUNT and p.last_nseg == COUNT
    p.matrix_doa_dev(0x1000, 100, 3, 128, 'G', 2, 0.5, 0x3000, 0x2000, 0x4000)
    p.matrix_doa_dev(0x1000, 100, 3, 128, 'G', 2, 0.5, bartlett_dev=0x3000)
    p.matrix_doa_dev(0x1000, 100, 3, 128, 'G', 2, 0.5, music_dev=0x4000)
    return [('oth_welch_matrix_doa_dev', (PH, 0x1000, 100, 3, 128, 0, 0, 0.0, None, 0x2000, None, R)),
            ('oth_welch_matrix_doa_dev', (PH, 0x1000, 100, 3, 128, 1, 2, 0.5, 0x3000, 0x2000, 0x4000, R)),
            ('oth_welch_matrix_doa_dev', (PH, 0x1000, 100, 3, 128, 1, 2, 0.5, 0x3000, None, None, R)),
            ('oth_welch_matrix_doa_dev', (PH, 0x1000, 100, 3, 128, 1, 2, 0.5, None, None, 0x4000, R))]


@case
def plan_matrix_gcc(lib):
    p, x = plan_of(lib), c64(32, 2)
    delays, peaks, phases, rows = p.matrix_gcc(x)      # band=None: -4 ... 3; maxlag=None at upsample 1: 8 / 2 - 1
    assert p.last_nseg == COUNT and (rows.shape, rows.dtype) == ((1, 7), np.complex64)
    lib.fills['oth_welch_matrix_gcc'] = {11: np.arange(1, 10, dtype=np.float32)}
    out = p.matrix_gcc(0x1000, 'scot', band=(-2, 1), upsample=4, return_rows=False, nsamples=(3, 100))      # maxlag: 32 / 2 - 1
    assert len(out) == 3 and all(t.shape == (3, 3) and t.dtype == np.float32 for t in out)
    assert np.array_equal(out[0], [[0, 1, 4], [-1, 0, 7], [-4, -7, 0]])
    assert np.array_equal(out[1], [[1, 2, 5], [2, 1, 8], [5, 8, 1]])
    assert np.array_equal(out[2], [[0, 3, 6], [-3, 0, 9], [-6, -9, 0]])
    lib.fills.clear()
    rows2 = p.matrix_gcc(x, _hip.GCC_PLAIN, upsample=2, maxlag=2)[3]
    assert rows2.shape == (1, 5)
    return [('oth_welch_matrix_gcc', (PH, adr(x), 32, 2, 0, 1, -4, 3, 1, 3, adr(rows), SOME, R)),
            ('oth_welch_matrix_gcc', (PH, 0x1000, 100, 3, 1, 2, -2, 1, 4, 15, None, SOME, R)),
            ('oth_welch_matrix_gcc', (PH, adr(x), 32, 2, 0, 0, -4, 3, 2, 2, adr(rows2), SOME, R))]


@case
def plan_matrix_gcc_dev(lib):
    p = plan_of(lib)
    assert p.matrix_gcc_dev(0x1000, 100, 3, 128) == COUNT and p.last_nseg == COUNT
    p.matrix_gcc_dev(0x1000, 100, 3, 128, 'plain', (-2, 1), 4, None, 0x2000, 0x3000)
    p.matrix_gcc_dev(0x1000, 100, 3, 128, maxlag=0, gcc_dev=0x2000)
    p.matrix_gcc_dev(0x1000, 100, 3, 128, peak_dev=0x3000)
    return [('oth_welch_matrix_gcc_dev', (PH, 0x1000, 100, 3, 128, 1, -4, 3, 1, 3, None, None, R)),
            ('oth_welch_matrix_gcc_dev', (PH, 0x1000, 100, 3, 128, 0, -2, 1, 4, 15, 0x2000, 0x3000, R)),
            ('oth_welch_matrix_gcc_dev', (PH, 0x1000, 100, 3, 128, 1, -4, 3, 1, 0, 0x2000, None, R)),
            ('oth_welch_matrix_gcc_dev', (PH, 0x1000, 100, 3, 128, 1, -4, 3, 1, 3, None, 0x3000, R))]


@case
def plan_exec(lib):
    p, x = plan_of(lib), c64(64)
    out = p.exec(x)
    assert p.last_nseg == COUNT
    p.last_nseg = UNTOUCHED
    out2 = p.exec_device_src(0x1000, 100)
    assert p.last_nseg == COUNT
    rows_ok([out, out2], 2)
    return [('oth_welch_exec', (PH, adr(x), 64, 0, adr(out), R)), ('oth_welch_exec', (PH, 0x1000, 100, 1, adr(out2), R))]


@case
def plan_exec_copies_what_is_not_complex64(lib):
    p = plan_of(lib)
    x = np.arange(6, dtype=np.complex128).reshape(2, 3)
    p.exec(x)
    (name, args), = lib.calls
    assert args[1] != adr(x)
    return [('oth_welch_exec', (PH, SOME, 6, 0, SOME, R))]


@case
def plan_async(lib):
    p, x = plan_of(lib), c64(64)
    assert p.exec_async(x) == COUNT and p.exec_async(0x1000, nsamples=100) == COUNT
    assert p.outstanding == 1 and p.last_nseg == UNTOUCHED
    lib.ready = 0
    assert p.poll(COUNT) is None and p.outstanding == 1 and p.last_nseg == UNTOUCHED
    lib.ready = 1
    out = p.poll(COUNT)
    assert p.outstanding == 0 and p.last_nseg == COUNT
    p.last_nseg = UNTOUCHED
    out2 = p.wait(3)
    assert p.last_nseg == COUNT
    rows_ok([out, out2], 2)
    return [('oth_welch_exec_async', (PH, adr(x), 64, 0, R)), ('oth_welch_exec_async', (PH, 0x1000, 100, 1, R)),
            ('oth_welch_poll', (PH, COUNT, SOME, R, R)), ('oth_welch_poll', (PH, COUNT, adr(out), R, R)), ('oth_welch_wait', (PH, 3, adr(out2), R))]


@case
def plan_device_forms(lib):
    p, x = plan_of(lib), c64(64)
    assert p.exec_dev(0x1000, 100, 0x2000) == COUNT
    assert p.exec_dev(0x1000, 100, 0x2000, nstreams=3, stream_stride=128) == COUNT
    assert p.partial_dev(0x1000, 100, 0x2000) == COUNT
    assert p.scale_dev(0x2000, 31, 0x3000) is None
    assert p.accumulate(x) is None and p.last_nseg == UNTOUCHED
    out = p.finalize()
    assert p.last_nseg == COUNT
    rows_ok([out], 1)
    return [('oth_welch_exec_dev', (PH, 0x1000, 100, 1, 100, 0x2000, R)), ('oth_welch_exec_dev', (PH, 0x1000, 100, 3, 128, 0x2000, R)),
            ('oth_welch_partial_dev', (PH, 0x1000, 100, 0x2000, R)), ('oth_welch_scale_dev', (PH, 0x2000, 31, 0x3000)),
            ('oth_welch_accumulate', (PH, adr(x), 64)), ('oth_welch_finalize', (PH, adr(out), R))]


@case
def plan_csd(lib):
    p, x, y = plan_of(lib), c64(64), c64(64)
    host = p.csd(x, y)
    assert p.last_nseg == COUNT
    p.last_nseg = UNTOUCHED
    dev = p.csd_device_src(0x1000, 0x2000, 100)
    assert p.last_nseg == COUNT
    for pxx, pyy, pxy, cxy in (host, dev):
        rows_ok([pxx, pyy, cxy], 3)
        rows_ok([pxy], 1, dtype=np.complex64)
    return [('oth_csd_exec', (PH, adr(x), adr(y), 64, 0) + tuple(adr(r) for r in host) + (R,)),
            ('oth_csd_exec', (PH, 0x1000, 0x2000, 100, 1) + tuple(adr(r) for r in dev) + (R,))]


@case
def plan_csd_device_forms(lib):
    p = plan_of(lib)
    assert p.csd_exec_dev(0x1000, 0x2000, 100) == COUNT
    assert p.csd_exec_dev(0x1000, 0x2000, 100, 0x3000, 0x4000, 0x5000, 0x6000) == COUNT
    assert p.csd_partial_dev(0x1000, 0x2000, 100, 0x3000) == COUNT
    assert p.csd_scale_dev(0x3000, 31) is None
    p.csd_scale_dev(0x3000, 31, pxx=0x4000, pyy=0x5000, pxy=0x6000, cxy=0x7000)
    p.csd_scale_dev(0x3000, 31, cxy=0x7000)
    assert p.last_nseg == UNTOUCHED
    return [('oth_csd_exec_dev', (PH, 0x1000, 0x2000, 100, None, None, None, None, R)),
            ('oth_csd_exec_dev', (PH, 0x1000, 0x2000, 100, 0x3000, 0x4000, 0x5000, 0x6000, R)),
            ('oth_csd_partial_dev', (PH, 0x1000, 0x2000, 100, 0x3000, R)),
            ('oth_csd_scale_dev', (PH, 0x3000, 31, None, None, None, None)),
            ('oth_csd_scale_dev', (PH, 0x3000, 31, 0x4000, 0x5000, 0x6000, 0x7000)),
            ('oth_csd_scale_dev', (PH, 0x3000, 31, None, None, None, 0x7000))]


# ---- MtmPlan, MtmCsdPlan ---------------------------------------------------------------------------------------------------

@case
def mtm_set_ratios(lib):
    p = plan_of(lib, _hip.MtmPlan)
    p.set_ratios([0.75, 0.5, 0.25])
    assert p.ratios.dtype == np.float64 and list(p.ratios) == [0.75, 0.5, 0.25] and p.last_nseg == UNTOUCHED
    p.last_nseg = 4
    assert p.dof == (8, 16)
    return [('oth_mtm_set_ratios', (PH, (0.75, 0.5, 0.25)))]


@case
def mtm_adaptive(lib):
    p, x = plan_of(lib, _hip.MtmPlan), c64(64)
    psd = p.adaptive(x)
    assert p.last_nseg == COUNT
    both = p.adaptive(0x1000, iters=2, return_dof=True, nsamples=100)
    rows_ok([psd], 1)
    rows_ok(both, 2)
    p.last_nseg = UNTOUCHED
    assert p.adaptive_dev(0x1000, 100, 2, 128, 0x2000) == COUNT and p.last_nseg == COUNT
    p.adaptive_dev(0x1000, 100, 2, 128, 0x2000, dof_dev=0x3000, iters=6)
    return [('oth_mtm_adaptive', (PH, adr(x), 64, 0, 4, adr(psd), None, R)), ('oth_mtm_adaptive', (PH, 0x1000, 100, 1, 2, adr(both[0]), adr(both[1]), R)),
            ('oth_mtm_adaptive_dev', (PH, 0x1000, 100, 2, 128, 4, 0x2000, None, R)),
            ('oth_mtm_adaptive_dev', (PH, 0x1000, 100, 2, 128, 6, 0x2000, 0x3000, R))]


@case
def mtm_ftest(lib):
    p, x = plan_of(lib, _hip.MtmPlan), c64(64)
    F = p.ftest(x)
    assert p.last_nseg == COUNT
    three = p.ftest(0x1000, return_rows=True, nsamples=100)
    rows_ok([F], 1)
    rows_ok(three, 3)
    p.last_nseg = UNTOUCHED
    assert p.ftest_dev(0x1000, 100, 2, 128, 0x2000) == COUNT and p.last_nseg == COUNT
    p.ftest_dev(0x1000, 100, 2, 128, 0x2000, line_dev=0x3000, resid_dev=0x4000)
    p.ftest_dev(0x1000, 100, 2, 128, 0x2000, resid_dev=0x4000)
    return [('oth_mtm_ftest', (PH, adr(x), 64, 0, adr(F), None, None, R)),
            ('oth_mtm_ftest', (PH, 0x1000, 100, 1, adr(three[0]), adr(three[1]), adr(three[2]), R)),
            ('oth_mtm_ftest_dev', (PH, 0x1000, 100, 2, 128, 0x2000, None, None, R)),
            ('oth_mtm_ftest_dev', (PH, 0x1000, 100, 2, 128, 0x2000, 0x3000, 0x4000, R)),
            ('oth_mtm_ftest_dev', (PH, 0x1000, 100, 2, 128, 0x2000, None, 0x4000, R))]


@case
def mtm_jackknife(lib):
    p, x = plan_of(lib, _hip.MtmPlan), c64(64)
    lnsd = p.jackknife(x)
    assert p.last_nseg == COUNT
    both = p.jackknife(0x1000, return_psd=True, nsamples=100)
    rows_ok([lnsd], 1)
    rows_ok(both, 2)
    p.last_nseg = UNTOUCHED
    assert p.jackknife_dev(0x1000, 100, 2, 128, 0x2000) == COUNT and p.last_nseg == COUNT
    p.jackknife_dev(0x1000, 100, 2, 128, 0x2000, psd_dev=0x3000)
    return [('oth_mtm_jackknife', (PH, adr(x), 64, 0, adr(lnsd), None, R)), ('oth_mtm_jackknife', (PH, 0x1000, 100, 1, adr(both[0]), adr(both[1]), R)),
            ('oth_mtm_jackknife_dev', (PH, 0x1000, 100, 2, 128, 0x2000, None, R)),
            ('oth_mtm_jackknife_dev', (PH, 0x1000, 100, 2, 128, 0x2000, 0x3000, R))]


@case
def mtm_csd_jackknife(lib):
    p, x, y = plan_of(lib, _hip.MtmCsdPlan), c64(64), c64(64)
    host = p.csd_jackknife(x, y)
    assert p.last_nseg == COUNT
    dev = p.csd_jackknife(0x1000, 0x2000, nsamples=100)
    rows_ok(host, 4)
    rows_ok(dev, 4)
    p.last_nseg = UNTOUCHED
    assert p.csd_jackknife_dev(0x1000, 0x2000, 100, 0x3000) == COUNT and p.last_nseg == COUNT
    p.csd_jackknife_dev(0x1000, 0x2000, 100, 0x3000, cxy_dev=0x4000, lnsdx_dev=0x5000, lnsdy_dev=0x6000)
    return [('oth_mtm_csd_jackknife', (PH, adr(x), adr(y), 64, 0) + tuple(adr(r) for r in host) + (R,)),
            ('oth_mtm_csd_jackknife', (PH, 0x1000, 0x2000, 100, 1) + tuple(adr(r) for r in dev) + (R,)),
            ('oth_mtm_csd_jackknife_dev', (PH, 0x1000, 0x2000, 100, None, 0x3000, None, None, R)),
            ('oth_mtm_csd_jackknife_dev', (PH, 0x1000, 0x2000, 100, 0x4000, 0x3000, 0x5000, 0x6000, R))]


# ---- Chain -----------------------------------------------------------------------------------------------------------------

@case
def chain_setters(lib):
    c = chain_of(lib)
    c.set_keep_one_in_n(3)
    c.set_iir_log(0.5, 10)
    c.set_kernel(_hip.KERNEL_GENERIC)
    c.set_peak_hold(True)
    c.set_peak_hold(False)
    c.reset()
    peak, iir = c.peak(), c.iir()
    rows_ok([peak, iir], 2, (NFFT,))
    c.close()
    c.close()
    assert c.h is None and not hasattr(c, 'last_nseg')
    return [('oth_chain_set_keep_one_in_n', (PH, 3)), ('oth_chain_set_iir_log', (PH, 0.5, 10.0)), ('oth_chain_set_kernel', (PH, 1)),
            ('oth_chain_set_peak_hold', (PH, 1)), ('oth_chain_set_peak_hold', (PH, 0)), ('oth_chain_reset', (PH,)),
            ('oth_chain_get_peak', (PH, adr(peak))), ('oth_chain_get_iir', (PH, adr(iir))), ('oth_chain_destroy', (PH,))]


@case
def chain_push(lib):
    c, x = chain_of(lib), c64(64)
    rows, n = c.push(x)      # room for 64 / 8 + 2 rows
    assert (rows.shape, rows.dtype, n, type(n)) == ((COUNT, NFFT), np.float32, COUNT, int)
    last, n2 = c.push(x, max_rows=2)
    assert (last.shape, n2) == ((2, NFFT), COUNT)
    assert c.push_dev(0x1000, 100) == COUNT
    assert c.push_dev(0x1000, 100, 0x2000, 4) == COUNT and not hasattr(c, 'last_nseg')
    return [('oth_chain_push', (PH, adr(x), 64, 0, adr(rows), 10, R)), ('oth_chain_push', (PH, adr(x), 64, 0, adr(last), 2, R)),
            ('oth_chain_push_dev', (PH, 0x1000, 100, None, 0, R)), ('oth_chain_push_dev', (PH, 0x1000, 100, 0x2000, 4, R))]


@case
def chain_async(lib):
    c, x = chain_of(lib), c64(64)
    assert c.push_async(x) == COUNT and c.last_push_ops() == COUNT and c.ticket_rows(5) == COUNT
    lib.ready = 0
    assert c.poll(5) is None
    lib.ready = 1
    row, n = c.poll(5)
    row2, n2 = c.wait(6)
    rows_ok([row, row2], 2, (NFFT,))
    assert (n, n2) == (COUNT, COUNT)
    lib.count = 0      # a push that produced no row
    assert c.poll(5) == (None, 0) and c.wait(6) == (None, 0) and not hasattr(c, 'last_nseg')
    return [('oth_chain_push_async', (PH, adr(x), 64, R)), ('oth_chain_last_push_ops', (PH, R)), ('oth_chain_ticket_rows', (PH, 5, R)),
            ('oth_chain_poll', (PH, 5, SOME, R, R)), ('oth_chain_poll', (PH, 5, adr(row), R, R)), ('oth_chain_wait', (PH, 6, adr(row2), R)),
            ('oth_chain_poll', (PH, 5, SOME, R, R)), ('oth_chain_wait', (PH, 6, SOME, R))]


# ---- Channelizer -----------------------------------------------------------------------------------------------------------

@case
def channelizer_calls(lib):
    c, x = chan_of(lib), c64(100)
    c.reset()
    assert c.frames_for(100) == COUNT and c.pending == COUNT and c.last_recipe() == ''
    out = c.push(x)
    out2 = c.push(0x1000, nsamples=100)
    assert (out.shape, out.dtype, out2.shape) == ((64, COUNT), np.complex64, (64, COUNT))
    assert c.push_dev(0x1000, 100, 0x2000, 16) == COUNT
    lib.count = 0      # a push that yields no frame
    none = c.push(x)
    assert none.shape == (64, 0) and c.push_dev(0x1000, 10, None, 0) == 0 and c.push_dev(0, 0, 0, 0) == 0
    c.close()
    c.close()
    assert c.h is None and not hasattr(c, 'last_nseg')
    return [('oth_channelizer_reset', (PH,)), ('oth_channelizer_frames', (PH, 100, R)), ('oth_channelizer_pending', (PH, R)),
            ('oth__debug_channelizer_recipe', (PH, BUF, 512)),
            ('oth_channelizer_frames', (PH, 100, R)), ('oth_channelizer_push', (PH, adr(x), 100, 0, adr(out), COUNT, R)),
            ('oth_channelizer_frames', (PH, 100, R)), ('oth_channelizer_push', (PH, 0x1000, 100, 1, adr(out2), COUNT, R)),
            ('oth_channelizer_push_dev', (PH, 0x1000, 100, 0x2000, 16, R)),
            ('oth_channelizer_frames', (PH, 100, R)), ('oth_channelizer_push', (PH, adr(x), 100, 0, None, 0, R)),
            ('oth_channelizer_push_dev', (PH, 0x1000, 10, None, 0, R)), ('oth_channelizer_push_dev', (PH, None, 0, None, 0, R)),
            ('oth_channelizer_destroy', (PH,))]


# ---- the checks ------------------------------------------------------------------------------------------------------------

IDS = [fn.__name__ for fn in CASES]


@pytest.mark.parametrize('fn', CASES, ids=IDS)
def test_recorded_calls(fn):
    lib = Lib()
    want = fn(lib)
    assert lib.calls == want


# calls the binding makes without check() on purpose (the close paths), and the one label that names another symbol today:
# Context.__init__ reports a failure of either constructor as oth_ctx_create
UNCHECKED = {'oth_ctx_destroy', 'oth_plan_destroy', 'oth_chain_destroy', 'oth_channelizer_destroy'}
LABEL = {'oth_ctx_create_on_stream': 'oth_ctx_create'}


@pytest.mark.parametrize('fn', CASES, ids=IDS)
def test_error_label_is_the_symbol_called(fn):
    ok = Lib()
    fn(ok)
    for i, (name, _) in enumerate(ok.calls):
        if name in UNCHECKED:
            continue
        lib = Lib(rc=OTH_ERR_INVALID, fail_at=i)
        with pytest.raises(_hip.HipError) as ei:
            fn(lib)
        assert lib.calls[i][0] == name and ei.value.code == OTH_ERR_INVALID
        assert str(ei.value) == '%s failed (-1): stand-in detail' % LABEL.get(name, name), (i, name)


def test_error_path_of_a_handful():
    lib = Lib(rc=OTH_ERR_INVALID)
    p, m, c, z, x = plan_of(lib), plan_of(lib, _hip.MtmCsdPlan), chain_of(lib), chan_of(lib), c64(64)
    for call, name in ((lambda: p.exec(x), 'oth_welch_exec'), (lambda: p.sk_dev(0x1000, 100, 1, 100, 0x2000), 'oth_welch_sk_dev'),
                       (lambda: p.matrix(c64(32, 2)), 'oth_welch_matrix'), (lambda: p.csd_exec_dev(0x1000, 0x2000, 100), 'oth_csd_exec_dev'),
                       (lambda: m.csd_jackknife(x, x), 'oth_mtm_csd_jackknife'), (lambda: m.ftest(x), 'oth_mtm_ftest'),
                       (lambda: c.push_async(x), 'oth_chain_push_async'), (lambda: z.push_dev(0x1000, 100, 0x2000, 16), 'oth_channelizer_push_dev'),
                       (lambda: p.ctx.cp_sync(x, HYPS), 'oth_cp_sync'), (lambda: p.ctx.sync(), 'oth_ctx_sync')):
        with pytest.raises(_hip.HipError) as ei:
            call()
        assert ei.value.code == OTH_ERR_INVALID and str(ei.value).startswith(name + ' failed ('), name
    assert p.last_nseg == UNTOUCHED and m.last_nseg == UNTOUCHED


def test_tickets():
    lib = Lib()
    p, x = plan_of(lib), c64(64)
    assert p.outstanding == 0 and p.next_ticket_slot_free()
    for t in (1, 2, 3, 4):
        lib.count = t
        assert p.exec_async(x) == t and type(p._last_ticket) is int
        assert p.outstanding == t
        assert p.next_ticket_slot_free() == (t < _hip.OUT_RING)      # ticket 5 would land in the slot of ticket 1
    lib.ready = 0
    assert p.poll(1) is None and p.outstanding == 4 and not p.next_ticket_slot_free()
    lib.ready = 1
    assert p.poll(1) is not None and p.outstanding == 3 and p.next_ticket_slot_free()
    assert p.wait(2) is not None and p.outstanding == 2
    p.last_nseg = UNTOUCHED
    lib.rc = OTH_ERR_INVALID
    with pytest.raises(_hip.HipError):
        p.poll(3)
    assert p.outstanding == 2      # a poll that failed collected nothing
    with pytest.raises(_hip.HipError):
        p.wait(3)
    assert p.outstanding == 1 and p._tickets == {4} and p.last_nseg == UNTOUCHED      # a wait that failed gave the ticket up all the same
    with pytest.raises(_hip.HipError):
        p.exec_async(x)
    assert p.outstanding == 1 and p._last_ticket == 4


def test_cached_plan_keeps_a_plan_that_owes_a_ticket():
    lib = Lib()
    ctx = ctx_of(lib)
    a, b, c = plan_of(lib), plan_of(lib), plan_of(lib)
    a.exec_async(c64(64))
    assert ctx.cached_plan('a', lambda: a, limit=1) is a and ctx.cached_plan('b', lambda: b, limit=1) is b
    assert a.h is not None and b.h is not None      # a owes a result: over the limit, nothing closed
    assert ctx.cached_plan('c', lambda: c, limit=1) is c
    assert a.h is not None and b.h is None and c.h is not None
    assert [name for name, _ in lib.calls] == ['oth_welch_exec_async', 'oth_plan_destroy']


def test_counts_that_reach_ctypes_as_the_caller_gave_them():
    """Most device forms pass nsamples and its kin through int(); these pass what they are given (a numpy integer stays one).
    Pinned as it is."""
    lib = Lib()
    p, c, n = plan_of(lib), chain_of(lib), np.int64(100)
    p.exec_dev(0x1000, n, 0x2000)
    p.exec_dev(0x1000, n, 0x2000, n, n)
    p.partial_dev(0x1000, n, 0x2000)
    p.scale_dev(0x1000, n, 0x2000)
    p.csd_exec_dev(0x1000, 0x2000, n)
    p.csd_partial_dev(0x1000, 0x2000, n, 0x3000)
    c.push_dev(0x1000, n)
    p.sk_dev(0x1000, n, n, n, 0x2000)
    p.csd_scale_dev(0x1000, n)
    p.segments_dev(0x1000, n, 0x2000, n)
    got = [(name, [type(a) for a in args if isinstance(a, numbers.Integral) and a == 100]) for name, args in lib.calls]
    assert got == [('oth_welch_exec_dev', [np.int64, np.int64]), ('oth_welch_exec_dev', [np.int64, np.int64, np.int64]),
                   ('oth_welch_partial_dev', [np.int64]), ('oth_welch_scale_dev', [np.int64]), ('oth_csd_exec_dev', [np.int64]),
                   ('oth_csd_partial_dev', [np.int64]), ('oth_chain_push_dev', [np.int64]),
                   ('oth_welch_sk_dev', [int, int, int]), ('oth_csd_scale_dev', [int]), ('oth_welch_segments_dev', [int, int])]


def test_counts_of_the_device_source_forms_go_through_int():
    """exec_device_src and csd_device_src share the body of exec / csd over _src / _src2, which takes int(nsamples) as it
    always did for exec_async: a numpy integer arrives as an int.  (Before that fold these two passed nsamples as given;
    the one place where this module asks something else than the binding did before it.)"""
    lib = Lib()
    p, n = plan_of(lib), np.int64(100)
    p.exec_device_src(0x1000, n)
    p.csd_device_src(0x1000, 0x2000, n)
    p.exec_async(0x1000, nsamples=n)
    got = [(name, [type(a) for a in args if isinstance(a, numbers.Integral) and a == 100]) for name, args in lib.calls]
    assert got == [('oth_welch_exec', [int]), ('oth_csd_exec', [int]), ('oth_welch_exec_async', [int])]


def raises_before_any_call(text, fn):
    lib = Lib()
    with pytest.raises(ValueError) as ei:
        fn(lib)
    assert str(ei.value) == text and lib.calls == []


X2, X1, X9 = c64(32, 2), c64(32), c64(4, 9)
CHANNELS = 'x must be a (C, n) array of C channels'
REFUSALS = [
    ('x and y must have the same length', lambda lib: plan_of(lib).csd(c64(64), c64(63))),
    ('x and y must have the same length', lambda lib: plan_of(lib, _hip.MtmCsdPlan).csd_jackknife(c64(64), c64(63))),
    ('window must have nperseg=8 entries', lambda lib: ctx_of(lib).welch_plan(8, window=f32(5))),
    ('input shorter than nperseg', lambda lib: plan_of(lib).segments(c64(7))),
    ("average must be 'mean' or 'median', not 'x'", lambda lib: plan_of(lib).set_average('x')),
    ('unknown average code 2', lambda lib: plan_of(lib).set_average(2)),
    ('alphas must be a sequence of cycle frequencies', lambda lib: plan_of(lib).set_cycles([[0.1]])),
    ('lags must be a sequence of integer lags in samples', lambda lib: plan_of(lib).set_lags([0.5])),
    ('the prototype holds ntaps * nfft taps: 10 is no multiple of 8', lambda lib: plan_of(lib).set_prototype(f32(10))),
    ('the prototype holds ntaps * nfft taps: 0 is no multiple of 8', lambda lib: plan_of(lib).set_prototype([])),
    ('the prototype holds ntaps * nfft = 16 taps, not 10', lambda lib: plan_of(lib).set_prototype(f32(10), ntaps=2)),
    (CHANNELS, lambda lib: plan_of(lib).matrix(X1)),
    (CHANNELS, lambda lib: plan_of(lib).matrix_eig(X1)),
    (CHANNELS, lambda lib: plan_of(lib).matrix_doa(X1, nsrc=1)),
    (CHANNELS, lambda lib: plan_of(lib).matrix_gcc(X1)),
    ('the spectral matrix takes 2 ... 8 channels, not 9', lambda lib: plan_of(lib).matrix(X9)),
    ('the spectral matrix takes 2 ... 8 channels, not 9', lambda lib: plan_of(lib).matrix_eig(X9)),
    ('the spectral matrix takes 2 ... 8 channels, not 9', lambda lib: plan_of(lib).matrix_doa(X9, nsrc=1)),
    ('the spectral matrix takes 2 ... 8 channels, not 9', lambda lib: plan_of(lib).matrix_gcc(X9)),
    ('the spectral matrix takes 2 ... 8 channels, not 1', lambda lib: plan_of(lib).matrix(0x1000, nsamples=(1, 100))),
    ('the spectral matrix takes 2 ... 8 channels, not 1', lambda lib: plan_of(lib).matrix_eig(0x1000, nsamples=(1, 100))),
    ('the spectral matrix takes 2 ... 8 channels, not 1', lambda lib: plan_of(lib).matrix_doa(0x1000, nsrc=1, nsamples=(1, 100))),
    ('the spectral matrix takes 2 ... 8 channels, not 1', lambda lib: plan_of(lib).matrix_gcc(0x1000, nsamples=(1, 100))),
    ("methods must name at least one of 'bartlett', 'capon', 'music'", lambda lib: plan_of(lib).matrix_doa(X2, methods=())),
    ("methods must name at least one of 'bartlett', 'capon', 'music'", lambda lib: plan_of(lib).matrix_doa(X2, methods=('capon', 'esprit'))),
    ('the MUSIC spectrum needs nsrc, the number of sources', lambda lib: plan_of(lib).matrix_doa(X2)),
    ('delays must be a (D, C) array: a row of C channel delays per direction', lambda lib: plan_of(lib).set_steering([1.0, 2.0], 0.0)),
    ('ratios must have ntapers=3 entries', lambda lib: plan_of(lib, _hip.MtmPlan).set_ratios([0.5, 0.5])),
    ('ntapers must be at least 1 (nw=0.5 gives int(2 nw) - 1 = 0)', lambda lib: ctx_of(lib).mtm_plan(8, nw=0.5)),
    ('tapers must have shape [ntapers, nperseg=8]', lambda lib: ctx_of(lib).mtm_plan(8, tapers=f32(2, 7))),
    ('tapers must have shape [ntapers, nperseg=8]', lambda lib: ctx_of(lib).mtm_csd_plan(8, ntapers=3, tapers=f32(2, 8))),
    ('weights must have ntapers=2 entries', lambda lib: ctx_of(lib).mtm_plan(8, tapers=f32(2, 8), weights=[1.0])),
    ("weights='eigen' needs the plan's own Slepian tapers (tapers=None)", lambda lib: ctx_of(lib).mtm_plan(8, tapers=f32(2, 8), weights='eigen')),
    ("weights must be 'unity', 'eigen' or an array, not 'flat'", lambda lib: ctx_of(lib).mtm_plan(8, tapers=f32(2, 8), weights='flat')),
    ('weights must be finite, non-negative and have a positive sum', lambda lib: ctx_of(lib).mtm_plan(8, tapers=f32(2, 8), weights=[1.0, -1.0])),
    ('weights must be finite, non-negative and have a positive sum', lambda lib: ctx_of(lib).mtm_csd_plan(8, tapers=f32(2, 8), weights=[0.0, 0.0])),
    ('weights must be finite, non-negative and have a positive sum', lambda lib: ctx_of(lib).mtm_csd_plan(8, tapers=f32(2, 8), weights=[1.0, np.inf])),
    ('window must have nfft entries', lambda lib: ctx_of(lib).chain(8, window=f32(7))),
    ('the channelizer takes a channel count that is a power of two from 64 to 4096, not 48', lambda lib: ctx_of(lib).channelizer(48)),
    ('the prototype holds taps * nchan = 512 taps, not 8', lambda lib: ctx_of(lib).channelizer(64, prototype=f32(8))),
    ('decim must be nchan, nchan / 2 or nchan / 4 (got 8 for 64 channels)', lambda lib: ctx_of(lib).channelizer(64, decim=8)),
    ('taps must lie in 1 ... 16 (got 17)', lambda lib: ctx_of(lib).channelizer(64, taps=17)),
    ('taps must lie in 1 ... 16 (got 0)', lambda lib: ctx_of(lib).channelizer(64, taps=0)),
    ('every tap of the prototype must be finite', lambda lib: ctx_of(lib).channelizer(64, taps=1, prototype=[np.nan] + [1.0] * 63)),
    ('the prototype is all zero', lambda lib: ctx_of(lib).channelizer(64, taps=1, prototype=np.zeros(64))),
]


@pytest.mark.parametrize('text,fn', REFUSALS, ids=['%02d' % i for i in range(len(REFUSALS))])
def test_value_errors_come_before_any_call(text, fn):
    raises_before_any_call(text, fn)


# not bound to a handle: the tests of the ABI and of windows.dpss call them
PROCESS_WIDE = {'oth_abi_version', 'oth_strerror', 'oth_device_count', 'oth_dpss', 'oth_last_error', 'oth__debug_recipe',
                'oth__debug_recipe_tuned', 'oth__debug_live_resources'}
UNBOUND = set()      # entry points no public method of the binding calls: adding one here is a decision


def test_every_entry_point_is_reached_by_a_public_method():
    reached = set()
    for fn in CASES:
        lib = Lib()
        fn(lib)
        reached |= set(name for name, _ in lib.calls)
    assert PROCESS_WIDE | UNBOUND <= set(_hip.SIGNATURES) and not reached & (PROCESS_WIDE | UNBOUND)
    assert set(_hip.SIGNATURES) - reached == PROCESS_WIDE | UNBOUND


def test_the_stand_in_refuses_what_a_library_would():
    lib = Lib()
    with pytest.raises(AttributeError):
        lib.oth_no_such_symbol
    with pytest.raises(AssertionError):
        lib.oth_ctx_sync()
    with pytest.raises((TypeError, C.ArgumentError)):
        lib.oth_ctx_sync(1.5)
    assert lib.calls == []
