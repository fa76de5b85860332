"""Every refusal of the per-bin statistics - oth_mtm_ftest, oth_welch_sk, oth_mtm_jackknife, oth_mtm_csd_jackknife,
oth_mtm_adaptive, oth_welch_cyclic, oth_welch_caf, oth_welch_matrix, each with its _dev form, and the three table setters -
as one table: the single violations the header documents and, per entry point, two double violations that pin which refusal goes first.  The codes
and texts are literals: what the library answered before the statistics' host sides were folded onto shared helpers
(csrc/abi_stat.h), so a helper that reorders or rewords a refusal fails here.  A refused host form has allocated and staged
nothing (oth__debug_live_resources)."""
import ctypes as C
import gc

import numpy as np
import pytest

from oracle import ref_cpu as R
from test_hip_parity import hann, hip  # noqa: F401 - hip is a fixture

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
N, NS = 64, 320                       # 64-point plans; 320 samples: 9 Welch segments at 50 % overlap, 5 multitaper segments
ROW = 6 * N                           # floats between the output rows: the packed matrix rows of two channels, the longest row
X = R.synth_iq(3 * NS, 4711)

BAD, STRIDE, SHORT = 'bad argument', 'stream_stride < nsamples', 'input shorter than nperseg'
MTM_STREAMS = 'multitaper plans take at most 65535 streams per launch'
FT_NOTAPERS = 'the harmonic F-test needs a multitaper plan (oth_mtm_plan): this plan has no tapers'
FT_ONE = 'the harmonic F-test needs at least two tapers'
FT_ZERO = 'the harmonic F-test needs tapers with a non-zero sum: every U_k of this plan is zero'
SK_MTM = "the spectral kurtosis is not available on a multitaper plan: its segments' periodograms are Welch's (oth_welch_plan)"
SK_MEDIAN = ('the spectral kurtosis is not available with OTH_AVERAGE_MEDIAN: its PSD row is the mean over segments '
             '(oth_plan_set_average(OTH_AVERAGE_MEAN) first)')
SK_SIZE = 'the spectral kurtosis takes a transform length that is a power of two from 64 to 16384, not 32'
SK_STREAMS = 'the spectral kurtosis takes at most 65535 streams per launch'
SK_ONE = 'the spectral kurtosis needs at least two segments: this input holds one'
JK_NOTAPERS = 'the jackknife needs a multitaper plan (oth_mtm_plan): this plan has no tapers'
JK_WEIGHTS = 'the jackknife needs exchangeable items: the weights of this plan are not all equal'
JK_ITEMS = 'the jackknife needs at least 2 (segment, taper) items: this input holds 1'
CJ_NOTAPERS = 'the coherence jackknife needs a multitaper plan (oth_mtm_plan): this plan has no tapers'
CJ_GATE = 'oth_mtm_csd_jackknife is not available on a multitaper plan: the taper loop holds one channel'
CJ_WEIGHTS = 'the coherence jackknife needs exchangeable items: the weights of this plan are not all equal'
CJ_ITEMS = 'the coherence jackknife needs at least 3 (segment, taper) items: this input holds 2'
AD_NOTAPERS = 'the adaptive estimate needs a multitaper plan (oth_mtm_plan): this plan has no tapers'
AD_ONE = 'the adaptive estimate needs at least two tapers'
AD_RATIOS = "the adaptive estimate needs the tapers' concentration ratios: call oth_mtm_set_ratios on this plan"
AD_ITERS = 'need 1 <= iters <= 64'
CY_MTM = "the cyclic spectrum is not available on a multitaper plan: its segments' transforms are Welch's (oth_welch_plan)"
CY_MEDIAN = ('the cyclic spectrum is not available with OTH_AVERAGE_MEDIAN: its rows are means over segments '
             '(oth_plan_set_average(OTH_AVERAGE_MEAN) first)')
CY_SIZE = 'the cyclic spectrum takes a transform length that is a power of two from 64 to 16384, not 32'
CY_NONE = 'the cyclic spectrum needs its cycle frequencies: call oth_welch_set_cycles on this plan'
CY_STREAMS = 'the cyclic spectrum takes at most 65535 streams per launch'
RT_NOTAPERS = 'concentration ratios belong to a multitaper plan (oth_mtm_plan): this plan has no tapers'
RT_NULL = 'ratios is NULL'
RT_RANGE = 'every concentration ratio must lie in (0, 1]'
SC_COUNT = 'ncycles must lie in 1 ... 64'
SC_NULL = 'alphas is NULL'
SC_RANGE = 'every cycle frequency must be finite with |alpha| <= 0.5 cycles per sample'
LG_MTM = "the cyclic autocorrelation is not available on a multitaper plan: its segments' transforms are Welch's (oth_welch_plan)"
LG_MEDIAN = ('the cyclic autocorrelation is not available with OTH_AVERAGE_MEDIAN: its rows are means over segments '
             '(oth_plan_set_average(OTH_AVERAGE_MEAN) first)')
LG_SIZE = 'the cyclic autocorrelation takes a transform length that is a power of two from 64 to 16384, not 32'
LG_NONE = 'the cyclic autocorrelation needs its lags: call oth_welch_set_lags on this plan'
LG_SHORT = 'input shorter than the largest lag + nperseg (5 + 64 samples)'
LG_STREAMS = 'the cyclic autocorrelation takes at most 65535 streams per launch'
SL_COUNT = 'nlags must lie in 1 ... 64'
SL_NULL = 'lags is NULL'
SL_RANGE = 'every lag must lie in 0 ... 65535 samples'
MT_MTM = "the spectral matrix is not available on a multitaper plan: its segments' transforms are Welch's (oth_welch_plan)"
MT_MEDIAN = ('the spectral matrix is not available with OTH_AVERAGE_MEDIAN: its rows are means over segments '
             '(oth_plan_set_average(OTH_AVERAGE_MEAN) first)')
MT_SIZE = 'the spectral matrix takes a transform length that is a power of two from 64 to 16384, not 32'
MT_NCHAN = 'nchan must lie in 2 ... 8'
MT_INPUT = 'the input is NULL'
MT_ROWS = 's_out and gcoh_out are both NULL'
MT_STRIDE = 'chan_stride < nsamples'

# plans by key (made once per module): w Welch, wc Welch with one cycle frequency, wl Welch with the lags 0 and 5, wmed median-averaging, w32 32 points,
# m multitaper (3 Slepian tapers, ratios set), m1 one taper, mw unequal weights, mz two user tapers that sum to zero (no
# ratios either), mc / mc1 / mcw two-channel multitaper with 3 tapers / one / unequal weights


def make_plans(c):
    odd = np.tile(np.array([[1.0, -1.0], [1.0, -1.0]], np.float32), (1, N // 2))
    odd[1, :N // 2] *= -1.0
    p = dict(w=c.welch_plan(N, window=hann(N)), wc=c.welch_plan(N, window=hann(N)), wl=c.welch_plan(N, window=hann(N)),
             wmed=c.welch_plan(N, window=hann(N), average='median'), w32=c.welch_plan(32, window=hann(32)),
             m=c.mtm_plan(N, nw=2.0, ntapers=3), m1=c.mtm_plan(N, nw=2.0, ntapers=1),
             mw=c.mtm_plan(N, nw=2.0, ntapers=3, weights=[1.0, 1.0, 0.5]), mz=c.mtm_plan(N, tapers=odd),
             mc=c.mtm_csd_plan(N, nw=2.0, ntapers=3), mc1=c.mtm_csd_plan(N, nw=2.0, ntapers=1),
             mcw=c.mtm_csd_plan(N, nw=2.0, ntapers=3, weights=[1.0, 1.0, 0.5]))
    p['wc'].set_cycles([0.125])
    p['wl'].set_lags([0, 5])
    return p


# entry point -> (arguments in ABI order, '@' marks device pointers); the defaults are a valid call on the right plan
FORMS = {
    'oth_mtm_ftest': ('x n dev o0 o1 o2 nseg', False), 'oth_mtm_ftest_dev': ('@x n ns stride @o0 @o1 @o2 nseg', True),
    'oth_welch_sk': ('x n dev o0 o1 nseg', False), 'oth_welch_sk_dev': ('@x n ns stride @o0 @o1 nseg', True),
    'oth_mtm_jackknife': ('x n dev o0 o1 nseg', False), 'oth_mtm_jackknife_dev': ('@x n ns stride @o0 @o1 nseg', True),
    'oth_mtm_csd_jackknife': ('x y n dev o1 o0 o2 o3 nseg', False), 'oth_mtm_csd_jackknife_dev': ('@x @y n @o1 @o0 @o2 @o3 nseg', True),
    'oth_mtm_adaptive': ('x n dev iters o0 o1 nseg', False), 'oth_mtm_adaptive_dev': ('@x n ns stride iters @o0 @o1 nseg', True),
    'oth_welch_cyclic': ('x n dev o1 o0 o2 nseg', False), 'oth_welch_cyclic_dev': ('@x n ns stride @o1 @o0 @o2 nseg', True),
    'oth_welch_caf': ('x n dev o0 o1 nseg', False), 'oth_welch_caf_dev': ('@x n ns stride @o0 @o1 nseg', True),
    'oth_welch_matrix': ('x n nchan dev o0 o1 nseg', False), 'oth_welch_matrix_dev': ('@x n nchan stride @o0 @o1 nseg', True),
}
# o0 is the output every call needs (f, sk, lnsd, zsd, psd, coh, caf; the matrix needs one of s = o0 and gcoh = o1);
# NULL-able by o0=None.  Overrides: x / y / o0 / o1 = None, n, ns, nchan, stride, iters.
BIG = 70000


def rows_for(name, good, other, bad_plans, extra=(), streams=MTM_STREAMS, first=None, short=SHORT):
    """The shared part of a family's table for the host form `name` and its _dev form on the plan `good`."""
    t = []
    for form in (name, name + '_dev'):
        dev = form.endswith('_dev')
        for key, code, text in bad_plans:
            t.append((form, key, {}, code, text))
        t += [(form, good, dict(x=None), INVALID, BAD), (form, good, dict(o0=None), INVALID, BAD), (form, good, dict(n=N - 1), INVALID, short)]
        t += [(form, good, ov, code, text) for ov, code, text in extra]
        if dev and ' ns ' in FORMS[form][0]:
            t += [(form, good, dict(ns=0), INVALID, BAD), (form, good, dict(ns=3, stride=NS - 1), INVALID, STRIDE),
                  (form, good, dict(ns=BIG, stride=NS), UNSUPPORTED, streams),
                  # two at once: which goes first
                  (form, good, dict(o0=None, ns=BIG, stride=NS), *(first or (INVALID, BAD))),
                  (form, good, dict(n=N - 1, ns=3, stride=N - 2), INVALID, STRIDE)]
        else:
            t += [(form, other[0], dict(x=None), *other[1]), (form, other[2], dict(n=N - 1), *other[3])]
    return t


TABLE = (
    # the F-test: the host form tests its pointers in front of the plan (NULL input on a one-taper plan: bad argument),
    # the _dev form behind it
    rows_for('oth_mtm_ftest', 'm', ('m1', (INVALID, BAD), 'mz', (UNSUPPORTED, FT_ZERO)),
             [('w', UNSUPPORTED, FT_NOTAPERS), ('m1', UNSUPPORTED, FT_ONE), ('mz', UNSUPPORTED, FT_ZERO)])
    + [('oth_mtm_ftest_dev', 'm1', dict(x=None), UNSUPPORTED, FT_ONE)]
    + rows_for('oth_welch_sk', 'w', ('m', (UNSUPPORTED, SK_MTM), 'wmed', (UNSUPPORTED, SK_MEDIAN)),
               [('m', UNSUPPORTED, SK_MTM), ('wmed', UNSUPPORTED, SK_MEDIAN), ('w32', UNSUPPORTED, SK_SIZE)],
               extra=[(dict(n=N), INVALID, SK_ONE)], streams=SK_STREAMS)
    # the jackknife tests the stream limit in front of "bad argument"
    + rows_for('oth_mtm_jackknife', 'm', ('mw', (UNSUPPORTED, JK_WEIGHTS), 'm1', (INVALID, SHORT)),
               [('w', UNSUPPORTED, JK_NOTAPERS), ('mw', UNSUPPORTED, JK_WEIGHTS)], first=(UNSUPPORTED, MTM_STREAMS))
    + [(f, 'm1', dict(n=N), INVALID, JK_ITEMS) for f in ('oth_mtm_jackknife', 'oth_mtm_jackknife_dev')]
    + rows_for('oth_mtm_csd_jackknife', 'mc', ('m', (UNSUPPORTED, CJ_GATE), 'mc1', (INVALID, SHORT)),
               [('w', UNSUPPORTED, CJ_NOTAPERS), ('m', UNSUPPORTED, CJ_GATE), ('mcw', UNSUPPORTED, CJ_WEIGHTS)],
               extra=[(dict(y=None), INVALID, BAD)])
    + [(f, 'mc1', dict(n=2 * N), INVALID, CJ_ITEMS) for f in ('oth_mtm_csd_jackknife', 'oth_mtm_csd_jackknife_dev')]
    + [('oth_mtm_csd_jackknife_dev', 'mc', dict(y=None, n=N - 1), INVALID, BAD)]
    # adaptive: iters between "bad argument" and the stride
    + rows_for('oth_mtm_adaptive', 'm', ('mz', (UNSUPPORTED, AD_RATIOS), 'm1', (UNSUPPORTED, AD_ONE)),
               [('w', UNSUPPORTED, AD_NOTAPERS), ('m1', UNSUPPORTED, AD_ONE), ('mz', UNSUPPORTED, AD_RATIOS)],
               extra=[(dict(iters=0), INVALID, AD_ITERS), (dict(iters=65), INVALID, AD_ITERS), (dict(iters=0, o0=None), INVALID, BAD),
                      (dict(iters=0, n=N - 1), INVALID, AD_ITERS)])
    + [('oth_mtm_adaptive_dev', 'm', dict(iters=0, ns=3, stride=NS - 1), INVALID, AD_ITERS)]
    # cyclic: no cycle frequencies goes in front of a NULL input
    + rows_for('oth_welch_cyclic', 'wc', ('w', (UNSUPPORTED, CY_NONE), 'wmed', (UNSUPPORTED, CY_MEDIAN)),
               [('m', UNSUPPORTED, CY_MTM), ('wmed', UNSUPPORTED, CY_MEDIAN), ('w32', UNSUPPORTED, CY_SIZE), ('w', UNSUPPORTED, CY_NONE)],
               streams=CY_STREAMS)
    + [('oth_welch_cyclic_dev', 'w', dict(x=None), UNSUPPORTED, CY_NONE)]
    # caf: no lags goes in front of a NULL input; the length rule carries the largest lag (69 samples: 68 is too short)
    + rows_for('oth_welch_caf', 'wl', ('w', (UNSUPPORTED, LG_NONE), 'wmed', (UNSUPPORTED, LG_MEDIAN)),
               [('m', UNSUPPORTED, LG_MTM), ('wmed', UNSUPPORTED, LG_MEDIAN), ('w32', UNSUPPORTED, LG_SIZE), ('w', UNSUPPORTED, LG_NONE)],
               extra=[(dict(n=N + 4), INVALID, LG_SHORT)], streams=LG_STREAMS, short=LG_SHORT)
    + [('oth_welch_caf_dev', 'w', dict(x=None), UNSUPPORTED, LG_NONE)]
    # the matrix: the plan, nchan, the input, the rows, the stride, the length - it has no stream count and no "bad argument"
    + [(f, key, ov, code, text) for f in ('oth_welch_matrix', 'oth_welch_matrix_dev') for key, ov, code, text in (
        ('m', {}, UNSUPPORTED, MT_MTM), ('wmed', {}, UNSUPPORTED, MT_MEDIAN), ('w32', {}, UNSUPPORTED, MT_SIZE),
        ('w', dict(nchan=1), INVALID, MT_NCHAN), ('w', dict(nchan=0), INVALID, MT_NCHAN), ('w', dict(nchan=9), INVALID, MT_NCHAN),
        ('w', dict(x=None), INVALID, MT_INPUT), ('w', dict(o0=None, o1=None), INVALID, MT_ROWS), ('w', dict(n=N - 1), INVALID, SHORT),
        # two at once: which goes first
        ('m', dict(nchan=9), UNSUPPORTED, MT_MTM), ('wmed', dict(x=None), UNSUPPORTED, MT_MEDIAN),
        ('w', dict(nchan=9, x=None), INVALID, MT_NCHAN), ('w', dict(x=None, o0=None, o1=None), INVALID, MT_INPUT),
        ('w', dict(o0=None, o1=None, n=N - 1), INVALID, MT_ROWS))]
    + [('oth_welch_matrix_dev', 'w', dict(stride=NS - 1), INVALID, MT_STRIDE),
       ('oth_welch_matrix_dev', 'w', dict(n=N - 1, stride=N - 2), INVALID, MT_STRIDE),
       ('oth_welch_matrix_dev', 'w', dict(o0=None, o1=None, stride=NS - 1), INVALID, MT_ROWS)]
)

SETTERS = [
    ('oth_mtm_set_ratios', 'w', [0.9], UNSUPPORTED, RT_NOTAPERS), ('oth_mtm_set_ratios', 'm', None, INVALID, RT_NULL),
    ('oth_mtm_set_ratios', 'm', [0.9, 0.0, 0.5], INVALID, RT_RANGE), ('oth_mtm_set_ratios', 'm', [0.9, 1.5, 0.5], INVALID, RT_RANGE),
    ('oth_mtm_set_ratios', 'm', [0.9, float('nan'), 0.5], INVALID, RT_RANGE), ('oth_mtm_set_ratios', 'w', None, UNSUPPORTED, RT_NOTAPERS),
    ('oth_welch_set_cycles', 'm', [0.1], UNSUPPORTED, CY_MTM), ('oth_welch_set_cycles', 'wmed', [0.1], UNSUPPORTED, CY_MEDIAN),
    ('oth_welch_set_cycles', 'w32', [0.1], UNSUPPORTED, CY_SIZE), ('oth_welch_set_cycles', 'w', [], INVALID, SC_COUNT),
    ('oth_welch_set_cycles', 'w', [0.0] * 65, INVALID, SC_COUNT), ('oth_welch_set_cycles', 'w', None, INVALID, SC_NULL),
    ('oth_welch_set_cycles', 'w', [0.1, 0.6], INVALID, SC_RANGE), ('oth_welch_set_cycles', 'w', [float('inf')], INVALID, SC_RANGE),
    ('oth_welch_set_cycles', 'm', [], UNSUPPORTED, CY_MTM), ('oth_welch_set_cycles', 'w', (0, None), INVALID, SC_COUNT),
    ('oth_welch_set_lags', 'm', [1], UNSUPPORTED, LG_MTM), ('oth_welch_set_lags', 'wmed', [1], UNSUPPORTED, LG_MEDIAN),
    ('oth_welch_set_lags', 'w32', [1], UNSUPPORTED, LG_SIZE), ('oth_welch_set_lags', 'w', [], INVALID, SL_COUNT),
    ('oth_welch_set_lags', 'w', [0] * 65, INVALID, SL_COUNT), ('oth_welch_set_lags', 'w', None, INVALID, SL_NULL),
    ('oth_welch_set_lags', 'w', [1, -1], INVALID, SL_RANGE), ('oth_welch_set_lags', 'w', [65536], INVALID, SL_RANGE),
    ('oth_welch_set_lags', 'm', [], UNSUPPORTED, LG_MTM), ('oth_welch_set_lags', 'w', (0, None), INVALID, SL_COUNT),
]


@pytest.fixture(scope='module')
def rig(hip):
    c = hip.Context(0)
    plans = make_plans(c)
    d_in, d_out = c.alloc(2 * X.nbytes), c.alloc(4 * 4 * ROW)
    c.h2d(d_in, np.concatenate([X, X]))
    yield c, plans, d_in, d_out
    c.free(d_in)
    c.free(d_out)
    for p in plans.values():
        p.close()
    c.close()


def call(hip, rig, form, key, ov):
    """The entry point with valid arguments but for the overrides -> (code, last-error text, resources it left behind)."""
    c, plans, d_in, d_out = rig
    spec, dev = FORMS[form]
    host = [np.zeros(ROW, np.float32) for _ in range(4)]
    nseg = C.c_uint64()
    val = dict(n=NS, dev=0, ns=1, nchan=2, stride=NS, iters=4)
    val.update({k: v for k, v in ov.items() if k in val})
    args = []
    for a in spec.split():
        name = a.lstrip('@')
        if name == 'nseg':
            args.append(C.byref(nseg))
        elif name in val:
            args.append(val[name])
        elif name in ov and ov[name] is None:
            args.append(None)
        elif name in ('x', 'y'):
            src = d_in + (X.nbytes if name == 'y' else 0)
            args.append(C.c_void_p(src) if dev else X.ctypes.data_as(C.c_void_p))
        else:
            r = int(name[1])
            args.append(C.c_void_p(d_out + 4 * ROW * r) if dev else host[r].ctypes.data_as(C.POINTER(C.c_float)))
    gc.collect()
    before = hip.live_resources()
    rc = getattr(c.lib, form)(plans[key].h, *args)
    return rc, c.lib.oth_last_error(c.h).decode(), tuple(np.subtract(hip.live_resources(), before))


@pytest.mark.parametrize('form,key,ov,code,text', TABLE, ids=['%s-%s-%s' % (f, k, ','.join('%s=%s' % i for i in sorted(o.items())) or 'plan')
                                                               for f, k, o, _, _ in TABLE])
def test_refusal(hip, rig, form, key, ov, code, text):
    rc, said, left = call(hip, rig, form, key, ov)
    print(form, key, ov, rc, repr(said), left)
    assert (rc, said) == (code, text)
    assert left == (0, 0, 0)      # refused before anything is allocated or staged


@pytest.mark.parametrize('form,key,values,code,text', SETTERS, ids=['%s-%s-%d' % (f, k, i) for i, (f, k, _, _, _) in enumerate(SETTERS)])
def test_setter_refusal(hip, rig, form, key, values, code, text):
    c, plans, _, _ = rig
    count = None
    if isinstance(values, tuple):
        count, values = values
    lags = form == 'oth_welch_set_lags'
    arr = None if values is None else np.asarray(values + [0], np.int32 if lags else np.float64)      # (never an empty buffer)
    ptr = None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int if lags else C.c_double))
    gc.collect()
    before = hip.live_resources()
    if form == 'oth_mtm_set_ratios':
        rc = c.lib.oth_mtm_set_ratios(plans[key].h, ptr)
    else:
        rc = getattr(c.lib, form)(plans[key].h, (1 if values is None else len(values)) if count is None else count, ptr)
    said = c.lib.oth_last_error(c.h).decode()
    print(form, key, values, rc, repr(said))
    assert (rc, said) == (code, text)
    assert hip.live_resources() == before


def test_the_valid_calls_of_the_table_succeed(hip, rig):
    """The defaults the table overrides are valid: each entry point returns OTH_OK on its plan, with the segment count."""
    for form, key in (('oth_mtm_ftest', 'm'), ('oth_welch_sk', 'w'), ('oth_mtm_jackknife', 'm'), ('oth_mtm_csd_jackknife', 'mc'),
                      ('oth_mtm_adaptive', 'm'), ('oth_welch_cyclic', 'wc'), ('oth_welch_caf', 'wl'), ('oth_welch_matrix', 'w')):
        for f in (form, form + '_dev'):
            rc, said, _ = call(hip, rig, f, key, {})
            assert rc == 0, (f, said)
    rig[0].sync()
