"""The seeded random-shape cases of the per-bin statistic families (test_stat_fuzz_cpu.py, test_stat_fuzz_gpu.py,
tools/stat_fuzz.py) - a plain module, no fixtures, no GPU: the case generator, the family table and the memory layout.

cases(family, nfft, seed) draws from numpy.random.default_rng((seed, family index, nfft)) exactly three cases, one of each
class: A full segments (nperseg = nfft, overlap 0 or 50 %, one stream, output stage / detrend / scaling drawn), B awkward
segments (nperseg < nfft, any overlap, fftshift with a trim, dB drawn, 2 ... 5 streams), C many items per workgroup (a
short odd-or-even step of nfft / 16 ... nfft / 8 samples and as many streams as fit under CAP samples; a family that takes
one capture per launch - the matrix, the two-channel multitaper calls - takes as many segments instead).  What has to occur
over a family's 27 cases whatever the seed - every build, every output stage (class A), every optional-row pattern, the
minimum segment count - is picked through a seeded permutation of the case's ordinal, not by an independent draw.

Every family's input comes from that family's own builder and amplitude rule (FAMILY[...].stream), and every comparison is
the family's own (imported from its test file, unchanged).  Where the draw of a family is narrower than the classes above:
  pfb      takes nperseg == nfft only (the header's rule): its class B is an arbitrary hop with fftshift, trim and dB, and it
           has no nperseg < 64; ntaps is drawn from what CAP leaves room for (2 or 3 in class C).  The 35 - 20j offset goes
           on detrending plans only, as in its parity list.  Above 512 points a case has at least three frames' worth of
           new samples, (nseg - 1) step >= 2 nfft, as the parity list has: the gate is per bin, and one frame - or a few
           that share nearly every sample - is a single periodogram whose deepest bins float32 does not hold
           (welch_pfb_oracle.emulate32 on one frame of noise: 2.6e-5 at 1024 x 5 taps, 2.1e-4 at 4096 x 11, 4.3e-4 at
           16384 x 12).  The one-frame case is the class-A case at 64 points.
  jack,    the comparisons run with caps=False, as the families' own many-stream tests do: the caps on the share of
  csdjack  ill-conditioned bins describe the parity list's inputs, and at the minimum M = K = 3 on 64 bins a random draw
           passes them by chance only.  The bound itself, RTOL ref / (1 - tmax), is unchanged.
  mtmcsd,  one pair per launch (the entry points take no stream count); dB is never set (every oth_csd_* call refuses it).
  csdjack  Class C bounds the segment count by 2^21 / (K nfft) items so that the oracle's per-item arrays stay small.
  csdjack  Class C has at most 2500 items (M = K nseg).  d_i = z(C_i) - z(C) is of the size of 1 / M and the difference
           of two float32 atanh of the size of 1, so every d_i carries an error of an ulp of z and the sum of their
           squares a bias that grows as M^2: the header's formulas evaluated in float32 on the CPU (CsdJack.emulate) read
           1.95 of the zsd bound at M = 16384 (128 points x 4096 segments x K 4; the GPU read 2.16 there, and 0.72 at
           M = 9000 in test_mtm_jackknife_gpu.py), 0.31 at 4096 - where the GPU read up to 0.86 (256 points x 1365
           segments x K 3 at a step of 20 samples).  2500 items are still more than the 1280 workgroups the device holds of
           the 1024-point build, so a class-C launch walks runs of unequal length there.
  caf      lags up to 200 samples (0 in the list or not): a longer reach only moves the first sample.  A one-segment case
           (one segment occurs up to 512 points only, three and more above, as in the parity list: at 16384 points one
           segment read 1.6e-4 of the row's mean in float32) always detrends and has no offset: its gate is RTOL of the row's mean, and a strong line in the lag product -
           its own mean without detrend (the power, at lag 0; a tone times its own lagged conjugate at any lag), the
           offset times the tone under it - is a bin float32 reads to 2 eps of its peak: 5.6e-5 and 5.3e-5 of the row's
           mean at 1024 points (pocketfft on complex64).
  cyc      above 512 points a case has two segments or more, as its parity list has: one periodogram's deepest bin read
           0.44 of the PSD gate in float32 at 8192 points.
  jack,    above 512 points a case has M = K nseg >= 7 items (the parity lists' smallest M there).  lnsd is the spread of the
  csdjack  items' l_i, and the bound RTOL ref / (1 - tmax) conditions on tmax -> 1 only: in a bin whose three or four items
           are nearly equal ref -> 0, and among 16384 bins some are (18 bins with ref < 0.02 at K = 3, one segment).  On
           an MI355X one of them read 2.29 of the bound - ref 0.0043, off by 1.5e-6 absolute, the PSD of the same bin
           good to 3.7e-7 - where pocketfft on complex64 read 0.37 in another such bin; with seven items no bin comes near.
  jack,    class C has seven segments or more: two segments that share 15 / 16 of their samples read 0.86 of the lnsd
  csdjack  bound in float32 at 16384 points.
  sk, cyc, the strong tone's amplitude is test_welch_sk_gpu.amp_for of the segments that share no sample
  mat      (independent_segments), not of nseg: at a step of nfft / 16 the rule's "M independent periodograms" are two or
           three, and amp_for(nseg) read 0.80 of the matrix gate in float32 at 16384 points x 92 segments.
In every multitaper family NW and K come from the pairs of the parity lists with 4 NW <= nperseg.  mtm, mtmcsd, ftest, adapt
and sk passed the half-gate emulation of test_stat_fuzz_cpu.py as drawn (adapt and pfb through their kernel-order emulations)."""
import collections
import contextlib
import functools
import zlib

import numpy as np

import fuzz_layout as FL
import median_oracle as MO
from fuzz_layout import BEHIND, NAN64, float32_transform  # noqa: F401 - the layout's names, as this module had them
from stat_support import FS, POWERS

SEED = 68                  # the suite's seed
CAP = 1 << 18              # complex samples a launch reads, over streams or channels
PILOT = 64
FAMILIES = ('mtm', 'mtmcsd', 'ftest', 'jack', 'csdjack', 'adapt', 'sk', 'cyc', 'caf', 'mat', 'pfb')
CLASSES = 'ABC'
NW_K = ((2.0, 3), (2.5, 4), (3.0, 5), (4.0, 7), (8.0, 15))
OFFSET = 35.0 - 20.0j
RTOL = 1e-4                # the project's parity tolerance (tests/test_hip_parity.py), spelled out: this module loads without a GPU
WELCH_SCALINGS = ('density', 'spectrum', 'raw', 'over_n2')
MTM_SCALINGS = ('density', 'raw', 'over_n2')

Case = collections.namedtuple('Case', 'family cls nfft nperseg noverlap nseg tail nstreams gap lead lead_y detrend scaling '
                                      'fftshift trim db offset rows extra seed')


def segs(minimum):
    return (minimum, minimum + 1, 3, 7, 8, 9, 11, 19)


def segs_c(minimum):
    return (minimum + 1, 7, 8, 9, 11, 13, 19)


# ---- what follows from a case ---------------------------------------------------------------------------------------------------

def step(c):
    return c.nperseg - c.noverlap


def nsamples(c):
    """samples of one stream or channel: the reach, nseg whole segments, the tail"""
    return FAMILY[c.family].reach(c) + c.noverlap + c.nseg * step(c) + c.tail


def owned(c):
    """... of which the oracle reads these; the tail behind them is NaN in the layout"""
    return nsamples(c) - c.tail


def stride(c):
    return nsamples(c) + c.gap


def lanes(c):
    """streams, or the matrix's channels: what lies one stride apart in the input buffer"""
    return FAMILY[c.family].lanes(c)


def out_len(c):
    return c.nfft - 2 * c.trim


def samples_read(c):
    F = FAMILY[c.family]
    return lanes(c) * (2 if F.pair else 1) * nsamples(c)


def items(c):
    """work items of one stream: segments, or (segment, taper) pairs where the launch splits those"""
    return c.nseg * (c.extra[1] if c.family in ('mtm', 'mtmcsd', 'jack', 'csdjack') else 1)


def independent_segments(c):
    """What the amplitude rule test_welch_sk_gpu.amp_for counts: segments that share no sample.  The parity lists overlap by
    half at most and pass nseg; a drawn step may be a sixteenth of the segment, whose nseg periodograms are a few
    independent ones seen many times."""
    return max(1, min(c.nseg, (owned(c) - FAMILY[c.family].reach(c)) // c.nperseg))


def shape_text(c):
    return '%s %s nfft=%d nperseg=%d noverlap=%d nseg=%d streams=%d n=%d gap=%d %s%s%s %s%s%s %s' % (
        c.family, c.cls, c.nfft, c.nperseg, c.noverlap, c.nseg, lanes(c), nsamples(c), c.gap, c.scaling, '' if c.detrend else ' raw-mean',
        ' +offset' if c.offset else '', 'shift ' if c.fftshift else '', 'trim=%d ' % c.trim if c.trim else '', 'dB ' if c.db else '',
        'rows=%s extra=%s' % (''.join('1' if r else '0' for r in c.rows), (c.extra,)))


# ---- the draw -------------------------------------------------------------------------------------------------------------------

def _perm(seed, family, name, count=27):
    return np.random.default_rng((seed, FAMILIES.index(family), zlib.crc32(name.encode()))).permutation(count)


def cases(family, nfft, seed=SEED):
    """exactly three cases, one of each class, for one family and size"""
    rng = np.random.default_rng((seed, FAMILIES.index(family), nfft))
    return [_draw(family, cls, nfft, seed, rng) for cls in CLASSES]


def all_cases(seed=SEED, families=FAMILIES):
    return [c for f in families for n in POWERS for c in cases(f, n, seed)]


def _draw(family, cls, nfft, seed, rng):
    F = FAMILY[family]
    size_i, cls_i = POWERS.index(nfft), CLASSES.index(cls)
    ordinal = 3 * size_i + cls_i

    def pick(name, options, among_a=False):
        """one of `options`, so that over the 27 cases of (seed, family) - among_a: over its nine of class A - each occurs"""
        k = _perm(seed, family, name, 9)[size_i] if among_a else _perm(seed, family, name)[ordinal]
        return options[int(k) % len(options)]

    # segments
    if cls == 'A':
        nperseg = nfft
        noverlap = int(rng.choice([0, nfft // 2]))
    elif cls == 'B':
        lo = max(8, nfft // 8)
        hi = nfft - 1
        if nfft <= 256 and (seed + nfft // 128) % 2 == 0:
            hi = min(hi, PILOT - 1)      # shorter than the pilot
        nperseg = nfft if F.full_segments else int(rng.integers(lo, hi + 1))
        noverlap = int(rng.integers(1, nperseg))
    else:
        nperseg = nfft
        noverlap = nperseg - int(rng.integers(max(1, nfft // 16), nfft // 8 + 1))
    stp = nperseg - noverlap
    tail = int(rng.integers(0, stp))
    # the output stage, detrend, scaling
    if cls == 'A':
        stage = pick('stage', range(8), among_a=True)
        fftshift, trimmed, db = bool(stage & 1), bool(stage & 2), bool(stage & 4)
    elif cls == 'B':
        fftshift, trimmed, db = True, True, bool(rng.integers(2))
    else:
        fftshift, trimmed, db = (bool(v) for v in rng.integers(2, size=3))
    trim = int(rng.integers(1, nfft // 2)) if trimmed else 0
    db = db and F.db
    mean = pick('mean', ('none',) * 6 + ('detrend',) * 5 + ('offset',))      # detrend on in half, the offset in one of six of those
    detrend, offset = mean != 'none', mean == 'offset'
    scaling = str(rng.choice(F.scalings))
    rows = pick('rows', F.row_patterns)
    extra = F.extra(rng, pick, nfft, nperseg, cls)
    gap = int(rng.choice([0, 1, 67, 64 * int(rng.integers(1, 5)) + 3]))
    lead, lead_y = (int(v) for v in rng.integers(1, 8, size=2))
    data_seed = int(rng.integers(1 << 30))
    # counts: the class pins one of (segments, streams), the cap reduces the other
    probe = Case(family, cls, nfft, nperseg, noverlap, 0, tail, 1, gap, lead, lead_y, detrend, scaling, fftshift, trim, db, offset, rows,
                 extra, data_seed)
    per_lane = CAP // (F.lanes(probe) * (2 if F.pair else 1))      # samples one stream or channel may hold

    def fits(nseg):
        return F.reach(probe) + noverlap + nseg * stp + tail <= per_lane

    def most():
        return (per_lane - F.reach(probe) - noverlap - tail) // stp

    minimum = F.min_nseg
    if cls == 'C' and F.single:
        nseg = min(most(), F.most_segments(probe))
        nstreams = 1
    else:
        counts = segs_c(minimum) if cls == 'C' else segs(minimum)
        want = pick('nseg', counts, among_a=True) if cls == 'A' else int(rng.choice(counts))
        allowed = [s for s in sorted(set(counts)) if (s <= want and fits(s)) or s == min(counts)]
        nseg = allowed[-1]
        n = F.reach(probe) + noverlap + nseg * stp + tail
        if F.single or cls == 'A':
            nstreams = 1
        elif cls == 'B':
            nstreams = max(1, min(int(rng.integers(2, 6)), per_lane // n))
        else:
            nstreams = max(1, min(65535, per_lane // n))
    return F.narrow(probe._replace(nseg=int(nseg), nstreams=int(nstreams)))


def with_nseg(c, nseg):
    """the case at another segment count: the streams follow from the cap again (one capture: the count must fit)"""
    c = c._replace(nseg=int(nseg))
    if FAMILY[c.family].single or c.cls == 'A':
        assert samples_read(c._replace(nstreams=1)) <= CAP, shape_text(c)
        return c._replace(nstreams=1)
    return c._replace(nstreams=int(max(1, min(c.nstreams if c.cls == 'B' else 65535, CAP // nsamples(c)))))


def digest(seed=SEED):
    import hashlib
    return hashlib.sha256(repr(all_cases(seed)).encode()).hexdigest()


# ---- the domain, restated from include/ofdm_tools_hip.h --------------------------------------------------------------------------

def check_domain(c):
    F = FAMILY[c.family]
    n, K = nsamples(c), c.extra[1] if F.kind != 'welch' else 0
    assert c.nfft in POWERS                                                   # a power of two from 64 to 16384
    assert 1 <= c.nperseg <= c.nfft and 0 <= c.noverlap < c.nperseg
    assert 0 <= c.trim and 2 * c.trim < c.nfft
    assert stride(c) >= n and n >= F.reach(c) + c.nperseg                     # stream_stride >= nsamples >= reach + nperseg
    assert (n - F.reach(c) - c.noverlap) // step(c) == c.nseg and 0 <= c.tail < step(c)
    assert 1 <= c.nstreams <= 65535 and samples_read(c) <= CAP
    assert c.nseg >= F.min_nseg
    assert c.scaling in F.scalings and (F.db or not c.db)
    assert 1 <= c.lead <= 7 and 1 <= c.lead_y <= 7
    assert len(c.rows) == len(F.row_names) and c.rows in F.row_patterns
    if F.kind != 'welch':
        nw = c.extra[0]
        assert 1 <= K <= 64 and K <= c.nperseg and 0.0 < nw < 0.5 * c.nperseg and (nw, K) in NW_K
    if F.single:
        assert c.nstreams == 1
    if c.family in ('ftest', 'adapt'):
        assert K >= 2
    if c.family == 'adapt':
        assert 1 <= c.extra[2] <= 64                                          # iters
    if c.family == 'jack':
        assert K * c.nseg >= 2
    if c.family == 'csdjack':
        assert K * c.nseg >= 3
    if c.family in ('jack', 'csdjack'):
        assert c.extra[2] == 'unity'                                          # the items must be exchangeable
    if c.family == 'sk':
        assert c.nseg >= 2
    if c.family == 'cyc':
        alphas, group = c.extra
        assert 1 <= len(alphas) <= 64 and all(np.isfinite(a) and abs(a) <= 0.5 for a in alphas) and group in (1, 2, 4)
    if c.family == 'caf':
        lags, group = c.extra
        assert 1 <= len(lags) <= 64 and all(0 <= t <= 65535 for t in lags) and group in (1, 2) and n >= max(lags) + c.nperseg
    if c.family == 'mat':
        assert 2 <= c.extra[0] <= 8 and any(c.rows)
    if c.family == 'pfb':
        assert c.nperseg == c.nfft and 2 <= c.extra[0] <= 16 and n >= c.extra[0] * c.nfft
        assert (n - c.extra[0] * c.nfft) // step(c) + 1 == c.nseg


# ---- the memory layout ----------------------------------------------------------------------------------------------------------

def lane_data(c):
    """the finite samples of every lane: [lanes][nsamples] complex64, or for a pair (x, y) each [1][nsamples]"""
    return _lane_data(c)


@functools.lru_cache(maxsize=4)
def _lane_data(c):
    data = FAMILY[c.family].stream(c)
    for a in (data if isinstance(data, tuple) else (data,)):
        assert a.dtype == np.complex64 and a.shape == (lanes(c), nsamples(c)) and np.all(np.isfinite(a.view(np.float32)))
        a.setflags(write=False)
    return data


def with_nan_tail(c, lane):
    """one lane as the layout holds it: the tail behind its last whole segment reads NaN"""
    return FL.nan_tail(lane, owned(c))


def _buffer(c, lead, data):
    assert len(data) == lanes(c)
    return FL.nan_buffer(data, lead, stride(c), nsamples(c), owned(c))


def layout(c):
    """-> [(buffer, lead)]: one NaN-filled complex64 buffer per input pointer of the call (x, and y for a pair) with the
    oracle's samples in place; the call's pointer is `lead` samples in."""
    data = lane_data(c)
    if isinstance(data, tuple):
        return [(_buffer(c, c.lead, data[0]), c.lead), (_buffer(c, c.lead_y, data[1]), c.lead_y)]
    return [(_buffer(c, c.lead, data), c.lead)]


def lane_input(c, i):
    """what the oracle of lane i takes: the lane with its NaN tail (a pair: (x, y); the matrix: every channel)"""
    data = lane_data(c)
    if isinstance(data, tuple):
        return tuple(with_nan_tail(c, d[i]) for d in data)
    if c.family == 'mat':
        return with_nan_tail(c, data)
    return with_nan_tail(c, data[i])


def units(c):
    """independent results of a launch: its streams; one for the matrix and for a pair"""
    return 1 if FAMILY[c.family].single else c.nstreams


# ---- the families ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dpss(nperseg, nw, K):
    from ofdm_tools import windows
    tapers, ratios = windows.dpss(nperseg, nw, K, return_ratios=True)
    tapers.setflags(write=False)
    ratios.setflags(write=False)
    return tapers, ratios


def _st(c, row, db=False):
    return MO.shift_trim_db(np.asarray(row), c.fftshift, c.trim, db)


def _n_of(c):
    return nsamples(c)


def _with_offset(c, x):
    return (x + np.complex64(OFFSET)).astype(np.complex64) if c.offset else x


def _mtm_scale(scaling, nfft):
    return {'density': 1.0 / FS, 'raw': 1.0, 'over_n2': 1.0 / float(nfft) ** 2}[scaling]


def _complex_rows(a):
    """device rows of re, im pairs [..., 2] -> complex"""
    return a[..., 0] + 1j * a[..., 1]


class Family(object):
    """One row of the family table.  kind: the plan ('welch', 'mtm', 'mtmcsd'); kernel: what last_recipe starts with;
    row_names / required: the output rows of the _dev call in the order the methods below use, and which may be NULL;
    floats(c, name): a row's floats per unit; pair: x and y pointers; single: one capture per launch."""
    kind, kernel, scalings, db, pair, single, full_segments, min_nseg = 'welch', '', WELCH_SCALINGS, True, False, False, False, 1
    row_names, required = (), ()
    env = None

    def __init__(self):
        import itertools
        self.row_patterns = tuple(p for p in itertools.product((True, False), repeat=len(self.row_names))
                                  if all(p[i] for i, n in enumerate(self.row_names) if n in self.required) and self.pattern_ok(p))

    def pattern_ok(self, p):
        return True

    def reach(self, c):
        return 0

    def lanes(self, c):
        return c.nstreams

    def most_segments(self, c):
        return 1 << 30

    def floats(self, c, name):
        return out_len(c)

    def forced(self, c):
        """(environment variable, value, recipe text) of the build the case forces (no variable: the build follows from the
        call), or None"""
        return None

    def shaped(self, c, name, a):
        """one unit's device row `name`, float32 [floats(c, name)], as the comparison takes it"""
        return a

    lone_from = None      # above 512 points a case takes at least this many segments (None: the family's minimum)
    c_from = None         # class C takes at least this many

    def narrow(self, c):
        """the drawn case, or the nearest one the family's gate is reachable at in float32 (the module's docstring says why)"""
        if self.lone_from and c.cls == 'A' and c.nfft == 64:
            return with_nseg(c, self.min_nseg)      # the family's minimum, in every seed
        need = max(c.nseg, self.lone_from if self.lone_from and c.nfft > 512 else 0, self.c_from if self.c_from and c.cls == 'C' else 0)
        if need == c.nseg:
            return c
        counts = segs_c(self.min_nseg) if c.cls == 'C' else segs(self.min_nseg)
        return with_nseg(c, min(s for s in counts if s >= need))

    def recipe_front(self, c):
        return 'kernel=%s nfft=%d ' % (self.kernel, c.nfft)

    # -- multitaper plumbing
    def nwk(self, rng, pick, nperseg):
        return pick('nwk', [p for p in NW_K if 4.0 * p[0] <= nperseg and p[1] <= nperseg] or NW_K[:1])

    def tapers(self, c):
        return _dpss(c.nperseg, c.extra[0], c.extra[1])

    def weights(self, c):
        return 'unity' if c.extra[2] == 'unity' else self.tapers(c)[1]

    def mtm_plan(self, ctx, hip, c, make=None):
        from test_median_gpu import SCALINGS
        make = make or ctx.mtm_plan
        w = c.extra[2] if len(c.extra) > 2 and isinstance(c.extra[2], str) else 'unity'
        return make(c.nfft, nperseg=c.nperseg, noverlap=c.noverlap, nw=c.extra[0], ntapers=c.extra[1], weights=w,
                    detrend=hip.DETREND_CONSTANT if c.detrend else hip.DETREND_NONE, scaling=SCALINGS[c.scaling], fs=FS,
                    fftshift=c.fftshift, trim_bins=c.trim, db=c.db)

    def welch_plan(self, ctx, hip, c):
        from stat_support import welch_plan
        return welch_plan(ctx, hip, c.nfft, c.nperseg, c.noverlap, c.detrend, c.scaling, c.fftshift, c.trim, c.db)


class Mtm(Family):
    kind, kernel, scalings = 'mtm', 'mtm', MTM_SCALINGS
    row_names, required = ('psd',), ('psd',)

    def extra(self, rng, pick, nfft, nperseg, cls):
        return self.nwk(rng, pick, nperseg) + (pick('weights', ('unity', 'eigen')),)

    def recipe_front(self, c):
        return 'kernel=%s nfft=%d ntapers=%d ' % (self.kernel, c.nfft, c.extra[1])

    def stream(self, c):
        from test_median_gpu import noise_tones
        return np.stack([_with_offset(c, noise_tones(_n_of(c), c.seed + s)) for s in range(c.nstreams)])

    def oracle(self, c, x):
        import mtm_oracle as O
        return O.mtm_psd(x, c.nfft, c.nperseg, c.noverlap, c.extra[0], c.extra[1], self.weights(c), c.detrend, c.scaling, FS,
                         self.tapers(c)[0])

    def rows_of(self, c, ref):
        return {'psd': _st(c, ref, c.db)}

    def check(self, c, rows, ref, what=''):
        """the comparison test_mtm_gpu.py::test_parity_with_the_float64_oracle makes"""
        from test_hip_parity import relerr
        got = np.asarray(rows['psd'], np.float64)
        want = _st(c, ref)
        assert got.shape == want.shape and np.all(np.isfinite(got))
        err = relerr(10.0 ** (got / 10.0) if c.db else got, want)
        assert err < RTOL, (what, err)
        return {'psd': err / RTOL}

    def plan(self, ctx, hip, c):
        return self.mtm_plan(ctx, hip, c)

    def call_dev(self, plan, c, ins, outs):
        return plan.exec_dev(ins[0], nsamples(c), outs['psd'], nstreams=c.nstreams, stream_stride=stride(c))

    def call_host(self, plan, c, lane):
        return {'psd': plan.exec(lane)}


class MtmCsd(Mtm):
    kind, kernel, db, pair, single = 'mtmcsd', 'mtmcsd', False, True, True
    row_names, required = ('pxx', 'pyy', 'pxy', 'cxy'), ('cxy',)

    def lanes(self, c):
        return 1

    def most_segments(self, c):
        return max(self.min_nseg + 1, (1 << 21) // (c.extra[1] * c.nfft))

    def floats(self, c, name):
        return out_len(c) * (2 if name == 'pxy' else 1)

    def stream(self, c):
        from test_csd_gpu import _pair
        x, y = _pair(_n_of(c), c.seed)
        return _with_offset(c, np.array(x))[None, :], _with_offset(c, np.array(y))[None, :]

    def oracle(self, c, xy):
        import mtm_csd_oracle as MC
        return MC.mtm_csd(xy[0], xy[1], c.nfft, c.nperseg, c.noverlap, c.extra[0], c.extra[1], self.weights(c), c.detrend, c.scaling,
                          FS, self.tapers(c)[0], c.fftshift, c.trim)

    def rows_of(self, c, ref):
        return dict(zip(self.row_names, ref))

    def check(self, c, rows, ref, what=''):
        """test_mtm_csd_gpu.py's parity comparison: test_csd_gpu.errors, each of the five under RTOL"""
        from test_csd_gpu import errors
        got = [np.asarray(rows[k]) for k in self.row_names]
        assert all(g.shape == r.shape and np.all(np.isfinite(g)) for g, r in zip(got, ref))
        e = errors(got, ref)
        assert max(e) < RTOL, (what, e)
        return dict(zip(('pxx', 'pyy', 'pxy', 'impxy', 'cxy'), (v / RTOL for v in e)))

    def plan(self, ctx, hip, c):
        return self.mtm_plan(ctx, hip, c, ctx.mtm_csd_plan)

    def call_dev(self, plan, c, ins, outs):
        return plan.csd_exec_dev(ins[0], ins[1], nsamples(c), **{k: outs[k] or 0 for k in self.row_names})

    def call_host(self, plan, c, lane):
        return dict(zip(self.row_names, plan.csd(lane[0], lane[1])))

    def shaped(self, c, name, a):
        return _complex_rows(a.reshape(-1, 2)) if name == 'pxy' else a


class Ftest(Mtm):
    kernel = 'mtmftest'
    row_names, required = ('f', 'line', 'resid'), ('f',)

    def extra(self, rng, pick, nfft, nperseg, cls):
        return self.nwk(rng, pick, nperseg)

    def stream(self, c):
        from test_median_gpu import noise_tones
        from test_mtm_ftest_gpu import on_off_tones
        return np.stack([_with_offset(c, noise_tones(_n_of(c), c.seed + s, on_off_tones(c.nfft))) for s in range(c.nstreams)])

    def oracle(self, c, x):
        import mtm_ftest_oracle as FO
        return FO.ftest(x, c.nfft, c.nperseg, c.noverlap, c.extra[0], c.extra[1], c.detrend, c.scaling, FS, self.tapers(c)[0])

    def rows_of(self, c, ref):
        return {'f': _st(c, ref['F']), 'line': _st(c, ref['line']), 'resid': _st(c, ref['resid'])}

    def check(self, c, rows, ref, what=''):
        from test_mtm_ftest_gpu import check_rows
        sums, f = check_rows((rows['f'], rows['line'], rows['resid']), ref, _mtm_scale(c.scaling, c.nfft), c.fftshift, c.trim)
        return {'sums': sums / RTOL, 'f': f}

    def call_dev(self, plan, c, ins, outs):
        return plan.ftest_dev(ins[0], nsamples(c), c.nstreams, stride(c), outs['f'], outs['line'], outs['resid'])

    def call_host(self, plan, c, lane):
        return dict(zip(self.row_names, plan.ftest(lane, return_rows=True)))


class Jack(Mtm):
    kernel, c_from = 'mtmjack', 7
    row_names, required = ('lnsd', 'psd'), ('lnsd',)

    def extra(self, rng, pick, nfft, nperseg, cls):
        return self.nwk(rng, pick, nperseg) + ('unity',)

    def stream(self, c):
        return np.stack([self._capture(c, s)[0] for s in range(c.nstreams)])

    def _capture(self, c, s):
        """test_mtm_jackknife_gpu.captures, line for line, at this case's length (its own arguments fix the tail at a third
        of a step and the overlap at whole per cents)"""
        from test_median_gpu import noise_tones
        from test_mtm_ftest_gpu import on_off_tones
        n, seed = _n_of(c), c.seed + s
        off = OFFSET if c.offset else 0.0
        x0 = noise_tones(n, seed, on_off_tones(c.nfft)).astype(np.complex128)
        rng = np.random.default_rng(seed + 100000)
        w = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
        y = 0.7 * np.roll(x0, 5) + w + off
        return (x0 + off).astype(np.complex64), y.astype(np.complex64)

    def narrow(self, c):
        c = Family.narrow(self, c)
        if c.cls == 'A' and c.nfft == 64:
            return with_nseg(c, self.min_nseg)      # the family's minimum, in every seed
        if c.nfft > 512 and c.extra[1] * c.nseg < self.LARGE_M:
            counts = segs_c(self.min_nseg) if c.cls == 'C' else segs(self.min_nseg)
            return with_nseg(c, min(s for s in counts if c.extra[1] * s >= self.LARGE_M))
        return c

    LARGE_M = 7      # items a case above 512 points has at least

    def kw(self, c):
        return dict(nperseg=c.nperseg, noverlap=c.noverlap, nw=c.extra[0], K=c.extra[1], detrend=c.detrend, scaling=c.scaling,
                    tapers=self.tapers(c)[0])

    def oracle(self, c, x):
        import mtm_jackknife_oracle as JO
        return JO.jackknife(x, c.nfft, **self.kw(c))

    def psd_of(self, c, S):
        return S * MO.plan_scale(np.ones(1), c.scaling, FS, c.nfft) / c.nseg

    def rows_of(self, c, ref):
        return {'lnsd': _st(c, ref['lnsd']), 'psd': _st(c, self.psd_of(c, ref['S']), c.db)}

    def check(self, c, rows, ref, what=''):
        from test_hip_parity import relerr
        from test_mtm_jackknife_gpu import check_lnsd
        share = check_lnsd(rows['lnsd'], ref['lnsd'], ref['tmax'], c.fftshift, c.trim, caps=False)
        psd = np.asarray(rows['psd'], np.float64)
        err = relerr(10.0 ** (psd / 10.0) if c.db else psd, _st(c, self.psd_of(c, ref['S'])))      # the row exec_dev gives: its gate
        assert err < RTOL, (what, err)
        return {'lnsd': share, 'psd': err / RTOL}

    def call_dev(self, plan, c, ins, outs):
        return plan.jackknife_dev(ins[0], nsamples(c), c.nstreams, stride(c), outs['lnsd'], outs['psd'])

    def call_host(self, plan, c, lane):
        return dict(zip(self.row_names, plan.jackknife(lane, return_psd=True)))


class CsdJack(Jack):
    kind, kernel, db, pair, single = 'mtmcsd', 'mtmcsdjack', False, True, True
    row_names, required = ('zsd', 'cxy', 'lnsdx', 'lnsdy'), ('zsd',)
    lanes = MtmCsd.lanes
    plan = MtmCsd.plan
    MOST_ITEMS = 2500

    def most_segments(self, c):
        return max(self.min_nseg + 1, min((1 << 21) // (c.extra[1] * c.nfft), self.MOST_ITEMS // c.extra[1]))

    def emulate(self, c, xy):
        """The closer emulation: single-precision transforms and the header's formulas per item in float32 - the ratios,
        log1p, the delete-one coherence with each factor kept at 2^-24 of its total, atanh and the difference d - with the
        totals and the sums over the items in double, as the finalize launch adds them."""
        import mtm_jackknife_oracle as JO
        f = np.float32
        with float32_transform():
            X, ck = JO.items(xy[0], c.nfft, **self.kw(c))
            Y, _ = JO.items(xy[1], c.nfft, **self.kw(c))
        p, q = (ck[:, None] * np.abs(X) ** 2).astype(f), (ck[:, None] * np.abs(Y) ** 2).astype(f)
        r = (ck[:, None] * np.conj(X) * Y).astype(np.complex64)
        M = p.shape[0]
        Sxx, Syy = p.sum(axis=0, dtype=np.float64).astype(f), q.sum(axis=0, dtype=np.float64).astype(f)
        Sxy = r.sum(axis=0, dtype=np.complex128).astype(np.complex64)
        CL, floor = f(JO.CL), f(2.0 ** -24)

        def z(v):
            return np.arctanh(np.minimum(np.sqrt(v, dtype=f), CL), dtype=f)

        def sd(v):
            v = v.astype(np.float64)
            return np.sqrt(np.maximum((M - 1.0) / M * ((v * v).sum(axis=0) - v.sum(axis=0) ** 2 / M), 0.0))

        C = ((Sxy.real * Sxy.real + Sxy.imag * Sxy.imag) / (Sxx * Syy)).astype(f)
        rest = Sxy[None, :] - r
        Ci = ((rest.real * rest.real + rest.imag * rest.imag) /
              (np.maximum(Sxx[None, :] - p, floor * Sxx[None, :]) * np.maximum(Syy[None, :] - q, floor * Syy[None, :]))).astype(f)
        return {'zsd': sd(z(Ci) - z(C)[None, :]), 'cxy': C.astype(np.float64),
                'lnsdx': sd(np.log1p(-np.minimum(p / Sxx[None, :], CL), dtype=f)),
                'lnsdy': sd(np.log1p(-np.minimum(q / Syy[None, :], CL), dtype=f))}

    def stream(self, c):
        x, y = self._capture(c, 0)
        return x[None, :], y[None, :]

    def oracle(self, c, xy):
        import mtm_jackknife_oracle as JO
        return JO.csd_jackknife(xy[0], xy[1], c.nfft, **self.kw(c))

    def rows_of(self, c, ref):
        return {'zsd': _st(c, ref['zsd']), 'cxy': _st(c, ref['cxy']), 'lnsdx': _st(c, ref['lnsd_x']), 'lnsdy': _st(c, ref['lnsd_y'])}

    def check(self, c, rows, ref, what=''):
        from test_mtm_jackknife_gpu import check_lnsd, check_zsd
        out = {'zsd': check_zsd(rows['zsd'], ref, c.fftshift, c.trim, caps=False),
               'lnsdx': check_lnsd(rows['lnsdx'], ref['lnsd_x'], ref['tmax_x'], c.fftshift, c.trim, caps=False),
               'lnsdy': check_lnsd(rows['lnsdy'], ref['lnsd_y'], ref['tmax_y'], c.fftshift, c.trim, caps=False)}
        cxy = np.asarray(rows['cxy'], np.float64)      # the plan's own Cxy: the gate of test_csd_gpu.errors on it
        err = float(np.max(np.abs(cxy - _st(c, ref['cxy']))))
        assert cxy.shape == (out_len(c),) and err < RTOL, (what, err)
        out['cxy'] = err / RTOL
        return out

    def call_dev(self, plan, c, ins, outs):
        return plan.csd_jackknife_dev(ins[0], ins[1], nsamples(c), outs['zsd'], outs['cxy'], outs['lnsdx'], outs['lnsdy'])

    def call_host(self, plan, c, lane):
        cxy, zsd, lx, ly = plan.csd_jackknife(lane[0], lane[1])
        return {'zsd': zsd, 'cxy': cxy, 'lnsdx': lx, 'lnsdy': ly}


class Adapt(Mtm):
    kernel = 'mtmadapt'
    row_names, required = ('psd', 'dof'), ('psd',)

    def extra(self, rng, pick, nfft, nperseg, cls):
        return self.nwk(rng, pick, nperseg) + (pick('iters', (1, 4)),)

    def recipe_front(self, c):
        return 'kernel=%s nfft=%d ntapers=%d iters=%d ' % (self.kernel, c.nfft, c.extra[1], c.extra[2])

    def stream(self, c):
        import mtm_adaptive_oracle as AO
        return np.stack([AO.band_capture(_n_of(c), c.seed + s, 40.0, c.nfft, OFFSET if c.offset else 0.0) for s in range(c.nstreams)])

    def oracle(self, c, x):
        import mtm_adaptive_oracle as AO
        return AO.adaptive(x, c.nfft, c.nperseg, c.noverlap, c.extra[0], c.extra[1], c.extra[2], c.detrend, c.scaling, FS)

    def emulate(self, c, x):
        """the closer emulation: the kernel's own float32 order (mtm_adaptive_oracle.emulate32)"""
        import mtm_adaptive_oracle as AO
        Sm, dof = AO.emulate32(x[:owned(c)], c.nfft, c.nperseg, c.noverlap, c.extra[0], c.extra[1], c.extra[2], c.detrend)
        return {'psd': _mtm_scale(c.scaling, c.nfft) * Sm, 'dof': dof}

    def rows_of(self, c, ref):
        return {'psd': _st(c, ref['psd'], c.db), 'dof': _st(c, ref['dof'])}

    def check(self, c, rows, ref, what=''):
        from test_mtm_adaptive_gpu import check_rows
        s, nu = check_rows(rows['psd'], rows['dof'], ref, _mtm_scale(c.scaling, c.nfft), c.fftshift, c.trim, c.db)
        return {'psd': s, 'dof': nu}

    def call_dev(self, plan, c, ins, outs):
        return plan.adaptive_dev(ins[0], nsamples(c), c.nstreams, stride(c), outs['psd'], outs['dof'], iters=c.extra[2])

    def call_host(self, plan, c, lane):
        return dict(zip(self.row_names, plan.adaptive(lane, iters=c.extra[2], return_dof=True)))


class Sk(Family):
    kernel, min_nseg = 'welchsk', 2
    row_names, required = ('sk', 'psd'), ('sk',)

    def extra(self, rng, pick, nfft, nperseg, cls):
        return ()

    def tones(self, c):
        from test_welch_sk_gpu import amp_for, tones_for
        return tones_for(c.nfft, amp_for(independent_segments(c), c.nfft * c.nstreams))

    def stream(self, c):
        from test_median_gpu import noise_tones
        return np.stack([_with_offset(c, noise_tones(_n_of(c), c.seed + s, self.tones(c))) for s in range(c.nstreams)])

    def oracle(self, c, x):
        import welch_sk_oracle as SO
        ref = SO.sk(x, c.nfft, c.nperseg, c.noverlap, 'hann', c.detrend)
        ref['psd'] = SO.psd(ref, 'hann', c.nperseg, c.scaling, FS, c.nfft)
        return ref

    def rows_of(self, c, ref):
        return {'sk': _st(c, ref['SK']), 'psd': _st(c, ref['psd'], c.db)}

    def check(self, c, rows, ref, what=''):
        from test_welch_sk_gpu import RTOL_R, check_rows
        e_p, e_r = check_rows(rows['sk'], rows['psd'], ref, ref['psd'], c.fftshift, c.trim, c.db)
        return {'psd': e_p / RTOL, 'r': e_r / RTOL_R}

    def plan(self, ctx, hip, c):
        return self.welch_plan(ctx, hip, c)

    def call_dev(self, plan, c, ins, outs):
        return plan.sk_dev(ins[0], nsamples(c), c.nstreams, stride(c), outs['sk'], outs['psd'])

    def call_host(self, plan, c, lane):
        return dict(zip(self.row_names, plan.sk(lane, return_psd=True)))


class Cyc(Sk):
    kernel, min_nseg, lone_from = 'welchcyc', 1, 2
    row_names, required = ('coh', 'scf', 'psd'), ('coh',)
    POOL = (0.0, 0.0123456789, -0.37, 1.0 / 80.0, 0.5, -0.5)

    def extra(self, rng, pick, nfft, nperseg, cls):
        A = pick('ncyc', (1, 2, 3, 4, 5))
        alphas = [float(self.POOL[i]) if rng.integers(2) else float(np.round(rng.uniform(-0.5, 0.5), 9))
                  for i in rng.permutation(len(self.POOL))[:A]]
        return tuple(alphas), pick('group', (1, 2, 4))

    def forced(self, c):
        return 'OTH_CYC_GROUP', c.extra[1], ' ncyc=%d group=%d ' % (len(c.extra[0]), c.extra[1])

    def floats(self, c, name):
        return out_len(c) * {'coh': len(c.extra[0]), 'scf': 2 * len(c.extra[0]), 'psd': 1}[name]

    def oracle(self, c, x):
        import welch_cyclic_oracle as CO
        return CO.cyclic(x, c.nfft, c.extra[0], c.nperseg, c.noverlap, 'hann', c.detrend, c.scaling, FS)

    def rows_of(self, c, ref):
        # (coh is clamped to [0, 1], as the library's is: alpha = 0 reads 1 up to a rounding of the oracle's)
        return {'coh': np.clip(_st(c, ref['coh']), 0.0, 1.0), 'scf': _st(c, ref['scf']), 'psd': _st(c, ref['psd'], c.db)}

    def check(self, c, rows, ref, what=''):
        from test_welch_cyclic_gpu import check_rows
        e_p, e_s, e_c = check_rows(rows['scf'], rows['coh'], rows['psd'], ref, c.fftshift, c.trim, c.db)
        return {'psd': e_p / RTOL, 'scf': e_s / RTOL, 'coh': e_c / (4 * RTOL)}

    def plan(self, ctx, hip, c):
        plan = self.welch_plan(ctx, hip, c)
        plan.set_cycles(c.extra[0])
        return plan

    def call_dev(self, plan, c, ins, outs):
        return plan.cyclic_dev(ins[0], nsamples(c), c.nstreams, stride(c), outs['coh'], outs['scf'], outs['psd'])

    def call_host(self, plan, c, lane):
        scf, coh, psd = plan.cyclic(lane, return_psd=True)
        return {'coh': coh, 'scf': scf, 'psd': psd}

    def shaped(self, c, name, a):
        A = len(c.extra[0])
        if name == 'scf':
            return _complex_rows(a.reshape(A, -1, 2))
        return a.reshape(A, -1) if name == 'coh' else a


class Caf(Sk):
    kernel, min_nseg = 'welchlag', 1
    row_names, required = ('caf', 'r'), ('caf',)

    def extra(self, rng, pick, nfft, nperseg, cls):
        L = pick('nlags', (1, 2, 3, 4, 5))
        lags = [int(v) for v in rng.permutation(np.arange(1, 201))[:L]]
        if rng.integers(2):
            lags[int(rng.integers(L))] = 0
        return tuple(lags), pick('group', (1, 2))

    def reach(self, c):
        return max(c.extra[0])

    lone_from = 3

    def narrow(self, c):
        c = Family.narrow(self, c)
        return c._replace(detrend=True, offset=False) if c.nseg == 1 else c

    def forced(self, c):
        return 'OTH_LAG_GROUP', c.extra[1], ' nlags=%d group=%d ' % (len(c.extra[0]), c.extra[1])

    def floats(self, c, name):
        return len(c.extra[0]) * (out_len(c) if name == 'caf' else 2)

    def stream(self, c):
        from test_median_gpu import noise_tones
        return np.stack([_with_offset(c, noise_tones(_n_of(c), c.seed + s)) for s in range(c.nstreams)])

    def oracle(self, c, x):
        import welch_caf_oracle as LO
        ref = LO.caf(x, c.nfft, c.extra[0], c.nperseg, c.noverlap, 'hann', c.detrend, c.scaling, FS)
        assert ref['M'] == c.nseg
        return ref

    def rows_of(self, c, ref):
        return {'caf': _st(c, ref['caf'], c.db), 'r': ref['r']}

    def check(self, c, rows, ref, what=''):
        from test_welch_caf_gpu import check_rows
        e_c, e_r = check_rows(rows['caf'], rows['r'], ref, c.fftshift, c.trim, c.db, one_segment=c.nseg == 1)
        return {'caf': e_c / RTOL, 'r': e_r / RTOL}

    def plan(self, ctx, hip, c):
        plan = self.welch_plan(ctx, hip, c)
        plan.set_lags(list(c.extra[0]))
        return plan

    def call_dev(self, plan, c, ins, outs):
        return plan.caf_dev(ins[0], nsamples(c), c.nstreams, stride(c), outs['caf'], outs['r'])

    def call_host(self, plan, c, lane):
        return dict(zip(self.row_names, plan.caf(lane, return_r=True)))

    def shaped(self, c, name, a):
        L = len(c.extra[0])
        return a.reshape(L, -1) if name == 'caf' else _complex_rows(a.reshape(L, 2))


class Mat(Sk):
    kernel, min_nseg, single = 'welchmat', 1, True
    row_names, required = ('s', 'gcoh'), ()

    def pattern_ok(self, p):
        return any(p)

    def extra(self, rng, pick, nfft, nperseg, cls):
        return (pick('nchan', (2, 3, 4, 5, 6, 8)),)

    def lanes(self, c):
        return c.extra[0]

    def most_segments(self, c):
        return max(2, (1 << 22) // (c.extra[0] * c.nfft))

    def forced(self, c):
        C = c.extra[0]
        return None, None, ' nchan=%d cap=%d ' % (C, 2 if C == 2 else 4 if C <= 4 else 8)

    def floats(self, c, name):
        C = c.extra[0]
        return out_len(c) * (C * (C + 1) if name == 's' else 1)

    def stream(self, c):
        from test_welch_matrix_gpu import capture
        return capture(c.extra[0], _n_of(c), c.seed, c.nfft, independent_segments(c), OFFSET if c.offset else 0.0)

    def oracle(self, c, x):
        import welch_matrix_oracle as XO
        return XO.matrix(x, c.nfft, c.nperseg, c.noverlap, 'hann', c.detrend, c.scaling, FS)

    def rows_of(self, c, ref):
        import welch_matrix_oracle as XO
        return {'s': XO.shape_out(ref['S'], c.fftshift, c.trim), 'gcoh': XO.shape_out(ref['gcoh'], c.fftshift, c.trim)}

    def check(self, c, rows, ref, what=''):
        from test_welch_matrix_gpu import check_matrix
        C = c.extra[0]
        e_s, e_g = check_matrix(rows['s'], rows['gcoh'], ref, c.fftshift, c.trim)
        return {'s': e_s / RTOL, 'gcoh': e_g / (2 * C * (C - 1) * RTOL)}

    def call_dev(self, plan, c, ins, outs):
        return plan.matrix_dev(ins[0], nsamples(c), c.extra[0], stride(c), outs['s'], outs['gcoh'])

    def call_host(self, plan, c, lane):
        return dict(zip(self.row_names, plan.matrix(lane)))

    def shaped(self, c, name, a):
        from ofdm_tools import _hip
        C = c.extra[0]
        return _hip.unpack_matrix(_complex_rows(a.reshape(C * (C + 1) // 2, -1, 2)), C) if name == 's' else a


class Pfb(Sk):
    kernel, min_nseg, full_segments = 'welchpfb', 1, True
    row_names, required = ('pfb',), ('pfb',)

    def extra(self, rng, pick, nfft, nperseg, cls):
        # a frame is ntaps nfft samples: at least three frames' worth of room at the largest hop; few taps where streams count
        most = 3 if cls == 'C' else max(2, min(16, CAP // nfft - 3))
        return (int(rng.integers(2, most + 1)),)

    def narrow(self, c):
        if c.nfft <= 512:
            return with_nseg(c, 1) if c.cls == 'A' and c.nfft == 64 else c      # the family's minimum, in every seed
        # above 512 points: at least three frames' worth of new samples, (nseg - 1) step >= 2 nfft
        counts = sorted(set(segs_c(1) if c.cls == 'C' else segs(1)))
        enough = [s for s in counts if (s - 1) * step(c) >= 2 * c.nfft and nsamples(c._replace(nseg=s)) <= CAP]
        if enough:
            return with_nseg(c, min(enough, key=lambda s: (s < c.nseg, abs(s - c.nseg))))
        nseg = max(c.nseg, 3 if c.cls == 'A' else 7)
        stp = -(-2 * c.nfft // (nseg - 1))
        return with_nseg(c._replace(noverlap=c.nfft - stp, tail=c.tail % stp), nseg)

    def reach(self, c):
        return (c.extra[0] - 1) * c.nfft

    def recipe_front(self, c):
        return 'kernel=%s nfft=%d ntaps=%d ' % (self.kernel, c.nfft, c.extra[0])

    def taps(self, c):
        from test_welch_pfb_cpu import prototype
        return prototype(c.nfft, c.extra[0])

    def stream(self, c):
        from test_median_gpu import noise_tones
        return np.stack([_with_offset(c, noise_tones(_n_of(c), c.seed + s)) for s in range(c.nstreams)])

    def oracle(self, c, x):
        import welch_pfb_oracle as PO
        ref = PO.pfb(x, c.nfft, c.extra[0], self.taps(c).astype(np.float32), c.noverlap, c.detrend, c.scaling, FS)
        assert ref['M'] == c.nseg
        return ref

    def emulate(self, c, x):
        """the closer emulation: the kernel's own float32 order (welch_pfb_oracle.emulate32)"""
        import welch_pfb_oracle as PO
        return {'pfb': PO.emulate32(x[:owned(c)], c.nfft, c.extra[0], self.taps(c).astype(np.float32), c.noverlap, c.detrend, c.scaling, FS)}

    def rows_of(self, c, ref):
        return {'pfb': _st(c, ref['pfb'], c.db)}

    def check(self, c, rows, ref, what=''):
        from test_welch_pfb_gpu import check_row
        return {'pfb': check_row(rows['pfb'], ref, c.fftshift, c.trim, c.db) / RTOL}

    def plan(self, ctx, hip, c):
        plan = self.welch_plan(ctx, hip, c)
        plan.set_prototype(self.taps(c))
        return plan

    def call_dev(self, plan, c, ins, outs):
        return plan.pfb_dev(ins[0], nsamples(c), c.nstreams, stride(c), outs['pfb'])

    def call_host(self, plan, c, lane):
        return {'pfb': plan.pfb(lane)}


FAMILY = collections.OrderedDict(zip(FAMILIES, (Mtm(), MtmCsd(), Ftest(), Jack(), CsdJack(), Adapt(), Sk(), Cyc(), Caf(), Mat(), Pfb())))


# ---- one unit of a case against its oracle ------------------------------------------------------------------------------------

def reference(c, i):
    """the float64 oracle of unit i on its own samples alone (the NaN tail in place: it reads none of it)"""
    return FAMILY[c.family].oracle(c, lane_input(c, i))


def emulated_rows(c, i):
    """the rows of unit i as float32 transforms give them (section 2e): the family's closer emulation where it has one, else
    its oracle under float32_transform(); through the case's output stage"""
    F = FAMILY[c.family]
    x = lane_input(c, i)
    if hasattr(F, 'emulate'):
        plain = F.emulate(c, x)
        return {k: _st(c, v, c.db and k in ('psd', 'pfb')) for k, v in plain.items()}
    with float32_transform():
        return F.rows_of(c, F.oracle(c, x))


def compare(c, rows, ref, what=''):
    """rows: {name: array} of one unit, a row the case leaves NULL absent - the oracle's own row stands in for it, so that
    the family's comparison runs unchanged.  -> {gate: worst reading as a share of it}"""
    F = FAMILY[c.family]
    full = F.rows_of(c, ref)
    full.update(rows)
    return F.check(c, full, ref, what)


# ---- one case on the GPU (test_stat_fuzz_gpu.py, tools/stat_fuzz.py) ------------------------------------------------------------

def run_case(ctx, hip, c, check=True, say=print):
    """The _dev call of case `c` on the layout of layout(c), every output row a device block of its own: SENTINEL words, GUARD
    in front of the first row, a spare row and GUARD behind the last.  Asserts the return value, the recipe, every unit's
    rows against the float64 oracle of that unit's samples alone, the guards, the spare rows, the input read back, and for a
    class-A case the host form's bits.  check=False: the launch, the recipe and the guards only.
    -> (recipe, {gate: worst share over the units})"""
    from call_order_cases import GUARD, SENTINEL
    from stat_support import forced_env
    F = FAMILY[c.family]
    forced = F.forced(c)
    U, held = units(c), []

    def put(arr):
        p = ctx.alloc(arr.nbytes)
        held.append(p)
        ctx.h2d(p, arr)
        return p

    with forced_env(*forced[:2]) if forced and forced[0] else contextlib.nullcontext():
        plan = F.plan(ctx, hip, c)
    try:
        bufs = layout(c)
        bases = [put(buf) for buf, _ in bufs]
        ins = [base + 8 * lead for base, (_, lead) in zip(bases, bufs)]
        blocks, outs = {}, {}
        for name, present in zip(F.row_names, c.rows):
            outs[name] = None
            if present:      # (a row passed as NULL has no storage at all)
                blocks[name] = put(FL.row_block(U, F.floats(c, name)))
                outs[name] = blocks[name] + 4 * GUARD
        nseg = F.call_dev(plan, c, ins, outs)
        recipe = plan.last_recipe()
        assert nseg == c.nseg, (nseg, shape_text(c))
        assert recipe.startswith(F.recipe_front(c)) and ' nfft=%d ' % c.nfft in recipe, (recipe, shape_text(c))
        assert forced is None or forced[2] in recipe + ' ', (recipe, forced)
        rows = {}
        for name, base in blocks.items():
            w = F.floats(c, name)
            rows[name] = FL.rows_of_block(ctx.d2h(base, (2 * GUARD + (U + 1) * w,), np.uint32), U, w, name, shape_text(c))
        for base, (buf, _) in zip(bases, bufs):
            assert ctx.d2h(base, buf.shape, np.complex64).tobytes() == buf.tobytes(), 'the input buffer changed [%s]' % shape_text(c)
        worst = {}
        if check:
            for i in range(U):
                got = {name: F.shaped(c, name, rows[name][i]) for name in rows}
                for k, v in compare(c, got, reference(c, i), '%s unit %d [%s]' % (shape_text(c), i, recipe)).items():
                    worst[k] = max(worst.get(k, 0.0), v)
            if c.family == 'jack' and c.rows[1]:      # the PSD row is exec_dev's, bit for bit
                twin = put(np.full(U * out_len(c), SENTINEL, np.uint32))
                plan.exec_dev(ins[0], nsamples(c), twin, nstreams=c.nstreams, stream_stride=stride(c))
                assert ctx.d2h(twin, (U, out_len(c)), np.float32).tobytes() == rows['psd'].tobytes()
            if c.family == 'csdjack' and c.rows[1]:      # Cxy is csd_exec_dev's, bit for bit
                twin = put(np.full(out_len(c), SENTINEL, np.uint32))
                plan.csd_exec_dev(ins[0], ins[1], nsamples(c), cxy=twin)
                assert ctx.d2h(twin, (1, out_len(c)), np.float32).tobytes() == rows['cxy'].tobytes()
            if c.cls == 'A':      # the host form on the same samples: the same bits
                host = F.call_host(plan, c, lane_input(c, 0))
                for name in rows:
                    dev = F.shaped(c, name, rows[name][0])
                    want = np.asarray(host[name])
                    assert np.asarray(dev).astype(want.dtype).tobytes() == want.tobytes(), 'host form, row %s [%s]' % (name, shape_text(c))
            k = max(worst, key=worst.get)
            say('stat fuzz %s [%s]: worst %s %.3f of its gate' % (shape_text(c), recipe, k, worst[k]))
        return recipe, worst
    finally:
        for p in held:
            ctx.free(p)
        plan.close()


def walks(c, recipe):
    """the recipe shows W < items with items no multiple of W: runs of unequal length, more than one item each"""
    from stat_support import recipe_field
    W = recipe_field(recipe, 'W')
    return W < items(c) and items(c) % W != 0
