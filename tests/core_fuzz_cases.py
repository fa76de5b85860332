"""The seeded random-shape cases of the core Welch and CSD routes (test_core_fuzz_cpu.py, test_core_fuzz_gpu.py,
tools/core_fuzz.py) - a plain module, no fixtures, no GPU: the route set, the case generator and the memory layout.  It
follows stat_fuzz_cases.py and shares its layout pieces (fuzz_layout.py).

ROUTES.  A route is (channels, forcing word, kernel= label with its :variant suffixes, form=, pilot=) of a recipe string.
witnesses() derives the set from recipes.recipe() (oth__debug_recipe_tuned; no device): every power-of-two size 64 ... 16384,
one and two channels, nperseg = nfft, nfft / 2, nfft / 4, nfft - 1 (and 256 at 4096 points), four overlaps, the window
classes of oth__debug_recipe (0, 1, 2, and 3 at 8192 / 16384 points), three detrend modes, 3 and 9 segments - and the same grid under each word of WORDS, the builds routing never picks
by itself and the parity suite forces through set_tuning.  A word's routes are the shapes at which its recipe differs from
the unforced one: at 9 segments, because any word but 'td' / 'plaunch' also forces the frequency-domain detrend below
kFdMinSegments - which is what 'fd' is for, so 'fd' counts at 3 segments only; 'wsgen' leaves the text as it is and counts
wherever the label is welch4096:ws.  The channel count is part of the key because the two-channel entry points run other
instances of the coverage kernel.  DRAWN lists the routes the generator draws, by id; test_core_fuzz_cpu.py asks that it
equals the derived set, so a route added to resolve_recipe() fails there until it is listed here.

CASES.  cases(route, seed) draws from numpy.random.default_rng((seed, index of the route in DRAWN)) three cases on shapes
taken from the route's own witnesses, each accepted only if its predicted recipe names the route (the window - Hann, flattop,
Blackman-Harris, rectangular, a symmetric Hamming, a random positive one - is drawn by name and its class MEASURED by the
library's criterion, window_class(): a symmetric Hamming is wide for the |k| < 16 table only, class 3):
  A  the plain shape (nperseg = nfft where the route has it), one stream, one launch under the contiguous schedule; nseg
     from (1, 2, 3, 7, 8, 9, 11, 19); the output stage, the scaling and nseg picked through seeded permutations of the
     route's index so that all occur; the host form must give the same bits.
  B  2 ... 5 streams (two channels: one pair), a gap of 0 / 1 / 67 / 64 k + 3 samples, leads of 1 ... 7 samples, a ragged
     tail, any overlap and nperseg < nfft where the route admits them, the library's own schedule.
  C  launches that walk runs of unequal length: for every schedule the route honours under set_tuning(sched=) one launch
     (streams, segments) with the predicted W < nseg and nseg % W != 0 at the fewest samples that do it, the stream count
     alternating between the two sides of 64 (the ticket words), the chunk drawn from (1, 2, 3, default); the first launch
     also has nseg / W > chunk - a run crosses a chunk boundary - where CAP leaves room.  The coverage kernel takes no
     schedule: one launch per side of 64.  A two-channel call takes one pair: segments alone make nseg > W.
A launch reads at most CAP = 2^22 complex samples and transforms at most WORK = 2^24 points in the oracle.

INPUT.  One-channel streams are R.synth_iq or test_median_gpu.noise_tones (drawn per case), two-channel pairs
test_csd_gpu._pair, seeded per stream.  A detrending case with the pilot (OTH_DETREND_CONSTANT) gets, in a drawn half,
the offset OFFSET (-1)^s (1 + s % 5) on stream s (x: s = 0, y: s = 1), so a pilot or mean from the wrong stream shows.
The buffer is NaN but for the samples of each stream's whole segments: gap, lead, 64 samples behind and the ragged tail
inside nsamples read NaN.  No route reads that tail: include/ofdm_tools_hip.h gives oth_welch_exec_dev the whole segments
of nsamples and nothing else to read.

GATES, imported: test_hip_parity.plan_err (the comparison of test_randomized_welch_plans_vs_oracle) under RTOL for one
channel, test_csd_gpu.errors, each of the five under RTOL, for two.  The oracles are R.welch_np and csd_oracle.csd (R's
segmentation and windows) on the float32 window the plan is given.

WHERE THE DRAW IS NARROWER, because float32 does not hold the gate (the half-gate emulation of test_core_fuzz_cpu.py, the
oracle under fuzz_layout.float32_transform, reads at most 0.38 of a gate on the suite's seed as drawn now: 16384 points,
five segments, 'fd'):
  * a rectangular window is drawn with OTH_DETREND_NONE only: under a constant detrend its bin 0 is sum(x - mean) = 0 in
    the oracle and rounding noise in any float32 transform (test_csd_gpu.test_tuned_4096_every_step_window_and_detrend);
  * OTH_DETREND_CONSTANT_FAST takes no offset: it has no pilot, and the float32 mean of a segment 175 units off zero is
    good to 1e-5 of the noise only (test_hip_parity's _f32_mean_bound);
  * one- and two-segment launches: see least_nseg() below."""
import collections
import functools
import hashlib
import zlib

import numpy as np

import fuzz_layout as FL
import median_oracle as MO
import recipes
from stat_fuzz_cases import OFFSET, RTOL
from stat_support import FS

SEED = 71                  # the suite's seed
CAP = 1 << 22              # complex samples a launch reads, over all streams or both channels
WORK = 1 << 24             # points the oracle transforms for a launch: nstreams x nseg x nfft (x 2 for a pair)
SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
WORDS = ('wsgen', 'plaunch', 'seg3', 'seg4', 'csd1', '8k1role', '16k4', '16kplain', 'td', 'fd')
WINDOWS = ('hann', 'flattop', 'blackmanharris', 'rect', 'hamming', 'random')      # (their class: window_class())
DETREND_CODE = collections.OrderedDict([('none', 0), ('constant', 1), ('fast', 3)])
SCALINGS = ('density', 'spectrum', 'raw', 'over_n2')
SCHEDS = ('contiguous', 'interleaved', 'dynamic')
CHUNKS = (1, 2, 3, 0)      # 0: the route's default
NSEGS = (1, 2, 3, 7, 8, 9, 11, 19)
CLASSES = 'ABC'
ROW_NAMES = ('pxx', 'pyy', 'pxy', 'cxy')
# LONE: the fewest segments of a launch.  A lone periodogram's deepest bins are not held by float32 at half the gate - the
# oracle under float32_transform() (pocketfft on complex64), 12 ... 40 seeds x both generators x the three cosine-sum windows,
# read of the gate: one segment 0.32 at 64 points, 0.77 at 128, 0.71 at 512, 0.75 at 4096, 0.85 at 16384; two segments 0.06 ...
# 0.18 up to 1024 points, 0.20 at 4096, 0.45 at 16384; three 0.29 at 4096 and 16384.  So one segment is drawn at 64 points only,
# two up to 1024 points, three and more above.
def least_nseg(nfft):
    return 1 if nfft == 64 else (2 if nfft <= 1024 else 3)

Route = collections.namedtuple('Route', 'two word kernel form pilot')
Witness = collections.namedtuple('Witness', 'nfft npk ovk wclass detrend few')
Shape = collections.namedtuple('Shape', 'nfft nperseg noverlap wclass detrend two word')
Launch = collections.namedtuple('Launch', 'nseg nstreams sched chunk')
Case = collections.namedtuple('Case', 'route cls nfft nperseg noverlap window detrend scaling fftshift trim db offset gap lead lead_y '
                                      'tail rows source launches seed')

# the routes the generator draws (route_id): one line each, so that a route can be struck out to see the coverage test fail
DRAWN = (
    'seg.full-none-none',
    'seg.full-time-launch',
    'seg.full-time-none',
    'seg.half-none-none',
    'seg.half-time-launch',
    'seg.half-time-none',
    'seg_padded.full-none-none',
    'seg_padded.full-time-launch',
    'seg_padded.full-time-none',
    'seg_padded.half-none-none',
    'seg_padded.half-time-launch',
    'seg_padded.half-time-none',
    'segws-freq-launch',
    'segws-freq-none',
    'segws-none-none',
    'segws-time-launch',
    'segws-time-none',
    'welch16k-freq-launch',
    'welch16k-freq-none',
    'welch16k-none-none',
    'welch16k-time-launch',
    'welch16k-time-none',
    'welch16k1x.pipe-none-none',
    'welch16k1x.plain.window-none-none',
    'welch16k1x_half-freq-inline',
    'welch16k1x_half-freq-none',
    'welch16k1x_half-none-none',
    'welch16k1x_half.ws-freq-inline',
    'welch16k1x_half.ws-freq-none',
    'welch16k1x_half.ws-none-none',
    'welch4096.dpp-none-none',
    'welch4096.dpp-time-launch',
    'welch4096.dpp-time-none',
    'welch4096.pipe-time-launch',
    'welch4096.pipe-time-none',
    'welch4096.ws-freq-inline',
    'welch4096.ws-freq-none',
    'welch4096.ws-none-none',
    'welch_generic-none-none',
    'welch_generic-time-launch',
    'welch_generic-time-none',
    'welch16k-freq-launch+16k4',
    'welch16k-freq-none+16k4',
    'welch16k-none-none+16k4',
    'welch16k-none-none+16kplain',
    'welch16k1x.plain-none-none+16kplain',
    'welch16k1x_half-freq-inline+8k1role',
    'welch16k1x_half-freq-none+8k1role',
    'welch16k1x_half-none-none+8k1role',
    'segws-freq-launch+fd',
    'segws-freq-none+fd',
    'welch16k-freq-launch+fd',
    'welch16k-freq-none+fd',
    'welch16k1x_half-freq-inline+fd',
    'welch16k1x_half-freq-none+fd',
    'welch16k1x_half.ws-freq-inline+fd',
    'welch16k1x_half.ws-freq-none+fd',
    'welch4096.ws-freq-inline+fd',
    'welch4096.ws-freq-none+fd',
    'welch16k1x_half-freq-launch+plaunch',
    'welch16k1x_half.ws-freq-launch+plaunch',
    'welch4096.ws-freq-launch+plaunch',
    'seg.half-none-none+seg3',
    'seg.half-time-launch+seg3',
    'seg.half-time-none+seg3',
    'seg.full.wps4-none-none+seg4',
    'seg.full.wps4-time-launch+seg4',
    'seg.full.wps4-time-none+seg4',
    'seg.half.wps4-none-none+seg4',
    'seg.half.wps4-time-launch+seg4',
    'seg.half.wps4-time-none+seg4',
    'seg.half-time-launch+td',
    'seg.half-time-none+td',
    'welch16k-time-launch+td',
    'welch16k-time-none+td',
    'welch4096.pipe-time-launch+td',
    'welch4096.pipe-time-none+td',
    'welch4096.ws-freq-inline+wsgen',
    'welch4096.ws-freq-none+wsgen',
    'welch4096.ws-none-none+wsgen',
    'csd-csd4096-none-none',
    'csd-csd4096-time-launch',
    'csd-csd4096-time-none',
    'csd-csd4096ws-freq-inline',
    'csd-csd4096ws-freq-none',
    'csd-csd4096ws-none-none',
    'csd-welch_generic-none-none',
    'csd-welch_generic-time-launch',
    'csd-welch_generic-time-none',
    'csd-csd4096-none-none+csd1',
    'csd-csd4096-time-launch+csd1',
    'csd-csd4096-time-none+csd1',
    'csd-csd4096ws-freq-inline+fd',
    'csd-csd4096ws-freq-none+fd',
    'csd-csd4096ws-freq-launch+plaunch',
    'csd-csd4096-time-launch+td',
    'csd-csd4096-time-none+td',
)

# Routes no launch inside CAP walks (test_core_fuzz_cpu.py asks that every other route has one); their class C is 70 streams (40 or 20
# where 70 do not fit) of as few segments as the route takes.  The one-exchange kernels for vectors that do not overlap: 256 resident workgroups of
# 16384 points (512 of 8192) are 2^22 samples with one segment each.  The two-channel 'fd' routes exist below kFdMinSegments
# only, where a pair's seven segments never outnumber the 256 workgroups.
NO_WALK = ('welch16k1x.pipe-none-none', 'welch16k1x.plain.window-none-none', 'welch16k-none-none+16kplain',
           'welch16k1x.plain-none-none+16kplain', 'csd-csd4096ws-freq-inline+fd', 'csd-csd4096ws-freq-none+fd')

# Routes whose class C crosses no chunk boundary, because the cap leaves no room for it: a run longer than a chunk is two
# segments and more for every resident workgroup, and 2 x 256 bpc x step samples are CAP or more on every shape these have
# (test_core_fuzz_cpu.py asserts the arithmetic, and that every other route's class C crosses one).
NO_CROSSING = (
    'welch16k-freq-launch', 'welch16k-freq-none', 'welch16k1x_half-freq-inline', 'welch16k1x_half-freq-none',
    'welch16k1x_half-none-none', 'welch4096.pipe-time-launch', 'welch4096.pipe-time-none', 'welch16k-freq-launch+16k4',
    'welch16k-freq-none+16k4', 'welch16k-none-none+16k4', 'welch16k1x_half-freq-inline+8k1role',
    'welch16k1x_half-freq-none+8k1role', 'welch16k1x_half-none-none+8k1role', 'welch16k-freq-launch+fd',
    'welch16k-freq-none+fd', 'welch16k1x_half-freq-inline+fd', 'welch16k1x_half-freq-none+fd',
    'welch16k1x_half-freq-launch+plaunch', 'seg.half.wps4-none-none+seg4', 'seg.half.wps4-time-launch+seg4',
    'seg.half.wps4-time-none+seg4', 'welch16k-time-launch+td', 'welch16k-time-none+td', 'welch4096.pipe-time-launch+td',
    'welch4096.pipe-time-none+td', 'csd-csd4096-none-none+csd1', 'csd-csd4096-time-launch+csd1',
    'csd-csd4096-time-none+csd1', 'csd-csd4096-time-launch+td', 'csd-csd4096-time-none+td')


# ---- routes from data -----------------------------------------------------------------------------------------------------------

def route_id(r):
    return '%s%s-%s-%s%s' % ('csd-' if r.two else '', r.kernel.replace(':', '.'), r.form, r.pilot, '+' + r.word if r.word else '')


def fields(text):
    return dict(f.split('=') for f in text.split())


def triple(text):
    f = fields(text)
    return f['kernel'], f['form'], f['pilot']


def names(text, route):
    return not text.startswith('error') and triple(text) == (route.kernel, route.form, route.pilot)


def nperseg_of(nfft, npk):
    return {'full': nfft, 'half': nfft // 2, 'quarter': nfft // 4, 'odd': nfft - 1, '256': 256}[npk]


def noverlap_of(nperseg, ovk):
    return {'none': 0, 'half': nperseg // 2, 'quarter': nperseg // 4, 'threequarter': nperseg - nperseg // 4}[ovk]


def predict(lib, sh, nseg, nstreams=1, sched=-1, chunk=0, runtime=0):
    """the recipe string of a launch of shape sh (sched / chunk: set_tuning's overrides; runtime=1 needs a device)"""
    return recipes.recipe(lib, sh.nfft, sh.nperseg, sh.noverlap, window=sh.wclass, detrend=DETREND_CODE[sh.detrend],
                          two_channel=sh.two, kernel=0, variant=sh.word or None, sched=2, nseg=nseg, nstreams=nstreams,
                          runtime=runtime, tune_sched=sched, chunk=chunk)


@functools.lru_cache(maxsize=1)
def witnesses():
    """-> {Route: [Witness]}, sorted: every route of the grid in the module's docstring with the shapes that reach it"""
    lib = recipes._lib()
    out = {}
    for nfft in SIZES:
        for two in (0, 1):
            for npk in ('full', 'half', 'quarter', 'odd') + (('256',) if nfft == 4096 else ()):
                nperseg = nperseg_of(nfft, npk)
                for ovk in ('none', 'half', 'quarter', 'threequarter'):
                    for wclass in (0, 1, 2) + ((3,) if nfft >= 8192 and npk == 'full' else ()):
                        for det in DETREND_CODE:
                            for nseg in (3, 9):
                                sh = Shape(nfft, nperseg, noverlap_of(nperseg, ovk), wclass, det, two, '')
                                base = predict(lib, sh, nseg)
                                for word in ('',) + WORDS:
                                    text = predict(lib, sh._replace(word=word), nseg) if word else base
                                    if text.startswith('error') or 'kernel=anyfft' in text:
                                        continue
                                    if word == 'wsgen':
                                        keep = fields(text)['kernel'] == 'welch4096:ws'
                                    elif word == 'fd':
                                        keep = nseg < 8 and text != base
                                    else:
                                        keep = not word or (nseg >= 8 and text != base)
                                    if keep:
                                        out.setdefault(Route(two, word, *triple(text)), []).append(Witness(nfft, npk, ovk, wclass, det, nseg < 8))
    return collections.OrderedDict(sorted(out.items()))


def routes():
    """the routes of DRAWN, in its order"""
    by_id = {route_id(r): r for r in witnesses()}
    return [by_id[i] for i in DRAWN]


# ---- what follows from a case ---------------------------------------------------------------------------------------------------

def step(c):
    return c.nperseg - c.noverlap


def tail(c):
    return c.tail % step(c)


def nsamples(c, L):
    return c.noverlap + L.nseg * step(c) + tail(c)


def owned(c, L):
    return nsamples(c, L) - tail(c)


def stride(c, L):
    return nsamples(c, L) + c.gap


def out_len(c):
    return c.nfft - 2 * c.trim


def samples_read(c, L):
    return (2 if c.route.two else 1) * L.nstreams * nsamples(c, L)


def shape_of(c):
    return Shape(c.nfft, c.nperseg, c.noverlap, window_class(window_of(c), c.nfft), c.detrend, c.route.two, c.route.word)


def window_class(w, nfft):
    """oth__debug_recipe's window_class of a plan's window, by the criterion the header and csrc/abi_welch.hip state for the
    detrend tables (they exist at nperseg = nfft = 2048 ... 16384): |FFT(w)[k]|^2 <= 1e-10 sum(w^2) outside |k| < 16 (class 1)
    or outside the 256 nfft / 4096 bins at either end (class 3; at 2048 and 4096 points: 256 bins, and the same routes as
    class 1), else 2; all ones: 0.  A symmetric Hamming is wide by the first and confined by the second."""
    w = np.asarray(w, np.float64)
    if np.all(w == 1.0):
        return 0
    if len(w) != nfft or nfft < 2048:
        return 2 if nfft >= 2048 else -1      # no table: the class takes no part in the routing (-1: any)
    p = np.abs(np.fft.fft(w)) ** 2
    bound = 1e-10 * np.sum(w * w)
    if np.all(p[16:nfft - 16] <= bound):
        return 1
    band = 256 * max(1, nfft // 4096)
    return 3 if np.all(p[band:nfft - band] <= bound) else 2


def shape_text(c, L=None):
    text = '%s %s nfft=%d nperseg=%d noverlap=%d %s %s %s%s %s%s%s' % (
        route_id(c.route), c.cls, c.nfft, c.nperseg, c.noverlap, c.window, c.detrend, c.scaling, ' +offset' if c.offset else '',
        'shift ' if c.fftshift else '', 'trim=%d ' % c.trim if c.trim else '', 'dB ' if c.db else '')
    if c.route.two:
        text += 'rows=%s ' % ''.join('1' if r else '0' for r in c.rows)
    if L is not None:
        text += '| nseg=%d streams=%d n=%d gap=%d sched=%s chunk=%d' % (L.nseg, L.nstreams, nsamples(c, L), c.gap,
                                                                        SCHEDS[L.sched] if L.sched >= 0 else 'auto', L.chunk)
    return text.rstrip()


def predicted(c, L, lib=None, runtime=0):
    return predict(lib or recipes._lib(), shape_of(c), L.nseg, L.nstreams, L.sched, L.chunk, runtime)


def walks(text, L):
    """the recipe shows W < nseg with a remainder: runs of unequal length, more than one segment each"""
    W = int(fields(text)['W'])
    return W < L.nseg and L.nseg % W != 0


def crosses(text, L):
    """... and a run longer than a chunk: it crosses a chunk boundary"""
    f = fields(text)
    return L.nseg // int(f['W']) > int(f['chunk'])


def guided_tail(text, L):
    """under tickets (sched=dynamic in the recipe) the quarter-size chunks of the tail are handed out: nbig < nseg / chunk"""
    f = fields(text)
    return f['sched'] == 'dynamic' and int(f['nbig']) < L.nseg // int(f['chunk'])


# ---- the draw -------------------------------------------------------------------------------------------------------------------

def _perm(seed, name):
    return np.random.default_rng((seed, zlib.crc32(name.encode()))).permutation(len(DRAWN))


def cases(route, seed=SEED):
    """exactly three cases, one of each class, for one route"""
    idx = DRAWN.index(route_id(route))
    rng = np.random.default_rng((seed, idx))
    return [_draw(route, cls, seed, idx, rng) for cls in CLASSES]


def all_cases(seed=SEED):
    return [c for r in routes() for c in cases(r, seed)]


def digest(seed=SEED):
    return hashlib.sha256(repr(all_cases(seed)).encode()).hexdigest()


def _admitted(route):
    """the route's witnesses inside the draw's bounds (the module's docstring): no rectangular window under a detrend"""
    return [w for w in witnesses()[route] if not (w.wclass == 0 and w.detrend != 'none')]


def _counts(lib, sh, route, nstreams, sched):
    lo = least_nseg(sh.nfft)
    return [n for n in NSEGS if n >= lo and names(predict(lib, sh, n, nstreams, sched), route)]


def _draw(route, cls, seed, idx, rng):
    lib = recipes._lib()
    W = _admitted(route)
    assert W, route
    if cls != 'A' and any(w.wclass == 3 for w in W) and rng.integers(2):
        W = [w for w in W if w.wclass == 3]      # (the one window of that class, a symmetric Hamming, is a rare draw)
    if cls == 'A':
        W = [w for w in W if w.npk == 'full'] or W
    elif cls == 'B':
        W = [w for w in W if w.npk != 'full'] or W
    gap = int(rng.choice([0, 1, 67, 64 * int(rng.integers(1, 5)) + 3]))
    lead, lead_y = (int(v) for v in rng.integers(1, 8, size=2))
    data_seed = int(rng.integers(1 << 30))
    source = str(rng.choice(['synth', 'noise']))
    rows, lone_row = tuple(bool(v) for v in rng.integers(2, size=4)), int(rng.integers(4))      # the NULL pattern of a pair's rows
    if not any(rows):
        rows = tuple(k == lone_row for k in range(4))
    if not route.two:
        rows = (True,)
    fallback = []
    for _ in range(400):
        w = W[int(rng.integers(len(W)))]
        nfft = w.nfft
        nperseg = nperseg_of(nfft, w.npk)
        if cls == 'B' and w.npk == 'odd':
            nperseg = int(rng.integers(max(8, nfft // 8), nfft))
        if cls == 'B' and w.npk == '256':
            nperseg = int(rng.choice([256, 512, 1024, 2048]))
        noverlap = noverlap_of(nperseg, w.ovk)
        if cls == 'B' and rng.integers(2):
            noverlap = int(rng.integers(1, nperseg))
        window = str(rng.choice(WINDOWS))
        if window == 'rect' and w.detrend != 'none':
            continue
        seen = window_class(_window(window, nperseg, data_seed), nfft)
        if seen >= 0 and seen != w.wclass and not (nfft <= 4096 and {seen, w.wclass} == {1, 3}):
            continue
        if seen < 0 and (window == 'rect') != (w.wclass == 0):
            continue
        sh = Shape(nfft, nperseg, noverlap, seen if seen >= 0 else w.wclass, w.detrend, route.two, route.word)
        stp = nperseg - noverlap
        # the output stage, scaling, offset
        if cls == 'A':
            stage = int(_perm(seed, 'stage')[idx]) % 8
            fftshift, trimmed, db = bool(stage & 1), bool(stage & 2), bool(stage & 4)
            scaling = SCALINGS[int(_perm(seed, 'scaling')[idx]) % 4]
        else:
            fftshift, trimmed, db = (bool(v) for v in rng.integers(2, size=3))
            scaling = str(rng.choice(SCALINGS))
        trim = int(rng.integers(1, nfft // 2)) if trimmed else 0
        db = db and not route.two                                    # every oth_csd_* call refuses dB
        offset = w.detrend == 'constant' and bool(rng.integers(2))
        tail_ = int(rng.integers(0, 1 << 20))
        if cls == 'A':
            ok = _counts(lib, sh, route, 1, 0)
            if not ok:
                continue
            launches = (Launch(ok[int(_perm(seed, 'nseg')[idx]) % len(ok)], 1, 0, 0),)
        elif cls == 'B':
            ns = 1 if route.two else int(rng.integers(2, 6))
            ok = [n for n in _counts(lib, sh, route, ns, -1) if (2 if route.two else 1) * ns * (noverlap + (n + 1) * stp) <= CAP]
            if not ok:
                continue
            launches = (Launch(int(rng.choice(ok)), ns, -1, 0),)
        else:
            launches = _walking(lib, sh, route, w, rng)
            if not launches and route_id(route) in NO_WALK:      # as many streams as fit, then
                for ns in ((1,) if route.two else (70, 40, 20)):
                    ok = [n for n in _counts(lib, sh, route, ns, -1) if (2 if route.two else 1) * ns * (noverlap + (n + 1) * stp) <= CAP]
                    if ok:
                        launches = (Launch(ok[0], ns, -1, 0),)
                        break
            if not launches:
                continue
            if route_id(route) not in NO_WALK and not any(crosses(predict(lib, sh, L.nseg, L.nstreams, L.sched, L.chunk), L) for L in launches):
                # no run of this shape crosses a chunk boundary under the cap: kept, should none of the next shapes do better
                fallback.append(Case(route, cls, nfft, nperseg, noverlap, window, w.detrend, scaling, fftshift, trim, db, offset, gap,
                                     lead, lead_y, tail_, rows, source, launches, data_seed))
                if len(fallback) < 10:
                    continue
                return fallback[0]
        return Case(route, cls, nfft, nperseg, noverlap, window, w.detrend, scaling, fftshift, trim, db, offset, gap, lead, lead_y,
                    tail_, rows, source, launches, data_seed)
    if fallback:
        return fallback[0]
    raise AssertionError('no %s case found for %s' % (cls, route_id(route)))


def honoured(lib, sh, route, nseg, nstreams):
    """the schedules set_tuning(sched=) gets from this route: the recipe names the schedule and still names the route"""
    out = []
    for s in (0, 1, 2):
        text = predict(lib, sh, nseg, nstreams, s)
        if names(text, route) and fields(text)['sched'] == SCHEDS[s]:
            out.append(s)
    return out


def schedules(lib, sh, route):
    """... of a shape, at nine segments or at three (a route below kFdMinSegments); the coverage kernel takes none"""
    if route.kernel == 'welch_generic':
        return []
    for probe in (9, 3):
        got = honoured(lib, sh, route, probe, 1 if sh.two else 2)
        if got:
            return got
    return []


def _find(lib, sh, route, w, sched, chunk, side, cross, rng, every=False):
    """the launch of the fewest samples that walks under (sched, chunk) with its stream count on `side` of 64 -> Launch or
    None (every=True: over every stream count of that side, not a drawn handful - the test of what the cap leaves room for)"""
    few_only = all(v.few for v in witnesses()[route])
    many_only = not any(v.few for v in witnesses()[route])
    stp = sh.nperseg - sh.noverlap
    per = 2 if sh.two else 1
    if sh.two:
        options = [1]
    elif every:
        options = list(range(2, 65)) if side == 0 else list(range(65, 513))
    elif side == 0:
        options = sorted({int(v) for v in rng.integers(2, 65, size=5)} | {64})
    else:
        options = sorted({int(v) for v in rng.integers(65, 513, size=5)} | {65})
    best = None
    for ns in options:
        most = min((CAP // (per * ns) - sh.noverlap) // stp - 1, WORK // (per * ns * sh.nfft), 7 if few_only else 1 << 30)
        if most < 2:
            continue
        f = fields(predict(lib, sh, most, ns, sched, chunk))
        W0, ce = int(f['W']), int(f['chunk'])
        lo = max(W0 + 1, (ce + 1) * W0 if cross else 0, 8 if many_only else 1, least_nseg(sh.nfft))
        for nseg in range(lo, min(most, lo + 12) + 1):
            text = predict(lib, sh, nseg, ns, sched, chunk)
            L = Launch(nseg, ns, sched, chunk)
            if not names(text, route) or not walks(text, L) or (cross and not crosses(text, L)):
                continue
            got = fields(text)['sched']
            if sched >= 0 and got != SCHEDS[sched] and not (sched == 2 and ns > 64 and got == 'interleaved'):
                continue
            if got == 'dynamic' and not guided_tail(text, L):
                continue
            cost = ns * (sh.noverlap + nseg * stp)
            if best is None or cost < best[0]:
                best = (cost, L)
            break
    return best[1] if best else None


def _walking(lib, sh, route, w, rng):
    """the launches of a class-C case on shape sh, or () where none walks inside CAP"""
    scheds = schedules(lib, sh, route)
    plan = [(s, k) for k, s in enumerate(scheds)] or [(-1, 0)] + ([] if sh.two else [(-1, 1)])
    flip = int(rng.integers(2))
    out = []
    for sched, k in plan:
        drawn = [int(rng.choice(CHUNKS[:3])), int(rng.choice(CHUNKS))]      # (drawn whether used or not: the stream of draws is fixed)
        tries = [(False, drawn[1]), (False, 1)]
        if not out:
            tries = [(True, drawn[0]), (True, 1)] + tries
        found = None
        for cross, chunk in tries:
            for side in ((k + flip) % 2, (k + flip + 1) % 2):
                found = found or _find(lib, sh, route, w, sched, chunk if sched >= 0 else 0, side, cross, rng)
        if found:
            out.append(found)
    return tuple(out)


# ---- the domain, restated from include/ofdm_tools_hip.h --------------------------------------------------------------------------

def check_domain(c):
    assert c.nfft in SIZES and 1 <= c.nperseg <= c.nfft and 0 <= c.noverlap < c.nperseg
    assert 0 <= c.trim and 2 * c.trim < c.nfft
    assert c.scaling in SCALINGS and c.detrend in DETREND_CODE and c.window in WINDOWS
    assert not (c.route.two and c.db)                                          # oth_csd_*: dB refused
    assert 1 <= c.lead <= 7 and 1 <= c.lead_y <= 7 and len(c.launches) >= 1
    assert len(c.rows) == (4 if c.route.two else 1) and any(c.rows)
    assert not (c.window == 'rect' and c.detrend != 'none') and not (c.offset and c.detrend != 'constant')
    for L in c.launches:
        n = nsamples(c, L)
        assert n >= c.nperseg and stride(c, L) >= n                            # stream_stride >= nsamples >= nperseg
        assert (n - c.noverlap) // step(c) == L.nseg and 0 <= tail(c) < step(c)
        assert 1 <= L.nstreams <= 65535 and (L.nstreams == 1 or not c.route.two)
        assert samples_read(c, L) <= CAP, shape_text(c, L)                     # the cap
        assert (2 if c.route.two else 1) * L.nstreams * L.nseg * c.nfft <= WORK or c.cls != 'C', shape_text(c, L)
        assert -1 <= L.sched <= 2 and L.chunk in CHUNKS
        assert L.nseg >= least_nseg(c.nfft)


# ---- the input and its layout -----------------------------------------------------------------------------------------------------

def window_of(c):
    """the plan's window: float32 [nperseg] (the oracle takes the same values)"""
    return _window(c.window, c.nperseg, c.seed)


@functools.lru_cache(maxsize=8)
def _window(name, nperseg, seed):
    from ofdm_tools import windows
    if name == 'rect':
        w = np.ones(nperseg)
    elif name == 'hamming':
        w = np.hamming(nperseg)                                                # symmetric: no table below |k| < 16
    elif name == 'random':
        w = 0.2 + np.random.default_rng(seed + 7).random(nperseg)
    else:
        w = windows.get_window(name, nperseg)
    w = np.ascontiguousarray(w, np.float32)
    w.setflags(write=False)
    return w


def stream_offset(c, s, same=False):
    """the offset of stream s (two channels: x is s = 0, y is s = 1).  same=True: every stream gets stream 0's - the rule
    broken, for the layout's mutation check"""
    s = 0 if same else s
    return OFFSET * (-1) ** s * (1 + s % 5) if c.offset else 0.0


def lane_data(c, li=0, same_offset=False):
    """the finite samples of launch li: complex64 [nstreams][nsamples], or for a pair (x, y) each [1][nsamples]"""
    return _lane_data(c, li, same_offset)


@functools.lru_cache(maxsize=6)
def _lane_data(c, li, same_offset):
    from oracle import ref_cpu as R
    from test_csd_gpu import _pair
    from test_median_gpu import noise_tones
    L = c.launches[li]
    n = nsamples(c, L)
    if c.route.two:
        x, y = _pair(n, c.seed + li)
        data = tuple((np.asarray(v) + np.complex64(stream_offset(c, s, same_offset))).astype(np.complex64)[None, :] for s, v in enumerate((x, y)))
    else:
        gen = (lambda s: R.synth_iq(n, c.seed + 1000 * li + s)) if c.source == 'synth' else (lambda s: noise_tones(n, c.seed + 1000 * li + s))
        data = np.stack([(gen(s) + np.complex64(stream_offset(c, s, same_offset))).astype(np.complex64) for s in range(L.nstreams)])
    for a in (data if isinstance(data, tuple) else (data,)):
        assert a.dtype == np.complex64 and a.shape[1] == n and np.all(np.isfinite(a.view(np.float32)))
        a.setflags(write=False)
    return data


def layout(c, li=0):
    """-> [(buffer, lead)]: one NaN-filled complex64 buffer per input pointer of the call (x, and y for a pair) with the
    oracle's samples in place; the call's pointer is `lead` samples in."""
    L = c.launches[li]
    data = lane_data(c, li)
    pairs = list(zip(data, (c.lead, c.lead_y))) if isinstance(data, tuple) else [(data, c.lead)]
    return [(FL.nan_buffer(d, lead, stride(c, L), nsamples(c, L), owned(c, L)), lead) for d, lead in pairs]


def lane_input(c, li, i, data=None):
    """what the oracle of stream i takes: the lane with its NaN tail (a pair: (x, y))"""
    data = lane_data(c, li) if data is None else data
    own = owned(c, c.launches[li])
    if isinstance(data, tuple):
        return tuple(FL.nan_tail(d[0], own) for d in data)
    return FL.nan_tail(data[i], own)


def units(c, L):
    return 1 if c.route.two else L.nstreams


# ---- one stream against its oracle -------------------------------------------------------------------------------------------------

def reference(c, x):
    """the float64 oracle of one stream's (pair's) samples, linear, through the case's fftshift and trim:
    one channel -> [out_len]; two -> [pxx, pyy, pxy, cxy]"""
    from oracle import ref_cpu as R
    win = window_of(c).astype(np.float64)
    det = 'constant' if c.detrend != 'none' else False
    if c.route.two:
        import csd_oracle as O
        return [O.shift_trim(v, c.fftshift, c.trim) for v in O.csd(x[0], x[1], FS, win, c.nperseg, c.noverlap, c.nfft, det, c.scaling)]
    _, p = R.welch_np(x, fs=FS, window=win, nperseg=c.nperseg, noverlap=c.noverlap, nfft=c.nfft, detrend=det,
                      scaling=c.scaling if c.scaling in ('density', 'spectrum') else 'raw')
    if c.scaling == 'over_n2':
        p = p / float(c.nfft) ** 2
    return MO.shift_trim_db(p, c.fftshift, c.trim, False)


def emulated(c, x):
    """the same with a single-precision transform, as rows a device would have left (dB applied where the case has it)"""
    with FL.float32_transform():
        ref = reference(c, x)
    return ref if c.route.two else (10.0 * np.log10(ref) if c.db else ref)


def compare(c, got, ref, what=''):
    """got: one channel the device row (dB or linear as the case has it); two: [pxx, pyy, pxy, cxy] with None for a row the
    case leaves NULL - the oracle's own row stands in.  Asserts the project's gates -> {gate: reading as a share of it}"""
    if c.route.two:
        from test_csd_gpu import errors
        full = [r if g is None else np.asarray(g) for g, r in zip(got, ref)]
        assert all(g.shape == r.shape for g, r in zip(full, ref)), what
        e = errors(full, ref)
        assert max(e) < RTOL, (what, e)                                        # (a NaN fails: NaN < RTOL is False)
        assert all(np.all(np.isfinite(g)) for g in full), what
        return dict(zip(('pxx', 'pyy', 'pxy', 'impxy', 'cxy'), (v / RTOL for v in e)))
    from test_hip_parity import plan_err
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, what
    err = plan_err(10.0 ** (got / 10.0) if c.db else got, ref)
    assert err < RTOL, (what, err)
    return {'psd': err / RTOL}


# ---- one case on the GPU (test_core_fuzz_gpu.py, tools/core_fuzz.py) ----------------------------------------------------------------

def make_plan(ctx, hip, c):
    from test_median_gpu import SCALINGS as CODES
    code = {'none': hip.DETREND_NONE, 'constant': hip.DETREND_CONSTANT, 'fast': hip.DETREND_CONSTANT_FAST}[c.detrend]
    return ctx.welch_plan(c.nfft, nperseg=c.nperseg, noverlap=c.noverlap, window=window_of(c), detrend=code, scaling=CODES[c.scaling],
                          fs=FS, fftshift=c.fftshift, trim_bins=c.trim, db=c.db)


def run_case(ctx, hip, c, check=True, say=print):
    """Every launch of case `c` through exec_dev / csd_exec_dev on the layout of layout(c, li), every output row a device
    block of its own (fuzz_layout.row_block).  Asserts the return value, last_recipe() equal to the predicted string (the
    resident workgroups from the device's occupancy calculator), every stream's row against the float64 oracle of that
    stream's samples alone, guards and spare rows, no sentinel left in a written row, the input read back byte for byte,
    and for a class-A case the host form's bits.  check=False: the launch, the recipe and the guards only.
    -> [(recipe, {gate: worst share over the streams})] per launch"""
    from call_order_cases import GUARD
    lib = hip.load()
    plan = make_plan(ctx, hip, c)
    held, out = [], []

    def put(arr):
        p = ctx.alloc(arr.nbytes)
        held.append(p)
        ctx.h2d(p, arr)
        return p

    try:
        for li, L in enumerate(c.launches):
            text = shape_text(c, L)
            plan.set_tuning(c.route.word or None, sched=L.sched, chunk=L.chunk)
            bufs = layout(c, li)
            bases = [put(buf) for buf, _ in bufs]
            ins = [base + 8 * lead for base, (_, lead) in zip(bases, bufs)]
            U, n = units(c, L), nsamples(c, L)
            widths = dict(zip(ROW_NAMES, (out_len(c), out_len(c), 2 * out_len(c), out_len(c)))) if c.route.two else {'psd': out_len(c)}
            blocks = {name: put(FL.row_block(U, widths[name])) for name, present in zip(widths, c.rows) if present}
            ptrs = {name: blocks[name] + 4 * GUARD for name in blocks}      # (a row passed as NULL has no storage at all)
            if c.route.two:
                nseg = plan.csd_exec_dev(ins[0], ins[1], n, **{k: ptrs.get(k, 0) for k in ROW_NAMES})
            else:
                nseg = plan.exec_dev(ins[0], n, ptrs['psd'], nstreams=L.nstreams, stream_stride=stride(c, L))
            recipe = plan.last_recipe()
            assert nseg == L.nseg, (nseg, text)
            want = predicted(c, L, lib, runtime=1)
            assert recipe == want and names(recipe, c.route), (recipe, want, text)
            rows = {}
            for name, base in blocks.items():
                w = widths[name]
                rows[name] = FL.rows_of_block(ctx.d2h(base, (2 * GUARD + (U + 1) * w,), np.uint32), U, w, name, text)
            for base, (buf, _) in zip(bases, bufs):
                assert ctx.d2h(base, buf.shape, np.complex64).tobytes() == buf.tobytes(), 'the input buffer changed [%s]' % text
            worst = {}
            if check:
                for i in range(U):
                    ref = reference(c, lane_input(c, li, i))
                    got = [_shaped(name, rows[name][0]) if name in rows else None for name in ROW_NAMES] if c.route.two else rows['psd'][i]
                    for k, v in compare(c, got, ref, '%s stream %d [%s]' % (text, i, recipe)).items():
                        worst[k] = max(worst.get(k, 0.0), v)
                if c.cls == 'A':      # the host form on the same samples: the same bits (a static schedule)
                    x = lane_input(c, li, 0)
                    if c.route.two:
                        host = dict(zip(ROW_NAMES, plan.csd(x[0], x[1])))
                    else:
                        host = {'psd': plan.exec(x)}
                    for name in rows:
                        dev = _shaped(name, rows[name][0])
                        assert np.asarray(dev).astype(host[name].dtype).tobytes() == host[name].tobytes(), 'host form, row %s [%s]' % (name, text)
                k = max(worst, key=worst.get)
                say('core fuzz %s [%s]: worst %s %.3f of its gate' % (text, recipe, k, worst[k]))
            out.append((recipe, worst))
            for p in held:
                ctx.free(p)
            del held[:]
        return out
    finally:
        for p in held:
            ctx.free(p)
        plan.close()


def _shaped(name, a):
    return (a.reshape(-1, 2)[:, 0] + 1j * a.reshape(-1, 2)[:, 1]).astype(np.complex64) if name == 'pxy' else a
