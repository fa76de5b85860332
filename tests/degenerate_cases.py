"""What test_degenerate_cpu.py and test_degenerate_gpu.py share (test infrastructure, no GPU): the route table of the
one-channel Welch average, its inputs - nine segments of R.synth_iq and a third of a step, one bad sample, a constant, gains
that are powers of two - the float64 references, and the classification of bins under a gain that makes float32 |X|^2
overflow.  Everything here is float64 NumPy on the oracle's own segmentation; the CPU file pins what the GPU file assumes
of it."""
import functools

import numpy as np

import median_oracle as M
import mtm_oracle as MO
from oracle import ref_cpu as R

NSEG = 9
SEED = 5
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)      # smallest normal
BAD = {'nan': float('nan'), '+inf': float('inf'), '-inf': float('-inf')}
DETRENDS = ('constant', 'fast', 'none')
ALL = DETRENDS
CONSTANT = 3 - 2j              # sums of up to 2^22 such samples are exact in float32
ULP4 = 4.0 * 2.0 ** -23        # the project's criterion: 4 ulp of the row's peak amplitude (check_single_rows)

# name: nfft, then what differs from {nperseg = nfft, 50 % overlap, Hann, OTH_KERNEL_AUTO, no tuning variant, every detrend
# mode}; `recipe`: how last_recipe() starts on finite input, `family`: the kernel family the overflow case takes one route of
ROUTES = {
    'generic-256': dict(nfft=256, kernel='generic', recipe='kernel=welch_generic ', family='generic'),
    'seg-512': dict(nfft=512, noverlap=100, recipe='kernel=seg:full '),
    # (one row more than the issue's table: the overflow case of the seg family - at 512 points and this step the gain lands
    # where a third of the noise bins may read either way, 169 of 512 against a cap of 2 %; 256 points: 4)
    'seg-256': dict(nfft=256, recipe='kernel=seg:half ', family='seg'),
    'segws-1024': dict(nfft=1024, recipe='kernel=segws ', family='segws'),
    'segpad-1024': dict(nfft=1024, nperseg=256, recipe='kernel=seg_padded:half '),
    'w4096-ws': dict(nfft=4096, kernel='tuned', tuning='ws', recipe='kernel=welch4096:ws ', family='w4096'),
    'w4096-pipe': dict(nfft=4096, kernel='tuned', tuning='pipe', recipe='kernel=welch4096:pipe '),
    'w4096-dpp': dict(nfft=4096, kernel='tuned', tuning='dpp', recipe='kernel=welch4096:dpp '),
    'w4096-step': dict(nfft=4096, kernel='tuned', noverlap=1000, recipe='kernel=welch4096:dpp '),
    'w16k-8192-step': dict(nfft=8192, noverlap=1000, recipe='kernel=welch16k ', family='w16k'),
    'w8192-split': dict(nfft=8192, recipe='kernel=welch16k1x_half:ws '),
    'w16384-half': dict(nfft=16384, recipe='kernel=welch16k1x_half ', family='w16k1x'),
    'w16384-x1': dict(nfft=16384, window='boxcar', noverlap=0, detrends=('none',), recipe='kernel=welch16k1x:'),
    'any-1000': dict(nfft=1000, recipe='kernel=anyfft:direct ', family='any-direct'),
    'any-1021': dict(nfft=1021, recipe='kernel=anyfft:bluestein ', family='any-bluestein'),
    'any-10007': dict(nfft=10007, recipe='kernel=anyfft:bluestein2 '),
    'any-32768-onewg': dict(nfft=32768, recipe='kernel=anyfft:onewg ', family='w32k'),
    'any-32768-r16': dict(nfft=32768, tuning='r16', recipe='kernel=anyfft:twolevel:r16 ', family='twolevel'),
    'any-32768-cov': dict(nfft=32768, tuning='anycov', recipe='kernel=anyfft:twolevel '),
    'mtm-1024': dict(nfft=1024, noverlap=0, mtm=4, recipe='kernel=mtm nfft=1024 ntapers=4 ', family='mtm'),
}
OVERFLOW_ROUTES = sorted(k for k, v in ROUTES.items() if 'family' in v)


def shape(route):
    """-> the route's entry with the defaults filled in"""
    r = dict(nperseg=None, noverlap=None, window='hann', kernel='auto', tuning=None, detrends=ALL, mtm=0)
    r.update(ROUTES[route])
    r['nperseg'] = r['nfft'] if r['nperseg'] is None else r['nperseg']
    r['noverlap'] = r['nperseg'] // 2 if r['noverlap'] is None else r['noverlap']
    r['step'] = r['nperseg'] - r['noverlap']
    r['nsamples'] = r['noverlap'] + NSEG * r['step'] + r['step'] // 3
    return r


@functools.lru_cache(maxsize=None)
def _stream(n, seed):
    x = R.synth_iq(n, seed)
    x.setflags(write=False)
    return x


def stream(route, seed=SEED):
    """nine segments of the route's shape and a third of a step (read-only; copy before poisoning)"""
    return _stream(shape(route)['nsamples'], seed)


def poisoned(x, pos, value, part='re'):
    """a copy of x with `value` in the real or imaginary part of sample pos"""
    v = np.array(x, np.complex64)
    f = v.view(np.float32)
    f[2 * pos + (1 if part == 'im' else 0)] = np.float32(value)
    return v


def positions(n):
    """the issue's two: the middle of the stream plus one, and sample 0 (where the in-launch pilot of the role-split
    4096-point kernel probes)"""
    return (n // 2 + 1, 0)


def segments_holding(route, pos):
    """indices of the segments that contain sample pos"""
    r = shape(route)
    return [s for s in range(NSEG) if s * r['step'] <= pos < s * r['step'] + r['nperseg']]


def reference(route, x, detrend='constant'):
    """float64 PSD of the route's plan (density, fs = 1, natural bin order)"""
    r = shape(route)
    det = False if detrend == 'none' else 'constant'
    if r['mtm']:
        return MO.mtm_psd(x, r['nfft'], r['nperseg'], r['noverlap'], 4.0, r['mtm'], detrend=bool(det))
    return R.welch_np(x, window=r['window'], nperseg=r['nperseg'], noverlap=r['noverlap'], nfft=r['nfft'], detrend=det)[1]


@functools.lru_cache(maxsize=None)
def clean_reference(route, detrend='constant', seed=SEED):
    ref = reference(route, stream(route, seed), detrend)
    ref.setflags(write=False)
    return ref


def segment_powers(route, x, detrend='constant'):
    """float64 |X_s[k]|^2 [nseg, nfft] of the windowed, detrended transforms, unscaled; a multitaper route: the segment's
    largest taper"""
    r = shape(route)
    det = False if detrend == 'none' else 'constant'
    if r['mtm']:
        tapers, _ = MO.tapers_and_weights(r['nperseg'], 4.0, r['mtm'])
        return np.max([M.welch_rows(x, 1.0, v, r['nperseg'], r['noverlap'], r['nfft'], det, 'raw') for v in tapers], axis=0)
    return M.welch_rows(x, 1.0, r['window'], r['nperseg'], r['noverlap'], r['nfft'], det, 'raw')


@functools.lru_cache(maxsize=None)
def overflow_case(route, detrend='constant'):
    """The gain 2^g under which only the squaring overflows, and what each bin must then read.
    g: the largest integer with max_s,k |X_s[k]|^2 4^g < 2^134 (amplitudes stay below 2^67).  Per bin, from the float64
    values: must_nan - some single segment has |X_s[k]|^2 4^g > 2 FLT_MAX, so a float32 square has overflowed whatever the
    rounding; must_right - sum_s |X_s[k]|^2 4^g < FLT_MAX / 2, so no float32 sum can have; the rest may read either.
    -> (g, must_nan, must_right, either) with boolean [nfft] masks"""
    p = segment_powers(route, stream(route), detrend)
    g = int(np.floor((134.0 - np.log2(p.max())) / 2.0))
    while p.max() * 4.0 ** g >= 2.0 ** 134:
        g -= 1
    while p.max() * 4.0 ** (g + 1) < 2.0 ** 134:
        g += 1
    scaled = p * 4.0 ** g
    must_nan = (scaled > 2.0 * FLT_MAX).any(axis=0)
    must_right = scaled.sum(axis=0) < FLT_MAX / 2.0
    return g, must_nan, must_right, ~(must_nan | must_right)


def gained(x, g):
    """x 2^g in complex64 (exact: a power of two, inside the normal range for the gains used here)"""
    return (np.asarray(x, np.complex64) * np.float32(2.0 ** g)).astype(np.complex64)


def constant_fast_bound(route):
    """CONSTANT_FAST on a constant input: (4 ulp)^2 of the power the undetrended line has in bin 0 - |c sum(w)|^2 times the
    density scale 1 / sum(w^2); a multitaper route: of its strongest taper's line, over that taper's own scale"""
    r = shape(route)
    if r['mtm']:
        tapers, _ = MO.tapers_and_weights(r['nperseg'], 4.0, r['mtm'])
        line = max(abs(CONSTANT * v.sum()) ** 2 / np.sum(v * v) for v in tapers)
    else:
        w = R.get_window(r['window'], r['nperseg'])
        line = abs(CONSTANT * w.sum()) ** 2 / np.sum(w * w)
    return ULP4 ** 2 * line


# ---- the chain ----------------------------------------------------------------------------------------------------------------
CHAIN_VECTORS = 12
CHAIN_BAD_VECTOR = 5
# (16384 points is one size more than the issue lists: chain16k1x_kernel holds two of the peak-hold sites)
CHAIN_SIZES = ((64, 'auto'), (256, 'auto'), (1024, 'auto'), (4096, 'auto'), (8192, 'auto'), (16384, 'auto'), (1000, 'auto'),
               (1024, 'generic'))
CHAIN_FORMS = ('sensor', 'peak', 'iir')      # EPI_MAG2_OVER_N2 rectangular | EPI_MAG Blackman-Harris, peak hold | EPI_MAG2, IIR + log
IIR_ALPHA = 0.25


def chain_stream(nfft, nvec=CHAIN_VECTORS, seed=SEED):
    return _stream(nfft * nvec, seed + nfft)


def chain_cuts(nfft, nvec=CHAIN_VECTORS):
    """two pushes that split inside vector 7 (12 vectors), so that leftover samples and the state cross a push; longer
    streams: inside the vector behind the middle"""
    v = 7 if nvec == CHAIN_VECTORS else nvec // 2 + 2
    return (0, v * nfft + nfft // 3, nvec * nfft)


def chain_reference(form, x, nfft, decim=1):
    """-> (raw rows, state rows): per kept vector the raw row the chain hands back (the dB row for 'iir') and the state after
    it (running peak / linear IIR memory; None for 'sensor'), float64, in the chain's own bin order"""
    if form == 'sensor':
        return R.chain_sensor_v2(x, nfft, decim), None
    if form == 'peak':
        return R.chain_psd_logger(x, nfft, decim)
    lin, db = R.chain_local_worker(x, nfft, 1.0, IIR_ALPHA, decim)
    return db, lin
