#!/usr/bin/env python3
"""One peak-hold push of the periodogram chain - 2^24 device-resident samples, the latest row only - at 1024 and 4096
points: this tree's library against another build of it (the parent commit's, before the peak hold kept NaN: v_max_u32 where
v_max_f32 stood in the transform kernels, a NaN-keeping compare in the two tail kernels), both loaded into ONE process and
alternating push by push on one stream, stat_time.py's loop: two warm-up pushes each, then `reps` timed windows per arm in
turn and the median; `rounds` such medians per arm give its run-to-run range within the session.

  python tools/degenerate_time.py --other OLD.so [reps] [--rounds N] [--out FILE]      (default: profiles/degenerate_time.txt,
                                                                                        appended to: one block per session)
"""
import ctypes as C
import sys

import stat_time
from stat_time import _hip, np

NSAMPLES = 1 << 24
SIZES = (1024, 4096)
INNER = 8


def context_of(path, stream):
    """a Context on `stream` served by the library at `path` (a second copy next to the one _hip.load() holds)"""
    lib = C.CDLL(path)
    for name, (res, args) in _hip.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    ctx = _hip.Context.__new__(_hip.Context)
    ctx.lib = lib
    h = C.c_void_p()
    rc = lib.oth_ctx_create_on_stream(0, C.c_void_p(int(stream)), C.byref(h))
    if rc != _hip.OK:
        raise _hip.HipError(rc, 'oth_ctx_create_on_stream', lib.oth_last_error(None).decode())
    ctx.h, ctx.device, ctx.stream = h, 0, int(stream)
    import threading
    ctx._plans_lock = threading.Lock()
    return ctx


def main():
    argv = sys.argv[1:]
    other, rounds = None, 5
    for flag in ('--other', '--rounds'):
        if flag in argv:
            i = argv.index(flag)
            if flag == '--other':
                other = argv[i + 1]
            else:
                rounds = int(argv[i + 1])
            del argv[i:i + 2]
    sys.argv[1:] = argv
    if not other:
        sys.exit(__doc__)
    s = stat_time.Session('degenerate_time.txt', reps=30, inner=INNER)
    from ofdm_tools import windows
    old = context_of(other, s.stream.cuda_stream)
    x = s.capture(NSAMPLES)
    s.say('peak-hold push, %d device-resident samples, latest row only (max_rows = 1), %d pushes per timed window; %s'
          % (NSAMPLES, INNER, s.library))
    s.say('"other": %s; arms alternate window by window, median of %d windows, %d rounds' % (other.split('/')[-1], s.reps, rounds))
    for nfft in SIZES:
        arms, rows = [], []
        for label, ctx in (('other', old), ('this', s.ctx)):
            ch = ctx.chain(nfft, windows.blackmanharris(nfft), False, _hip.EPI_MAG, 1)
            ch.set_peak_hold(True)
            row = ctx.alloc(4 * nfft)
            rows.append(row)
            arms.append((label, ch, lambda ch=ch, row=row: ch.push_dev(x.data_ptr(), NSAMPLES, row, 1)))
        for _, _, fn in arms:
            fn()
            fn()
        peaks = [ch.peak() for _, ch, _ in arms]
        same = np.array_equal(peaks[0].view(np.uint32), peaks[1].view(np.uint32))
        meds = {label: [] for label, _, _ in arms}
        for _ in range(rounds):
            ms = {label: [] for label, _, _ in arms}
            for _ in range(s.reps):
                for label, _, fn in arms:
                    ms[label].append(s.timed(fn))
            for label in ms:
                meds[label].append(float(np.median(ms[label])))
        s.say('')
        s.say('%d points (%d vectors per push); the two peaks are bit-identical: %s' % (nfft, NSAMPLES // nfft, same))
        for label, _, _ in arms:
            v = meds[label]
            s.say('  %-5s  medians per round, us per push: %s   range %.1f ... %.1f' % (label, ' '.join('%.1f' % (1e3 * t) for t in v),
                                                                                       1e3 * min(v), 1e3 * max(v)))
        lo, hi = min(meds['other']), max(meds['other'])
        worst = max(meds['this'])
        s.say('  this build %s the other build\'s own range (its slowest round %.1f us against %.1f ... %.1f us)'
              % ('inside or below' if worst <= hi else 'ABOVE', 1e3 * worst, 1e3 * lo, 1e3 * hi))
        for (_, ch, _), ctx, row in zip(arms, (old, s.ctx), rows):
            ch.close()
            ctx.free(row)
    old.close()
    s.ctx.close()
    with open(s.out_path, 'a') as f:
        f.write('\n'.join(s.lines) + '\n\n')


if __name__ == '__main__':
    main()
