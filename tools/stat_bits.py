#!/usr/bin/env python3
"""Do two builds of the library give the same bits for the per-bin statistics?  The check behind a change to their host
sides or finalize kernels that must not move an operation: these launches are deterministic by construction (contiguous
runs per workgroup, fixed-order double sums), so every output row and every last_recipe string is compared byte for byte -
there is no tolerance.

  python tools/stat_bits.py OLD.so NEW.so [--out profiles/FILE.txt] [--timeout SECONDS] [--old-label TEXT] [--new-label TEXT]

runs the same cases in a fresh child process per library (OFDM_TOOLS_HIP_LIB), one after the other, each under its own
`timeout`; it stops at the first child that fails.  Exit status 1 if a row differs.  The summary names the two libraries by
their paths, or by the labels given.

Cases: the six families (F-test, spectral kurtosis, jackknife, two-channel jackknife, adaptive, cyclic with 1, 3 and 5
cycle frequencies), host and _dev forms, 64 / 4096 / 16384 points, 2 / 11 / 19 segments (11 and 19: the finalize slice
loop runs more than once, W not a multiple of 8), fftshift, trim 0 / 3 and dB on and off, 1 and 3 streams, each optional
row present and NULL; the spectral kurtosis of silence and of a constant under detrend; the F-test of a pure tone."""
import ctypes as C
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, SEGMENTS, K = (64, 4096, 16384), (2, 11, 19), 3
OUT_STAGES = list(itertools.product((0, 1), (0, 3), (0, 1)))      # fftshift, trim, db
# family -> (plan, entry point, rows in ABI order as multiples of out_len, index of the row every call needs)
FAMILIES = {
    'ftest': ('mtm', 'oth_mtm_ftest', (1, 1, 1), 0), 'sk': ('welch', 'oth_welch_sk', (1, 1), 0),
    'jack': ('mtm', 'oth_mtm_jackknife', (1, 1), 0), 'csdjack': ('mtmcsd', 'oth_mtm_csd_jackknife', (1, 1, 1, 1), 1),
    'adapt': ('mtm', 'oth_mtm_adaptive', (1, 1), 0), 'cyc1': ('welch', 'oth_welch_cyclic', (2, 1, 1), 1),
    'cyc3': ('welch', 'oth_welch_cyclic', (6, 3, 1), 1), 'cyc5': ('welch', 'oth_welch_cyclic', (10, 5, 1), 1),
}


def noise(n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal(n) + 1j * g.standard_normal(n)
    return (x + 0.5 * np.exp(2j * np.pi * 0.123 * np.arange(n))).astype(np.complex64)


def make_plan(ctx, fam, n, stage, tapers):
    from ofdm_tools import windows
    kind = FAMILIES[fam][0]
    kw = dict(fftshift=bool(stage[0]), trim_bins=stage[1], db=bool(stage[2]))
    if kind == 'welch':
        p = ctx.welch_plan(n, noverlap=0, window=windows.get_window('hann', n), **kw)
        if fam.startswith('cyc'):
            p.set_cycles([0.25, -0.0625, 0.001, 0.5, -0.3][:int(fam[3:])])
        return p
    p = (ctx.mtm_csd_plan if kind == 'mtmcsd' else ctx.mtm_plan)(n, tapers=tapers[n][0], **kw)
    p.set_ratios(np.clip(tapers[n][1], np.finfo(np.float64).tiny, 1.0))
    return p


def run(ctx, plan, fam, dev, x, y, ns, keep):
    """One call, host form or (dev) device form on ns streams; keep: the optional rows wanted.  -> the rows' bytes (b'' for
    a row left out) + the recipe"""
    _, entry, units, need = FAMILIES[fam]
    nsamp = len(x) // ns
    lens = [u * plan.out_len for u in units]
    want = [r == need or r in keep for r in range(len(units))]
    nseg = C.c_uint64()
    if dev:
        src = [ctx.alloc(v.nbytes) for v in ((x, y) if y is not None else (x,))]
        for d, v in zip(src, (x, y)):
            ctx.h2d(d, v)
        out = [ctx.alloc(4 * ns * n) if w else None for n, w in zip(lens, want)]
        args = [C.c_void_p(d) for d in src] + [nsamp] + ([ns, nsamp] if y is None else []) + ([4] if fam == 'adapt' else [])
        args += [C.c_void_p(o) if o else None for o in out]
        ctx.check(getattr(ctx.lib, entry + '_dev')(plan.h, *args, C.byref(nseg)), entry + '_dev')
        ctx.sync()
        rows = [ctx.d2h(o, (ns, n), np.float32).tobytes() if o else b'' for o, n in zip(out, lens)]
        for d in src + [o for o in out if o]:
            ctx.free(d)
    else:
        host = [np.full(n, np.nan, np.float32) if w else None for n, w in zip(lens, want)]
        args = [v.ctypes.data_as(C.c_void_p) for v in ((x, y) if y is not None else (x,))] + [nsamp, 0] + ([4] if fam == 'adapt' else [])
        args += [h.ctypes.data_as(C.POINTER(C.c_float)) if h is not None else None for h in host]
        ctx.check(getattr(ctx.lib, entry)(plan.h, *args, C.byref(nseg)), entry)
        rows = [h.tobytes() if h is not None else b'' for h in host]
    return rows + [('%s nseg=%d' % (plan.last_recipe(), nseg.value)).encode()]


def child(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'gr-ofdm_tools_amd')]
    from ofdm_tools import _hip, windows
    ctx = _hip.Context(0)
    tapers = {n: windows.dpss(n, 2.0, K, return_ratios=True) for n in SIZES}
    tapers = {n: (np.ascontiguousarray(t, np.float32), r) for n, (t, r) in tapers.items()}
    got = {}

    def record(key, rows):
        for r, b in enumerate(rows):
            got['%s/row%d' % (key, r)] = np.frombuffer(b, np.uint8)

    for f, fam in enumerate(FAMILIES):
        two = FAMILIES[fam][0] == 'mtmcsd'
        optional = [r for r in range(len(FAMILIES[fam][2])) if r != FAMILIES[fam][3]]
        for (i, n), (j, nseg) in itertools.product(enumerate(SIZES), enumerate(SEGMENTS)):
            x3, y3 = noise(3 * n * nseg, 100 * i + j), noise(3 * n * nseg, 100 * i + j + 50)
            for k in range(2):
                stage = OUT_STAGES[(f + 3 * i + 2 * j + k) % 8]
                plan = make_plan(ctx, fam, n, stage, tapers)
                key = '%s/n%d/seg%d/shift%d-trim%d-db%d' % ((fam, n, nseg) + stage)
                x1, y1 = x3[:n * nseg], (y3[:n * nseg] if two else None)
                record(key + '/host/all', run(ctx, plan, fam, False, x1, y1, 1, optional))
                record(key + '/host/none', run(ctx, plan, fam, False, x1, y1, 1, ()))
                record(key + '/dev1/all', run(ctx, plan, fam, True, x1, y1, 1, optional))
                for r in optional:      # each optional row on its own, the others NULL
                    record(key + '/dev1/only%d' % r, run(ctx, plan, fam, True, x1, y1, 1, (r,)))
                if not two:             # (the two-channel form takes one stream)
                    record(key + '/dev3/all', run(ctx, plan, fam, True, x3, None, 3, optional))
                    record(key + '/dev3/none', run(ctx, plan, fam, True, x3, None, 3, ()))
                plan.close()
    for n in SIZES:      # the empty-bin branches of the spectral kurtosis; the sd = 0 bins of the F-test
        for name, x in (('silence', np.zeros(11 * n, np.complex64)), ('constant', np.full(11 * n, 0.75 - 0.25j, np.complex64))):
            plan = make_plan(ctx, 'sk', n, (1, 3, 0), tapers)
            record('sk/n%d/%s/host' % (n, name), run(ctx, plan, 'sk', False, x, None, 1, (1,)))
            record('sk/n%d/%s/dev' % (n, name), run(ctx, plan, 'sk', True, x, None, 1, (1,)))
            plan.close()
        tone = np.exp(2j * np.pi * (n // 8) * np.arange(11 * n) / n).astype(np.complex64)
        plan = make_plan(ctx, 'ftest', n, (0, 0, 0), tapers)
        record('ftest/n%d/tone/host' % n, run(ctx, plan, 'ftest', False, tone, None, 1, (1, 2)))
        record('ftest/n%d/tone/dev' % n, run(ctx, plan, 'ftest', True, tone, None, 1, (1, 2)))
        plan.close()
    ctx.close()
    np.savez(path, **got)
    print('%d rows written' % len(got))


def main(argv):
    opt = {'--out': None, '--timeout': '600', '--old-label': None, '--new-label': None}
    for flag in opt:
        if flag in argv:
            i = argv.index(flag)
            opt[flag] = argv[i + 1]
            del argv[i:i + 2]
    out, limit = opt['--out'], int(opt['--timeout'])
    if len(argv) != 2:
        sys.exit(__doc__)
    dumps = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, lib in zip(('old', 'new'), argv):
            path = os.path.join(tmp, tag + '.npz')
            env = dict(os.environ, OFDM_TOOLS_HIP_LIB=os.path.abspath(lib))
            rc = subprocess.call(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--child', path], env=env)
            if rc != 0:
                sys.exit('%s (%s): exit status %d - stopped' % (tag, lib, rc))
            dumps.append(dict(np.load(path)))
    old, new = dumps
    lines = ['old: %s' % (opt['--old-label'] or argv[0]), 'new: %s' % (opt['--new-label'] or argv[1]), '']
    bad = sorted(k for k in set(old) | set(new) if k not in old or k not in new or old[k].tobytes() != new[k].tobytes())
    for fam in FAMILIES:
        keys = [k for k in old if k.startswith(fam + '/')]
        live = [k for k in keys if old[k].size]
        lines.append('%-8s %5d rows compared (%d bytes), %d left NULL on purpose, %d differ' %
                     (fam, len(live), sum(old[k].size for k in live), len(keys) - len(live), sum(1 for k in bad if k.startswith(fam + '/'))))
    lines += ['DIFFERS  ' + k for k in bad]
    lines.append('%d rows, %d difference(s): %s' % (len(old), len(bad), 'every byte equal' if not bad else 'NOT the same bits'))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        child(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1:]))
