#!/usr/bin/env python3
"""Do two builds of the library give the same bits for the per-bin statistics?  The check behind a change to their host
sides or finalize kernels that must not move an operation: these launches are deterministic by construction (contiguous
runs per workgroup, fixed-order double sums), so every output row and every last_recipe string is compared byte for byte -
there is no tolerance.

  python tools/stat_bits.py OLD.so NEW.so [--cases stat|plain] [--twice] [--out profiles/FILE.txt] [--timeout SECONDS]
                             [--old-label TEXT] [--new-label TEXT]

runs the same cases in a fresh child process per library (OFDM_TOOLS_HIP_LIB), one after the other, each under its own
`timeout`; it stops at the first child that fails.  Exit status 1 if a row differs.  The summary names the two libraries by
their paths, or by the labels given.  --twice runs OLD a second time first and leaves out, by name, every row that differs
between its two runs.

Cases: the eight families (F-test, spectral kurtosis, jackknife, two-channel jackknife, adaptive, cyclic with 1, 3 and 5
cycle frequencies, cyclic autocorrelation with 1 and 5 lags on both builds through OTH_LAG_GROUP, spectral matrix of 2, 3
and 8 channels), host and _dev forms, 64 / 4096 / 16384 points, 2 / 11 / 19 segments (11 and 19: the finalize slice
loop runs more than once, W not a multiple of 8), fftshift, trim 0 / 3 and dB on and off, 1 and 3 streams, each optional
row present and NULL (the matrix takes channels, not streams, one capture per call, and one of its two rows at least); the
spectral kurtosis of silence and of a constant under detrend; the F-test of a pure tone.

--cases plain: the Welch / CSD / chain calls behind launch_finalize, launch_scale, launch_csd_scale and launch_chain_tail
instead (PLAIN below: every row layout and every route of launch_finalize), each under all eight output stages, the Welch
plans on the contiguous schedule (the ticket schedule is not reproducible run to run).  A refusal is a row too: its text."""
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
LAGS = [5, 0, 64, 1, 17]
# family -> (plan, entry point, rows in ABI order as multiples of out_len (negative: that many floats), index of the row every
# call needs (None: any one row will do))
FAMILIES = {
    'ftest': ('mtm', 'oth_mtm_ftest', (1, 1, 1), 0), 'sk': ('welch', 'oth_welch_sk', (1, 1), 0),
    'jack': ('mtm', 'oth_mtm_jackknife', (1, 1), 0), 'csdjack': ('mtmcsd', 'oth_mtm_csd_jackknife', (1, 1, 1, 1), 1),
    'adapt': ('mtm', 'oth_mtm_adaptive', (1, 1), 0), 'cyc1': ('welch', 'oth_welch_cyclic', (2, 1, 1), 1),
    'cyc3': ('welch', 'oth_welch_cyclic', (6, 3, 1), 1), 'cyc5': ('welch', 'oth_welch_cyclic', (10, 5, 1), 1),
    # cafLgG: L lags on the build OTH_LAG_GROUP=G, rows caf [L][out_len] and r [L] pairs
    'caf1g1': ('welch', 'oth_welch_caf', (1, -2), 0), 'caf1g2': ('welch', 'oth_welch_caf', (1, -2), 0),
    'caf5g1': ('welch', 'oth_welch_caf', (5, -10), 0), 'caf5g2': ('welch', 'oth_welch_caf', (5, -10), 0),
    # matC: C channels, rows S (C (C + 1) / 2 complex rows) and gcoh
    'mat2': ('welch', 'oth_welch_matrix', (6, 1), None), 'mat3': ('welch', 'oth_welch_matrix', (12, 1), None),
    'mat8': ('welch', 'oth_welch_matrix', (72, 1), None),
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
        if fam.startswith('caf'):
            os.environ['OTH_LAG_GROUP'] = fam[-1]      # read when the plan is created
        try:
            p = ctx.welch_plan(n, noverlap=0, window=windows.get_window('hann', n), **kw)
        finally:
            os.environ.pop('OTH_LAG_GROUP', None)
        if fam.startswith('cyc'):
            p.set_cycles([0.25, -0.0625, 0.001, 0.5, -0.3][:int(fam[3:])])
        if fam.startswith('caf'):
            p.set_lags(LAGS[:int(fam[3])])
        return p
    p = (ctx.mtm_csd_plan if kind == 'mtmcsd' else ctx.mtm_plan)(n, tapers=tapers[n][0], **kw)
    p.set_ratios(np.clip(tapers[n][1], np.finfo(np.float64).tiny, 1.0))
    return p


def run(ctx, plan, fam, dev, x, y, ns, keep):
    """One call, host form or (dev) device form on ns streams (the matrix: the ns channels of one capture); keep: the
    optional rows wanted.  -> the rows' bytes (b'' for a row left out) + the recipe"""
    _, entry, units, need = FAMILIES[fam]
    mat = fam.startswith('mat')
    nsamp = len(x) // ns
    lens = [u * plan.out_len if u > 0 else -u for u in units]
    want = [r == need or r in keep for r in range(len(units))]
    nseg = C.c_uint64()
    if dev:
        src = [ctx.alloc(v.nbytes) for v in ((x, y) if y is not None else (x,))]
        for d, v in zip(src, (x, y)):
            ctx.h2d(d, v)
        nrows = 1 if mat else ns
        out = [ctx.alloc(4 * nrows * n) if w else None for n, w in zip(lens, want)]
        args = [C.c_void_p(d) for d in src] + [nsamp] + ([ns, nsamp] if y is None else []) + ([4] if fam == 'adapt' else [])
        args += [C.c_void_p(o) if o else None for o in out]
        ctx.check(getattr(ctx.lib, entry + '_dev')(plan.h, *args, C.byref(nseg)), entry + '_dev')
        ctx.sync()
        rows = [ctx.d2h(o, (nrows, n), np.float32).tobytes() if o else b'' for o, n in zip(out, lens)]
        for d in src + [o for o in out if o]:
            ctx.free(d)
    else:
        host = [np.full(n, np.nan, np.float32) if w else None for n, w in zip(lens, want)]
        args = [v.ctypes.data_as(C.c_void_p) for v in ((x, y) if y is not None else (x,))] + [nsamp] + [ns] * mat + [0] + ([4] if fam == 'adapt' else [])
        args += [h.ctypes.data_as(C.POINTER(C.c_float)) if h is not None else None for h in host]
        ctx.check(getattr(ctx.lib, entry)(plan.h, *args, C.byref(nseg)), entry)
        rows = [h.tobytes() if h is not None else b'' for h in host]
    return rows + [('%s nseg=%d' % (plan.last_recipe(), nseg.value)).encode()]


# --cases plain: (nfft, segments, detrend, window, tuning word) - 64 / 999: layout 0, the odd-length shift; 1024 x 1100: the
# row-group stage; 4096: layout 1 through finalize_kernel (5 rows), the two-stage route (40) and the wide kernel (70); 8192 /
# 16384: layouts 5 / 4 (no detrend; 16384 with 5 rows: finalize_l4_kernel) and 3 / 2 (detrend); 32768 / 65536: 7 / 8, r16: 6
PLAIN = [(64, 5, 1, 'hann', None), (999, 5, 1, 'hann', None), (1024, 1100, 1, 'hann', None), (4096, 5, 1, 'hann', None),
         (4096, 40, 1, 'hann', None), (4096, 70, 1, 'hann', None), (8192, 5, 0, None, None), (8192, 5, 1, 'hann', None),
         (16384, 5, 0, None, None), (16384, 70, 0, None, None), (16384, 5, 1, 'hann', None), (32768, 5, 1, 'hann', None),
         (65536, 5, 1, 'hann', None), (32768, 5, 1, 'hann', 'r16')]
PLAIN_CALLS = ('exec_dev', 'exec_dev3', 'partial+scale', 'accumulate', 'csd_exec_dev', 'csd_partial+scale', 'segments_dev', 'median')


def plain_cases(ctx, record_rows):
    from ofdm_tools import _hip, windows

    def record(key, call):
        try:
            record_rows(key, call())
        except _hip.HipError as e:
            record_rows(key, [str(e).encode()])

    for c, (n, nseg, det, win, tune) in enumerate(PLAIN):
        N = n * nseg
        x3, y = noise(3 * N, c), noise(N, c + 50)
        d3, dy, sums = ctx.alloc(x3.nbytes), ctx.alloc(y.nbytes), ctx.alloc(16 * n)
        out = ctx.alloc(4 * n * 8)      # five rows of a two-channel call, three streams' rows, eight segments' rows
        ctx.h2d(d3, x3)
        ctx.h2d(dy, y)
        for stage in OUT_STAGES:
            p = ctx.welch_plan(n, noverlap=0, window=windows.get_window(win, n) if win else None,
                               detrend=_hip.DETREND_CONSTANT if det else _hip.DETREND_NONE, fftshift=bool(stage[0]), trim_bins=stage[1],
                               db=bool(stage[2]))
            p.set_schedule(_hip.SCHED_CONTIGUOUS)
            if tune:
                p.set_tuning(tune)
            m = p.out_len
            grab = lambda ptr, count: ctx.d2h(ptr, (count,), np.float32).tobytes()      # noqa: E731
            four = lambda: (out, out + 4 * m, out + 8 * m, out + 16 * m)      # noqa: E731  pxx, pyy, pxy (2 m), cxy

            def accumulate():
                p.accumulate(x3[:N // 2 + 17])
                p.accumulate(x3[N // 2 + 17:N])
                return [p.finalize().tobytes()]

            def median():
                p.set_average('median')
                return [b'%d' % p.exec_dev(d3, N, out, 3, N), grab(out, 3 * m)]

            calls = {
                'exec_dev': lambda: [b'%d' % p.exec_dev(d3, N, out), grab(out, m), p.last_recipe().encode()],
                'exec_dev3': lambda: [b'%d' % p.exec_dev(d3, N, out, 3, N), grab(out, 3 * m), p.last_recipe().encode()],
                'partial+scale': lambda: [grab(sums, n), grab(out, m)] if p.scale_dev(sums, p.partial_dev(d3, N, sums), out) is None else [],
                'accumulate': accumulate,
                'csd_exec_dev': lambda: [b'%d' % p.csd_exec_dev(d3, dy, N, *four()), grab(out, 5 * m), p.last_recipe().encode()],
                'csd_partial+scale': lambda: [grab(sums, 4 * n), grab(out, 5 * m)]
                if p.csd_scale_dev(sums, p.csd_partial_dev(d3, dy, N, sums), *four()) is None else [],
                'segments_dev': lambda: [grab(out, m * p.segments_dev(d3, n * min(nseg, 8), out, 8))],
                'median': median,      # last: the plan stays on the median
            }
            for name in PLAIN_CALLS:
                record('%s/n%d%s/seg%d/det%d/shift%d-trim%d-db%d' % ((name, n, '-' + tune if tune else '', nseg, det) + stage), calls[name])
            p.close()
        for d in (d3, dy, sums, out):
            ctx.free(d)
    # a fused chain push with the IIR and with peak hold: launch_chain_tail on natural rows and on layouts 3 and 4
    for n, shift, mode in itertools.product((1024, 4096, 8192, 16384), (0, 1), ('iir', 'peak')):
        x = noise(n * 300, n + shift)
        d, rows = ctx.alloc(x.nbytes), ctx.alloc(4 * 4 * n)
        ctx.h2d(d, x)
        ch = ctx.chain(n, windows.blackmanharris(n), bool(shift), _hip.EPI_MAG2, 1)
        ch.set_iir_log(0.8, -10.0) if mode == 'iir' else ch.set_peak_hold(True)
        record('chain/n%d/shift%d/%s' % (n, shift, mode), lambda: [b'%d' % ch.push_dev(d, len(x), rows, 4),
                                                                     ctx.d2h(rows, (4 * n,), np.float32).tobytes(),
                                                                     (ch.iir() if mode == 'iir' else ch.peak()).tobytes()])
        ch.close()
        ctx.free(d)
        ctx.free(rows)


def child(path, plain):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'gr-ofdm_tools_amd')]
    from ofdm_tools import _hip
    ctx = _hip.Context(0)
    got = {}

    def record(key, rows):
        for r, b in enumerate(rows):
            got['%s/row%d' % (key, r)] = np.frombuffer(b, np.uint8)

    (plain_cases if plain else stat_cases)(ctx, record)
    ctx.close()
    np.savez(path, **got)
    print('%d rows written' % len(got))


def stat_cases(ctx, record):
    from ofdm_tools import windows
    tapers = {n: windows.dpss(n, 2.0, K, return_ratios=True) for n in SIZES}
    tapers = {n: (np.ascontiguousarray(t, np.float32), r) for n, (t, r) in tapers.items()}
    for f, fam in enumerate(FAMILIES):
        two = FAMILIES[fam][0] == 'mtmcsd'
        chans = int(fam[3:]) if fam.startswith('mat') else 0
        optional = [r for r in range(len(FAMILIES[fam][2])) if r != FAMILIES[fam][3]]
        for (i, n), (j, nseg) in itertools.product(enumerate(SIZES), enumerate(SEGMENTS)):
            # a stream holds nseg segments: the caf counts them on what the largest lag leaves
            per = n * nseg + (max(LAGS[:int(fam[3])]) if fam.startswith('caf') else 0)
            xs, y3 = noise(max(3, chans) * per, 100 * i + j), noise(3 * n * nseg, 100 * i + j + 50)
            x3 = xs[:3 * per]
            for k in range(2):
                stage = OUT_STAGES[(f + 3 * i + 2 * j + k) % 8]
                plan = make_plan(ctx, fam, n, stage, tapers)
                key = '%s/n%d/seg%d/shift%d-trim%d-db%d' % ((fam, n, nseg) + stage)
                if chans:      # channels, not streams: one capture per call, and one of the two rows at least
                    for form, dev in (('host', False), ('dev', True)):
                        record('%s/%s/all' % (key, form), run(ctx, plan, fam, dev, xs[:chans * per], None, chans, optional))
                        for r in optional:
                            record('%s/%s/only%d' % (key, form, r), run(ctx, plan, fam, dev, xs[:chans * per], None, chans, (r,)))
                    plan.close()
                    continue
                x1, y1 = x3[:per], (y3[:per] if two else None)
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


def main(argv):
    opt = {'--out': None, '--timeout': '600', '--old-label': None, '--new-label': None, '--cases': 'stat'}
    for flag in opt:
        if flag in argv:
            i = argv.index(flag)
            opt[flag] = argv[i + 1]
            del argv[i:i + 2]
    out, limit, plain = opt['--out'], int(opt['--timeout']), opt['--cases'] == 'plain'
    twice = '--twice' in argv      # OLD runs twice first: a row that differs there is not deterministic and leaves the list
    argv = [a for a in argv if a != '--twice']
    if len(argv) != 2:
        sys.exit(__doc__)
    dumps = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, lib in [('old', argv[0])] + [('old-again', argv[0])] * twice + [('new', argv[1])]:
            path = os.path.join(tmp, tag + '.npz')
            env = dict(os.environ, OFDM_TOOLS_HIP_LIB=os.path.abspath(lib))
            rc = subprocess.call(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__),
                                  '--child-plain' if plain else '--child', path], env=env)
            if rc != 0:
                sys.exit('%s (%s): exit status %d - stopped' % (tag, lib, rc))
            dumps.append(dict(np.load(path)))
    old, new = dumps[0], dumps[-1]
    lines = ['old: %s' % (opt['--old-label'] or argv[0]), 'new: %s' % (opt['--new-label'] or argv[1]), '']
    loose = sorted(k for k in old if k not in dumps[1] or old[k].tobytes() != dumps[1][k].tobytes()) if twice else []
    for k in loose:
        del old[k]
        new.pop(k, None)
    bad = sorted(k for k in set(old) | set(new) if k not in old or k not in new or old[k].tobytes() != new[k].tobytes())
    for fam in PLAIN_CALLS + ('chain',) if plain else FAMILIES:
        keys = [k for k in old if k.startswith(fam + '/')]
        live = [k for k in keys if old[k].size]
        lines.append('%-*s %5d rows compared (%d bytes), %d left NULL on purpose, %d differ' %
                     (17 if plain else 8, fam, len(live), sum(old[k].size for k in live), len(keys) - len(live), sum(1 for k in bad if k.startswith(fam + '/'))))
    lines += ['NOT DETERMINISTIC (old against old: left out)  ' + k for k in loose] + ['DIFFERS  ' + k for k in bad]
    lines.append('%d rows, %d difference(s): %s' % (len(old), len(bad), 'every byte equal' if not bad else 'NOT the same bits'))
    text = '\n'.join(lines)
    print(text)
    if out:
        with open(out, 'w') as f:
            f.write(text + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] in ('--child', '--child-plain'):
        child(sys.argv[2], sys.argv[1] == '--child-plain')
    else:
        sys.exit(main(sys.argv[1:]))
