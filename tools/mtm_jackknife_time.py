#!/usr/bin/env python3
"""The jackknife step (oth_mtm_jackknife_dev / oth_mtm_csd_jackknife_dev: the plan's own averaging launch and reduction, then
csrc/mtmjack.hip and its finalize launch) against exec_dev / csd_exec_dev of the SAME plan on the SAME input, at

  64 streams x 16384 points x 1 segment, K 7   (one channel: one row per scanner channel)
  2^24 samples at 4096 points, no overlap, K 4 (one channel: a long capture)
  16384 points x 1 segment, K 7                (two channels: one work()-sized vector pair)
  2^24 samples at 4096 points, no overlap, K 4 (two channels: a long capture)

The step reads its input twice and adds a log1p (one channel) or two log1p and two atanh (two channels) per bin and item to
the K transforms per segment both passes make.  Whole steps are timed with HIP events on one stream, the two alternating
inside one session; the median over the repetitions is reported.  Nothing is gated.  Then the resource table of every
mtm_jack_kernel and mtmcsd_jack_kernel build, from the library's code objects.

usage: mtm_jackknife_time.py [reps] [--out profiles/mtm_jackknife_time.txt]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gr-ofdm_tools_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from ofdm_tools import _hip  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
out_path = os.path.join(ROOT, 'profiles', 'mtm_jackknife_time.txt')
if '--out' in sys.argv:
    out_path = sys.argv[sys.argv.index('--out') + 1]
    args = [a for a in args if a != out_path]
reps = int(args[0]) if args else 30
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


dev = torch.device('cuda', 0)
stream = torch.cuda.current_stream(dev)
ctx = _hip.Context(0, stream=stream.cuda_stream)
say('library %s on %s, %d repetitions per shape, the two steps alternating' % (os.path.basename(_hip.LIB_PATH), ctx.device_name(), reps))

# name, two channels, nfft, streams, samples per stream, NW, K
SHAPES = [('one channel: 64 x 16384 x 1 segment, K 7', False, 16384, 64, 16384, 4.0, 7),
          ('one channel: 2^24 samples at 4096, no overlap, K 4', False, 4096, 1, 1 << 24, 2.5, 4),
          ('two channels: 16384 x 1 segment, K 7', True, 16384, 1, 16384, 4.0, 7),
          ('two channels: 2^24 samples at 4096, no overlap, K 4', True, 4096, 1, 1 << 24, 2.5, 4)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


for name, two, nfft, nstreams, per_stream, nw, K in SHAPES:
    n = nstreams * per_stream
    x = torch.empty(2 * n, dtype=torch.float32, device=dev)
    y = torch.empty(2 * n if two else 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.synth_iq(x.data_ptr(), n, 2026, ((0.5, 0.1234), (0.05, -0.31), (2.0, 0.4071)), 0.1 + 0.05j)
    if two:
        ctx.synth_iq(y.data_ptr(), n, 2027, ((0.35, 0.1234), (2.0, 0.4071)), 0.1 + 0.05j)
    ref = torch.empty((5, nstreams, nfft), dtype=torch.float32, device=dev)
    rows = torch.empty((4, nstreams, nfft), dtype=torch.float32, device=dev)
    plan = (ctx.mtm_csd_plan if two else ctx.mtm_plan)(nfft, nw=nw, ntapers=K)
    recipes = {}

    if two:
        def run_base():
            plan.csd_exec_dev(x.data_ptr(), y.data_ptr(), per_stream, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref[4].data_ptr())

        def run_jack():
            plan.csd_jackknife_dev(x.data_ptr(), y.data_ptr(), per_stream, rows[1].data_ptr(), rows[0].data_ptr(), rows[2].data_ptr(),
                                   rows[3].data_ptr())
        cands = [('CSD (csd_exec_dev, four rows)', run_base), ('jackknife (csd_jackknife_dev, four rows)', run_jack)]
    else:
        def run_base():
            plan.exec_dev(x.data_ptr(), per_stream, ref[0].data_ptr(), nstreams=nstreams)

        def run_jack():
            plan.jackknife_dev(x.data_ptr(), per_stream, nstreams, per_stream, rows[0].data_ptr(), rows[1].data_ptr())
        cands = [('PSD (exec_dev)', run_base), ('jackknife (jackknife_dev, lnsd + PSD)', run_jack)]
    for label, fn in cands:      # warm-up: workspaces, first launches
        fn()
        fn()
        recipes[label] = plan.last_recipe()
    torch.cuda.synchronize(dev)
    ms = {label: [] for label, _ in cands}
    for _ in range(reps):
        for label, fn in cands:
            ms[label].append(timed(fn))
    say('')
    say(name)
    base = float(np.median(ms[cands[0][0]]))
    for label, _ in cands:
        v = float(np.median(ms[label]))
        say('  %-42s %9.3f ms per step (median of %d, min %.3f)  %8.0f Msamples/s  x%.2f of the first   [%s]'
            % (label, v, reps, min(ms[label]), n / v / 1e3, v / base, recipes[label]))
    # the two agree where they overlap, bit for bit: the PSD row, or the coherence
    same = torch.equal(rows[0], ref[4]) if two else torch.equal(rows[1], ref[0])
    say('  the %s row of the jackknife step against the first step: %s' % ('Cxy' if two else 'PSD', 'the same bits' if same else 'DIFFERENT'))
    plan.close()
    del x, y, ref, rows
ctx.close()

say('')
import kernel_resources  # noqa: E402
ks = {n: v for n, v in kernel_resources.kernels(_hip.LIB_PATH).items() if 'jack_kernel<' in n or 'jack_finalize_kernel' in n}
say('%-72s %5s %5s %6s %9s' % ('kernel <N, T, KEEP, [two LDS buffers,] sums in registers>', 'VGPR', 'SGPR', 'spills', 'scratch B'))
for n in sorted(ks, key=lambda q: ('mtmcsd' in q, int(q.split('<')[1].split(',')[0]) if '<' in q else 0)):
    k = ks[n]
    say('%-72s %5d %5d %6d %9d' % (n.split('(')[0], k['vgpr'] + k['agpr'], k['sgpr'], k['spill_vgpr'], k['scratch']))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
