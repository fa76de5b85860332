#!/usr/bin/env python3
"""The adaptive-weight launch (oth_mtm_adaptive_dev, csrc/mtmadapt.hip + its finalize launch, 4 iterations, both rows) against
exec_dev of the SAME plan on the SAME input - the PSD kernel of csrc/mtm.hip doing the same K transforms per segment, with
its finalize launch - at

  64 streams x 16384 points x 1 segment, K 7   (one row per scanner channel)
  2^24 samples at 4096 points, no overlap, K 4 (a long capture)

The two differ in the work split - the PSD kernel spreads a segment's K tapers over K workgroups, the adaptive kernel keeps
a segment in one workgroup (the weights are not linear in the tapers), so a launch of few segments fills fewer CUs - and in
the K eigenspectra per bin the adaptive kernel stores and reads back in each of its iters + 1 passes.  Whole steps are timed
with HIP events on one stream, the two alternating inside one session; the median over the repetitions is reported.
Nothing is gated.  Then the resource table of every mtm_adapt_kernel build, from the library's code objects.

usage: mtm_adaptive_time.py [reps] [--out profiles/mtm_adaptive_time.txt]
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
out_path = os.path.join(ROOT, 'profiles', 'mtm_adaptive_time.txt')
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
say('library %s on %s, %d repetitions per shape, the two launches alternating' % (os.path.basename(_hip.LIB_PATH), ctx.device_name(), reps))

SHAPES = [('64 x 16384 x 1 segment, K 7', 16384, 64, 16384, 4.0, 7),
          ('2^24 samples at 4096, no overlap, K 4', 4096, 1, 1 << 24, 2.5, 4)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


for name, nfft, nstreams, per_stream, nw, K in SHAPES:
    n = nstreams * per_stream
    x = torch.empty(2 * n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.synth_iq(x.data_ptr(), n, 2026, ((0.5, 0.1234), (0.05, -0.31), (2.0, 0.4071)), 0.1 + 0.05j)
    psd = torch.empty((nstreams, nfft), dtype=torch.float32, device=dev)
    rows = torch.empty((2, nstreams, nfft), dtype=torch.float32, device=dev)
    plan = ctx.mtm_plan(nfft, nw=nw, ntapers=K)
    recipes = {}

    def run_psd():
        plan.exec_dev(x.data_ptr(), per_stream, psd.data_ptr(), nstreams=nstreams)

    def run_adaptive():
        plan.adaptive_dev(x.data_ptr(), per_stream, nstreams, per_stream, rows[0].data_ptr(), rows[1].data_ptr(), iters=4)

    cands = [('PSD (exec_dev)', run_psd), ('adaptive (adaptive_dev, 4 iterations)', run_adaptive)]
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
        say('  %-38s %9.3f ms per step (median of %d, min %.3f)  %8.0f Msamples/s  x%.2f of the PSD   [%s]'
            % (label, v, reps, min(ms[label]), n / v / 1e3, v / base, recipes[label]))
    # where the two stand to each other: on this input (noise and three tones, no empty band) the adaptive weights stay near 1
    ratio = rows[0].double() / psd.double()
    say('  adaptive / PSD row: %.3f ... %.3f; dof %.2f ... %.2f of 2 K = %d'
        % (ratio.min().item(), ratio.max().item(), rows[1].min().item(), rows[1].max().item(), 2 * K))
    plan.close()
    del x, psd, rows
ctx.close()

say('')
import kernel_resources  # noqa: E402
ks = {n: v for n, v in kernel_resources.kernels(_hip.LIB_PATH).items() if 'mtm_adapt_kernel<' in n or 'adapt_finalize_kernel' in n}
say('%-64s %5s %5s %6s %9s' % ('kernel <N, T, KEEP, eigenspectra in LDS>', 'VGPR', 'SGPR', 'spills', 'scratch B'))
for n in sorted(ks, key=lambda q: (int(q.split('<')[1].split(',')[0]) if '<' in q else 0)):
    k = ks[n]
    say('%-64s %5d %5d %6d %9d' % (n.split('(')[0], k['vgpr'] + k['agpr'], k['sgpr'], k['spill_vgpr'], k['scratch']))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
