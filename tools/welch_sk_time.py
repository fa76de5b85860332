#!/usr/bin/env python3
"""The spectral kurtosis launch (oth_welch_sk_dev: csrc/welchsk.hip + its finalize launch, SK and PSD rows) against the
composition a user had before it, on the SAME plan in the SAME session:

  segments_dev into a rows buffer ([nseg][nfft] floats), then in torch the sum and the sum of squares over the rows
  and the SK formula

at

  2^24 samples at 4096 points, no overlap            (a long capture: 4096 segments, 64 MiB of rows)
  64 captures of 4 x 16384 points                    (one row per scanner channel; the composition loops over the captures
                                                      with segments_dev - it takes one stream - and reduces all rows at once)

and, not gated, exec_dev of a plan of the same shape under OTH_KERNEL_GENERIC - the coverage kernel doing the same
transforms with one accumulator per bin.  Whole steps are timed with HIP events on one stream, the arms alternating inside
one session; the median over the repetitions is reported.

Gate (the exit status): the fused call is no slower than the composition at either shape, with 5 % allowed for box noise.
Then the resource table of every welch_sk_kernel build, from the library's code objects.

usage: welch_sk_time.py [reps] [--out profiles/welch_sk_time.txt]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gr-ofdm_tools_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from ofdm_tools import _hip, windows  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
out_path = os.path.join(ROOT, 'profiles', 'welch_sk_time.txt')
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
say('library %s on %s, %d repetitions per shape, the arms alternating' % (os.path.basename(_hip.LIB_PATH), ctx.device_name(), reps))

SHAPES = [('2^24 samples at 4096, no overlap', 4096, 1, 1 << 24),
          ('64 captures of 4 x 16384', 16384, 64, 4 * 16384)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


failed = False
for name, nfft, nstreams, per_stream in SHAPES:
    n = nstreams * per_stream
    M = per_stream // nfft
    x = torch.empty(2 * n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.synth_iq(x.data_ptr(), n, 2026, ((0.5, 0.1234), (0.05, -0.31), (2.0, 0.4071)), 0.1 + 0.05j)
    win = windows.get_window('hann', nfft)
    plan = ctx.welch_plan(nfft, noverlap=0, window=win)
    generic = ctx.welch_plan(nfft, noverlap=0, window=win, kernel=_hip.KERNEL_GENERIC)
    out = torch.empty((2, nstreams, nfft), dtype=torch.float32, device=dev)
    rows = torch.empty((nstreams, M, nfft), dtype=torch.float32, device=dev)
    psd = torch.empty((nstreams, nfft), dtype=torch.float32, device=dev)
    comp = {}
    recipes = {}

    def run_fused():
        plan.sk_dev(x.data_ptr(), per_stream, nstreams, per_stream, out[0].data_ptr(), out[1].data_ptr())

    def run_composition():
        for s in range(nstreams):
            plan.segments_dev(x.data_ptr() + 8 * s * per_stream, per_stream, rows[s].data_ptr(), M)
        s1 = rows.sum(dim=1)
        s2 = (rows * rows).sum(dim=1)
        comp['sk'] = (M + 1.0) / (M - 1.0) * (M * s2 / (s1 * s1) - 1.0)
        comp['psd'] = s1 / M

    def run_generic():
        generic.exec_dev(x.data_ptr(), per_stream, psd.data_ptr(), nstreams=nstreams)

    cands = [('composition (segments_dev + torch)', run_composition, plan), ('fused (sk_dev, SK and PSD rows)', run_fused, plan),
             ('exec_dev, OTH_KERNEL_GENERIC', run_generic, generic)]
    for label, fn, pl in cands:      # warm-up: workspaces, first launches
        fn()
        fn()
        recipes[label] = pl.last_recipe()
    torch.cuda.synchronize(dev)
    ms = {label: [] for label, _, _ in cands}
    for _ in range(reps):
        for label, fn, _ in cands:
            ms[label].append(timed(fn))
    say('')
    say(name)
    med = {label: float(np.median(ms[label])) for label, _, _ in cands}
    base = med[cands[0][0]]
    for label, _, _ in cands:
        v = med[label]
        say('  %-36s %9.3f ms per step (median of %d, min %.3f)  %8.0f Msamples/s  x%.2f of the composition   [%s]'
            % (label, v, reps, min(ms[label]), n / v / 1e3, v / base, recipes[label]))
    fused = med[cands[1][0]]
    say('  fused / exec_dev under OTH_KERNEL_GENERIC: x%.2f' % (fused / med[cands[2][0]]))
    # the two arms agree: R = M S2 / S1^2 recovered from either SK row, and the PSD rows
    r_f = out[0].double() * (M - 1.0) / (M + 1.0) + 1.0
    r_c = comp['sk'].double() * (M - 1.0) / (M + 1.0) + 1.0
    say('  R of the fused row against the composition: worst bin %.1e; PSD rows: %.1e'
        % ((r_f - r_c).abs().div(r_c).max().item(), (out[1].double() - comp['psd'].double()).abs().div(comp['psd'].double()).max().item()))
    ok = fused <= 1.05 * base
    failed = failed or not ok
    say('  gate: fused %.3f ms <= 1.05 x composition %.3f ms: %s' % (fused, base, 'ok' if ok else 'FAILED'))
    plan.close()
    generic.close()
    del x, out, rows, psd, comp
ctx.close()

say('')
import kernel_resources  # noqa: E402
ks = {n: v for n, v in kernel_resources.kernels(_hip.LIB_PATH).items() if 'welch_sk_kernel<' in n or 'sk_finalize_kernel' in n}
say('%-64s %5s %5s %6s %9s' % ('kernel <N, T, KEEP, sums in registers>', 'VGPR', 'SGPR', 'spills', 'scratch B'))
for n in sorted(ks, key=lambda q: (int(q.split('<')[1].split(',')[0]) if '<' in q else 0)):
    k = ks[n]
    say('%-64s %5d %5d %6d %9d' % (n.split('(')[0], k['vgpr'] + k['agpr'], k['sgpr'], k['spill_vgpr'], k['scratch']))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
sys.exit(1 if failed else 0)
