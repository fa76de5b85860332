#!/usr/bin/env python3
"""The two-channel multitaper launch (oth_mtm_csd_plan, csrc/mtmcsd.hip: Pxx, Pyy, Pxy, Cxy in one launch) against what
the library could do before it - two one-channel oth_mtm_plan launches, exec_dev on x and then on y, which give Pxx and
Pyy and no cross terms - on device-resident data, at

  64 single segments of 4096 points, K 7     (one csd_exec_dev per segment pair against two exec_dev)
  64 single segments of 8192 points, K 7
  64 single segments of 16384 points, K 7
  2^24 samples at 4096 points, no overlap, K 4

Two figures per arm, the arms alternating inside one session, medians over the repetitions: the averaging kernels' time
between HIP events (oth_ctx_set_timing / oth_ctx_get_timing: mtmcsd_kernel against the two mtm_kernel launches) and the
whole step on the host's clock (every launch, the finalize stages included, to oth_ctx_sync).  Nothing is gated: the
expectation - the fused launch costs no more than the two launches together plus about 10 % - is printed next to the ratio.
The resource table of every mtmcsd_kernel build, read from the library's code objects, closes the file.

usage: mtm_csd_time.py [reps] [--out profiles/mtm_csd.txt]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gr-ofdm_tools_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from ofdm_tools import _hip, windows  # noqa: E402

import numpy as np  # noqa: E402

import kernel_resources  # noqa: E402

argv = sys.argv[1:]
out_path = os.path.join(ROOT, 'profiles', 'mtm_csd.txt')
if '--out' in argv:
    i = argv.index('--out')
    out_path = argv[i + 1]
    del argv[i:i + 2]
reps = int(argv[0]) if argv else 30
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


ctx = _hip.Context(0)
say('library %s on %s, %d repetitions per shape, arms alternating' % (os.path.basename(_hip.LIB_PATH), ctx.device_name(), reps))

SHAPES = [('64 single segments of 4096 points, K 7', 4096, 64, 4096, 4.0, 7),      # name, nfft, calls, samples per call, NW, K
          ('64 single segments of 8192 points, K 7', 8192, 64, 8192, 4.0, 7),
          ('64 single segments of 16384 points, K 7', 16384, 64, 16384, 4.0, 7),
          ('2^24 samples at 4096 points, no overlap, K 4', 4096, 1, 1 << 24, 2.5, 4)]
TONES = ((0.5, 0.1234), (0.05, -0.31), (2.0, 0.4071))


def measure(fn):
    """-> (kernel ms between events, whole step ms on the host's clock) of one step"""
    ctx.sync()
    ctx.get_timing(reset=True)
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    step = 1e3 * (time.perf_counter() - t0)
    return ctx.get_timing(reset=True)[0], step


for name, nfft, calls, per_call, nw, K in SHAPES:
    n = calls * per_call
    dx, dy, out = ctx.alloc(8 * n), ctx.alloc(8 * n), ctx.alloc(4 * 5 * nfft)
    ctx.synth_iq(dx, n, 2026, TONES, 0.1 + 0.05j)
    ctx.synth_iq(dy, n, 2027, TONES[:2], -0.2 + 0.1j)
    tapers = windows.dpss(nfft, nw, K)
    fused = ctx.mtm_csd_plan(nfft, nw=nw, ntapers=K, tapers=tapers)
    single = ctx.mtm_plan(nfft, nw=nw, ntapers=K, tapers=tapers)
    o = [out + 4 * nfft * i for i in (0, 1, 2, 4)]

    def run_fused():
        for c in range(calls):
            off = 8 * c * per_call
            fused.csd_exec_dev(dx + off, dy + off, per_call, *o)

    def run_pair():
        for c in range(calls):
            off = 8 * c * per_call
            single.exec_dev(dx + off, per_call, o[0])
            single.exec_dev(dy + off, per_call, o[1])

    arms = [('fused: one mtmcsd launch', run_fused), ('pair: two mtm launches', run_pair)]
    for _, fn in arms:      # warm-up: workspaces, LDS attributes, first launches
        fn()
        fn()
    ctx.sync()
    ctx.set_timing(True)
    got = {label: [] for label, _ in arms}
    for _ in range(reps):
        for label, fn in arms:
            got[label].append(measure(fn))
    ctx.set_timing(False)
    say('')
    say('%s   [%s | %s]' % (name, fused.last_recipe(), single.last_recipe()))
    med = {}
    for label, _ in arms:
        k, s = (float(np.median([v[i] for v in got[label]])) for i in (0, 1))
        med[label] = (k, s)
        say('  %-26s kernels %9.3f ms (min %.3f)   whole step %9.3f ms (min %.3f)   median of %d'
            % (label, k, min(v[0] for v in got[label]), s, min(v[1] for v in got[label]), reps))
    (fk, fs), (pk, ps) = med[arms[0][0]], med[arms[1][0]]
    say('  fused / pair: kernels x%.2f, whole step x%.2f   (expectation: no more than x1.10)' % (fk / pk, fs / ps))
    fused.close()
    single.close()
    for p in (dx, dy, out):
        ctx.free(p)
ctx.close()

say('')
say('%-48s %5s %5s %6s %9s' % ('build (library code objects)', 'VGPR', 'SGPR', 'spills', 'scratch B'))
ks = kernel_resources.kernels(_hip.LIB_PATH)
for kname in sorted((k for k in ks if 'mtmcsd_kernel<' in k), key=lambda k: int(k.split('<')[1].split(',')[0])):
    v = ks[kname]
    say('%-48s %5d %5d %6d %9d' % (kname.split('(')[0], v['vgpr'] + v['agpr'], v['sgpr'], v['spill_vgpr'] + v['spill_sgpr'], v['scratch']))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
