#!/usr/bin/env python3
"""The fused multitaper plan (oth_mtm_plan, csrc/mtm.hip: one launch for all K tapers) against the composition a user had
before it - K Welch plans with window v_k through exec_dev and the weighted sum of their K rows - on the same library,
at the three shapes the plan is for:

  64 streams x 16384 points x 1 segment, K 7   (one row per scanner channel)
  1 stream   x 4096 points  x 1 segment, K 7   (one work()-sized vector)
  2^26 samples at 4096 points, no overlap, K 4 (a long capture)

The composition runs once with OTH_KERNEL_GENERIC (the same butterflies as the fused kernel) and once with OTH_KERNEL_AUTO
(the tuned kernels).  Whole steps are timed - every launch from the first kernel to the finished PSD rows - with HIP
events on one stream, the three candidates alternating inside one session; the median over the repetitions is reported.
Then the host side: the same estimate with SciPy on one core, and oth_dpss next to scipy.signal.windows.dpss.

Gate (exit status 1 when it fails): at every shape the fused step takes at most 1.05 x the GENERIC composition's time -
the same butterflies with K - 1 fewer reads and launches; 5 % for box noise.  The AUTO composition is recorded, not gated.

usage: mtm_time.py [reps] [--out profiles/mtm_shapes.txt] [--fused-only] [--no-host]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gr-ofdm_tools_amd'))
from ofdm_tools import _hip, windows  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
reps = int(args[0]) if args else 30
out_path = os.path.join(ROOT, 'profiles', 'mtm_shapes.txt')
if '--out' in sys.argv:
    out_path = sys.argv[sys.argv.index('--out') + 1]
    args = [a for a in args if a != out_path]
    reps = int(args[0]) if args else 30
fused_only = '--fused-only' in sys.argv
no_host = '--no-host' in sys.argv
lines = []
gate_failed = False
GENERIC = 'K Welch plans, OTH_KERNEL_GENERIC'


def say(text):
    print(text, flush=True)
    lines.append(text)


dev = torch.device('cuda', 0)
stream = torch.cuda.current_stream(dev)
ctx = _hip.Context(0, stream=stream.cuda_stream)      # the library's launches and torch's weighted sum on one stream
say('library %s on %s, %d repetitions per shape, candidates alternating' % (os.path.basename(_hip.LIB_PATH), ctx.device_name(), reps))

SHAPES = [('64 x 16384 x 1 segment, K 7', 16384, 64, 16384, 4.0, 7),
          ('1 x 4096 x 1 segment, K 7', 4096, 1, 4096, 4.0, 7),
          ('2^26 samples at 4096, no overlap, K 4', 4096, 1, 1 << 26, 2.5, 4)]


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
    tapers = windows.dpss(nfft, nw, K)
    fused_out = torch.empty((nstreams, nfft), dtype=torch.float32, device=dev)
    rows = torch.empty((K, nstreams, nfft), dtype=torch.float32, device=dev)
    comp_out = torch.empty((nstreams, nfft), dtype=torch.float32, device=dev)
    weights = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
    fused = ctx.mtm_plan(nfft, nw=nw, ntapers=K, tapers=tapers)

    def run_fused():
        fused.exec_dev(x.data_ptr(), per_stream, fused_out.data_ptr(), nstreams=nstreams)

    cands = [('fused mtm plan', run_fused)]
    plans = {}
    if not fused_only:
        for label, kern in ((GENERIC, _hip.KERNEL_GENERIC), ('K Welch plans, OTH_KERNEL_AUTO', _hip.KERNEL_AUTO)):
            plans[label] = [ctx.welch_plan(nfft, noverlap=0, window=tapers[k], kernel=kern) for k in range(K)]

            def run_comp(ps=plans[label]):
                for k, p in enumerate(ps):
                    p.exec_dev(x.data_ptr(), per_stream, rows[k].data_ptr(), nstreams=nstreams)
                torch.sum(rows * weights[:, None, None], dim=0, out=comp_out)
            cands.append((label, run_comp))
    for _, fn in cands:      # warm-up: workspaces, first launches
        fn()
        fn()
    torch.cuda.synchronize(dev)
    ms = {label: [] for label, _ in cands}
    for _ in range(reps):
        for label, fn in cands:
            ms[label].append(timed(fn))
    say('')
    say('%s   [%s]' % (name, fused.last_recipe()))
    base = float(np.median(ms['fused mtm plan']))
    for label, _ in cands:
        v = float(np.median(ms[label]))
        extra = ''
        if plans.get(label):
            extra = '  x%.2f of fused   [%s]' % (v / base, plans[label][0].last_recipe())
        say('  %-36s %9.3f ms per step (median of %d, min %.3f)  %8.0f Msamples/s%s' % (label, v, reps, min(ms[label]), n / v / 1e3, extra))
    if not fused_only:
        d = (fused_out - comp_out).abs().div(comp_out).max().item()
        say('  fused against the last composition: worst bin %.1e' % d)
        gen = float(np.median(ms[GENERIC]))
        ok = base <= 1.05 * gen
        gate_failed = gate_failed or not ok
        say('  gate: fused %.3f ms <= 1.05 x %.3f ms of the GENERIC composition: %s' % (base, gen, 'ok' if ok else 'FAILED'))
    fused.close()
    for ps in plans.values():
        for p in ps:
            p.close()
    del x, rows, fused_out, comp_out
ctx.close()

if not fused_only and not no_host:
    say('')
    import scipy.fft
    from scipy.signal.windows import dpss as scipy_dpss
    t0 = time.perf_counter()
    windows.dpss(16384, 4.0, 7, return_ratios=True)
    t1 = time.perf_counter()
    scipy_dpss(16384, 4.0, 7, return_ratios=True)
    t2 = time.perf_counter()
    say('tapers (16384, NW 4, K 7) with ratios, one core: oth_dpss %.3f s, scipy.signal.windows.dpss %.3f s' % (t1 - t0, t2 - t1))
    rng = np.random.default_rng(3)
    for name, nfft, nstreams, per_stream, nw, K in SHAPES:
        m = min(nstreams * per_stream, 1 << 22)                      # (the long capture: 2^22 of its samples)
        x = ((rng.standard_normal(m) + 1j * rng.standard_normal(m)) / np.sqrt(2)).astype(np.complex64)
        v = scipy_dpss(nfft, nw, K).astype(np.float32)
        t0 = time.perf_counter()
        seg = x.reshape(-1, nfft)
        seg = seg - seg.mean(axis=1, keepdims=True)
        psd = np.zeros(nfft, np.float32) if nstreams == 1 else np.zeros((nstreams, nfft), np.float32)
        for k in range(K):
            X = scipy.fft.fft(seg * v[k], axis=1)
            p = (X.real ** 2 + X.imag ** 2) / K
            psd += p.mean(axis=0) if nstreams == 1 else p
        dt = time.perf_counter() - t0
        say('SciPy side (complex64 pocketfft, one core), %-40s %8.2f ms for %d samples  %7.1f Msamples/s' % (name + ':', 1e3 * dt, m, m / dt / 1e6))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
sys.exit(1 if gate_failed else 0)
