#!/usr/bin/env python3
"""Median average against the mean at the C2 shape (2^28 complex64 samples, 4096-pt Hann, 50 % overlap, constant detrend,
density), interleaved on the same box: HIP-event time of the averaging step of each (mean: the averaging kernel; median:
rows producer + the four select passes; the finalize launch is outside both), Msamples/s and the bytes each part moves.
Then SciPy's welch(average='median') on complex64, 2^24 samples, one host core.

usage: median_time.py [reps] [log2_samples]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gr-ofdm_tools_amd'))
from ofdm_tools import _hip, windows  # noqa: E402

import numpy as np  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 28)
NFFT = 4096
ctx = _hip.Context(0)
w = windows.get_window('hann', NFFT)
d = ctx.alloc(8 * n)
out = ctx.alloc(4 * NFFT)
ctx.synth_iq(d, n, 2024, ((0.5, 0.1234), (0.05, -0.31), (2.0, 0.4071)), 0.1 + 0.05j)
plans = {a: ctx.welch_plan(NFFT, window=w, average=a) for a in ('mean', 'median')}
nseg = plans['mean'].nseg(n)
ms = {a: [] for a in plans}
ctx.set_timing(True)
for a, p in plans.items():      # warm-up (workspace allocation, first launch)
    p.exec_dev(d, n, out)
ctx.sync()
ctx.get_timing(reset=True)
for _ in range(reps):
    for a, p in plans.items():
        p.exec_dev(d, n, out)
        t, k = ctx.get_timing(reset=True)
        ms[a].append(t / max(k, 1))
rows_bytes = 4 * nseg * NFFT
in_bytes = 8 * n
print('shape: %d samples, nfft %d, %d segments; recipe %s' % (n, NFFT, nseg, plans['median'].last_recipe()))
for a in plans:
    v = float(np.median(ms[a]))
    print('%-6s %8.3f ms per step (median of %d, min %.3f)  %9.0f Msamples/s' % (a, v, reps, min(ms[a]), n / v / 1e3))
print('bytes: mean step reads %.2f GB; median: rows producer reads %.2f GB + writes %.2f GB, each of 4 select passes reads '
      '%.2f GB (+ count atomics)' % (in_bytes / 1e9, in_bytes / 1e9, rows_bytes / 1e9, rows_bytes / 1e9))
med = float(np.median(ms['median']))
print('median step: %.0f GB/s over input + rows written + 4 passes read' % ((in_bytes + 5 * rows_bytes) / med / 1e6))
ctx.set_timing(False)
for p in plans.values():
    p.close()
ctx.free(d)
ctx.free(out)
try:
    import scipy.signal as S
except ImportError:
    S = None
if S is not None:
    m = 1 << 24
    t = np.arange(m)
    rng = np.random.default_rng(1)
    x = ((rng.standard_normal(m) + 1j * rng.standard_normal(m)) / np.sqrt(2) + 0.5 * np.exp(2j * np.pi * 0.1234 * t)).astype(np.complex64)
    best = []
    for _ in range(3):
        t0 = time.perf_counter()
        S.welch(x, window='hann', nperseg=NFFT, average='median', return_onesided=False)
        best.append(time.perf_counter() - t0)
    v = float(np.median(best))
    print('scipy.signal.welch(average=median), complex64, 2^24 samples, one core: %.3f s  %.1f Msamples/s' % (v, m / v / 1e6))
