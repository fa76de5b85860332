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
import sys

import torch

from stat_time import Session

from ofdm_tools import _hip, windows  # noqa: E402 - stat_time sets the path

s = Session('welch_sk_time.txt')
ctx, dev = s.ctx, s.dev
s.say('%s, %d repetitions per shape, the arms alternating' % (s.library, s.reps))

SHAPES = [('2^24 samples at 4096, no overlap', 4096, 1, 1 << 24),
          ('64 captures of 4 x 16384', 16384, 64, 4 * 16384)]

failed = False
for name, nfft, nstreams, per_stream in SHAPES:
    n = nstreams * per_stream
    M = per_stream // nfft
    x = s.capture(n)
    win = windows.get_window('hann', nfft)
    plan = ctx.welch_plan(nfft, noverlap=0, window=win)
    generic = ctx.welch_plan(nfft, noverlap=0, window=win, kernel=_hip.KERNEL_GENERIC)
    out = torch.empty((2, nstreams, nfft), dtype=torch.float32, device=dev)
    rows = torch.empty((nstreams, M, nfft), dtype=torch.float32, device=dev)
    psd = torch.empty((nstreams, nfft), dtype=torch.float32, device=dev)
    comp = {}

    def run_fused():
        plan.sk_dev(x.data_ptr(), per_stream, nstreams, per_stream, out[0].data_ptr(), out[1].data_ptr())

    def run_composition():
        for i in range(nstreams):
            plan.segments_dev(x.data_ptr() + 8 * i * per_stream, per_stream, rows[i].data_ptr(), M)
        s1 = rows.sum(dim=1)
        s2 = (rows * rows).sum(dim=1)
        comp['sk'] = (M + 1.0) / (M - 1.0) * (M * s2 / (s1 * s1) - 1.0)
        comp['psd'] = s1 / M

    def run_generic():
        generic.exec_dev(x.data_ptr(), per_stream, psd.data_ptr(), nstreams=nstreams)

    cands = [('composition (segments_dev + torch)', run_composition, plan), ('fused (sk_dev, SK and PSD rows)', run_fused, plan),
             ('exec_dev, OTH_KERNEL_GENERIC', run_generic, generic)]
    med = s.report(name, cands, 36, 'composition', n)
    base, fused = med[cands[0][0]], med[cands[1][0]]
    s.say('  fused / exec_dev under OTH_KERNEL_GENERIC: x%.2f' % (fused / med[cands[2][0]]))
    # the two arms agree: R = M S2 / S1^2 recovered from either SK row, and the PSD rows
    r_f = out[0].double() * (M - 1.0) / (M + 1.0) + 1.0
    r_c = comp['sk'].double() * (M - 1.0) / (M + 1.0) + 1.0
    s.say('  R of the fused row against the composition: worst bin %.1e; PSD rows: %.1e'
          % ((r_f - r_c).abs().div(r_c).max().item(), (out[1].double() - comp['psd'].double()).abs().div(comp['psd'].double()).max().item()))
    ok = fused <= 1.05 * base
    failed = failed or not ok
    s.say('  gate: fused %.3f ms <= 1.05 x composition %.3f ms: %s' % (fused, base, 'ok' if ok else 'FAILED'))
    plan.close()
    generic.close()
    del x, out, rows, psd, comp

s.finish('kernel <N, T, KEEP, sums in registers>', ('welch_sk_kernel<', 'sk_finalize_kernel'))
sys.exit(1 if failed else 0)
