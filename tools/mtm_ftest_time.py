#!/usr/bin/env python3
"""The harmonic F-test launch (oth_mtm_ftest_dev, csrc/mtmftest.hip + its finalize launch) against exec_dev of the SAME plan
on the SAME input - the PSD kernel of csrc/mtm.hip doing the same K transforms per segment, with its finalize launch - at

  64 streams x 16384 points x 1 segment, K 7   (one row per scanner channel)
  2^26 samples at 4096 points, no overlap, K 4 (a long capture)

The two differ in the work split: the PSD kernel spreads a segment's K tapers over K workgroups, the F-test keeps a segment
in one workgroup (|sum_k U_k y_k|^2 is not linear in the tapers), so a launch of few segments fills fewer CUs.  Whole steps
are timed with HIP events on one stream, the two alternating inside one session; the median over the repetitions is
reported.  Nothing is gated.  Then the resource table of every mtm_ftest_kernel build, from the library's code objects.

usage: mtm_ftest_time.py [reps] [--out profiles/mtm_ftest_time.txt]
"""
import numpy as np
import torch

from stat_time import Session

s = Session('mtm_ftest_time.txt')
ctx, dev = s.ctx, s.dev
s.say('%s, %d repetitions per shape, the two launches alternating' % (s.library, s.reps))

SHAPES = [('64 x 16384 x 1 segment, K 7', 16384, 64, 16384, 4.0, 7),
          ('2^26 samples at 4096, no overlap, K 4', 4096, 1, 1 << 26, 2.5, 4)]

for name, nfft, nstreams, per_stream, nw, K in SHAPES:
    n = nstreams * per_stream
    x = s.capture(n)
    psd = torch.empty((nstreams, nfft), dtype=torch.float32, device=dev)
    rows = torch.empty((3, nstreams, nfft), dtype=torch.float32, device=dev)
    plan = ctx.mtm_plan(nfft, nw=nw, ntapers=K)

    def run_psd():
        plan.exec_dev(x.data_ptr(), per_stream, psd.data_ptr(), nstreams=nstreams)

    def run_ftest():
        plan.ftest_dev(x.data_ptr(), per_stream, nstreams, per_stream, rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr())

    s.report(name, [('PSD (exec_dev)', run_psd, plan), ('F-test (ftest_dev, three rows)', run_ftest, plan)], 32, 'PSD', n)
    # the two agree where they overlap: (line S + resid (K - 1) / scale) / K against the density PSD needs the tapers' unit
    # energy only, which Slepian tapers have
    S = float(np.sum(plan.tapers.astype(np.float64).sum(axis=1) ** 2))
    tie = (rows[1].double() * S + rows[2].double() * (K - 1)) / K
    s.say('  (line S + resid (K - 1)) / K against the PSD row: worst bin %.1e' % (tie - psd.double()).abs().div(psd.double()).max().item())
    plan.close()
    del x, psd, rows

s.finish('kernel <N, T, KEEP, sy / p in registers, sums in registers>', ('mtm_ftest_kernel<', 'ftest_finalize_kernel'))
