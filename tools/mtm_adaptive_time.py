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
import torch

from stat_time import Session

s = Session('mtm_adaptive_time.txt')
ctx, dev = s.ctx, s.dev
s.say('%s, %d repetitions per shape, the two launches alternating' % (s.library, s.reps))

SHAPES = [('64 x 16384 x 1 segment, K 7', 16384, 64, 16384, 4.0, 7),
          ('2^24 samples at 4096, no overlap, K 4', 4096, 1, 1 << 24, 2.5, 4)]

for name, nfft, nstreams, per_stream, nw, K in SHAPES:
    n = nstreams * per_stream
    x = s.capture(n)
    psd = torch.empty((nstreams, nfft), dtype=torch.float32, device=dev)
    rows = torch.empty((2, nstreams, nfft), dtype=torch.float32, device=dev)
    plan = ctx.mtm_plan(nfft, nw=nw, ntapers=K)

    def run_psd():
        plan.exec_dev(x.data_ptr(), per_stream, psd.data_ptr(), nstreams=nstreams)

    def run_adaptive():
        plan.adaptive_dev(x.data_ptr(), per_stream, nstreams, per_stream, rows[0].data_ptr(), rows[1].data_ptr(), iters=4)

    s.report(name, [('PSD (exec_dev)', run_psd, plan), ('adaptive (adaptive_dev, 4 iterations)', run_adaptive, plan)], 38, 'PSD', n)
    # where the two stand to each other: on this input (noise and three tones, no empty band) the adaptive weights stay near 1
    ratio = rows[0].double() / psd.double()
    s.say('  adaptive / PSD row: %.3f ... %.3f; dof %.2f ... %.2f of 2 K = %d'
          % (ratio.min().item(), ratio.max().item(), rows[1].min().item(), rows[1].max().item(), 2 * K))
    plan.close()
    del x, psd, rows

s.finish('kernel <N, T, KEEP, eigenspectra in LDS>', ('mtm_adapt_kernel<', 'adapt_finalize_kernel'))
