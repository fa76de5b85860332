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
import torch

from stat_time import TONES, Session

s = Session('mtm_jackknife_time.txt')
ctx, dev = s.ctx, s.dev
s.say('%s, %d repetitions per shape, the two steps alternating' % (s.library, s.reps))

# name, two channels, nfft, streams, samples per stream, NW, K
SHAPES = [('one channel: 64 x 16384 x 1 segment, K 7', False, 16384, 64, 16384, 4.0, 7),
          ('one channel: 2^24 samples at 4096, no overlap, K 4', False, 4096, 1, 1 << 24, 2.5, 4),
          ('two channels: 16384 x 1 segment, K 7', True, 16384, 1, 16384, 4.0, 7),
          ('two channels: 2^24 samples at 4096, no overlap, K 4', True, 4096, 1, 1 << 24, 2.5, 4)]

for name, two, nfft, nstreams, per_stream, nw, K in SHAPES:
    n = nstreams * per_stream
    x = s.capture(n)
    y = s.capture(n, 2027, ((0.35, 0.1234), TONES[2])) if two else None
    ref = torch.empty((5, nstreams, nfft), dtype=torch.float32, device=dev)
    rows = torch.empty((4, nstreams, nfft), dtype=torch.float32, device=dev)
    plan = (ctx.mtm_csd_plan if two else ctx.mtm_plan)(nfft, nw=nw, ntapers=K)

    if two:
        def run_base():
            plan.csd_exec_dev(x.data_ptr(), y.data_ptr(), per_stream, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref[4].data_ptr())

        def run_jack():
            plan.csd_jackknife_dev(x.data_ptr(), y.data_ptr(), per_stream, rows[1].data_ptr(), rows[0].data_ptr(), rows[2].data_ptr(),
                                   rows[3].data_ptr())
        cands = [('CSD (csd_exec_dev, four rows)', run_base, plan), ('jackknife (csd_jackknife_dev, four rows)', run_jack, plan)]
    else:
        def run_base():
            plan.exec_dev(x.data_ptr(), per_stream, ref[0].data_ptr(), nstreams=nstreams)

        def run_jack():
            plan.jackknife_dev(x.data_ptr(), per_stream, nstreams, per_stream, rows[0].data_ptr(), rows[1].data_ptr())
        cands = [('PSD (exec_dev)', run_base, plan), ('jackknife (jackknife_dev, lnsd + PSD)', run_jack, plan)]
    s.report(name, cands, 42, 'first', n)
    # the two agree where they overlap, bit for bit: the PSD row, or the coherence
    same = torch.equal(rows[0], ref[4]) if two else torch.equal(rows[1], ref[0])
    s.say('  the %s row of the jackknife step against the first step: %s' % ('Cxy' if two else 'PSD', 'the same bits' if same else 'DIFFERENT'))
    plan.close()
    del x, y, ref, rows

s.finish('kernel <N, T, KEEP, [two LDS buffers,] sums in registers>', ('jack_kernel<', 'jack_finalize_kernel'), 72,
         key=lambda name, length: ('mtmcsd' in name, length))
