#!/usr/bin/env python3
"""The cyclic-autocorrelation launch (oth_welch_caf_dev: csrc/welchlag.hip + its finalize launch; caf rows and r at L lags)
on an MI355X, two tables:

default       against what a user had before it, in the SAME session: L times (a torch product x[n + tau] conj(x[n]) of
              the capture into an [L][n] buffer), then oth_welch_exec_dev on a Welch plan of the same parameters with the
              products as streams.  4096 points, Hann, no overlap, detrend on:  one capture of 2^24 samples with L = 1, 4
              and 16;  64 streams of 8 segments with L = 4.  Per (sample, lag) the composition moves 32 bytes - two 8-byte
              reads and an 8-byte write for the product, then Welch's 8-byte read; the fused call asks for 8 bytes of
              lagged samples per (sample, lag) and 8 bytes of base samples per (sample, group of lags), and writes rows only.
              No gate: both figures and their ratio are the result.  -> profiles/welch_caf_time.txt
--ab          the two builds of welchlag.hip against each other (OTH_LAG_GROUP=1: one lag per workgroup; OTH_LAG_GROUP=2:
              two, the base segment loaded once for both) at 256, 1024, 4096, 8192 and 16384 points, L = 2, 4, 5
              and 16, for 64 streams of 8 segments and for one stream of 2^24 samples.  -> profiles/welch_caf_ab.txt

Whole steps are timed with HIP events on one stream, ten calls per timed window, the arms alternating inside one session
after two warm-up steps each; the median over the repetitions is reported per call.

usage: welch_caf_time.py [reps] [--ab] [--out FILE]
"""
import os

import torch

from stat_time import Session

from ofdm_tools import _hip, windows  # noqa: E402 - stat_time sets the path

s = Session({'--ab': 'welch_caf_ab.txt', None: 'welch_caf_time.txt'}, reps=20, inner=10, flags=('--ab',))
ctx, dev, say, reps, INNER = s.ctx, s.dev, s.say, s.reps, s.inner
GROUPS = (1, 2)
PAD = 2048      # the largest lag of lags_for


def lags_for(L):
    """lag 0 and CP-OFDM's 64 first, then the other candidate lengths and lags between them"""
    return ([0, 64, 128, 256, 512, 1024, 2048, 32, 16, 48, 96, 192, 384, 768, 1536, 80][:L] if L > 1 else [64])


def caf_plan(nfft, lags, group=None):
    old = os.environ.pop('OTH_LAG_GROUP', None)
    if group is not None:
        os.environ['OTH_LAG_GROUP'] = str(group)      # read when the plan is created
    try:
        plan = ctx.welch_plan(nfft, noverlap=0, window=windows.get_window('hann', nfft))
    finally:
        os.environ.pop('OTH_LAG_GROUP', None)
        if old is not None:
            os.environ['OTH_LAG_GROUP'] = old
    plan.set_lags(lags)
    return plan


def ab_table():
    say('%s: the two builds of welch_lag_kernel, %d repetitions of %d calls per shape, the arms alternating' % (s.library, reps, INNER))
    say('ms per call (kernel + finalize launch, caf rows + r); the ratio is to group 1')
    say('')
    say('%-34s %3s  %9s %9s  %6s   %s' % ('shape', 'L', 'group 1', 'group 2', 'g2/g1', 'W and workgroups per CU'))
    for nfft in (256, 1024, 4096, 8192, 16384):
        for name, nstreams, segs in (('64 streams x 8 segments', 64, 8), ('one stream of 2^24 samples', 1, ((1 << 24) - PAD) // nfft)):
            stride = segs * nfft + PAD      # room for the largest lag behind the segments
            x = s.capture(nstreams * stride, dc=0j)
            for L in (2, 4, 5, 16):
                lags = lags_for(L)
                per_stream = segs * nfft + max(lags)
                out = torch.empty((nfft + 2) * L * nstreams, dtype=torch.float32, device=dev)
                caf, r = out.data_ptr(), out.data_ptr() + 4 * nfft * L * nstreams
                plans = {g: caf_plan(nfft, lags, g) for g in GROUPS}

                def arm(g):
                    return lambda: plans[g].caf_dev(x.data_ptr(), per_stream, nstreams, stride, caf, r)

                med, low, recipes = s.run_arms([('g%d' % g, arm(g), plans[g]) for g in GROUPS])
                shape = ' | '.join('%s %s' % (recipes[k].split(' W=')[1].split()[0], recipes[k].split(' bpc=')[1]) for k in ('g1', 'g2'))
                say('%-34s %3d  %9.4f %9.4f  %6.2f   %s' % ('%d: %s' % (nfft, name), L, med['g1'], med['g2'], med['g2'] / med['g1'], shape))
                for p in plans.values():
                    p.close()
                del out
            del x


def time_table():
    say('%s, %d repetitions of %d calls per shape, the arms alternating' % (s.library, reps, INNER))
    nfft = 4096
    for name, nstreams, segs, L in (('2^24 samples at 4096 points, no overlap, L = 1', 1, 4095, 1),
                                    ('2^24 samples at 4096 points, no overlap, L = 4', 1, 4095, 4),
                                    ('2^24 samples at 4096 points, no overlap, L = 16', 1, 4095, 16),
                                    ('64 streams of 8 x 4096 points, L = 4', 64, 8, 4)):
        lags = lags_for(L)
        stride = segs * nfft + PAD
        per = segs * nfft                   # the samples of a stream's segments
        per_stream = per + max(lags)        # what the fused call is given: the same M segments
        x = s.capture(nstreams * stride, dc=0j)
        xc = torch.view_as_complex(x.view(nstreams * stride, 2)).view(nstreams, stride)
        z = torch.empty((L, nstreams, per), dtype=torch.complex64, device=dev)
        fused, welch = caf_plan(nfft, lags), ctx.welch_plan(nfft, noverlap=0, window=windows.get_window('hann', nfft))
        out = torch.empty((nfft + 2) * L * nstreams, dtype=torch.float32, device=dev)
        caf, r = out.data_ptr(), out.data_ptr() + 4 * nfft * L * nstreams
        rows = torch.empty((L, nstreams, nfft), dtype=torch.float32, device=dev)
        base = torch.conj(xc[:, :per])

        def run_fused():
            fused.caf_dev(x.data_ptr(), per_stream, nstreams, stride, caf, r)

        def run_composition():
            for l, tau in enumerate(lags):
                torch.mul(xc[:, tau:tau + per], base, out=z[l])
            welch.exec_dev(z.data_ptr(), per, rows.data_ptr(), nstreams=L * nstreams, stream_stride=per)

        cands = [('composition (L x torch product, then exec_dev on L x streams)', run_composition, welch), ('fused (caf_dev: caf rows, r)', run_fused, fused)]
        med = s.report(name, cands, 62, 'composition')
        G = -(-L // int(fused.last_recipe().split(' group=')[1].split()[0]))
        n = nstreams * per
        say('  bytes per call: composition %.0f MiB (32 per sample and lag); fused %.0f MiB asked for (8 per sample and lag, 8 per sample and '
            'group), %.0f MiB of capture behind them' % (32.0 * n * L / 2 ** 20, 8.0 * n * (L + G) / 2 ** 20, 8.0 * n / 2 ** 20))
        c_f = out[:nfft * L * nstreams].view(nstreams, L, nfft).permute(1, 0, 2).double()
        say('  caf rows, fused against the composition: worst bin %.1e relative' % ((c_f - rows.double()).abs() / rows.double()).max().item())
        say('  fused / composition: x%.2f' % (med[cands[1][0]] / med[cands[0][0]]))
        fused.close()
        welch.close()
        del x, xc, z, out, rows, base


if '--ab' in s.flags:
    ab_table()
else:
    time_table()
s.finish('kernel <N, T, GL, KEEP, sums in registers>', ('welch_lag_kernel<', 'lag_finalize_kernel'), key=lambda name, length: (length, name))
