#!/usr/bin/env python3
"""The cyclic-spectrum launch (oth_welch_cyclic_dev: csrc/welchcyc.hip + its finalize launch; scf, coh and PSD rows at A
cycle frequencies) on an MI355X, two tables:

default       against what a user had before it, in the SAME session: A times (a torch mix of the capture by
              e^{-j 2 pi alpha n} into a second buffer - the phasors are built once, outside the timed window, which favours
              this arm - then oth_csd_exec_dev on a Welch plan of the same parameters, which takes one stream), at 4096
              points with A = 4:  2^24 samples,  and 64 streams of 8 segments.  Both arms run WITHOUT detrend: on a
              detrending plan the composition takes the mean off the mixed segment - the capture's component at alpha -
              and so empties the bins around -alpha of U (its coherence rows are off by up to 0.4 there), while the fused
              call detrends the segment before the mix, as the definition says.
              No gate: both figures and their ratio are the result.  -> profiles/welch_cyclic_time.txt
--ab          the three builds of welchcyc.hip against each other (OTH_CYC_GROUP=1: one cycle frequency per workgroup, two
              transforms per (segment, alpha); OTH_CYC_GROUP=2 / 4: up to GA, 1 + GA transforms per segment) at 256, 4096,
              8192 and 16384 points, A = 1, 2, 3, 4 and 16, for 64 streams of 8 segments and for one stream of 2^24 samples.
              -> profiles/welch_cyclic_ab.txt

Whole steps are timed with HIP events on one stream, ten calls per timed window, the arms alternating inside one session
after two warm-up steps each; the median over the repetitions is reported per call.

usage: welch_cyclic_time.py [reps] [--ab] [--out FILE]
"""
import os

import numpy as np
import torch

from stat_time import Session

from ofdm_tools import _hip, windows  # noqa: E402 - stat_time sets the path

s = Session({'--ab': 'welch_cyclic_ab.txt', None: 'welch_cyclic_time.txt'}, reps=20, inner=10, flags=('--ab',))
ctx, dev, say, reps, INNER = s.ctx, s.dev, s.say, s.reps, s.inner


def alphas_for(A):
    """the first is CP-OFDM's 1 / 80; the rest spread over (-0.5, 0.5), none on a bin"""
    return np.array([1.0 / 80.0] + [((0.0123456789 + 0.137 * k) % 1.0) - 0.5 for k in range(1, A)])[:A]


def cyclic_plan(nfft, alphas, group=None, detrend=_hip.DETREND_CONSTANT):
    old = os.environ.pop('OTH_CYC_GROUP', None)
    if group is not None:
        os.environ['OTH_CYC_GROUP'] = str(group)      # read when the plan is created
    try:
        plan = ctx.welch_plan(nfft, noverlap=0, window=windows.get_window('hann', nfft), detrend=detrend)
    finally:
        os.environ.pop('OTH_CYC_GROUP', None)
        if old is not None:
            os.environ['OTH_CYC_GROUP'] = old
    plan.set_cycles(alphas)
    return plan


def ab_table():
    say('%s: the three builds of welch_cyc_kernel, %d repetitions of %d calls per shape, the arms alternating' % (s.library, reps, INNER))
    say('ms per call (kernel + finalize launch, scf + coh + psd rows); the ratios are to group 1')
    say('')
    say('%-34s %3s  %9s %9s %9s  %6s %6s   %s' % ('shape', 'A', 'group 1', 'group 2', 'group 4', 'g2/g1', 'g4/g1', 'W and workgroups per CU'))
    for nfft in (256, 4096, 8192, 16384):
        for name, nstreams, per_stream in (('64 streams x 8 segments', 64, 8 * nfft), ('one stream of 2^24 samples', 1, 1 << 24)):
            x = s.capture(nstreams * per_stream, dc=0j)
            for A in (1, 2, 3, 4, 16):
                alphas = alphas_for(A)
                out = torch.empty((3 * A + 1) * nstreams * nfft, dtype=torch.float32, device=dev)
                coh, scf, psd = out.data_ptr(), out.data_ptr() + 4 * A * nstreams * nfft, out.data_ptr() + 12 * A * nstreams * nfft
                plans = {g: cyclic_plan(nfft, alphas, g) for g in (1, 2, 4)}

                def arm(g):
                    return lambda: plans[g].cyclic_dev(x.data_ptr(), per_stream, nstreams, per_stream, coh, scf, psd)

                med, low, recipes = s.run_arms([('g%d' % g, arm(g), plans[g]) for g in (1, 2, 4)])
                shape = ' | '.join('%s %s' % (recipes[k].split(' W=')[1].split()[0], recipes[k].split(' bpc=')[1]) for k in ('g1', 'g2', 'g4'))
                say('%-34s %3d  %9.4f %9.4f %9.4f  %6.2f %6.2f   %s' % ('%d: %s' % (nfft, name), A, med['g1'], med['g2'], med['g4'], med['g2'] / med['g1'],
                                                                         med['g4'] / med['g1'], shape))
                for p in plans.values():
                    p.close()
                del out
            del x


def time_table():
    say('%s, %d repetitions of %d calls per shape, the arms alternating' % (s.library, reps, INNER))
    nfft, A = 4096, 4
    alphas = alphas_for(A)
    for name, nstreams, per_stream in (('2^24 samples at 4096 points, no overlap, A = 4', 1, 1 << 24),
                                       ('64 streams of 8 x 4096 points, A = 4', 64, 8 * 4096)):
        n = nstreams * per_stream
        x = s.capture(n, dc=0j)
        xc = torch.view_as_complex(x.view(n, 2))
        t = torch.arange(per_stream, dtype=torch.float64, device=dev)
        # the phasors in double, once: [A][n], every stream's time starting at 0
        ph = torch.stack([torch.polar(torch.ones_like(t), -2.0 * np.pi * torch.remainder(a * t, 1.0)).to(torch.complex64).repeat(nstreams)
                          for a in alphas])
        y = torch.empty_like(xc)
        fused = cyclic_plan(nfft, alphas, detrend=_hip.DETREND_NONE)
        welch = ctx.welch_plan(nfft, noverlap=0, window=windows.get_window('hann', nfft), detrend=_hip.DETREND_NONE)
        out = torch.empty((3 * A + 1) * nstreams * nfft, dtype=torch.float32, device=dev)
        coh, scf, psd = out.data_ptr(), out.data_ptr() + 4 * A * nstreams * nfft, out.data_ptr() + 12 * A * nstreams * nfft
        rows = torch.empty((A, nstreams, 5, nfft), dtype=torch.float32, device=dev)      # pxx, pyy, pxy re / im, cxy

        def run_fused():
            fused.cyclic_dev(x.data_ptr(), per_stream, nstreams, per_stream, coh, scf, psd)

        def run_composition():
            for a in range(A):
                torch.mul(xc, ph[a], out=y)
                for i in range(nstreams):
                    r = rows[a, i].data_ptr()
                    welch.csd_exec_dev(x.data_ptr() + 8 * i * per_stream, y.data_ptr() + 8 * i * per_stream, per_stream,
                                       r, r + 4 * nfft, r + 8 * nfft, r + 16 * nfft)

        cands = [('composition (A x (torch mix + csd_exec_dev per stream))', run_composition, welch), ('fused (cyclic_dev: scf, coh, psd)', run_fused, fused)]
        med = s.report(name, cands, 56, 'composition')
        base = med[cands[0][0]]
        # the arms agree (no detrend: file header)
        c_f = out[:A * nstreams * nfft].view(nstreams, A, nfft).permute(1, 0, 2).double()
        c_c = rows[:, :, 4, :].double()
        say('  coherence rows, fused against the composition: worst bin %.1e' % (c_f - c_c).abs().max().item())
        say('  fused / composition: x%.2f' % (med[cands[1][0]] / base))
        fused.close()
        welch.close()
        del x, xc, ph, y, out, rows


if '--ab' in s.flags:
    ab_table()
else:
    time_table()
s.finish('kernel <N, T, GA, KEEP, two LDS buffers, sums in registers>', ('welch_cyc_kernel<', 'cyc_finalize_kernel'),
         key=lambda name, length: (length, name))
