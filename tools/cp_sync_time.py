#!/usr/bin/env python3
"""The cyclic-prefix synchroniser (oth_cp_sync_dev: csrc/cpsync.hip - the fold launch, the totals launch, the window launch;
gamma, phi and est per stream and hypothesis) on an MI355X against what a user had before it, in the SAME session and on the
same device-resident capture: per hypothesis the torch composition
    z = x[Tu:Tu + S Ts] * conj(x[:S Ts])                  F = z.view(S, Ts).sum(0)
    p = |x|^2;  e = (p[:S Ts] + p[Tu:Tu + S Ts]) / 2      G = e.view(S, Ts).sum(0)
    Gamma, Phi = differences of cumsum over the row repeated once,   theta = argmax(|Gamma| - rho Phi)
which moves, per (sample, hypothesis), 24 bytes for the product, 8 for its sum, 12 for e, 4 for its sum and (once per capture)
12 for p: 48 and more, in about ten launches and with float32 prefix sums.  The fused call asks for 16 - the 8-byte base
sample from HBM, the 8-byte lagged sample, which is the base sample of a later symbol, out of L2 - and writes rows only.
Shapes: 2^26 samples, one stream, (64, 16);  the same at (1024, 256);  64 streams of 2^18 samples, (64, 16);  the first with
4 hypotheses.  No gate: both figures and their ratio are the result.  -> profiles/cp_sync_time.txt

Whole steps are timed with HIP events on one stream, the arms alternating inside one session after two warm-up steps each;
the median over the repetitions is reported per call.

usage: cp_sync_time.py [reps] [--out FILE]
"""
import torch

from stat_time import Session

s = Session('cp_sync_time.txt', reps=20, inner=4)
ctx, dev, say, reps = s.ctx, s.dev, s.say, s.reps
RHO = 1.0
PEAK = 8e12      # bytes per second


class Arm(object):
    """what Session.run_arms asks of a plan"""

    def __init__(self, text):
        self.text = text

    def last_recipe(self):
        return self.text


def composition(xc, p, hyps, keep):
    """xc [streams, n] complex64, p = |xc|^2 -> keep[h] = (Gamma, Phi, theta) per hypothesis"""
    n = xc.shape[1]
    for h, (tu, cp) in enumerate(hyps):
        ts = tu + cp
        S = (n - tu) // ts
        z = xc[:, tu:tu + S * ts] * torch.conj(xc[:, :S * ts])
        F = z.view(-1, S, ts).sum(1)
        G = (0.5 * (p[:, :S * ts] + p[:, tu:tu + S * ts])).view(-1, S, ts).sum(1)
        cF = torch.cumsum(torch.cat([torch.zeros_like(F[:, :1]), F, F[:, :cp]], 1), 1)
        cG = torch.cumsum(torch.cat([torch.zeros_like(G[:, :1]), G, G[:, :cp]], 1), 1)
        gamma, phi = cF[:, cp:cp + ts] - cF[:, :ts], cG[:, cp:cp + ts] - cG[:, :ts]
        keep[h] = (gamma, phi, torch.argmax(gamma.abs() - RHO * phi, 1))


say('%s, %d repetitions of %d calls per shape, the arms alternating' % (s.library, reps, s.inner))
for name, nstreams, n, hyps in (('2^26 samples, one stream, (64, 16)', 1, 1 << 26, [(64, 16)]),
                                ('2^26 samples, one stream, (1024, 256)', 1, 1 << 26, [(1024, 256)]),
                                ('64 streams of 2^18 samples, (64, 16)', 64, 1 << 18, [(64, 16)]),
                                ('2^26 samples, one stream, (64, 16) (64, 8) (128, 32) (128, 16)', 1, 1 << 26, [(64, 16), (64, 8), (128, 32), (128, 16)])):
    x = s.capture(nstreams * n, dc=0j)
    xc = torch.view_as_complex(x.view(nstreams * n, 2)).view(nstreams, n)
    H = len(hyps)
    row = max(tu + cp for tu, cp in hyps)
    gamma = torch.empty((nstreams, H, row), dtype=torch.complex64, device=dev)
    phi = torch.empty((nstreams, H, row), dtype=torch.float32, device=dev)
    est = torch.empty((nstreams, H, 4), dtype=torch.float32, device=dev)
    keep = [None] * H

    def run_fused():
        ctx.cp_sync_dev(x.data_ptr(), n, hyps, est.data_ptr(), gamma.data_ptr(), phi.data_ptr(), row_stride=row, rho=RHO, nstreams=nstreams, stride=n)

    def run_composition():
        composition(xc, xc.real * xc.real + xc.imag * xc.imag, hyps, keep)

    cands = [('composition (torch: product, sums, cumsum window, argmax)', run_composition, Arm('torch')),
             ('fused (cp_sync_dev: gamma, phi, est)', run_fused, Arm('cpsync: fold, totals, window'))]
    med = s.report(name, cands, 58, 'composition')
    work = float(nstreams) * n * H
    for label, _, _ in cands:
        say('  %-58s %5.1f %% of 8 TB/s at 16 bytes per (sample, hypothesis)' % (label, 100.0 * 16.0 * work / (med[label] * 1e-3) / PEAK))
    say('  bytes asked for per (sample, hypothesis): composition 48 + 12 / %d, fused 16; capture %.0f MiB' % (H, 8.0 * nstreams * n / 2 ** 20))
    torch.cuda.synchronize(dev)
    worst_g, worst_t = 0.0, 0
    for h, (tu, cp) in enumerate(hyps):
        ts = tu + cp
        g_c, _, t_c = keep[h]
        scale = g_c.abs().max().item()
        worst_g = max(worst_g, ((gamma[:, h, :ts] - g_c).abs().max().item()) / scale)
        worst_t = max(worst_t, int((est[:, h, 0].long() - t_c).abs().max().item()))
    say('  fused against the composition: Gamma within %.1e of its largest entry, theta differs by at most %d' % (worst_g, worst_t))
    say('  fused / composition: x%.2f' % (med[cands[1][0]] / med[cands[0][0]]))
    del x, xc, gamma, phi, est, keep

s.finish('kernel <tile, threads>', ('cps_fold_kernel<', 'cps_total_kernel', 'cps_window_kernel'), key=lambda name, length: (length, name))
