#!/usr/bin/env python3
"""The polyphase filter-bank launch (oth_welch_pfb_dev: csrc/welchpfb.hip + the finalize launch; one row per stream) on an
MI355X against two comparators in the SAME session:

(a) what a user had before it: oth_welch_exec_dev on a Welch plan of P N points with the prototype as its window and
    noverlap = P N - N, of which every P-th bin is the filter bank's row (the decimation is not timed) - P times the
    transforms at P times the length;
(b) the fold's cost: oth_welch_sk_dev on the same N-point plan and hop, given as many segments as the filter bank has
    frames - the same body (whole segments per workgroup, fft_lds, running rows) with one read per sample where the fold
    reads a frame's P N samples.

Shapes: 4096 points with P = 4 and 8, 1024 points with P = 16; for each, one capture of 2^24 samples at hop N, and 64
streams of 8 frames.  The fold asks for 8 P bytes per new sample, of which 8 (P - 1) are re-reads of the run's earlier
frames; algorithmically a sample is needed once (8 bytes).  No gate: the figures and their ratios are the result.
-> profiles/welch_pfb_time.txt

Whole steps are timed with HIP events on one stream, ten calls per timed window, the arms alternating inside one session
after two warm-up steps each; the median over the repetitions is reported per call.

usage: welch_pfb_time.py [reps] [--out FILE]
"""
import numpy as np
import torch

from stat_time import Session

from ofdm_tools import _hip, windows  # noqa: E402 - stat_time sets the path

s = Session('welch_pfb_time.txt', reps=20, inner=10)
ctx, dev, say, reps, INNER = s.ctx, s.dev, s.say, s.reps, s.inner

say('%s, %d repetitions of %d calls per shape, the arms alternating' % (s.library, reps, INNER))
for nfft, P in ((4096, 4), (4096, 8), (1024, 16)):
    L = nfft * P
    h = windows.pfb_prototype(nfft, P).astype(np.float32)
    for name, nstreams, M in (('one capture of 2^24 samples', 1, ((1 << 24) - L) // nfft + 1), ('64 streams of 8 frames', 64, 8)):
        per = L + (M - 1) * nfft      # samples of a stream: exactly M frames
        x = s.capture(nstreams * per, dc=0j)
        bank = ctx.welch_plan(nfft, noverlap=0, window=windows.get_window('hann', nfft))
        bank.set_prototype(h, P)
        long = ctx.welch_plan(L, nperseg=L, noverlap=L - nfft, window=h)
        row = torch.empty(nstreams * nfft, dtype=torch.float32, device=dev)
        rows_long = torch.empty(nstreams * L, dtype=torch.float32, device=dev)
        rows_sk = torch.empty(2 * nstreams * nfft, dtype=torch.float32, device=dev)

        def run_bank():
            bank.pfb_dev(x.data_ptr(), per, nstreams, per, row.data_ptr())

        def run_long():
            long.exec_dev(x.data_ptr(), per, rows_long.data_ptr(), nstreams=nstreams, stream_stride=per)

        def run_sk():      # M segments of the same streams
            bank.sk_dev(x.data_ptr(), M * nfft, nstreams, per, rows_sk.data_ptr(), rows_sk.data_ptr() + 4 * nstreams * nfft)

        cands = [('pfb_dev (the fold, one %d-point transform per frame)' % nfft, run_bank, bank),
                 ('(a) exec_dev on the %d-point plan, window h' % L, run_long, long),
                 ('(b) sk_dev on the %d-point plan, %d segments' % (nfft, M), run_sk, bank)]
        try:
            run_long()
        except _hip.HipError as e:      # a shape the long plan does not take: the fold has no such limit
            say('')
            say('%d points, P = %d: %s: (a) is refused (%s)' % (nfft, P, name, e))
            for plan in (bank, long):
                plan.close()
            continue
        med = s.report('%d points, P = %d: %s (M = %d)' % (nfft, P, name, M), cands, 56, 'filter bank', n=nstreams * M * nfft)
        run_bank()
        run_long()
        torch.cuda.synchronize(dev)
        a, b = row.view(nstreams, nfft).double(), rows_long.view(nstreams, L)[:, ::P].double()
        say('  rows, fold against every %d-th bin of (a): worst bin %.1e relative' % (P, ((a - b).abs() / b).max().item()))
        say('  bytes per step: %.0f MiB of capture; the fold asks for %.0f MiB (8 P per new sample)' %
            (8.0 * nstreams * per / 2 ** 20, 8.0 * nstreams * M * L / 2 ** 20))
        say('  (a) / fold: x%.2f   fold / (b): x%.2f' % (med[cands[1][0]] / med[cands[0][0]], med[cands[0][0]] / med[cands[2][0]]))
        bank.close()
        long.close()
        del x, row, rows_long, rows_sk
s.finish('kernel <N, T>', ('welch_pfb_kernel<', 'lag_finalize_kernel'), key=lambda name, length: (length, name))
