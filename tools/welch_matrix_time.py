#!/usr/bin/env python3
"""The spectral-matrix launch (oth_welch_matrix_dev: csrc/welchmat.hip + its two finalize launches; the packed matrix rows and
gcoh of C coherent channels) on an MI355X against what a user had before it, in the SAME session: C (C - 1) / 2 calls of
oth_csd_exec_dev, one per pair of channels, on the same device-resident capture (pxx, pyy, pxy and cxy per pair; the
determinant would still have to be formed on the host, which is not timed).  Hann, no overlap, detrend on; 1024 and 4096
points; C = 2, 4 and 8; one capture of 2^22 samples per channel and a short one of 8 segments.  Per segment the composition
transforms 2 channels per pair, C (C - 1) of them, the fused call C.  No gate: both figures and their ratio are the result.
-> profiles/welch_matrix_time.txt

Whole steps are timed with HIP events on one stream, ten calls per timed window, the arms alternating inside one session
after two warm-up steps each; the median over the repetitions is reported per call.

usage: welch_matrix_time.py [reps] [--out FILE]
"""
import torch

from stat_time import Session

from ofdm_tools import windows  # noqa: E402 - stat_time sets the path

s = Session('welch_matrix_time.txt', reps=20, inner=10)
ctx, dev, say, reps, INNER = s.ctx, s.dev, s.say, s.reps, s.inner

say('%s, %d repetitions of %d calls per shape, the arms alternating' % (s.library, reps, INNER))
for nfft in (1024, 4096):
    for C in (2, 4, 8):
        for name, n in (('2^22 samples per channel', 1 << 22), ('8 segments per channel', 8 * nfft)):
            x = s.capture(C * n, dc=0j)
            pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]
            fused = ctx.welch_plan(nfft, noverlap=0, window=windows.get_window('hann', nfft))
            two = ctx.welch_plan(nfft, noverlap=0, window=windows.get_window('hann', nfft))
            packed = torch.empty((C * (C + 1) // 2, nfft, 2), dtype=torch.float32, device=dev)
            gcoh = torch.empty(nfft, dtype=torch.float32, device=dev)
            rows = torch.empty((len(pairs), 5, nfft), dtype=torch.float32, device=dev)      # pxx, pyy, pxy re im, cxy per pair
            chan = [x.data_ptr() + 8 * n * c for c in range(C)]

            def run_fused():
                fused.matrix_dev(x.data_ptr(), n, C, n, packed.data_ptr(), gcoh.data_ptr())

            def run_composition():
                for k, (a, b) in enumerate(pairs):
                    base = rows[k].data_ptr()
                    two.csd_exec_dev(chan[a], chan[b], n, base, base + 4 * nfft, base + 8 * nfft, base + 16 * nfft)

            cands = [('composition (%d x csd_exec_dev)' % len(pairs), run_composition, two), ('fused (matrix_dev: S, gcoh)', run_fused, fused)]
            med = s.report('%d points, C = %d, %s: %d segments' % (nfft, C, name, n // nfft), cands, 34, 'composition')
            torch.cuda.synchronize(dev)
            pxy = torch.view_as_complex(rows[0, 2:4].reshape(nfft, 2).contiguous()).to(torch.complex128)
            size = torch.sqrt(rows[0, 0].double() * rows[0, 1].double())
            got = torch.view_as_complex(packed[1].contiguous()).to(torch.complex128)
            say('  S_01, fused against the composition: worst bin %.1e of sqrt(S_00 S_11); transforms per segment %d against %d'
                % (((got - pxy).abs() / size).max().item(), C, 2 * len(pairs)))
            say('  fused / composition: x%.2f' % (med[cands[1][0]] / med[cands[0][0]]))
            fused.close()
            two.close()
            del x, packed, gcoh, rows
s.finish('kernel <N, T, capacity, KEEP, state in registers>', ('welch_mat_kernel<', 'mat_finalize_kernel', 'mat_det_kernel'),
         key=lambda name, length: (length, name))
