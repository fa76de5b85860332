#!/usr/bin/env python3
"""The eigenvalue launch of the spectral matrix (oth_welch_matrix_eig_dev: the matrix family's averaging and totals launches,
then csrc/mateig.hip's per-bin Jacobi) on an MI355X against what a user had before it, in the SAME session: matrix_dev, the
packed rows copied to the host, unpack_matrix and numpy.linalg.eigh per bin.  Four arms: matrix_dev alone (its difference from
the eigenvalue arm is the eigen stage's cost against the determinant stage's), matrix_eig_dev with the eigenvalues only, with
the vector too, and the host composition.  Hann, no overlap, detrend on; 1024, 4096 and 16384 points; C = 2, 4 and 8; a short
capture of 8 segments per channel and one of 2^20 samples per channel.  No gate: the figures and their ratios are the result.
-> profiles/welch_matrix_eig_time.txt

Whole steps are timed with HIP events on one stream, three calls per timed window, the arms alternating inside one session
after two warm-up steps each; the median over the repetitions is reported per call.  The host arm's window holds its copy and
its host arithmetic: the closing event is recorded after them.

usage: welch_matrix_eig_time.py [reps] [--out FILE]
"""
import numpy as np
import torch

from stat_time import Session

from ofdm_tools import _hip, windows  # noqa: E402 - stat_time sets the path

s = Session('welch_matrix_eig_time.txt', reps=10, inner=3)
ctx, dev, say, reps, INNER = s.ctx, s.dev, s.say, s.reps, s.inner

say('%s, %d repetitions of %d calls per shape, the arms alternating' % (s.library, reps, INNER))
for nfft in (1024, 4096, 16384):
    for C in (2, 4, 8):
        for name, n in (('8 segments per channel', 8 * nfft), ('2^20 samples per channel', 1 << 20)):
            x = s.capture(C * n, dc=0j)
            pairs = C * (C + 1) // 2
            plans = [ctx.welch_plan(nfft, noverlap=0, window=windows.get_window('hann', nfft)) for _ in range(4)]
            packed = torch.empty((pairs, nfft, 2), dtype=torch.float32, device=dev)
            eig = torch.empty((C, nfft), dtype=torch.float32, device=dev)
            vec = torch.empty((C, nfft, 2), dtype=torch.float32, device=dev)
            host = {}

            def run_matrix():
                plans[0].matrix_dev(x.data_ptr(), n, C, n, packed.data_ptr(), None)

            def run_eig():
                plans[1].matrix_eig_dev(x.data_ptr(), n, C, n, 'S', eig.data_ptr(), None)

            def run_eig_vec():
                plans[2].matrix_eig_dev(x.data_ptr(), n, C, n, 'S', eig.data_ptr(), vec.data_ptr())

            def run_host():
                plans[3].matrix_dev(x.data_ptr(), n, C, n, packed.data_ptr(), None)
                S = _hip.unpack_matrix(ctx.d2h(packed.data_ptr(), (pairs, nfft), np.complex64), C)
                host['eig'] = np.linalg.eigh(np.moveaxis(S, 2, 0))[0]

            cands = [('matrix_dev alone (S rows)', run_matrix, plans[0]), ('matrix_eig_dev, eigenvalues', run_eig, plans[1]),
                     ('matrix_eig_dev, with the vector', run_eig_vec, plans[2]),
                     ('matrix_dev + copy + numpy eigh', run_host, plans[3])]
            med = s.report('%d points, C = %d, %s: %d segments' % (nfft, C, name, n // nfft), cands, 34, 'matrix_dev alone')
            torch.cuda.synchronize(dev)
            got, want = eig.cpu().numpy().astype(np.float64), host['eig'][:, ::-1].T.astype(np.float64)
            say('  eigenvalues, device against the host composition: worst bin %.1e of the trace' % np.max(np.abs(got - want) / want.sum(axis=0)))
            say('  eigen stage less determinant stage: %+.3f ms; with the vector %+.3f ms; host composition / matrix_eig_dev: x%.1f'
                % (med[cands[1][0]] - med[cands[0][0]], med[cands[2][0]] - med[cands[0][0]], med[cands[3][0]] / med[cands[1][0]]))
            for p in plans:
                p.close()
            del x, packed, eig, vec
s.finish('kernel <capacity, threads, vector>', ('mat_eig_kernel<', 'mat_finalize_kernel', 'mat_det_kernel'), key=lambda name, length: (length, name))
