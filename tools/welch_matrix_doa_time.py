#!/usr/bin/env python3
"""The direction spectra of the spectral matrix (oth_welch_matrix_doa_dev: the matrix family's averaging and totals launches,
csrc/mateig.hip's basis build, then csrc/matdoa.hip over bins x directions) on an MI355X against what a user had before
them, in the SAME session: the matrix rows copied to the host, numpy.linalg.eigh per bin, the steering vectors and the three
spectra in numpy over bins x directions.  Four arms: matrix_eig_dev with the vector (the Jacobi the basis build repeats),
matrix_doa_dev with all three spectra, with MUSIC alone, and the host composition.  Hann, no overlap, detrend on; 4096 points;
C = 4 and 8; D = 16, 181 and 1024 directions of a half-wavelength line array; 8 segments per channel.  No gate: the figures
and their ratios are the result.
-> profiles/welch_matrix_doa_time.txt

Whole steps are timed with HIP events on one stream, the arms alternating inside one session after two warm-up steps each;
the median over the repetitions is reported per call.  The host arm's window holds its copy and its host arithmetic: the
closing event is recorded after them.

usage: welch_matrix_doa_time.py [reps] [--out FILE]
"""
import numpy as np
import torch

from stat_time import Session

from ofdm_tools import _hip, ofdm_cr_tools, windows  # noqa: E402 - stat_time sets the path

s = Session('welch_matrix_doa_time.txt', reps=5, inner=1)
ctx, dev, say, reps = s.ctx, s.dev, s.say, s.reps
NFFT, FC, NSRC, LOADING = 4096, 2.0, 2, 1e-2
K = np.arange(NFFT)
FK = np.where(K < NFFT // 2, K, K - NFFT) / float(NFFT)

say('%s, %d repetitions per shape, the arms alternating' % (s.library, reps))
for C in (4, 8):
    n = 8 * NFFT
    x = s.capture(C * n, dc=0j)
    pairs = C * (C + 1) // 2
    packed = torch.empty((pairs, NFFT, 2), dtype=torch.float32, device=dev)
    eig = torch.empty((C, NFFT), dtype=torch.float32, device=dev)
    vec = torch.empty((C, NFFT, 2), dtype=torch.float32, device=dev)
    for D in (16, 181, 1024):
        delays = ofdm_cr_tools.ula_delays(C, np.linspace(-90.0, 90.0, D), 0.5, FC)
        plans = [ctx.welch_plan(NFFT, noverlap=0, window=windows.get_window('hann', NFFT)) for _ in range(4)]
        for p in plans[1:3]:
            p.set_steering(delays, FC)
        rows = [torch.empty((D, NFFT), dtype=torch.float32, device=dev) for _ in range(3)]
        host = {}

        def run_eig():
            plans[0].matrix_eig_dev(x.data_ptr(), n, C, n, 'S', eig.data_ptr(), vec.data_ptr())

        def run_doa():
            plans[1].matrix_doa_dev(x.data_ptr(), n, C, n, 'S', NSRC, LOADING, *[r.data_ptr() for r in rows])

        def run_music():
            plans[2].matrix_doa_dev(x.data_ptr(), n, C, n, 'S', NSRC, LOADING, None, None, rows[2].data_ptr())

        def run_host():
            plans[3].matrix_dev(x.data_ptr(), n, C, n, packed.data_ptr(), None)
            S = _hip.unpack_matrix(ctx.d2h(packed.data_ptr(), (pairs, NFFT), np.complex64), C).astype(np.complex128)
            lam, V = np.linalg.eigh(np.moveaxis(S, 2, 0))
            lam, V = np.maximum(lam[:, ::-1], 0.0), V[:, :, ::-1]
            w = np.exp(2j * np.pi * (np.mod(FC * delays, 1.0)[:, None, :] + FK[None, :, None] * delays[:, None, :]))
            p = np.abs(np.einsum('jci,djc->dji', np.conj(V), w)) ** 2
            delta = LOADING * lam.sum(axis=1) / C
            host['bartlett'] = (lam[None] * p).sum(axis=2) / C ** 2
            host['capon'] = 1.0 / (p / (lam + delta[:, None])[None]).sum(axis=2)
            host['music'] = C / p[:, :, NSRC:].sum(axis=2)

        cands = [('matrix_eig_dev, with the vector', run_eig, plans[0]), ('matrix_doa_dev, three spectra', run_doa, plans[1]),
                 ('matrix_doa_dev, MUSIC alone', run_music, plans[2]), ('matrix_dev + copy + numpy', run_host, plans[3])]
        med = s.report('%d points, C = %d, D = %d directions, %d segments' % (NFFT, C, D, n // NFFT), cands, 34, 'matrix_eig_dev')
        torch.cuda.synchronize(dev)
        worst = [float(np.max(np.abs(r.cpu().numpy().astype(np.float64) / host[k] - 1.0))) for k, r in zip(('bartlett', 'capon', 'music'), rows)]
        say('  device against the host composition, worst bin and direction, relative: bartlett %.1e, capon %.1e, music %.1e' % tuple(worst))
        say('  direction stage (three spectra less matrix_eig_dev): %+.3f ms, %.2f us per direction; host composition / matrix_doa_dev: x%.0f'
            % (med[cands[1][0]] - med[cands[0][0]], 1e3 * (med[cands[1][0]] - med[cands[0][0]]) / D, med[cands[3][0]] / med[cands[1][0]]))
        for p in plans:
            p.close()
        del rows
    del x, packed, eig, vec
s.finish('kernel <capacity, threads>', ('mat_doa_kernel<', 'mat_eig_basis_kernel<', 'mat_eig_kernel<'), key=lambda name, length: (name.split('<')[0], length))
