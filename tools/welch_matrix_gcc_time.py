#!/usr/bin/env python3
"""The generalized cross-correlation of the spectral matrix's pairs (oth_welch_matrix_gcc_dev: the matrix family's averaging
and totals launches, then csrc/matgcc.hip, one workgroup per pair) on an MI355X against what a user had before it, in the
SAME session: the matrix rows copied to the host and, per pair, the PHAT weighting, numpy.fft.ifft, the argmax and the parabola
in numpy.  Four arms: matrix_dev with gcoh alone (the family's two shared launches and its one-thread-per-bin determinant: the
cheapest complete call of the family), matrix_gcc_dev with both outputs, with the peaks alone, and the host composition.
Hann, no overlap, detrend on; 4096 points; C = 2, 4 and 8 (1, 6 and 28 pairs); upsample 1 and 4; 8 segments per channel.
No gate: the figures are the result.  The gcc stage is 1 ... 28 workgroups on a 256-CU part: it is bound by the latency of one
workgroup's passes over its LDS tile, not by throughput, and its time does not grow with the pairs.
-> profiles/welch_matrix_gcc_time.txt

Whole steps are timed with HIP events on one stream, the arms alternating inside one session after two warm-up steps each;
the median over the repetitions is reported per call.  The host arm's window holds its copy and its host arithmetic: the
closing event is recorded after them.  Next to them the kernel time of a call (oth_ctx_get_timing: the sum over its
timed windows) of the first two arms: their difference is the gcc stage less the determinant launch it stands in for, which
at 8 channels costs about as much.  The stage's own duration comes from a kernel trace (the profile's last block, added by
hand from `rocprofv3 --kernel-trace` over 30 calls per shape).

usage: welch_matrix_gcc_time.py [reps] [--out FILE]
"""
import numpy as np
import torch

from stat_time import Session

from ofdm_tools import _hip, windows  # noqa: E402 - stat_time sets the path

s = Session('welch_matrix_gcc_time.txt', reps=5, inner=1)
ctx, dev, say, reps = s.ctx, s.dev, s.say, s.reps
NFFT = 4096


def kernel_ms(fn, calls=10):
    """the sum over a call's launches of their time between events, per call"""
    fn()
    ctx.sync()
    ctx.set_timing(True)
    ctx.get_timing(reset=True)
    for _ in range(calls):
        fn()
    ctx.sync()
    ms, launches = ctx.get_timing(reset=True)
    ctx.set_timing(False)
    return ms / calls, launches // calls


say('%s, %d repetitions per shape, the arms alternating' % (s.library, reps))
for C in (2, 4, 8):
    n = 8 * NFFT
    # a common white signal, channel c later by 3 c samples, under independent unit noise: every pair has a peak to find
    rng = np.random.default_rng(2026 + C)
    common = (rng.standard_normal(n + 64) + 1j * rng.standard_normal(n + 64)) / np.sqrt(2.0)
    noise = (rng.standard_normal((C, n)) + 1j * rng.standard_normal((C, n))) / np.sqrt(2.0)
    host_x = np.stack([common[32 - 3 * c:32 - 3 * c + n] for c in range(C)]) + noise
    x = torch.from_numpy(np.ascontiguousarray(host_x, np.complex64).view(np.float32).reshape(-1)).to(dev)
    pairs, P = C * (C + 1) // 2, C * (C - 1) // 2
    packed = torch.empty((pairs, NFFT, 2), dtype=torch.float32, device=dev)
    gcoh = torch.empty(NFFT, dtype=torch.float32, device=dev)
    peak = torch.empty((P, 3), dtype=torch.float32, device=dev)
    for U in (1, 4):
        NI = U * NFFT
        L = NI // 2 - 1
        plans = [ctx.welch_plan(NFFT, noverlap=0, window=windows.get_window('hann', NFFT)) for _ in range(4)]
        rows = torch.empty((P, 2 * L + 1, 2), dtype=torch.float32, device=dev)
        host = {}

        def run_mat():
            plans[0].matrix_dev(x.data_ptr(), n, C, n, None, gcoh.data_ptr())

        def run_gcc():
            plans[1].matrix_gcc_dev(x.data_ptr(), n, C, n, 'phat', None, U, L, rows.data_ptr(), peak.data_ptr())

        def run_peaks():
            plans[2].matrix_gcc_dev(x.data_ptr(), n, C, n, 'phat', None, U, L, None, peak.data_ptr())

        def run_host():
            plans[3].matrix_dev(x.data_ptr(), n, C, n, packed.data_ptr(), None)
            S = _hip.unpack_matrix(ctx.d2h(packed.data_ptr(), (pairs, NFFT), np.complex64), C).astype(np.complex128)
            out = np.empty((P, 3))
            for p, (a, b) in enumerate(_hip.gcc_pairs(C)):
                mag = np.abs(S[a, b])
                spec = np.zeros(NI, np.complex128)
                k = np.arange(-NFFT // 2, NFFT // 2)
                spec[k % NI] = np.where(mag > 0, S[a, b] / np.where(mag > 0, mag, 1.0), 0.0)[k % NFFT]
                R = np.fft.ifft(spec)[np.arange(-L, L + 1) % NI] * (NI / max(np.count_nonzero(mag), 1))
                y = np.abs(R)
                i = int(np.argmax(y))
                d = 0.0
                if 0 < i < 2 * L:
                    den = y[i - 1] - 2.0 * y[i] + y[i + 1]
                    d = 0.5 * (y[i - 1] - y[i + 1]) / den if den < 0 else 0.0
                out[p] = (i - L + d) / U, y[i], np.angle(R[i])
            host['peak'] = out

        cands = [('matrix_dev, gcoh alone', run_mat, plans[0]), ('matrix_gcc_dev, rows and peaks', run_gcc, plans[1]),
                 ('matrix_gcc_dev, peaks alone', run_peaks, plans[2]), ('matrix_dev + copy + numpy per pair', run_host, plans[3])]
        med = s.report('%d points, C = %d (%d pairs), upsample %d (NI = %d), %d segments' % (NFFT, C, P, U, NI, n // NFFT), cands, 36,
                       'matrix_dev')
        torch.cuda.synchronize(dev)
        got = peak.cpu().numpy().astype(np.float64)
        say('  device against the host composition, worst pair: delay %.1e sample, |R| %.1e, arg R %.1e rad'
            % tuple(float(np.max(np.abs(got[:, j] - host['peak'][:, j]))) for j in range(3)))
        k_mat, l_mat = kernel_ms(run_mat)
        k_gcc, l_gcc = kernel_ms(run_gcc)
        say('  kernel time per call: matrix_dev %.1f us in %d timed windows (the second holds totals and determinant), matrix_gcc_dev %.1f us in %d: the gcc stage less the determinant launch %+.1f us'
            % (1e3 * k_mat, l_mat, 1e3 * k_gcc, l_gcc, 1e3 * (k_gcc - k_mat)))
        say('  whole calls: matrix_gcc_dev less matrix_dev %+.3f ms; host composition / matrix_gcc_dev: x%.0f'
            % (med[cands[1][0]] - med[cands[0][0]], med[cands[3][0]] / med[cands[1][0]]))
        for p in plans:
            p.close()
        del rows
    del x, packed, gcoh, peak
s.finish('kernel <NI, threads>', ('mat_gcc_kernel<', 'mat_finalize_kernel', 'mat_det_kernel'), key=lambda name, length: (name.split('<')[0], length))
