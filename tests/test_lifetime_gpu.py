"""Who owns what on the host side of the C ABI: every device buffer, pinned host buffer and event of a context, plan,
chain or any-length table set lives in a holder of csrc/abi_mem.h, and oth__debug_live_resources counts the live ones.
A round that creates, uses and closes one of everything must leave the counts where a first, identical round left them
(the context's caches - twiddles, scratch, slice bounds, timing events - are warm by then), closing the context must
return them to what they were before it existed, and a refused construction or workspace leaves nothing behind.

The counts are process-wide and other test modules keep contexts alive in this process, so they are read as deltas."""
import gc

import numpy as np
import pytest

from oracle import ref_cpu as R
from test_hip_parity import RTOL, check_single_rows, hann, hip, relerr  # noqa: F401 - hip is a fixture

pytestmark = pytest.mark.gpu

X = R.synth_iq(4 * 65536, 2024)
Y = R.synth_iq(4096 + 15 * 2048, 2025)
UNSUPPORTED, NOMEM = -3, -4


def live(hip):
    gc.collect()      # plans and chains other tests dropped without close() go now, not in the middle of a round
    return hip.live_resources()


def welch_256_matches_the_oracle(c):
    plan = c.welch_plan(256, window=hann(256))
    x = X[:256 * 9]
    _, ref = R.welch_np(x, fs=1.0, nperseg=256, nfft=256)
    assert relerr(plan.exec(x), ref) < RTOL
    plan.close()


def one_round(c, hip):
    """One of everything, created, used once and closed."""
    c.set_timing(True)
    # 4096 points, Hann, 50 % overlap, detrend, 16 segments: d_fd, the pilot, the partials, the output ring, the staging
    # ring, d_stream
    x = X[:4096 + 15 * 2048]
    _, ref = R.welch_np(x, fs=1.0, nperseg=4096, nfft=4096)
    p = c.welch_plan(4096, window=hann(4096))
    assert relerr(p.exec(x), ref) < RTOL and p.last_nseg == 16
    assert relerr(p.wait(p.exec_async(x)), ref) < RTOL
    p.accumulate(x[:3000])                                          # (d_stream regrows around a live carry)
    p.accumulate(x[3000:])
    assert relerr(p.finalize(), ref) < RTOL and p.last_nseg == 16
    pxx, pyy, _, _ = p.csd(x, Y)                                    # the two-channel run
    assert np.all(pxx > 0) and np.all(pyy > 0)
    # one call of each statistic family: their tables (d_cyc_tap, d_lags, d_pfb_h, d_doa_steer) and workspaces (d_cyc_ws,
    # d_lag_means, d_mat_ws, d_mat_totals, d_doa_basis) are counted too
    sk, psd = p.sk(x, return_psd=True)
    assert np.all(psd > 0) and np.all(np.isfinite(sk)) and p.last_nseg == 16
    p.set_cycles([0.0, 0.0125])
    assert np.all(p.cyclic(x)[1] >= 0)
    p.set_lags([0, 64])
    assert np.all(p.caf(x) > 0)
    p.set_prototype(np.ones(2 * 4096, np.float32))
    assert np.all(p.pfb(x) > 0)
    xc = X[:3 * len(x)].reshape(3, len(x))
    S, gcoh = p.matrix(xc)
    assert np.all(S[0, 0].real > 0) and np.all(gcoh >= 0)
    assert np.all(p.matrix_eig(xc, of='G')[0][0] > 0)
    p.set_steering(np.arange(6.0).reshape(2, 3), 0.0)
    assert all(np.all(r > 0) for r in p.matrix_doa(xc, nsrc=1, loading=1e-2).values())
    assert np.all(p.matrix_gcc(xc, maxlag=8)[1] > 0) and p.last_nseg == 16
    p.set_average('median')                                         # d_rows, d_med, d_msel
    assert np.all(p.exec(x) > 0)
    p.close()
    p = c.welch_plan(256, nperseg=128, window=hann(128), average='median')      # ... and rows_any
    assert np.all(p.exec(X[:4096]) > 0)
    p.close()
    for n, nseg in ((16384, 4), (65536, 3), (1021, 5), (10007, 3)):      # d_fd1x; d_wpm; chirp, midtab, mean; ws
        p = c.welch_plan(n, window=hann(n))
        assert np.all(p.exec(X[:n + (nseg - 1) * (n - n // 2)]) > 0) and p.last_nseg == nseg
        p.close()
    p = c.mtm_plan(256, nw=4.0, ntapers=7)
    assert np.all(p.exec(X[:2048]) > 0)
    assert np.all(p.adaptive(X[:2048]) > 0)                         # d_mtm_lam; d_adapt_ws and d_ftest_ws from 1024 points on
    assert np.all(p.ftest(X[:2048]) >= 0)
    assert np.all(p.jackknife(X[:2048]) > 0)                        # d_jack_tot
    p.close()
    p = c.mtm_csd_plan(1024, nw=3.0, ntapers=5)                     # d_mtm_ws's smaller builds; the two-channel jackknife
    assert np.all(p.adaptive(X[:4096]) > 0) and np.all(p.ftest(X[:4096]) >= 0)
    assert np.all(p.csd(X[:4096], Y[:4096])[0] > 0)
    assert np.all(p.csd_jackknife(X[:4096], Y[:4096])[1] > 0)
    p.close()
    ch = c.chain(1024, None, True, hip.EPI_MAG2, 1)                 # h_tail, h_in, h_row, the events
    ch.set_iir_log(0.3, -90.0)
    ch.set_peak_hold(True)
    assert ch.push(X[:4096])[1] == 4
    assert ch.wait(ch.push_async(X[4096:8192]))[1] == 4
    assert ch.push(X[:512])[1] == 0 and ch.push(X[512:1024])[1] == 1
    ch.close()
    rows = np.abs(X[:8 * 1024].reshape(8, 1024)).astype(np.float32) ** 2
    d = c.alloc(rows.nbytes)                                        # (oth_dev_alloc: the caller's memory, not counted)
    c.h2d(d, rows)
    for nch in (4, 9):                                              # the bounds cache regrows
        lo = np.arange(nch) * 100
        _, noise, power = c.scan_decide_dev(d, 8, 1024, 16, 2.0, lo, lo + 64)
        assert np.all(noise > 0) and power.shape == (8, nch)
    c.free(d)
    for L in (256, 1000):                                           # the context scratch; a table set of the call's own
        ref = R.xcorr(X[:200], X[50:250], L)
        assert np.max(np.abs(c.xcorr(X[:200], X[50:250], L) - ref)) / np.max(ref) < 1e-5
    c.get_timing()                                                  # the timing pairs go back to the context's pool
    c.set_timing(False)


def test_round_trip_returns_every_resource(hip):
    before = live(hip)
    c = hip.Context(0)
    assert live(hip)[0] > before[0]
    one_round(c, hip)
    first = live(hip)
    one_round(c, hip)
    assert live(hip) == first
    c.close()
    assert live(hip) == before


def test_refused_constructions_leave_nothing_behind(hip):
    import torch
    before = live(hip)
    c = hip.Context(0)
    welch_256_matches_the_oracle(c)                                 # (warms the 256-point twiddles)
    base = live(hip)
    with pytest.raises(hip.HipError) as ei:                         # a length any_describe refuses
        c.welch_plan((1 << 20) + 1)
    assert ei.value.code == UNSUPPORTED and live(hip) == base
    welch_256_matches_the_oracle(c)
    with pytest.raises(hip.HipError) as ei:                         # not a power of two
        c.mtm_plan(96, nw=4.0)
    assert ei.value.code == UNSUPPORTED and live(hip) == base
    welch_256_matches_the_oracle(c)
    # a median exec whose rows workspace (nstreams x nseg x nfft x 4 B) is twice the card's memory: hipMalloc refuses it
    # and nothing is written or launched
    nstreams, N = 64, 256
    total = torch.cuda.get_device_properties(0).total_memory
    nsamples = -(-2 * total // (4 * nstreams * N)) * N
    assert nstreams * (nsamples // N) * N * 4 >= 2 * total
    p = c.welch_plan(N, noverlap=0, window=hann(N), average='median')
    d_in, d_out = c.alloc(8 * N), c.alloc(4 * nstreams * N)
    held = live(hip)
    with pytest.raises(hip.HipError) as ei:
        p.exec_dev(d_in, nsamples, d_out, nstreams=nstreams, stream_stride=nsamples)
    assert ei.value.code == NOMEM and 'rows workspace' in str(ei.value)
    assert live(hip) == held
    p.close()
    c.free(d_in)
    c.free(d_out)
    assert live(hip) == base
    welch_256_matches_the_oracle(c)
    c.close()
    assert live(hip) == before


def test_growth_keeps_the_leftover(hip):
    """1.5 vectors, then 3.5: the second push completes the half vector the first left on the device while its staging
    and row buffers regrow."""
    N = 1024
    c = hip.Context(0)
    ch = c.chain(N, None, True, hip.EPI_MAG2_OVER_N2, 1)            # spectrum_sensor_v2's chain
    r1, n1 = ch.push(X[:N + N // 2])
    r2, n2 = ch.push(X[N + N // 2:5 * N])
    assert (n1, n2) == (1, 4)
    check_single_rows(np.concatenate([r1, r2]), R.chain_sensor_v2(X[:5 * N], N))
    ch.close()
    c.close()
