"""GPU tests of the cyclic-prefix synchroniser (oth_cp_sync / _dev, csrc/cpsync.hip, Context.cp_sync) against the float64
oracle of tests/cp_sync_oracle.py (its fold form, which tests/test_cp_sync_cpu.py holds to the definition at 1e-12 of A).
The gates, with the project's RTOL = 1e-4 and A[t] = Gamma's sum with |z| in place of z - the size every rounding of Gamma is
relative to:
    |Gamma - oracle| <= RTOL A[t]                                   |Phi - oracle| <= RTOL Phi[t]
    theta: the oracle's Lambda at the returned theta lies within RTOL ((A + rho Phi)[theta] + (A + rho Phi)[theta_oracle]) of
           the oracle's maximum - each of the two Lambdas the device compared is off by at most RTOL (A + rho Phi) of its own
           entry, so this is what a correct maximum search can miss by; at most 2 RTOL (A + rho Phi).  Equal outright on the
           detection cases.
    |eps - oracle| <= RTOL A / (2 pi |Gamma|) + 1e-6               |rho_hat - oracle| <= 2 RTOL A / Phi
    |Lambda[theta] - oracle| <= RTOL (A + rho Phi)                  (eps, rho_hat and Lambda against the oracle at the returned theta)
Every test prints its readings as fractions of these gates.
Measured on an MI355X, worst readings of this file as fractions of the gates (DESIGN.md 4.24 repeats them): the 11 parity
shapes and their S - 1 runs Gamma 7.1e-4 (7.1e-8 of A), Phi 8.0e-4, eps 4.1e-4, rho_hat 2.5e-4, Lambda 2.1e-4; five hypotheses
in one call 7.4e-4, 7.8e-4, 3.3e-5, 2.2e-4, 1.7e-4 and the bytes of five calls; OTH_CPS_WG 1, 3 and unset 7.4e-4, 8.3e-4,
7.6e-6, 1.5e-4, 2.4e-5; the long run Gamma and Phi 6.0e-3 (6.0e-7 of A, where a float32 running sum is off by 2.4e-5 after
4096 of the 65536 symbols); the channelizer's 64 rows 2.7e-4, 6.7e-4, 4.6e-4, 1.3e-4, 3.1e-4; after the refusals 5.1e-4,
5.3e-4, 7.7e-6, 1.4e-4, 1.4e-4.  theta was the oracle's own in every case (reading 0).  Detection, (64, 16) x 200 symbols,
seed 0: theta 37 = theta0 at 10 and at -3 dB, eps 0.19920 and 0.19900 against 0.2, rho_hat 0.908 and 0.330 against 0.909 and
0.334; ofdm_blind_sync on the 0 dB capture of the caf tests: (64, 16), theta 0, eps 0.0013, rho_hat 0.492 - the oracle's."""
import ctypes as C
import gc

import numpy as np
import pytest

import cp_sync_oracle as PO
from stat_support import forced_env
from test_cp_sync_cpu import ESTIMATOR_CASES, PARITY_CASES, parity_input
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
SENTINEL = np.float32(-7.25)
BEHIND = 64


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_dev(ctx, xs, hyps, rho=1.0, gap=0, pad=5, rows=True):
    """cp_sync_dev on the streams xs [nstreams, n], `gap` samples of NaN behind each, into buffers full of SENTINEL with
    BEHIND floats of it behind each and rows `pad` entries wider than the largest Ts
    -> (gamma [nstreams, nhyp, row_stride] complex64, phi, est [nstreams, nhyp, 4], nsym); the columns behind a hypothesis'
    Ts and the floats behind the buffers are checked to hold the sentinel"""
    xs = np.atleast_2d(xs)
    ns, n = xs.shape
    nhyp = len(hyps)
    stride = n + gap
    row = max(tu + cp for tu, cp in hyps) + pad
    buf = np.full((ns, stride), np.nan + 1j * np.nan, np.complex64)
    buf[:, :n] = xs
    ng, nph, ne = 2 * ns * nhyp * row, ns * nhyp * row, ns * nhyp * 4
    d_x, d_g, d_p, d_e = ctx.alloc(buf.nbytes), ctx.alloc(4 * (ng + BEHIND)), ctx.alloc(4 * (nph + BEHIND)), ctx.alloc(4 * (ne + BEHIND))
    try:
        ctx.h2d(d_x, buf)
        for d, count in ((d_g, ng), (d_p, nph), (d_e, ne)):
            ctx.h2d(d, np.full(count + BEHIND, SENTINEL, np.float32))
        nsym = ctx.cp_sync_dev(d_x, n, hyps, d_e, d_g if rows else 0, d_p if rows else 0, row_stride=row, rho=rho, nstreams=ns, stride=stride)
        g, p, e = (ctx.d2h(d, (count + BEHIND,), np.float32) for d, count in ((d_g, ng), (d_p, nph), (d_e, ne)))
    finally:
        for d in (d_x, d_g, d_p, d_e):
            ctx.free(d)
    assert np.all(g[ng:] == SENTINEL) and np.all(p[nph:] == SENTINEL) and np.all(e[ne:] == SENTINEL)
    gamma, phi, est = g[:ng].view(np.complex64).reshape(ns, nhyp, row), p[:nph].reshape(ns, nhyp, row), e[:ne].reshape(ns, nhyp, 4)
    for h, (tu, cp) in enumerate(hyps):
        assert np.all(gamma[:, h, tu + cp:].view(np.float32) == SENTINEL) and np.all(phi[:, h, tu + cp:] == SENTINEL)
        if not rows:
            assert np.all(gamma[:, h].view(np.float32) == SENTINEL) and np.all(phi[:, h] == SENTINEL)
    return gamma, phi, est, nsym


def check_rows(gamma, phi, ref, what):
    """the Gamma and Phi gates on one row -> their worst readings as fractions of the gates"""
    assert gamma.dtype == np.complex64 and phi.dtype == np.float32 and gamma.shape == phi.shape == ref['A'].shape
    assert np.all(np.isfinite(gamma.view(np.float32))) and np.all(np.isfinite(phi))
    eg = np.abs(gamma.astype(np.complex128) - ref['gamma'])
    ep = np.abs(phi.astype(np.float64) - ref['phi'])
    wg = float(np.max(np.where(eg == 0.0, 0.0, eg / (RTOL * np.maximum(ref['A'], 1e-300)))))
    wp = float(np.max(np.where(ep == 0.0, 0.0, ep / (RTOL * np.maximum(ref['phi'], 1e-300)))))
    assert wg <= 1.0 and wp <= 1.0, (what, wg, wp)
    return wg, wp


def check_est(est, ref, rho, what, exact=False):
    """the theta, eps, rho_hat and Lambda gates on one est row -> their worst readings as fractions of the gates"""
    assert est.dtype == np.float32 and est.shape == (4,) and np.all(np.isfinite(est))
    theta = int(est[0])
    assert theta == est[0] and 0 <= theta < len(ref['A'])
    theta_o, _, _, _, lam = PO.estimate(ref['gamma'], ref['phi'], rho)
    size = ref['A'] + rho * ref['phi']
    gate_t = RTOL * (size[theta] + size[theta_o])
    wt = 0.0 if theta == theta_o else float((lam[theta_o] - lam[theta]) / gate_t)
    assert wt <= 1.0 and gate_t <= 2.0 * RTOL * float(size.max()), (what, theta, theta_o, wt)
    if exact:
        assert theta == theta_o, (what, theta, theta_o)
    g, p, a = ref['gamma'][theta], ref['phi'][theta], ref['A'][theta]
    if abs(g) == 0.0:      # all-zero rows: est is exact
        assert est[1] == 0.0 and est[2] == 0.0 and est[3] == 0.0
        return wt, 0.0, 0.0, 0.0
    d = abs(float(est[1]) - np.angle(g) / (2.0 * np.pi))
    we = float(min(d, 1.0 - d) / (RTOL * a / (2.0 * np.pi * abs(g)) + 1e-6))      # (eps is an angle: -1/2 and 1/2 are neighbours)
    wr = float(abs(float(est[2]) - abs(g) / p) / (2.0 * RTOL * a / p))
    wl = float(abs(float(est[3]) - lam[theta]) / (RTOL * size[theta]))
    assert we <= 1.0 and wr <= 1.0 and wl <= 1.0, (what, we, wr, wl)
    return wt, we, wr, wl


def check_all(gamma, phi, est, x, tu, cp, rho, what, ref=None, exact=False):
    """every gate on the rows of one (stream, hypothesis) -> the six readings"""
    ref = ref or PO.fold(x, tu, cp)
    ts = tu + cp
    out = check_rows(gamma[:ts], phi[:ts], ref, what) + check_est(est, ref, rho, what, exact)
    print('cp_sync %s: Gamma %.1e Phi %.1e theta %.1e eps %.1e rho_hat %.1e Lambda %.1e of their gates' % ((what,) + out))
    return out


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tu,cp,S,streams', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, tu, cp, S, streams):
    """nsamples = S Ts + Tu exactly; + Ts - 1 (the same S, the same bytes: nothing behind the last symbol is read); - 1 gives
    S - 1.  Several streams lie stream_stride > nsamples apart with NaN in the gaps, and the host form gives stream 0's bytes."""
    ts = tu + cp
    n0 = S * ts + tu
    xs = np.stack([parity_input(11 + s, tu, cp, n0 + ts - 1) for s in range(streams)])
    rho = 0.75
    gap = 0 if streams == 1 else 37
    gamma, phi, est, nsym = run_dev(ctx, xs[:, :n0], [(tu, cp)], rho, gap=gap)
    assert nsym.tolist() == [S]
    for s in range(streams):
        check_all(gamma[s, 0], phi[s, 0], est[s, 0], xs[s, :n0], tu, cp, rho, '(%d, %d) S %d stream %d' % (tu, cp, S, s))
    longer = run_dev(ctx, xs, [(tu, cp)], rho, gap=gap)
    assert longer[3].tolist() == [S] and all(same_bytes(a, b) for a, b in zip(longer[:3], (gamma, phi, est)))
    hg, hp, he, hn = ctx.cp_sync(xs[0, :n0], [(tu, cp)], rho=rho)
    assert hn.tolist() == [S] and same_bytes(hg[0], gamma[0, 0, :ts]) and same_bytes(hp[0], phi[0, 0, :ts]) and same_bytes(he[0], est[0, 0])
    if S > 1:
        g1, p1, e1, n1 = run_dev(ctx, xs[:, :n0 - 1], [(tu, cp)], rho, gap=gap)
        assert n1.tolist() == [S - 1]
        for s in range(streams):
            check_all(g1[s, 0], p1[s, 0], e1[s, 0], xs[s, :n0 - 1], tu, cp, rho, '(%d, %d) S %d stream %d' % (tu, cp, S - 1, s))
    else:
        with pytest.raises(hip.HipError) as ei:
            ctx.cp_sync(xs[0, :n0 - 1], [(tu, cp)], rho=rho)
        assert ei.value.code == INVALID


# ---- 2. hypotheses ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,cap,hyps', [(1200, None, [(64, 16), (8, 1), (256, 64), (100, 7), (300, 20)]),
                                        (20000, 7, [(64, 16), (8, 1), (256, 64), (100, 7), (1000, 73)])])
def test_five_hypotheses_in_one_call_give_the_bytes_of_five_calls(ctx, hip, n, cap, hyps):
    """A hypothesis' bytes depend on its own runs of symbols alone (W: include/ofdm_tools_hip.h).  n = 1200: no S above 132, so
    that the 1320 runs of two streams and five hypotheses fit a device of 256 CUs and W = S alone and together; n = 20000
    under OTH_CPS_WG = 7.  The fold runs on other thread counts alone and together (the launch's largest Ts decides), which
    changes no sum."""
    xs = np.stack([parity_input(5 + s, 64, 16, n) for s in range(2)])
    with forced_env('OTH_CPS_WG', cap):
        gamma, phi, est, nsym = run_dev(ctx, xs, hyps, 0.5, gap=3)
        assert nsym.tolist() == [PO.nsym(n, tu, cp) for tu, cp in hyps]
        for h, (tu, cp) in enumerate(hyps):
            g1, p1, e1, n1 = run_dev(ctx, xs, [(tu, cp)], 0.5, gap=3, pad=5 + max(a + b for a, b in hyps) - tu - cp)
            assert n1.tolist() == [nsym[h]]
            assert same_bytes(g1[:, 0], gamma[:, h]) and same_bytes(p1[:, 0], phi[:, h]) and same_bytes(e1[:, 0], est[:, h])
            for s in range(2):
                check_all(gamma[s, h], phi[s, h], est[s, h], xs[s], tu, cp, 0.5, '%d hypotheses, (%d, %d) stream %d' % (len(hyps), tu, cp, s))
    # est alone: gamma and phi left out
    _, _, e2, _ = run_dev(ctx, xs, hyps[:3], 0.5, gap=3, rows=False)
    if cap is None:
        assert same_bytes(e2, est[:, :3])


# ---- 3. the work split --------------------------------------------------------------------------------------------------------

def test_every_work_split_is_inside_the_gates_and_repeats_its_bytes(ctx, hip):
    tu, cp, S = 64, 16, 200
    x = parity_input(21, tu, cp, S * 80 + tu)
    ref = PO.fold(x, tu, cp)
    for cap in (1, 3, None):
        with forced_env('OTH_CPS_WG', cap):
            a = run_dev(ctx, x, [(tu, cp)], 1.0)
            b = run_dev(ctx, x, [(tu, cp)], 1.0)
        assert all(same_bytes(u, v) for u, v in zip(a[:3], b[:3]))      # the same shape twice: the same bytes
        check_all(a[0][0, 0], a[1][0, 0], a[2][0, 0], x, tu, cp, 1.0, 'OTH_CPS_WG %s' % cap, ref=ref)
    # S = 2 under a cap above it: two runs of one symbol
    x2 = parity_input(22, tu, cp, 2 * 80 + tu)
    with forced_env('OTH_CPS_WG', 5):
        g, p, e, n = run_dev(ctx, x2, [(tu, cp)], 1.0)
    assert n.tolist() == [2]
    check_all(g[0, 0], p[0, 0], e[0, 0], x2, tu, cp, 1.0, 'S 2 under OTH_CPS_WG 5')


# ---- 4. a long run ------------------------------------------------------------------------------------------------------------

def test_a_long_run_of_one_workgroup_keeps_its_digits(ctx, hip):
    """x = 1.1 + 0j, (16, 4), 65536 symbols in ONE run: every z is 1.21 and a plain float32 running sum of 65536 of them is off
    by 6.1e-4 of the sum - six times the gate.  Blocks of 64 symbols in float32, the blocks in double, stay below 3e-6."""
    tu, cp, S = 16, 4, 65536
    x = np.full(S * 20 + tu, 1.1 + 0j, np.complex64)
    with forced_env('OTH_CPS_WG', 1):
        g, p, e, n = run_dev(ctx, x, [(tu, cp)], 1.0)
    assert n.tolist() == [S]
    ref = PO.fold(x, tu, cp)
    out = check_rows(g[0, 0, :20], p[0, 0, :20], ref, 'long run')
    plain = np.float32(0.0)
    for _ in range(4096):      # what a float32 running sum loses over the first 4096 symbols alone
        plain = np.float32(plain + np.float32(1.1) * np.float32(1.1))
    print('cp_sync long run: Gamma %.1e Phi %.1e of their gates; a float32 running sum is off by %.1e after 4096 symbols' %
          (out + (abs(float(plain) / (4096 * float(np.float32(1.1)) ** 2) - 1.0),)))
    assert e[0, 0, 1] == 0.0 and abs(float(e[0, 0, 2]) - 1.0) <= 2 * RTOL


# ---- 5. the channelizer's rows ------------------------------------------------------------------------------------------------

def test_the_rows_of_the_channelizer_as_they_are(ctx, hip):
    nchan, decim, taps, frames = 64, 32, 8, 400
    hyps = [(32, 8), (64, 16)]
    rng = np.random.default_rng(77)
    n = taps * nchan + (frames - 1) * decim
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0) + PO.cp_ofdm_sync(7, 256, 64, n // 320 + 1, 0.0, 11, 0.1, noise=False)[:n])
    x = x.astype(np.complex64)
    chan = ctx.channelizer(nchan, decim, taps)
    stride = frames + 9
    d_x, d_rows, d_est = ctx.alloc(x.nbytes), ctx.alloc(8 * nchan * stride), ctx.alloc(4 * nchan * len(hyps) * 4)
    d_g, d_p = ctx.alloc(8 * nchan * len(hyps) * 80), ctx.alloc(4 * nchan * len(hyps) * 80)
    try:
        ctx.h2d(d_x, x)
        ctx.h2d(d_rows, np.full(2 * nchan * stride, np.nan, np.float32))
        assert chan.push_dev(d_x, n, d_rows, stride) == frames
        nsym = ctx.cp_sync_dev(d_rows, frames, hyps, d_est, d_g, d_p, row_stride=80, rho=1.0, nstreams=nchan, stride=stride)
        rows = ctx.d2h(d_rows, (nchan, stride), np.complex64)[:, :frames]
        gamma, phi = ctx.d2h(d_g, (nchan, len(hyps), 80), np.complex64), ctx.d2h(d_p, (nchan, len(hyps), 80), np.float32)
        est = ctx.d2h(d_est, (nchan, len(hyps), 4), np.float32)
    finally:
        for d in (d_x, d_rows, d_est, d_g, d_p):
            ctx.free(d)
        chan.close()
    assert nsym.tolist() == [(frames - 32) // 40, (frames - 64) // 80]
    worst = np.zeros(6)
    for k in range(nchan):
        for h, (tu, cp) in enumerate(hyps):
            ref = PO.fold(rows[k], tu, cp)
            worst = np.maximum(worst, check_rows(gamma[k, h, :tu + cp], phi[k, h, :tu + cp], ref, 'channel %d' % k) +
                               check_est(est[k, h], ref, 1.0, 'channel %d' % k))
    print('cp_sync on the 64 rows of push_dev: Gamma %.1e Phi %.1e theta %.1e eps %.1e rho_hat %.1e Lambda %.1e of their gates' % tuple(worst))


# ---- 6. detection ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tu,cp,symbols,snr_db,theta0,eps0', ESTIMATOR_CASES[:2])
def test_timing_and_offset_of_a_cp_ofdm_capture(ctx, hip, tu, cp, symbols, snr_db, theta0, eps0):
    from ofdm_tools import ofdm_cr_tools as T
    x = PO.cp_ofdm_sync(0, tu, cp, symbols, snr_db, theta0, eps0)
    for rho in (0.0, 1.0):
        gamma, phi, est, nsym = ctx.cp_sync(x, [(tu, cp)], rho=rho)
        assert nsym.tolist() == [symbols]
        check_all(gamma[0], phi[0], est[0], x, tu, cp, rho, '(%d, %d) %+.0f dB rho %.0f' % (tu, cp, snr_db, rho), exact=True)
        assert est[0, 0] == theta0 and abs(float(est[0, 1]) - eps0) <= 0.02
    Sf = 20e6
    d = T.ofdm_sync_scan(x, tu, cp, Sf, ctx=ctx)
    snr = 10.0 ** (snr_db / 10.0)
    print('ofdm_sync_scan (%d, %d) %+.0f dB: %s' % (tu, cp, snr_db, {k: d[k] for k in ('timing', 'eps', 'cfo_hz', 'rho', 'snr_db', 'nsym')}))
    assert d['timing'] == theta0 and d['nsym'] == symbols and d['eps'] == float(est[0, 1]) and d['cfo_hz'] == d['eps'] * Sf / tu
    assert abs(d['rho'] - snr / (snr + 1.0)) <= 0.04 and d['snr_db'] == pytest.approx(10.0 * np.log10(d['rho'] / (1.0 - d['rho'])))
    assert same_bytes(d['gamma'], gamma[0]) and same_bytes(d['phi'], phi[0])


def test_blind_sync_finds_lengths_timing_and_offset(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    from test_welch_caf_cpu import BLIND_LENS, BLIND_NFFT, blind_capture
    x = blind_capture(0, 64, 16, 0.0)
    d = T.ofdm_blind_sync(x, 20e6, fft_lens=BLIND_LENS, nFFT=BLIND_NFFT, ctx=ctx)
    ref = PO.fold(x, 64, 16)
    theta_o, eps_o, rho_o, _, _ = PO.estimate(ref['gamma'], ref['phi'], 1.0)
    print('ofdm_blind_sync: %s (oracle theta %d eps %.4f rho_hat %.3f)' % ({k: d[k] for k in ('detected', 'fft_len', 'cp_len', 'timing', 'eps', 'rho', 'caf_rho')},
                                                                           theta_o, eps_o, rho_o))
    assert d['detected'] and (d['fft_len'], d['cp_len']) == (64, 16) and d['timing'] == theta_o and d['nsym'] == ref['S']
    assert abs(d['eps'] - eps_o) <= RTOL * ref['A'][theta_o] / (2 * np.pi * abs(ref['gamma'][theta_o])) + 1e-6
    assert 0.0 < d['caf_rho'] < 1.0 and abs(d['rho'] - rho_o) <= 2 * RTOL * ref['A'][theta_o] / ref['phi'][theta_o]
    noise = T.ofdm_blind_sync(blind_capture(0, signal=False), 20e6, fft_lens=BLIND_LENS, nFFT=BLIND_NFFT, ctx=ctx)
    assert not noise['detected'] and 'timing' not in noise


# ---- 7. special values and refusals -------------------------------------------------------------------------------------------

def test_silence_gives_exact_zeros(ctx, hip):
    hyps = [(64, 16), (8, 8)]
    gamma, phi, est, nsym = run_dev(ctx, np.zeros((2, 1000), np.complex64), hyps, 1.0, gap=2)
    for h, (tu, cp) in enumerate(hyps):
        assert not gamma[:, h, :tu + cp].view(np.uint32).any() and not phi[:, h, :tu + cp].view(np.uint32).any()
    assert not est.any() and nsym.tolist() == [11, 62]
    d = ctx.cp_sync(np.zeros(500, np.complex64), [(64, 16)])
    assert not d[0][0].any() and not d[1][0].any() and not d[2].any()


@pytest.mark.parametrize('cap', [None, 2])
def test_a_nan_and_an_inf_stay_in_their_windows(ctx, hip, cap):
    """stream 0 holds a NaN and an inf sample, stream 1 none: exactly the entries of stream 0 whose window covers a residue the
    two enter are NaN - never inf -, every other entry and all of stream 1 are the clean run's bytes, est of the poisoned rows
    is four NaNs"""
    hyps = [(64, 16), (100, 7), (16, 16)]
    n = 4000
    xs = np.stack([parity_input(31 + s, 64, 16, n) for s in range(2)])
    bad = xs.copy()
    at = {1234: np.complex64(complex(np.nan, 1.0)), 2501: np.complex64(complex(2.0, -np.inf))}
    for k, v in at.items():
        bad[0, k] = v
    with forced_env('OTH_CPS_WG', cap):
        clean = run_dev(ctx, xs, hyps, 1.0, gap=1)
        got = run_dev(ctx, bad, hyps, 1.0, gap=1)
    for h, (tu, cp) in enumerate(hyps):
        ts = tu + cp
        hit = PO.covered(set().union(*[PO.poisoned(k, n, tu, cp) for k in at]), tu, cp)
        assert 0 < hit.sum() < ts or (tu, cp) == (16, 16)
        g, p = got[0][0, h, :ts], got[1][0, h, :ts]
        assert not np.isinf(g.view(np.float32)).any() and not np.isinf(p).any()
        assert np.array_equal(np.isnan(g.real), hit) and np.array_equal(np.isnan(g.imag), hit) and np.array_equal(np.isnan(p), hit)
        assert same_bytes(g[~hit], clean[0][0, h, :ts][~hit]) and same_bytes(p[~hit], clean[1][0, h, :ts][~hit])
        assert np.all(np.isnan(got[2][0, h]))
        assert same_bytes(got[0][1, h], clean[0][1, h]) and same_bytes(got[1][1, h], clean[1][1, h]) and same_bytes(got[2][1, h], clean[2][1, h])
    # a sample behind the last symbol's lag is not read: nothing changes
    tail = xs.copy()
    tail[0, PO.nsym(n, 64, 16) * 80 + 64:] = np.nan
    with forced_env('OTH_CPS_WG', cap):
        t = run_dev(ctx, tail, hyps[:1], 1.0, gap=1)
    assert same_bytes(t[0][:, 0], clean[0][:, 0][:, :t[0].shape[2]]) and same_bytes(t[2][:, 0], clean[2][:, 0])


def refused(ctx, rc, code, text):
    assert rc == code and ctx.lib.oth_last_error(ctx.h).decode() == text, (rc, ctx.lib.oth_last_error(ctx.h))


def test_refusals_leave_the_context_usable_and_a_second_call_allocates_nothing(ctx, hip):
    lib = ctx.lib
    x = parity_input(41, 64, 16, 3000)
    hyps = [(64, 16), (100, 7)]
    want = ctx.cp_sync(x, hyps, rho=0.5)
    live = hip.live_resources()
    again = ctx.cp_sync(x, hyps, rho=0.5)
    assert hip.live_resources() == live      # the scratch is large enough: no allocation
    ip, vp = C.POINTER(C.c_int), lambda a: a.ctypes.data_as(C.c_void_p)
    fpt = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    gam, phi = np.full((2, 107), SENTINEL + 0j, np.complex64), np.full((2, 107), SENTINEL, np.float32)
    est, nsym = np.full((2, 4), SENTINEL, np.float32), np.zeros(16, np.uint64)
    u64 = nsym.ctypes.data_as(C.POINTER(C.c_uint64))
    ints = lambda *v: np.array(v, np.int32)

    def host(xv=x, n=None, nhyp=2, tu=ints(64, 100), cp=ints(16, 7), rho=0.5, row=107, g=gam, e=est, ns=u64):
        return lib.oth_cp_sync(ctx.h, vp(xv) if xv is not None else None, len(x) if n is None else n, 0, nhyp,
                               tu.ctypes.data_as(ip) if tu is not None else None, cp.ctypes.data_as(ip) if cp is not None else None,
                               C.c_float(rho), row, vp(g), fpt(phi), fpt(e) if e is not None else None, ns)

    def dev(nstreams=1, stride=3000, est_dev=4096, x_dev=4096):
        return lib.oth_cp_sync_dev(ctx.h, C.c_void_p(x_dev) if x_dev else None, 3000, nstreams, stride, 2, ints(64, 100).ctypes.data_as(ip),
                                   ints(16, 7).ctypes.data_as(ip), C.c_float(0.5), 107, None, None, C.c_void_p(est_dev) if est_dev else None, u64)

    attempts = [
        (lambda: host(xv=None), INVALID, 'bad argument'),
        (lambda: host(tu=None), INVALID, 'bad argument'),
        (lambda: host(cp=None), INVALID, 'bad argument'),
        (lambda: host(e=None), INVALID, 'bad argument'),
        (lambda: host(ns=None), INVALID, 'bad argument'),
        (lambda: dev(x_dev=0), INVALID, 'bad argument'),
        (lambda: dev(est_dev=0), INVALID, 'bad argument'),
        (lambda: dev(nstreams=0), INVALID, 'bad argument'),
        (lambda: dev(nstreams=-3), INVALID, 'bad argument'),
        (lambda: host(nhyp=0), INVALID, 'nhyp must lie in 1 ... 16'),
        (lambda: host(nhyp=17), INVALID, 'nhyp must lie in 1 ... 16'),
        (lambda: host(tu=ints(64, 7), cp=ints(16, 7)), INVALID, 'Tu must lie in 8 ... 16384, not 7'),
        (lambda: host(tu=ints(16385, 100)), INVALID, 'Tu must lie in 8 ... 16384, not 16385'),
        (lambda: host(cp=ints(0, 7)), INVALID, 'cp must lie in 1 ... Tu, not 0'),
        (lambda: host(cp=ints(16, 101)), INVALID, 'cp must lie in 1 ... Tu, not 101'),
        (lambda: host(rho=-0.01), INVALID, 'rho must be a finite value in 0 ... 1'),
        (lambda: host(rho=1.5), INVALID, 'rho must be a finite value in 0 ... 1'),
        (lambda: host(rho=float('nan')), INVALID, 'rho must be a finite value in 0 ... 1'),
        (lambda: host(rho=float('inf')), INVALID, 'rho must be a finite value in 0 ... 1'),
        (lambda: dev(nstreams=2, stride=2999), INVALID, 'stream_stride < nsamples'),
        (lambda: dev(nstreams=65536), UNSUPPORTED, 'cp_sync takes at most 65535 streams per launch'),
        (lambda: host(row=106), INVALID, 'row_stride below the largest Tu + cp (107)'),
        (lambda: host(n=206), INVALID, 'input shorter than one symbol and its lag (2 Tu + cp = 207 samples)'),
        (lambda: host(n=0), INVALID, 'input shorter than one symbol and its lag (2 Tu + cp = 144 samples)'),
        # the order: the pointers before nhyp before Tu before cp before rho before the stride before the row before the length
        (lambda: host(xv=None, nhyp=0), INVALID, 'bad argument'),
        (lambda: host(nhyp=17, tu=ints(1, 1), rho=2.0), INVALID, 'nhyp must lie in 1 ... 16'),
        (lambda: host(tu=ints(64, 3), cp=ints(0, 7), rho=2.0), INVALID, 'Tu must lie in 8 ... 16384, not 3'),
        (lambda: host(cp=ints(16, 0), rho=2.0, row=1), INVALID, 'cp must lie in 1 ... Tu, not 0'),
        (lambda: host(rho=2.0, row=1, n=5), INVALID, 'rho must be a finite value in 0 ... 1'),
        (lambda: host(row=1, n=5), INVALID, 'row_stride below the largest Tu + cp (107)'),
    ]
    for call, code, text in attempts:
        refused(ctx, call(), code, text)
        assert np.all(gam == np.complex64(SENTINEL)) and np.all(phi == SENTINEL) and np.all(est == SENTINEL)
        assert hip.live_resources() == live
        now = ctx.cp_sync(x, hyps, rho=0.5)      # ... and the context goes on working
        assert all(same_bytes(a, b) for a, b in zip(now[0] + now[1] + [now[2], now[3]], want[0] + want[1] + [want[2], want[3]]))
    assert all(same_bytes(a, b) for a, b in zip(again[0] + again[1] + [again[2]], want[0] + want[1] + [want[2]]))
    # the raw call that is not refused fills its rows up to Ts and nothing behind
    assert host() == 0 and nsym[:2].tolist() == want[3].tolist()
    assert same_bytes(gam[0, :80], want[0][0]) and same_bytes(gam[1], want[0][1]) and same_bytes(phi[0, :80], want[1][0]) and same_bytes(est, want[2])
    assert np.all(gam[0, 80:] == np.complex64(SENTINEL)) and np.all(phi[0, 80:] == SENTINEL)
    for h, (tu, cp) in enumerate(hyps):
        check_all(want[0][h], want[1][h], want[2][h], x, tu, cp, 0.5, 'after the refusals (%d, %d)' % (tu, cp))
    gc.collect()
    assert hip.live_resources() == live
