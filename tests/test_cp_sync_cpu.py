"""CPU checks of the cyclic-prefix synchroniser (no GPU): the float64 oracle by the definition against its fold form
(tests/cp_sync_oracle.py), the symbol count, the estimator on the oracle alone - so that the gates of
tests/test_cp_sync_gpu.py are known to be reachable -, the declared surface, the Python helpers, and the resource figures of
the kernels of csrc/cpsync.hip read from the code objects of the built library.
The estimator on the oracle, seeds 0 ... 5 of the five shapes below, rho 0 and 1: theta == theta0 in all 60; |eps - eps0| at
most 0.0103 at -3 dB and 0.0021 at 10 dB (bound 0.02); rho_hat 0.330 ... 0.349 against 0.334 and 0.904 ... 0.914 against
0.909 (bound 0.04); noise alone reads rho_hat 0.037."""
import numpy as np
import pytest

import cp_sync_oracle as PO
from stat_support import check_builds, check_surface

SYMBOLS = ('oth_cp_sync_dev', 'oth_cp_sync')
# Tu, cp, symbols, SNR dB, theta0, eps0
ESTIMATOR_CASES = [(64, 16, 200, 10.0, 37, 0.2), (64, 16, 200, -3.0, 37, 0.2), (256, 64, 60, 10.0, 300, 0.45), (1000, 73, 40, 10.0, 999, 0.1),
                   (16, 1, 2000, 10.0, 3, 0.25)]
# Tu, cp, S, streams: the parity shapes of the GPU suite
PARITY_CASES = [(8, 1, 5, 1), (16, 1, 2000, 1), (64, 16, 1, 1), (64, 16, 200, 3), (64, 64, 50, 1), (256, 64, 60, 2), (1000, 73, 40, 1),
                (1023, 1, 7, 1), (4096, 1024, 9, 1), (16384, 4096, 3, 2), (16384, 16384, 2, 1)]


def parity_input(seed, tu, cp, n):
    """unit complex noise + a CP-OFDM signal of the hypothesis' lengths (0 dB, theta0 = Ts / 3, eps0 = 0.15) + a 35 - 20j
    offset, n samples -> complex64"""
    ts = tu + cp
    rng = np.random.default_rng([seed, n])
    sig = PO.cp_ofdm_sync(seed, tu, cp, n // ts + 1, 0.0, ts // 3, 0.15, noise=False)[:n].astype(np.complex128)
    x = sig + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0) + (35.0 - 20.0j)
    return x.astype(np.complex64)


# ---- 1. the oracle -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tu,cp,S,extra', [(8, 1, 5, 0), (16, 1, 40, 3), (64, 16, 9, 79), (64, 64, 3, 0), (100, 7, 4, 50), (31, 31, 2, 61)])
def test_definition_against_the_fold_form(tu, cp, S, extra):
    x = parity_input(3, tu, cp, S * (tu + cp) + tu + extra)
    d = PO.definition(x, tu, cp)
    for direct in (True, False):
        f = PO.fold(x, tu, cp, direct=direct)
        assert d['S'] == f['S'] == S
        worst = [float(np.max(np.abs(f[k] - d[k]) / d['A'])) for k in ('gamma', 'phi', 'A')]
        print('definition against the fold form (%d, %d) S %d, direct %s: %s of A' % (tu, cp, S, direct, np.array(worst)))
        assert max(worst) <= 1e-12


def test_the_direct_window_keeps_a_nan_in_its_window():
    v = np.arange(1.0, 11.0)
    v[7] = np.nan
    for cp in (1, 3, 10):
        w = PO.window(v, cp)
        assert np.array_equal(np.isnan(w), PO.covered({7}, 10 - cp, cp)) and not np.isinf(w).any()
    assert PO.window(np.arange(1.0, 6.0), 2).tolist() == [3.0, 5.0, 7.0, 9.0, 6.0]


def test_symbol_count_arithmetic():
    assert PO.nsym(80 * 5 + 64, 64, 16) == 5 and PO.nsym(80 * 5 + 64 + 79, 64, 16) == 5 and PO.nsym(80 * 5 + 63, 64, 16) == 4
    assert PO.nsym(2 * 64 + 16, 64, 16) == 1 and PO.nsym(2 * 64 + 15, 64, 16) == 0 and PO.nsym(10, 64, 16) == 0
    assert PO.nsym(1 << 26, 64, 16) == ((1 << 26) - 64) // 80
    # the last sample the fold reads lies inside the stream
    for n, tu, cp in ((1000, 64, 16), (144, 64, 16), (32768 + 16384, 16384, 16384), (17, 8, 1)):
        S = PO.nsym(n, tu, cp)
        assert S >= 1 and S * (tu + cp) - 1 + tu <= n - 1 < (S + 1) * (tu + cp) - 1 + tu
    # a non-finite sample enters a residue only where the fold reads it
    assert PO.poisoned(5, 80 * 5 + 64, 64, 16) == {5} and PO.poisoned(70, 80 * 5 + 64, 64, 16) == {70, 6}
    assert PO.poisoned(80 * 5 + 10, 80 * 5 + 64, 64, 16) == {(80 * 5 + 10 - 64) % 80} and PO.poisoned(80 * 5 + 64, 80 * 5 + 70, 64, 16) == set()


# ---- 2. the estimator on the oracle alone ------------------------------------------------------------------------------------

@pytest.mark.parametrize('tu,cp,symbols,snr_db,theta0,eps0', ESTIMATOR_CASES)
def test_estimator_on_the_oracle(tu, cp, symbols, snr_db, theta0, eps0):
    snr = 10.0 ** (snr_db / 10.0)
    for seed in range(6):
        x = PO.cp_ofdm_sync(seed, tu, cp, symbols, snr_db, theta0, eps0)
        f = PO.fold(x, tu, cp)
        assert f['S'] == symbols
        for rho in (0.0, 1.0):
            theta, eps, rho_hat, lam, _ = PO.estimate(f['gamma'], f['phi'], rho)
            print('(%d, %d) %d symbols %+.0f dB seed %d rho %.0f: theta %d (%d), eps %.4f (%.2f), rho_hat %.3f (%.3f)' %
                  (tu, cp, symbols, snr_db, seed, rho, theta, theta0, eps, eps0, rho_hat, snr / (snr + 1.0)))
            assert theta == theta0
            assert abs(eps - eps0) <= 0.02
            assert abs(rho_hat - snr / (snr + 1.0)) <= 0.04


def test_estimator_on_noise_alone_and_on_silence():
    """Noise alone, (64, 16) over 200 symbols: Gamma is complex Gaussian of variance cp S = 3200 against Phi = 3200, so the
    largest of 80 entries sits near sqrt(ln 80 / 3200) = 0.037, and 0.08 is passed with probability 80 exp(-0.08^2 3200) = 1e-7."""
    rng = np.random.default_rng(9)
    x = ((rng.standard_normal(80 * 200 + 64) + 1j * rng.standard_normal(80 * 200 + 64)) / np.sqrt(2.0)).astype(np.complex64)
    f = PO.fold(x, 64, 16)
    rho_hat = PO.estimate(f['gamma'], f['phi'], 1.0)[2]
    print('noise alone: rho_hat %.3f' % rho_hat)
    assert rho_hat <= 0.08
    z = PO.fold(np.zeros(80 * 3 + 64, np.complex64), 64, 16)
    assert PO.estimate(z['gamma'], z['phi'], 1.0)[:4] == (0, 0.0, 0.0, 0.0)


# ---- 3. the surface and the Python helpers -----------------------------------------------------------------------------------

def test_the_entry_points_are_declared_bound_and_exported():
    check_surface(SYMBOLS, 'Context', ('cp_sync', 'cp_sync_dev'),
                  ('int oth_cp_sync_dev(oth_ctx *ctx, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,',
                   'int oth_cp_sync(oth_ctx *ctx, const void *iq, size_t nsamples, int src_is_device,',
                   ' * Not provided: a streaming form that carries F / G across calls, fractional-sample timing, the integer part of the carrier'))
    from ofdm_tools import ofdm_cr_tools as T
    assert callable(T.ofdm_sync_scan) and callable(T.ofdm_blind_sync)


def test_cp_sync_args_shape_the_hypotheses():
    from ofdm_tools import _hip
    tu, cp, nhyp, row = _hip.cp_sync_args([(64, 16), (1024, 256)])
    assert tu.dtype == cp.dtype == np.int32 and tu.tolist() == [64, 1024] and cp.tolist() == [16, 256] and (nhyp, row) == (2, 1280)
    assert _hip.cp_sync_args([])[2:] == (0, 1) and _hip.cp_sync_args([(1 << 20, 5)])[3] == 32768
    assert _hip.cp_sync_args((64, 16))[2:] == (1, 80)      # one pair passes as it is


# ---- 4. the kernels' resources ---------------------------------------------------------------------------------------------------

def test_every_cp_sync_kernel_build_has_no_scratch():
    """the fold's three builds (a tile of 256 / 512 / 1024 residues on 64 / 128 / 256 threads: twelve float32 and twelve
    double sums per thread) and the two finalize kernels, read from the code objects inside the built library: each with a
    private segment of 0 bytes and no spilled register; the 1024-thread window kernel inside its 128 registers"""
    import kernel_resources
    from ofdm_tools import _hip
    check_builds('cps_fold_kernel', [256, 512, 1024], {}, extra_kernels=('cps_total_kernel', 'cps_window_kernel'))
    win = [v for n, v in kernel_resources.kernels(_hip.LIB_PATH).items() if 'cps_window_kernel' in n]
    assert len(win) == 1 and win[0]['vgpr'] + win[0]['agpr'] <= 128
