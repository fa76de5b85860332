"""CPU checks of the generalized cross-correlation of the spectral matrix's pairs (no GPU): the float64 oracle
(tests/welch_gcc_oracle.py) recovers known delays and obeys the estimator's identities and the header's degenerate rules; the
conditions under which the GPU suite's delay gate holds are met by the oracle alone for every pair of every parity case;
channel_delays, tdoa_scan's unit conversions and refusals; the declared surface and the resource figures of every
mat_gcc_kernel build read from the code objects of the built library.
Measured here: delays of 3.3, -7.6 and -10.9 samples (256 points, 40 segments, 10 dB, PHAT) are recovered within 0.0070 sample
at upsample 8 and within 0.23 at upsample 1 - the parabola's bias on a sinc, the reason for upsample; over the parity cases
the oracle's |den| is at least 9.1 times 8 g and its top leads the window by at least 1.7 times 2 g."""
import numpy as np
import pytest

import welch_gcc_oracle as GO
import welch_matrix_oracle as XO
from stat_support import FS, POWERS, check_builds, check_surface

RTOL = 1e-4      # tests/test_hip_parity.py's, which the GPU suite imports (asserted there)
SYMBOLS = ('oth_welch_matrix_gcc_dev', 'oth_welch_matrix_gcc')
TRUE = np.array([0.0, 3.3, -7.6])


def sums(x, nfft, **kw):
    return XO.matrix(x, nfft, **kw)['T']


# ---- 1. the oracle recovers known delays, and what upsample is for ---------------------------------------------------------------

def test_oracle_recovers_the_delays_and_upsample_removes_the_bias():
    nfft, M = 256, 40
    T = sums(GO.delayed_capture(TRUE, nfft * M, 3, snr_db=10.0), nfft)
    want = np.array([TRUE[b] - TRUE[a] for a, b in GO.pairs(3)])      # 3.3, -7.6, -10.9
    err = {U: np.abs(GO.gcc(T, 'phat', upsample=U)['peak'][:, 0] - want) for U in (1, 8)}
    print('delays 3.3 / -7.6 / -10.9: off by at most %.4f sample at upsample 8, %.4f at upsample 1' % (err[8].max(), err[1].max()))
    assert err[8].max() <= 0.02
    assert err[1].max() > err[8].max() and err[1].max() > 0.02      # the parabola's bias between whole lags
    for w in GO.WEIGHTINGS:
        r = GO.gcc(T, w, upsample=8)
        assert np.all(np.abs(r['R']) <= 1.0 + 1e-12) and np.abs(r['peak'][:, 0] - want).max() <= 0.02


def test_upsample_identity():
    T = sums(GO.delayed_capture(TRUE, 64 * 6, 4), 64)
    for w in GO.WEIGHTINGS:
        for band in (None, (-20, 7)):
            one = GO.gcc(T, w, band, 1)['R']
            for U in (2, 4, 8):
                up = GO.gcc(T, w, band, U, maxlag=U * 31)['R']
                assert np.max(np.abs(up[:, ::U] - one)) <= 1e-12


def test_band_selection():
    """an interferer outside the band, 10 dB up and with another delay, owns the plain correlation of the whole band and is
    gone once the band is set"""
    nfft, M = 256, 24
    x = GO.delayed_capture((0.0, 5.0), nfft * M, 8, band=(-0.25, 0.0)).astype(np.complex128)
    x += GO.delayed_capture((0.0, -9.0), nfft * M, 9, snr_db=10.0, band=(0.1, 0.4), dtype=np.complex128)
    T = sums(x, nfft)
    whole = GO.gcc(T, 'plain')['peak'][0]
    inside = GO.gcc(T, 'plain', band=(-62, -2))['peak'][0]
    print('plain peak: %.2f samples (|R| %.2f) over the whole band, %.2f (|R| %.2f) inside the band' % (whole[0], whole[1], inside[0], inside[1]))
    assert abs(whole[0] + 9.0) <= 0.3 and abs(inside[0] - 5.0) <= 0.3


def test_channel_exchange_conjugates_and_mirrors():
    T = sums(GO.delayed_capture(TRUE[:2], 128 * 5, 6), 128)
    swapped = T[::-1][:, ::-1]
    for w in GO.WEIGHTINGS:
        ab, ba = GO.gcc(T, w, (-40, 33), 2), GO.gcc(swapped, w, (-40, 33), 2)
        assert np.max(np.abs(ba['R'][0] - np.conj(ab['R'][0][::-1]))) <= 1e-12
        assert abs(ba['peak'][0, 1] - ab['peak'][0, 1]) <= 1e-12


# ---- 2. degenerate rules of the oracle ---------------------------------------------------------------------------------------------

def test_oracle_degenerate_rules():
    nfft = 64
    x = GO.delayed_capture(TRUE, nfft * 5, 12)
    clean = {w: GO.gcc(sums(x, nfft), w, upsample=2) for w in GO.WEIGHTINGS}
    for fill in (0.0, 3.0 - 1.0j):      # silence, and a constant under detrend: Z = 0 for the channel's pairs
        y = x.copy()
        y[1] = fill
        for w in GO.WEIGHTINGS:
            r = GO.gcc(sums(y, nfft), w, upsample=2)
            for p, (a, b) in enumerate(GO.pairs(3)):
                if 1 in (a, b):
                    assert r['Z'][p] == 0.0 and not r['R'][p].any() and not r['peak'][p].any(), (fill, w, p)
                else:
                    assert r['R'][p].tobytes() == clean[w]['R'][p].tobytes() and np.all(np.isfinite(r['peak'][p]))
    y = x.copy()
    y[2, 100] = np.nan
    for w in GO.WEIGHTINGS:
        r = GO.gcc(sums(y, nfft), w, upsample=2)
        for p, (a, b) in enumerate(GO.pairs(3)):
            if 2 in (a, b):
                assert np.isnan(r['R'][p]).all() and np.isnan(r['peak'][p]).all()
            else:
                assert r['R'][p].tobytes() == clean[w]['R'][p].tobytes() and r['peak'][p].tobytes() == clean[w]['peak'][p].tobytes()
    one = GO.gcc(sums(x[:, :nfft], nfft, detrend=False), 'scot')      # M = 1: unit coherence in every bin, PHAT and SCOT agree
    assert np.max(np.abs(one['coh'] - 1.0)) <= 1e-12
    assert np.max(np.abs(one['R'] - GO.gcc(sums(x[:, :nfft], nfft, detrend=False), 'phat')['R'])) <= 1e-12
    twin = GO.gcc(sums(np.stack([x[0], x[0]]), nfft), 'phat')      # identical channels: lag 0, |R| = 1, phase 0
    assert np.allclose(twin['peak'][0], (0.0, 1.0, 0.0), atol=1e-12)
    assert GO.gcc(sums(x, nfft), 'phat', maxlag=0)['peak'][0, 0] == 0.0      # one lag: its own edge


# ---- 3. the conditions of the GPU suite's delay gate, on the oracle alone -------------------------------------------------------------

def test_the_parity_cases_cover_every_build_and_option():
    from test_welch_matrix_gpu import OPTIONS
    assert sorted({c[1] * c[0] for c in GO.PARITY}) == list(POWERS)      # every NI build
    assert {c[4] for c in GO.PARITY} == set(range(len(OPTIONS))) and {c[2] for c in GO.PARITY} == {2, 3, 5, 8}
    assert {c[3] for c in GO.PARITY} <= set(range(1, 13)) and {1, 12} <= {c[3] for c in GO.PARITY}


@pytest.mark.parametrize('case', GO.PARITY)
def test_every_pair_of_a_parity_case_meets_the_gate_s_conditions(case):
    """|den| > 8 g and the top of |R| leading every other lag of the window by more than 2 g, g the gate on R with the
    transform's term in it - for all three weightings and every pair, none left out"""
    nfft, U, C, M = case[:4]
    x, (nperseg, noverlap, detrend, scaling, _, _, _), band = GO.parity_input(*case)
    ref = XO.matrix(x, nfft, nperseg, noverlap, 'hann', detrend, scaling, FS)
    assert ref['M'] == M
    for w in GO.WEIGHTINGS:
        want = GO.gcc(ref['T'], w, band, U, case[6])
        g = GO.gates(want, w, U * nfft, RTOL)
        gate, ok = GO.delay_gate(want, g, U)
        inner = want['den'] != 0.0
        print('%s %s: |den| / 8 g at least %.1f, lead / 2 g at least %.1f, delay gate at most %.4f sample'
              % (case, w, (np.abs(want['den'][inner]) / (8 * g[inner])).min() if inner.any() else np.inf, (want['lead'] / (2 * g)).min(), gate.max()))
        assert ok.all() and np.all(np.isfinite(gate)) and gate.max() <= 0.05, (case, w, ok)


# ---- 4. channel_delays --------------------------------------------------------------------------------------------------------------

def test_channel_delays_inverts_a_consistent_matrix_and_honours_weights():
    from ofdm_tools import ofdm_cr_tools as T
    rng = np.random.default_rng(2)
    for C in (2, 3, 5, 8):
        tau = np.concatenate(([0.0], rng.uniform(-20.0, 20.0, C - 1)))
        pair = tau[None, :] - tau[:, None]      # pair[a][b] = tau_b - tau_a
        assert np.max(np.abs(T.channel_delays(pair) - tau)) <= 1e-12
        assert np.max(np.abs(T.channel_delays(pair, rng.uniform(0.1, 1.0, (C, C))) - tau)) <= 1e-12
    pair = tau[None, :] - tau[:, None]
    pair[2, 5] += 40.0      # one wrong pair: it pulls the equal-weight answer, and not the one that gives it no weight
    pair[5, 2] -= 40.0
    w = np.ones((8, 8))
    w[2, 5] = 0.0
    assert np.max(np.abs(T.channel_delays(pair) - tau)) > 1.0 and np.max(np.abs(T.channel_delays(pair, w) - tau)) <= 1e-12
    w[:] = 0.0
    w[0, 1] = 1.0
    for bad in (dict(pair_delays=pair, weights=w), dict(pair_delays=pair[:3]), dict(pair_delays=pair, weights=-np.ones((8, 8))),
                dict(pair_delays=np.full((3, 3), np.nan))):
        with pytest.raises(ValueError):
            T.channel_delays(**bad)


# ---- 5. tdoa_scan's conversions and refusals, before a context exists -----------------------------------------------------------------

class FakePlan:
    def matrix_gcc(self, x, **kw):
        self.kw = kw
        C, L = x.shape[0], kw['maxlag']
        z = np.zeros((C, C), np.float32)
        return z + 4.0 * (np.triu(np.ones((C, C)), 1) - np.tril(np.ones((C, C)), -1)).astype(np.float32), z, z, np.zeros((C * (C - 1) // 2, 2 * L + 1), np.complex64)


class FakeCtx:
    def __init__(self):
        self.plan = FakePlan()

    def cached_plan(self, key, make):
        self.key = key
        return self.plan


def test_tdoa_scan_converts_hertz_and_seconds():
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros((3, 256 * 4), np.complex64)
    fake = FakeCtx()
    delays, peaks, phases, axis, rows = T.tdoa_scan(x, 256, 20e6, ctx=fake)
    assert fake.plan.kw == dict(weighting='phat', band=None, upsample=1, maxlag=127) and fake.key == ('matrix', 256, 20e6)
    assert delays.dtype == np.float64 and delays[0, 1] == 4.0 / 20e6 and delays[1, 0] == -4.0 / 20e6
    assert axis.shape == (255,) and axis[0] == -127 / 20e6 and axis[127] == 0.0 and rows.shape == (3, 255)
    # a bin is 78125 Hz wide: -2.5 MHz is bin -32 exactly, 1 MHz lies between bins 12 and 13; 1 us is 80 lags of 1 / (4 Sf)
    T.tdoa_scan(x, 256, 20e6, weighting='scot', band=(-2.5e6, 1e6), upsample=4, maxlag=1e-6, ctx=fake)
    assert fake.plan.kw == dict(weighting='scot', band=(-32, 12), upsample=4, maxlag=80)
    axis = T.tdoa_scan(x, 256, 20e6, upsample=4, maxlag=1e-6, ctx=fake)[3]
    assert axis.shape == (161,) and np.isclose(axis[-1], 1e-6, rtol=1e-12) and np.isclose(axis[1] - axis[0], 1.0 / 80e6, rtol=1e-9)
    T.tdoa_scan(x, 256, 20e6, band=(-10e6, 9.99e6), ctx=fake)      # the whole axis
    assert fake.plan.kw['band'] == (-128, 127)
    T.tdoa_scan(x, 256, 20e6, maxlag=0.0, ctx=fake)
    assert fake.plan.kw['maxlag'] == 0


def test_tdoa_scan_refuses_in_python():
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros((4, 256 * 8), np.complex64)
    for nfft in (100, 32, 32768):
        with pytest.raises(ValueError) as ei:
            T.tdoa_scan(x, nfft, 1.0)
        assert str(ei.value).startswith('tdoa_scan needs nFFT a power of two from 64 to 16384')
    for bad in (x[0], x[:1], np.zeros((9, 2048), np.complex64)):
        with pytest.raises(ValueError) as ei:
            T.tdoa_scan(bad, 256, 1.0)
        assert str(ei.value).startswith('tdoa_scan needs a (C, n) array of 2 ... 8 channels')
    refusals = [
        (dict(vectors=x[:, :255]), 'tdoa_scan needs at least nFFT = 256 samples per channel'),
        (dict(Sf=0.0), 'tdoa_scan needs a sample rate Sf > 0'),
        (dict(weighting='ml'), "tdoa_scan needs weighting 'plain', 'phat' or 'scot', not 'ml'"),
        (dict(upsample=3), 'tdoa_scan needs upsample 1, 2, 4 or 8 with upsample * nFFT <= 16384, not 3'),
        (dict(vectors=np.zeros((2, 4096), np.complex64), nFFT=4096, upsample=8), 'tdoa_scan needs upsample 1, 2, 4 or 8 with upsample * nFFT <= 16384, not 8'),
        (dict(band=(0.1, -0.1)), 'tdoa_scan needs band = (f_lo, f_hi) in Hz with -Sf / 2 <= f_lo <= f_hi < Sf / 2'),
        (dict(band=(-0.6, 0.1)), 'tdoa_scan needs band = (f_lo, f_hi) in Hz with -Sf / 2 <= f_lo <= f_hi < Sf / 2'),
        (dict(band=(0.1, 0.5)), 'tdoa_scan needs band = (f_lo, f_hi) in Hz with -Sf / 2 <= f_lo <= f_hi < Sf / 2'),
        (dict(band=(0.0401, 0.0429)), 'tdoa_scan: the band (0.0401, 0.0429) Hz holds no bin of width 0.00390625 Hz'),
        (dict(maxlag=-1.0), 'tdoa_scan needs maxlag >= 0 in seconds'),
        (dict(maxlag=128.0), 'tdoa_scan: maxlag is 128 lags of 1 / (upsample Sf); upsample * nFFT / 2 - 1 = 127 at most'),
    ]
    for kw, text in refusals:
        args = dict(vectors=x, nFFT=256, Sf=1.0)
        args.update(kw)
        with pytest.raises(ValueError) as ei:
            T.tdoa_scan(**args)      # no ctx: a refusal comes before one is made
        assert str(ei.value) == text, kw


# ---- 6. surface, 7. resources ---------------------------------------------------------------------------------------------------------

def test_surface_is_declared_and_exported():
    from ofdm_tools import _hip, ofdm_cr_tools as T
    assert (_hip.GCC_PLAIN, _hip.GCC_PHAT, _hip.GCC_SCOT) == (0, 1, 2)
    assert _hip.gcc_pairs(4) == GO.pairs(4) and callable(T.tdoa_scan) and callable(T.channel_delays)
    check_surface(SYMBOLS, 'WelchPlan', ('matrix_gcc', 'matrix_gcc_dev'),
                  ['int weighting, int band_lo, int band_hi, int upsample, int maxlag,', 'float *gcc_out_dev, float *peak_out_dev, uint64_t *nseg_out);',
                   '#define OTH_GCC_PLAIN 0', '#define OTH_GCC_PHAT  1', '#define OTH_GCC_SCOT  2', '#define OTH_GCC_UPSAMPLE_MAX 8'])


def test_every_mat_gcc_kernel_build_has_no_scratch():
    """one workgroup per pair around an NI-point tile of LDS: read from the code objects inside the built library, the nine
    builds (NI = 64 ... 16384 at generic_threads(NI) threads) have a private segment of 0 bytes and no spilled register, and
    the 1024-thread build stays inside the 128 registers a lane has there; the family's shared launches next to them keep
    theirs"""
    builds = check_builds('mat_gcc_kernel', list(POWERS), {64: 512, 256: 512, 512: 256, 1024: 128},
                          extra_kernels=('mat_finalize_kernel', 'mat_det_kernel'))
    assert sorted(a[1] for a, _ in builds) == [64] * 4 + [256] * 3 + [512, 1024]
