"""CPU checks of the cyclic autocorrelation addition (no GPU): the float64 oracle by the definition
(tests/welch_caf_oracle.py) on its identities and on a CP-OFDM signal, the decision of ofdm_blind_parameters on the oracle's
rows, the Python helpers' refusals, the declared surface, and the resource figures of every welch_lag_kernel build read from
the code objects of the built library."""
import numpy as np
import pytest

import welch_caf_oracle as LO
from stat_support import POWERS, check_builds, check_surface
from test_welch_cyclic_cpu import cp_ofdm

SYMBOLS = ('oth_welch_set_lags', 'oth_welch_caf_dev', 'oth_welch_caf')
BLIND_NFFT, BLIND_M, BLIND_LENS = 4096, 32, (32, 64, 128, 256)
BLIND_CASES = [(64, 16, 0.0), (64, 16, -3.0), (128, 16, 0.0), (64, 4, 0.0), (256, 64, 0.0), (32, 8, 3.0)]      # Tu, Tcp, SNR dB


def blind_capture(seed, tu=64, tcp=16, snr_db=0.0, signal=True):
    """the capture of the blind cases: BLIND_M segments of BLIND_NFFT behind the largest candidate lag; `used` is 3 / 4 of
    Tu, rounded to even"""
    used = 2 * int(round(0.75 * tu / 2.0))
    return cp_ofdm(seed, BLIND_NFFT * BLIND_M + max(BLIND_LENS), tu, tcp, used, snr_db, signal)


def blind_oracle(x, Sf=1.0, lens=BLIND_LENS):
    """ofdm_blind_decision on the oracle's rows of the capture -> its dict"""
    from ofdm_tools import ofdm_cr_tools as T
    ref = LO.caf(x, BLIND_NFFT, (0,) + tuple(lens))
    return T.ofdm_blind_decision(ref['caf'], ref['r'], ref['M'], Sf, lens)


# ---- 1. oracle identities ------------------------------------------------------------------------------------------------------

def test_oracle_lag_zero_is_the_power():
    x = cp_ofdm(5, 256 * 7 + 40)
    ref = LO.caf(x, 256, [0, 3])
    z0 = LO.products(x, 0, 256, 0, ref['M'])
    assert not z0.imag.any()
    p = np.mean(np.abs(x[:256 * ref['M']].astype(np.complex128)) ** 2)
    assert ref['r'][0].imag == 0.0 and abs(ref['r'][0].real - p) <= 1e-12 * p


@pytest.mark.parametrize('tau', [0, 1, 37, 300])
def test_oracle_on_a_pure_tone(tau):
    """z = e^{j 2 pi f tau} at every n: r is that phase, and a detrending plan leaves nothing in the rows"""
    f, nfft = 0.0123, 128
    x = np.exp(2j * np.pi * f * np.arange(nfft * 6 + 300))
    on, off = LO.caf(x, nfft, [tau]), LO.caf(x, nfft, [tau], detrend=False)
    assert abs(on['r'][0] - np.exp(2j * np.pi * f * tau)) <= 1e-12 and abs(off['r'][0] - on['r'][0]) <= 1e-12
    print('tone, lag %d: detrended row max %.1e of the other' % (tau, on['caf'].max() / off['caf'].max()))
    assert on['caf'].max() <= 1e-20 * off['caf'].max()


def test_oracle_counts_segments_behind_the_largest_lag():
    x = cp_ofdm(1, 1000)
    assert LO.caf(x, 64, [0])['M'] == 15 and LO.caf(x, 64, [0, 40])['M'] == 15 and LO.caf(x, 64, [0, 41])['M'] == 14
    assert LO.caf(x, 64, [936])['M'] == 1
    assert LO.caf(x, 128, [5, 9], nperseg=100, noverlap=50)['M'] == (1000 - 9 - 50) // 50
    assert LO.nseg(65535 + 3 * 64, [65535], 64) == 3


# ---- 2. oracle detection on CP-OFDM -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1, 2])
def test_oracle_finds_the_symbol_rate_at_lag_tu_only(seed):
    """Tu 64, Tcp 16, 20 dB, 1024 points, 64 segments: 1024 / 80 = 12.8, so the lines are bins 13 and 1011 of the row of lag 64"""
    nfft, M, lags = 1024, 64, (64, 48, 128, 1)
    n = nfft * M + max(lags)
    rel = lambda row: row / np.median(row)      # noqa: E731
    ref = LO.caf(cp_ofdm(seed, n), nfft, lags)
    assert ref['M'] == M
    on = rel(ref['caf'][0])
    print('seed %d: lag 64 at bins 13 / 1011: %.1f / %.1f x the median' % (seed, on[13], on[1011]))
    assert on[13] >= 10.0 and on[1011] >= 10.0
    noise = LO.caf(cp_ofdm(seed, n, signal=False), nfft, lags)
    others = [rel(ref['caf'][i])[1:].max() for i in (1, 2, 3)] + [rel(noise['caf'][0])[1:].max()]
    print('seed %d: lags 48, 128, 1 and lag 64 on noise alone, bins 1 ... 1023: at most %s x the median' % (seed, np.round(others, 2)))
    assert max(others) <= 3.0


# ---- 3. the decision of ofdm_blind_parameters on the oracle's rows ------------------------------------------------------------

@pytest.mark.parametrize('tu,tcp,snr_db', BLIND_CASES)
def test_blind_decision_on_the_oracle_rows(tu, tcp, snr_db):
    for seed in (0, 1, 2):
        d = blind_oracle(blind_capture(seed, tu, tcp, snr_db), Sf=20e6)
        print('Tu %d Tcp %d %+.0f dB seed %d: %s' % (tu, tcp, snr_db, seed, {k: d[k] for k in ('detected', 'fft_len', 'cp_len', 'stat', 'threshold', 'rho')}))
        assert d['detected'] and (d['fft_len'], d['cp_len']) == (tu, tcp) and d['nseg'] == BLIND_M
        assert np.allclose(d['cycles_hz'][:2], [20e6 / (tu + tcp), -20e6 / (tu + tcp)], rtol=1e-12)
        assert 0.0 < d['rho'] < 1.0


def test_blind_decision_on_noise_alone():
    for seed in range(6):
        d = blind_oracle(blind_capture(seed, signal=False))
        print('noise alone, seed %d: stat %.2f, threshold %.2f' % (seed, d['stat'], d['threshold']))
        assert not d['detected'] and d['stat'] < d['threshold']


def test_blind_threshold_is_the_chi_square_ratio():
    from ofdm_tools import ofdm_cr_tools as T
    thr = T.ofdm_blind_threshold(32, 16, 1e-3)
    want = (T.chi2_quantile(1.0 - 1e-3 / 16.0, 128.0) / 128.0) / (T.chi2_quantile(0.5, 64.0) / 64.0)
    assert thr == want and 1.3 < thr < 1.8
    assert T.ofdm_blind_threshold(32, 1, 1e-3) < thr < T.ofdm_blind_threshold(32, 16, 1e-6)
    assert T.ofdm_blind_threshold(256, 16, 1e-3) < thr


# ---- 4. the helpers' refusals, before a context exists --------------------------------------------------------------------------

def test_caf_scan_refuses_in_python():
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros(256 * 8, np.complex64)
    for nfft in (100, 32, 32768):
        with pytest.raises(ValueError) as ei:
            T.caf_scan(x, nfft, 1.0, [64])
        assert 'power of two' in str(ei.value)
    for lags in ([], np.zeros(65, np.int64)):
        with pytest.raises(ValueError) as ei:
            T.caf_scan(x, 256, 1.0, lags)
        assert '64' in str(ei.value)
    for lags in ([0, -1], [65536], [1.5]):
        with pytest.raises(ValueError) as ei:
            T.caf_scan(x, 256, 1.0, lags)
        assert '65535' in str(ei.value)
    with pytest.raises(ValueError) as ei:
        T.caf_scan(x, 256, 1.0, [0, 256 * 7 + 1])      # max lag + nFFT is one sample more than the capture
    assert 'max(lags) + nFFT' in str(ei.value)


def test_blind_parameters_refuses_candidates_the_row_cannot_separate():
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros(4096 * 4, np.complex64)
    for kw in (dict(fft_lens=(64, 512), nFFT=4096),            # 4096 / 544 and 4096 / 528 both round to bin 8
               dict(fft_lens=(64,), cp_fractions=(4,), nFFT=256),      # 256 / 80: bin 3
               dict(fft_lens=(2048,), nFFT=4096)):             # bins 2, 2, 2, 2
        with pytest.raises(ValueError) as ei:
            T.ofdm_blind_parameters(x, 1.0, **kw)
        assert 'too small for these candidates' in str(ei.value)
    with pytest.raises(ValueError) as ei:
        T.ofdm_blind_parameters(x, 1.0, fft_lens=(64,), cp_fractions=(4,), nFFT=1000)
    assert 'power of two' in str(ei.value)
    hyp = T.ofdm_blind_hypotheses((32, 64, 128, 256), (4, 8, 16, 32), 4096)
    assert len(hyp) == 16 and (64, 16, 51) in hyp and (256, 64, 13) in hyp and (256, 8, 16) in hyp


# ---- 5. surface, 6. resources --------------------------------------------------------------------------------------------------

def test_surface_is_declared_and_exported():
    check_surface(SYMBOLS, 'WelchPlan', ('set_lags', 'caf', 'caf_dev'))


def test_every_welch_lag_kernel_build_has_no_scratch():
    """one running row per lag of the group next to the butterflies (or the partial rows where they do not fit): read from
    the code objects inside the built library, two builds (GL = 1, 2) per power of two 64 ... 16384, each with a private
    segment of 0 bytes and no spilled register; the 1024-thread builds inside their 128 registers."""
    check_builds('welch_lag_kernel', [(n, gl) for n in POWERS for gl in (1, 2)], {1024: 128})
