"""CPU checks of the median average: the float64 oracle of tests/median_oracle.py against scipy.signal.welch(...,
average='median') itself, and the ctypes table of the two new entry points."""
import numpy as np
import pytest

import median_oracle as M

scipy_signal = pytest.importorskip('scipy.signal')


def synth(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    x += 3.0 * np.exp(2j * np.pi * 0.123 * t) + 0.4 + 0.2j
    return x.astype(np.complex64)


CASES = []
for nseg in (1, 2, 3, 4, 7, 40):
    for ov in (0, 50, 75):
        CASES.append((nseg, ov, 64, 64, 'constant', 'density'))
CASES += [(40, 50, 48, 64, 'constant', 'density'),      # nfft > nperseg
          (7, 50, 64, 64, False, 'density'),
          (7, 75, 64, 64, 'constant', 'spectrum'),
          (4, 0, 100, 128, False, 'spectrum')]


@pytest.mark.parametrize('nseg,ov,nperseg,nfft,detrend,scaling', CASES)
def test_oracle_equals_scipy_median(nseg, ov, nperseg, nfft, detrend, scaling):
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    x = synth(noverlap + nseg * step, 100 + nseg + ov)
    _, ref = scipy_signal.welch(x.astype(np.complex128), fs=2.0, window='hann', nperseg=nperseg, noverlap=noverlap, nfft=nfft,
                                detrend=detrend, scaling=scaling, average='median', return_onesided=False)
    got = M.welch_median(x, fs=2.0, window='hann', nperseg=nperseg, noverlap=noverlap, nfft=nfft,
                         detrend='constant' if detrend else False, scaling=scaling)
    assert M.welch_rows(x, 2.0, 'hann', nperseg, noverlap, nfft).shape[0] == nseg
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


def test_oracle_median_bias_matches_scipy():
    from scipy.signal._spectral_py import _median_bias
    for n in (1, 2, 3, 4, 7, 40, 131071):
        assert M.median_bias(n) == pytest.approx(_median_bias(n), rel=1e-14)


def test_oracle_nan_sample_gives_nan_where_scipy_does():
    x = synth(64 * 9, 5)
    x[100] = np.nan
    _, ref = scipy_signal.welch(x.astype(np.complex128), window='hann', nperseg=128, average='median', return_onesided=False)
    got = M.welch_median(x, window='hann', nperseg=128)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any()
    np.testing.assert_allclose(got[~np.isnan(ref)], ref[~np.isnan(ref)], rtol=1e-12)


def test_signatures_list_the_median_entry_points():
    from ofdm_tools import _hip
    assert 'oth_plan_set_average' in _hip.SIGNATURES and 'oth_welch_segments_dev' in _hip.SIGNATURES
    assert (_hip.AVERAGE_MEAN, _hip.AVERAGE_MEDIAN) == (0, 1)
    assert _hip.average_code('median') == _hip.AVERAGE_MEDIAN and _hip.average_code(0) == _hip.AVERAGE_MEAN
    with pytest.raises(ValueError):
        _hip.average_code('mode')


def test_long_stream_refuses_a_median_plan():
    pytest.importorskip('torch')
    from ofdm_tools import _hip, sweep

    class Plan(object):
        average = _hip.AVERAGE_MEDIAN
    with pytest.raises(ValueError, match='median'):
        sweep.welch_long_stream(Plan(), 0, 0, 1 << 20, 'cpu', 0, 1)
