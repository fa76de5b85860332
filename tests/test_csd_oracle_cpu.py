"""tests/csd_oracle.py against scipy.signal.csd / coherence / welch (two-sided) to 1e-12, and against
oracle.ref_cpu.coherence_np for density scaling."""
import numpy as np
import pytest

import csd_oracle as O
from oracle import ref_cpu as R

TOL = 1e-12

SHAPES = [  # nfft, nperseg, noverlap, window, detrend, fs
    (256, 256, 128, 'hann', 'constant', 1.0),
    (512, 383, 127, 'flattop', 'constant', 2.5e6),      # odd and zero-padded
    (128, 128, 0, 'boxcar', False, 1.0),
    (1000, 250, 125, 'hann', 'constant', 48000.0),
]


def pair(n, seed):
    x = R.synth_iq(n, seed, dc=2 - 1j)
    y = (0.7 * np.roll(x, 5) + 0.5 * R.synth_iq(n, seed + 100, tones=(), dc=0.5 + 0.25j)).astype(np.complex64)
    return x, y


def rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize('nfft,nperseg,noverlap,window,detrend,fs', SHAPES)
def test_oracle_equals_scipy(nfft, nperseg, noverlap, window, detrend, fs):
    sg = pytest.importorskip('scipy.signal')
    step = nperseg - noverlap
    x, y = pair(noverlap + 9 * step + step // 3, nfft)
    kw = dict(fs=fs, window=window, nperseg=nperseg, noverlap=noverlap, nfft=nfft, detrend=detrend)
    for scaling in ('density', 'spectrum'):
        pxx, pyy, pxy, cxy = O.csd(x, y, scaling=scaling, **kw)
        for got, ref in ((pxx, sg.welch(x.astype(np.complex128), return_onesided=False, scaling=scaling, **kw)[1]),
                         (pyy, sg.welch(y.astype(np.complex128), return_onesided=False, scaling=scaling, **kw)[1]),
                         (pxy, sg.csd(x.astype(np.complex128), y.astype(np.complex128), return_onesided=False, scaling=scaling, **kw)[1])):
            assert got.shape == (nfft,) and np.max(np.abs(got - ref) / np.abs(ref)) < TOL
        _, cref = sg.coherence(x.astype(np.complex128), y.astype(np.complex128), **kw)      # (two-sided for complex input)
        assert np.max(np.abs(cxy - cref)) < TOL and 0.0 < cxy.min() and cxy.max() <= 1.0 + TOL
    # density is what oracle.ref_cpu states
    pxx, pyy, pxy, cxy = O.csd(x, y, **kw)
    _, rc, rxx, ryy, rxy = R.coherence_np(x, y, **kw)
    assert rel(pxx, rxx) < TOL and rel(pyy, ryy) < TOL and rel(pxy, rxy) < TOL and np.max(np.abs(cxy - rc)) < TOL
    # raw and over-n^2: the density result with its factor taken back out; the sums are raw times the segment count
    win = R.get_window(window, nperseg)
    k = fs * np.sum(win * win)
    raw, n2 = O.csd(x, y, scaling='raw', **kw), O.csd(x, y, scaling='over_n2', **kw)
    sxx, syy, sxy, nseg = O.csd_sums(x, y, window, nperseg, noverlap, nfft, detrend)
    assert nseg == 9
    for a, b, c, s in zip(raw[:3], n2[:3], (pxx, pyy, pxy), (sxx, syy, sxy)):
        assert rel(a, c * k) < TOL and rel(b, c * k / nfft ** 2) < TOL and rel(s, a * nseg) < TOL
    assert np.max(np.abs(raw[3] - cxy)) < TOL and np.max(np.abs(n2[3] - cxy)) < TOL      # Cxy carries no scale


def test_window_array_default_overlap_and_output_stage():
    x, y = pair(3000, 7)
    w = R.get_window('hann', 256)
    a, b = O.csd(x, y, window=w), O.csd(x, y)      # nperseg 256, noverlap 128
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert np.array_equal(O.shift_trim(a[0], True, 37), np.fft.fftshift(a[0])[37:-37])
    odd = np.arange(7.0)
    assert np.array_equal(O.shift_trim(odd, True, 1), np.fft.fftshift(odd)[1:-1]) and O.shift_trim(odd) is odd


def test_degenerate_inputs_follow_scipy():
    sg = pytest.importorskip('scipy.signal')
    x, _ = pair(2000, 3)
    zero = np.zeros_like(x)
    pxx, pyy, pxy, cxy = O.csd(x, zero, nperseg=256)
    with np.errstate(invalid='ignore', divide='ignore'):
        _, cref = sg.coherence(x.astype(np.complex128), zero.astype(np.complex128), nperseg=256)
    assert np.all(pyy == 0) and np.all(pxy == 0) and np.all(np.isnan(cxy)) and np.all(np.isnan(cref)) and np.all(pxx > 0)
