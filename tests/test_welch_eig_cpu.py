"""CPU checks of the eigenvalue addition to the spectral matrix (no GPU): the float64 transcription of the kernel's Jacobi loop
(tests/welch_eig_oracle.py) against numpy.linalg.eigh and the sweep cap that follows from it, identities and degenerate rules
of the oracle, eigenvalue_stats on the detection capture, eigen_scan's refusals, the declared surface and the resource figures
of every mat_eig_kernel build read from the code objects of the built library.
Measured here: the emulation needs at most 7 sweeps over the 1400 matrices below (the kernel's cap is 9); its worst eigenvalue
error is 1.0e-15 of the trace and its worst vector residual 5.5e-16 of the trace (gates 1e-12); on the oracle at most 3.1 %
of a parity case's bins (up to 1024 points) fall outside the gap condition of the GPU suite's direction gate."""
import os
import re

import numpy as np
import pytest

import welch_eig_oracle as EO
import welch_matrix_oracle as XO
from stat_support import ROOT, check_builds, check_surface
from test_welch_matrix_cpu import DET_BAND, DET_C, DET_GUARD, DET_M, DET_NFFT, detection_capture, noise

SYMBOLS = ('oth_welch_matrix_eig_dev', 'oth_welch_matrix_eig')
EMU_C, EMU_M, EMU_SEEDS = (2, 3, 4, 5, 8), (1, 2, 3, 5, 8, 12, 40), 10
EMU_KINDS = ('plain', 'common', 'twin', 'zero row')


def wishart(rng, C, M, kind):
    """sum over M snapshots of x x^H, C channels of unit noise: with a strong common component (30 dB, a phase per channel),
    with two identical channels, with a silent channel (a zero row and column)"""
    X = noise(rng, (C, M))
    if kind == 'common':
        X = X + 31.6 * noise(rng, M)[None, :] * np.exp(2j * np.pi * rng.random(C))[:, None]
    if kind == 'twin':
        X[C - 1] = X[0]
    if kind == 'zero row':
        X[rng.integers(C)] = 0.0
    return np.conj(X) @ X.T      # T_ab = sum_s conj(X_s,a) X_s,b


def kernel_cap():
    text = open(os.path.join(ROOT, 'gr-ofdm_tools_amd', 'csrc', 'mateig.hip')).read()
    return int(re.search(r'constexpr int kMatEigSweepCap = (\d+);', text).group(1))


# ---- 1. the emulation of the kernel's loop against eigh ------------------------------------------------------------------------

def test_emulation_against_eigh_and_the_sweep_cap():
    cap = kernel_cap()
    worst_sweeps, worst_l, worst_r, count = 0, 0.0, 0.0, 0
    for C in EMU_C:
        rng = np.random.default_rng(100 + C)
        batch = np.array([wishart(rng, C, M, kind) for M in EMU_M for kind in EMU_KINDS for _ in range(EMU_SEEDS)])
        kinds = [kind for M in EMU_M for kind in EMU_KINDS for _ in range(EMU_SEEDS)]
        count += len(batch)
        lam, vec, sweeps = EO.jacobi_emulation(batch, 64)      # far above the cap: the count is the loop's own
        ref = np.maximum(np.linalg.eigvalsh(batch)[:, ::-1], 0.0)
        trace = np.einsum('baa->b', batch).real
        worst_l = max(worst_l, float(np.max(np.abs(lam - ref) / trace[:, None])))
        resid = np.linalg.norm(np.einsum('bac,bc->ba', batch, vec) - lam[:, :1] * vec, axis=1)
        worst_r = max(worst_r, float(np.max(resid / trace)))
        worst_sweeps = max(worst_sweeps, int(sweeps.max()))
        assert np.max(np.abs(np.linalg.norm(vec, axis=1) - 1.0)) <= 1e-12
        assert not vec[:, 0].imag.any() and np.all(vec[:, 0].real >= 0)
        assert np.all(np.diff(lam, axis=1) <= 0) and lam.min() >= 0.0
        for b, kind in enumerate(kinds):      # a zero row is never rotated: its eigenvalue is exactly 0
            if kind == 'zero row':
                assert lam[b, -1] == 0.0
        capped = EO.jacobi_emulation(batch, cap)      # ... and the kernel's cap changes nothing
        assert capped[0].tobytes() == lam.tobytes() and capped[1].tobytes() == vec.tobytes()
    print('jacobi emulation, %d matrices: worst sweep count %d (kernel cap %d), eigenvalues %.1e of the trace, residual %.1e of the trace'
          % (count, worst_sweeps, cap, worst_l, worst_r))
    assert count == 1400
    assert worst_l <= 1e-12 and worst_r <= 1e-12
    assert cap == worst_sweeps + 2


def test_emulation_takes_one_matrix():
    A = wishart(np.random.default_rng(5), 4, 9, 'common')
    lam, vec, sweeps = EO.jacobi_emulation(A, kernel_cap())
    assert lam.shape == (4,) and vec.shape == (4,) and 1 <= sweeps <= kernel_cap()
    assert np.max(np.abs(lam - np.linalg.eigvalsh(A)[::-1])) <= 1e-12 * np.trace(A).real
    lam, vec, sweeps = EO.jacobi_emulation(np.zeros((3, 3)), kernel_cap())
    assert not lam.any() and sweeps == 0 and np.array_equal(vec, [1.0, 0.0, 0.0])


# ---- 2. identities of the oracle ----------------------------------------------------------------------------------------------

def test_oracle_identities():
    rng = np.random.default_rng(21)
    for C in (2, 3, 5, 8):
        x = noise(rng, (C, 128 * 12)) + 0.8 * noise(rng, 128 * 12)[None, :]
        s, g = EO.eig(x, 128, detrend=False, of='S'), EO.eig(x, 128, detrend=False, of='G')
        ref = s['ref']
        tr = np.einsum('aaj->j', ref['S']).real
        assert np.max(np.abs(s['eig'].sum(axis=0) - tr) / tr) <= 1e-12
        assert np.max(np.abs((1.0 - np.prod(g['eig'], axis=0)) - ref['gcoh'])) <= 1e-12
        assert np.max(np.abs(g['eig'].sum(axis=0) - C)) <= 1e-12
        gains = rng.uniform(0.01, 100.0, C) * np.exp(2j * np.pi * rng.random(C))
        g2 = EO.eig(x * gains[:, None], 128, detrend=False, of='G')
        assert np.max(np.abs(g2['eig'] - g['eig'])) <= 1e-12
        if C == 2:
            root = np.sqrt(ref['gcoh'])
            assert np.max(np.abs(g['eig'] - np.array([1.0 + root, 1.0 - root]))) <= 1e-12
        for r in (s, g):      # the vector: unit norm, the phase convention, an eigenvector of the matrix
            v, l1 = r['vec'].T, r['eig'][0]
            assert np.max(np.abs(np.linalg.norm(v, axis=1) - 1.0)) <= 1e-12 and not v[:, 0].imag.any() and np.all(v[:, 0].real >= 0)
            resid = np.linalg.norm(np.einsum('jac,jc->ja', r['A'], v) - l1[:, None] * v, axis=1)
            assert np.max(resid / np.einsum('jaa->j', r['A']).real) <= 1e-12


# ---- 3. degenerate rules of the oracle -----------------------------------------------------------------------------------------

def test_oracle_degenerate_rules():
    rng = np.random.default_rng(11)
    x = noise(rng, (3, 64 * 6))
    x[1] = 0.0
    s, g = EO.eig(x, 64, of='S'), EO.eig(x, 64, of='G')
    assert np.all(s['eig'][2] == 0.0) and np.all(s['eig'][1] > 0.0) and np.abs(s['vec'][1]).max() <= 1e-15
    assert np.all(g['eig'] == 1.0) and np.all(g['vec'][0] == 1.0) and not g['vec'][1:].any()
    z = EO.eig(np.zeros_like(x), 64, of='S')
    assert not z['eig'].any() and np.all(z['vec'][0] == 1.0) and not z['vec'][1:].any()
    x[1] = noise(rng, 64 * 6)
    x[1, 100] = np.nan
    for of in 'SG':
        r = EO.eig(x, 64, of=of)
        assert np.isnan(r['eig']).all() and np.isnan(r['vec'].real).all() and np.isnan(r['vec'].imag).all()
    for of in 'SG':
        one = EO.eig(noise(rng, (4, 64)), 64, detrend=False, of=of)      # M = 1: rank one
        assert one['M'] == 1
        tr = np.einsum('jaa->j', one['A']).real
        assert np.max(np.abs(one['eig'][0] - tr) / tr) <= 1e-12 and np.max(one['eig'][1:] / tr) <= 1e-12
        few = EO.eig(noise(rng, (4, 64 * 3)), 64, of=of)                 # M < C: singular
        assert few['M'] == 3 and np.max(few['eig'][3] / np.einsum('jaa->j', few['A']).real) <= 1e-12 and np.all(few['eig'][2] > 0)


# ---- 4. eigenvalue_stats -------------------------------------------------------------------------------------------------------

def check_source_count(nsrc_shifted, signal=True, what=''):
    """the MDL count on a fftshifted row of the detection capture: 1 in at least 90 % of the band's bins, 0 in at least 90 % of
    the bins outside (DET_GUARD bins on either side of a band edge count for neither, as in check_detection); without the
    signal 0 in at least 90 % of all bins -> the shares"""
    n = np.asarray(nsrc_shifted)
    assert n.shape == (DET_NFFT,)
    if not signal:
        share = float(np.mean(n == 0))
        print('nsrc %s: 0 in %.1f %% of all bins' % (what, 100 * share))
        assert share >= 0.9
        return share,
    inband = float(np.mean(n[DET_GUARD:DET_BAND - DET_GUARD] == 1))
    outband = float(np.mean(n[DET_BAND + DET_GUARD:DET_NFFT - DET_GUARD] == 0))
    print('nsrc %s: 1 in %.1f %% of the band, 0 in %.1f %% outside' % (what, 100 * inband, 100 * outband))
    assert inband >= 0.9 and outband >= 0.9
    return inband, outband


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_source_count_on_the_detection_capture(seed):
    from ofdm_tools import ofdm_cr_tools as T
    r = EO.eig(detection_capture(seed), DET_NFFT, detrend=False, of='S')
    assert r['M'] == DET_M
    stats = T.eigenvalue_stats(np.fft.fftshift(r['eig'], axes=-1), DET_M)
    assert stats['nsrc'].dtype.kind == 'i' and stats['mme'].shape == stats['agm'].shape == (DET_NFFT,)
    check_source_count(stats['nsrc'], True, 'oracle, seed %d' % seed)
    off = EO.eig(detection_capture(seed, signal=False), DET_NFFT, detrend=False, of='S')
    check_source_count(T.eigenvalue_stats(np.fft.fftshift(off['eig'], axes=-1), DET_M)['nsrc'], False, 'oracle, no signal, seed %d' % seed)
    assert np.all(T.eigenvalue_stats(r['eig'], DET_C - 1)['nsrc'] == -1)      # M < C


def test_eigenvalue_stats_rules():
    from ofdm_tools import ofdm_cr_tools as T
    nan = np.nan
    rows = np.array([[4.0, 1.0], [3.0, 0.0], [0.0, 0.0], [nan, nan], [2.0, 2.0], [np.inf, 1.0]]).T      # [C = 2, m = 6]
    st = T.eigenvalue_stats(rows, 10)
    assert st['mme'][0] == 4.0 and st['mme'][1] == np.inf and np.isnan(st['mme'][2]) and np.isnan(st['mme'][3]) and st['mme'][4] == 1.0
    assert st['agm'][0] == 2.5 / 2.0 and st['agm'][1] == np.inf and st['agm'][2] == np.inf and np.isnan(st['agm'][3])
    assert abs(st['agm'][4] - 1.0) <= 1e-15
    assert list(st['nsrc'][1:4]) == [-1, -1, -1] and st['nsrc'][5] == -1 and st['nsrc'][4] == 0
    # MDL by hand at C = 3, M = 50: eigenvalues (10, 1, 1) hold one source, (1, 1, 1) none
    st = T.eigenvalue_stats(np.array([[10.0, 1.0], [1.0, 1.0], [1.0, 1.0]]), 50)
    assert list(st['nsrc']) == [1, 0]
    M, C, l = 50, 3, np.array([10.0, 2.0, 1.0])
    mdl = [-M * (C - k) * np.log(np.exp(np.log(l[k:]).mean()) / l[k:].mean()) + 0.5 * k * (2 * C - k) * np.log(M) for k in range(C)]
    assert T.eigenvalue_stats(l[:, None], M)['nsrc'][0] == int(np.argmin(mdl))
    assert np.all(T.eigenvalue_stats(np.ones((4, 5)), 3)['nsrc'] == -1)
    with pytest.raises(ValueError):
        T.eigenvalue_stats(np.ones(4), 8)


# ---- the share of bins the GPU suite's direction gate leaves out, on the oracle --------------------------------------------------

def test_gap_condition_on_the_parity_cases():
    """the GPU suite checks the vector's direction where the oracle's gap l_1 - l_2 is at least 0.1 l_1 and lets at most 25 %
    of a case's bins fall outside: the same count on the oracle for every parity case up to 1024 points"""
    from test_welch_matrix_gpu import PARITY_CASES, capture
    from stat_support import FS
    worst = 0.0
    for nfft, C, M, frac, ov, detrend, scaling, fftshift, trim64, db, offset in PARITY_CASES:
        if nfft > 1024:
            continue
        nperseg = nfft * frac // 16
        noverlap = nperseg * ov // 100
        step = nperseg - noverlap
        x = capture(C, noverlap + M * step + step // 3, 7 * nfft + 13 * C + M, nfft, M, offset)
        ref = XO.matrix(x, nfft, nperseg, noverlap, 'hann', detrend, scaling, FS)
        for of in 'SG':
            lam = EO.eig(None, nfft, of=of, ref=ref)['eig']
            share = float(np.mean(lam[0] - lam[1] < 0.1 * lam[0]))
            worst = max(worst, share)
            assert share <= 0.25, (nfft, C, M, of, share)
    print('bins outside the gap condition, worst parity case up to 1024 points: %.1f %%' % (100 * worst))


# ---- 5. eigen_scan's refusals, before a context exists -------------------------------------------------------------------------

def test_eigen_scan_refuses_in_python():
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros((4, 256 * 8), np.complex64)
    for nfft in (100, 32, 32768):
        with pytest.raises(ValueError) as ei:
            T.eigen_scan(x, nfft, 1.0)
        assert str(ei.value).startswith('eigen_scan needs nFFT a power of two from 64 to 16384')
    for bad in (x[0], x[:1], np.zeros((9, 2048), np.complex64)):
        with pytest.raises(ValueError) as ei:
            T.eigen_scan(bad, 256, 1.0)
        assert str(ei.value).startswith('eigen_scan needs a (C, n) array of 2 ... 8 channels')
    with pytest.raises(ValueError) as ei:
        T.eigen_scan(x[:, :255], 256, 1.0)
    assert str(ei.value) == 'eigen_scan needs at least nFFT = 256 samples per channel'
    with pytest.raises(ValueError) as ei:
        T.eigen_scan(x, 256, 0.0)
    assert str(ei.value) == 'eigen_scan needs a sample rate Sf > 0'


# ---- 6. surface, 7. resources ---------------------------------------------------------------------------------------------------

def test_surface_is_declared_and_exported():
    from ofdm_tools import _hip
    assert (_hip.EIG_OF_S, _hip.EIG_OF_G) == (0, 1)
    check_surface(SYMBOLS, 'WelchPlan', ('matrix_eig', 'matrix_eig_dev'),
                  ['int of, float *eig_out_dev, float *vec_out_dev, uint64_t *nseg_out);', '#define OTH_EIG_OF_G 1'])


def test_every_mat_eig_kernel_build_has_no_scratch():
    """one thread per bin with its matrix in its own LDS column: read from the code objects inside the built library, the
    builds (channel capacity 2, 4, 8) x (without, with the vector), 64 threads each, have a private segment of 0 bytes and no
    spilled register; the matrix family's kernels next to them keep theirs"""
    check_builds('mat_eig_kernel', [(cc, vec) for cc in (2, 4, 8) for vec in (False, True)], {64: 512},
                 extra_kernels=('mat_finalize_kernel', 'mat_det_kernel'))
