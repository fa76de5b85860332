"""CPU checks of the direction spectra of the spectral matrix (no GPU): the oracle's eigen-form against its direct form
(tests/welch_doa_oracle.py), the resolution statement of the three methods on a synthesised line-array capture, the Python
helpers (ula_delays, doa_band_combine) and doa_scan's refusals, the declared surface and the resource figures of every
mat_doa_kernel build and of mateig.hip's basis build read from the code objects of the built library.
Measured here: the two forms of Bartlett agree to 1.3e-14 and of Capon to 4.2e-14 relative (gate 1e-10); on the two-source
capture (5 and 14 degrees, 10 dB each, 8 channels) the band-combined Capon and MUSIC spectra peak at 5 and 14 degrees for seeds
0, 1, 2 and Bartlett's one peak lies at 10, 9 and 10 degrees."""
import numpy as np
import pytest

import welch_doa_oracle as DO
from stat_support import check_builds, check_surface
from test_welch_matrix_cpu import noise

SYMBOLS = ('oth_welch_set_steering', 'oth_welch_matrix_doa_dev', 'oth_welch_matrix_doa')
GRID = np.arange(-90, 91)      # a 1 degree grid
RES = dict(C=8, nfft=256, M=32, angles=(5, 14), snr=(10, 10), fc=2.0, nsrc=2, loading=1e-2)


def angles_of(row, count):
    """the `count` highest local maxima of a row over GRID, in degrees, ascending"""
    return sorted(int(GRID[i]) for i in DO.peaks(row)[:count])


def check_resolution(combined, what=''):
    """the resolution statement on the band-combined spectra of the two-source capture: Capon's and MUSIC's two highest local
    maxima are the sources' own directions; Bartlett does not resolve them - its highest maximum lies between them, from 7 to
    12 degrees, it is the only one from the first source to the second, and neither source is one"""
    capon, music, bartlett = (angles_of(combined[m], 2) for m in ('capon', 'music', 'bartlett'))
    between = [int(GRID[i]) for i in DO.peaks(combined['bartlett']) if RES['angles'][0] <= GRID[i] <= RES['angles'][1]]
    top = int(GRID[DO.peaks(combined['bartlett'])[0]])
    print('resolution %s: capon %s, music %s, bartlett %s from source to source, its highest at %d' % (what, capon, music, between, top))
    assert capon == list(RES['angles']) and music == list(RES['angles'])
    assert 7 <= top <= 12 and between == [top]


# ---- 1. the two forms of the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C,loading', [(2, 0.0), (3, 1e-2), (5, 0.0), (8, 1e-2)])
def test_eigen_form_against_the_direct_form(C, loading):
    rng = np.random.default_rng(40 + C)
    nfft, M = 64, 12
    x = noise(rng, (C, nfft * M)) + 2.0 * noise(rng, nfft * M)[None, :] * np.exp(2j * np.pi * rng.random(C))[:, None]
    delays = rng.uniform(-3.0, 3.0, (9, C))
    worst = 0.0
    for of in 'SG':
        r = DO.doa(x, nfft, delays, 1000.25, of=of, nsrc=1, loading=loading, direct=True)
        for m in ('bartlett', 'capon'):
            assert np.all(np.isfinite(r[m])) and r[m].min() > 0.0
            worst = max(worst, float(np.max(np.abs(r[m + '_direct'] / r[m] - 1.0))))
        assert np.all(np.isfinite(r['music'])) and r['music'].min() >= 1.0 - 1e-12      # sum_{i > nsrc} p_i <= |w|^2 = C
    print('eigen-form against the direct form, C = %d loading %g: %.1e relative' % (C, loading, worst))
    assert worst <= 1e-10


def test_oracle_rules():
    rng = np.random.default_rng(3)
    nfft, C = 64, 3
    x = noise(rng, (C, nfft * 6))
    delays = rng.uniform(-2.0, 2.0, (4, C))
    zero = DO.doa(x, nfft, np.zeros((1, C)), 0.0, detrend=False, direct=True)      # w = 1: the sum of all entries
    total = zero['ref']['S'].sum(axis=(0, 1)).real / C ** 2
    assert np.max(np.abs(zero['bartlett'][0] - total) / total) <= 1e-12
    alone = DO.doa(x, nfft, delays[2:3], 0.3, nsrc=2, loading=1e-2)
    among = DO.doa(x, nfft, delays, 0.3, nsrc=2, loading=1e-2)
    for m in ('bartlett', 'capon', 'music'):
        assert np.array_equal(alone[m][0], among[m][2])
    # a whole number of carrier cycles per delay changes nothing; of G a positive gain per channel drops out
    a = DO.doa(x, nfft, delays, 0.0, of='G', loading=1e-2)
    b, c = (DO.doa(x, nfft, np.round(delays), fc, of='G', loading=1e-2) for fc in (5.0, 0.0))
    assert np.max(np.abs(b['capon'] / c['capon'] - 1.0)) <= 1e-9
    g = DO.doa(x * np.array([0.1, 7.0, 3.0])[:, None], nfft, delays, 0.0, of='G', loading=1e-2)      # (a phase would steer)
    assert np.max(np.abs(g['capon'] / a['capon'] - 1.0)) <= 1e-9 and np.max(np.abs(g['bartlett'] / a['bartlett'] - 1.0)) <= 1e-9
    y = x.copy()
    y[1] = 0.0
    silent = DO.doa(y, nfft, delays, 0.3, of='S', loading=0.0)
    assert not silent['capon'].any() and np.all(silent['bartlett'] > 0.0)
    y[1, 70] = np.inf
    nan = DO.doa(y, nfft, delays, 0.3)
    assert all(np.isnan(nan[m]).all() for m in ('bartlett', 'capon', 'music'))


# ---- 2. resolution ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1, 2])
def test_capon_and_music_resolve_what_bartlett_does_not(seed):
    x = DO.doa_capture(RES['C'], RES['nfft'], RES['M'], RES['angles'], RES['snr'], seed, fc=RES['fc'])
    r = DO.doa(x, RES['nfft'], DO.ula_delays(RES['C'], GRID, RES['fc']), RES['fc'], nsrc=RES['nsrc'], loading=RES['loading'])
    assert r['M'] == RES['M']
    check_resolution(DO.combine(r), 'oracle, seed %d' % seed)


def test_a_single_source_peaks_at_its_direction_in_all_three():
    x = DO.doa_capture(4, 256, 32, (-20,), (6,), 0, fc=2.0)
    c = DO.combine(DO.doa(x, 256, DO.ula_delays(4, GRID, 2.0), 2.0, nsrc=1, loading=1e-2))
    for m in ('bartlett', 'capon', 'music'):
        assert int(GRID[np.argmax(c[m])]) == -20 and angles_of(c[m], 1) == [-20], m


# ---- 3. the Python helpers and doa_scan's refusals, before a context exists ---------------------------------------------------

def test_python_helpers():
    from ofdm_tools import ofdm_cr_tools as T
    tab = T.ula_delays(8, GRID, 0.5, 2.0)
    assert tab.shape == (181, 8) and tab.dtype == np.float64 and np.array_equal(tab, DO.ula_delays(8, GRID, 2.0))
    assert T.ula_delays(2, 30.0, 1.0, 4.0).shape == (1, 2) and abs(T.ula_delays(2, 30.0, 1.0, 4.0)[0, 1] - 0.125) <= 1e-15
    for args in ((1, GRID, 0.5, 2.0), (9, GRID, 0.5, 2.0), (4, GRID, 0.5, 0.0), (4, GRID, 0.0, 2.0), (4, [91.0], 0.5, 2.0), (4, [], 0.5, 2.0)):
        with pytest.raises(ValueError):
            T.ula_delays(*args)
    rng = np.random.default_rng(8)
    rows = {m: rng.uniform(0.5, 2.0, (5, 64)) for m in ('bartlett', 'capon', 'music')}
    for band in (None, (3, 40)):
        got, want = T.doa_band_combine(rows, band), DO.combine(rows, band)
        assert all(np.array_equal(got[m], want[m]) for m in rows)


def test_doa_scan_refuses_in_python():
    from ofdm_tools import ofdm_cr_tools as T
    x = np.zeros((4, 256 * 8), np.complex64)
    tab = np.zeros((5, 4))
    for nfft in (100, 32, 32768):
        with pytest.raises(ValueError) as ei:
            T.doa_scan(x, nfft, 1.0, tab, 2.0, 1)
        assert str(ei.value).startswith('doa_scan needs nFFT a power of two from 64 to 16384')
    with pytest.raises(ValueError) as ei:
        T.doa_scan(x, 256, 0.0, tab, 2.0, 1)
    assert str(ei.value) == 'doa_scan needs a sample rate Sf > 0'
    for bad in (x[0], x[:1], np.zeros((9, 2048), np.complex64)):
        with pytest.raises(ValueError) as ei:
            T.doa_scan(bad, 256, 1.0, tab, 2.0, 1)
        assert str(ei.value).startswith('doa_scan needs a (C, n) array of 2 ... 8 channels')
    with pytest.raises(ValueError) as ei:
        T.doa_scan(x[:, :255], 256, 1.0, tab, 2.0, 1)
    assert str(ei.value) == 'doa_scan needs at least nFFT = 256 samples per channel'
    nan_tab = tab.copy()
    nan_tab[1, 2] = np.nan
    for bad in (tab[0], tab[:, :3], np.zeros((0, 4)), np.zeros((1025, 4)), nan_tab):
        with pytest.raises(ValueError) as ei:
            T.doa_scan(x, 256, 1.0, bad, 2.0, 1)
        assert str(ei.value).startswith('doa_scan needs finite delays of shape (D, 4), 1 <= D <= 1024')
    with pytest.raises(ValueError) as ei:
        T.doa_scan(x, 256, 1.0, tab, np.inf, 1)
    assert str(ei.value) == 'doa_scan needs a finite carrier fc in cycles per sample'
    for nsrc in (0, 4, 1.5, None):
        with pytest.raises(ValueError) as ei:
            T.doa_scan(x, 256, 1.0, tab, 2.0, nsrc)
        assert str(ei.value).startswith('doa_scan needs nsrc in 1 ... 3')
    for loading in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError) as ei:
            T.doa_scan(x, 256, 1.0, tab, 2.0, 1, loading=loading)
        assert str(ei.value) == 'doa_scan needs a finite loading >= 0'
    for band in ((5, 5), (-1, 9), (0, 257), (3,), (1.0, 9)):
        with pytest.raises(ValueError) as ei:
            T.doa_scan(x, 256, 1.0, tab, 2.0, 1, band=band)
        assert str(ei.value).startswith('doa_scan needs band = (lo, hi)')


# ---- 4. surface, 5. resources -----------------------------------------------------------------------------------------------------

def test_surface_is_declared_and_exported():
    from ofdm_tools import _hip
    assert _hip.WelchPlan.DOA_METHODS == ('bartlett', 'capon', 'music')
    check_surface(SYMBOLS, 'WelchPlan', ('set_steering', 'matrix_doa', 'matrix_doa_dev'),
                  ['int oth_welch_set_steering(oth_plan *plan, int ndir, int nchan, const double *delays, double fc);',
                   'double loading, float *bartlett_out_dev, float *capon_out_dev, float *music_out_dev, uint64_t *nseg_out);',
                   '#define OTH_DOA_DIRS_MAX 1024'])


def test_every_direction_stage_build_has_no_scratch():
    """read from the code objects inside the built library: mat_doa_kernel at the channel capacities 2, 4, 8 (256 threads: 64
    bins x 4 direction lanes) and mateig.hip's basis build at the same capacities (64 threads) have a private segment of 0
    bytes and no spilled register - every loop over channels is unrolled under uniform guards, nothing is indexed dynamically"""
    check_builds('mat_doa_kernel', [2, 4, 8], {256: 512})
    check_builds('mat_eig_basis_kernel', [2, 4, 8], {64: 512})
