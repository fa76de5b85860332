"""What tests/test_degenerate_gpu.py assumes of the oracle and of its own inputs, pinned without a GPU:
  * R.welch_np is NaN in every bin for one NaN / +inf / -inf sample, in either part, with and without the detrend
    (numpy's transform turns an inf into NaN everywhere: inf times a twiddle zero), and R.chain_psd_logger's peak is NaN from
    the bad vector on while the vectors before it are untouched;
  * zeros and a detrended constant give exact zeros in the oracle, -inf in dB;
  * the overflow gain of every route that takes the overflow case (58 at 256 points, 55 at 4096), a non-empty class of bins
    that must read NaN, at most 2 % of the bins in the class that may read either way;
  * gains of 2^+-20 keep every oracle value inside float32's normal range, so that out(x 2^k) = out(x) 4^k can hold bit for
    bit;
  * the route table names the kernels the library's routing gives for these shapes (oth__debug_recipe, no device)."""
import os

import numpy as np
import pytest

import degenerate_cases as D
from oracle import ref_cpu as R

SIZES = {256: 'generic-256', 1000: 'any-1000', 4096: 'w4096-ws'}


@pytest.mark.parametrize('nfft', sorted(SIZES))
def test_oracle_is_nan_in_every_bin_for_one_bad_sample(nfft):
    route = SIZES[nfft]
    x = D.stream(route)
    for pos in D.positions(len(x)):
        for name, bad in D.BAD.items():
            for part in ('re', 'im'):
                for detrend in ('constant', 'none'):
                    ref = D.reference(route, D.poisoned(x, pos, bad, part), detrend)
                    assert ref.shape == (nfft,) and np.isnan(ref).all(), (nfft, pos, name, part, detrend)
    assert np.isfinite(D.clean_reference(route)).all()


def test_poisoned_touches_one_float_only():
    x = D.stream('generic-256')
    for part in ('re', 'im'):
        v = D.poisoned(x, 7, float('inf'), part)
        changed = np.flatnonzero(v.view(np.uint32) != np.asarray(x).view(np.uint32))
        assert list(changed) == [14 + (part == 'im')] and not x.flags.writeable
    assert D.positions(100) == (51, 0)
    assert D.segments_holding('segws-1024', D.shape('segws-1024')['nsamples'] // 2 + 1) == [4, 5]
    assert D.segments_holding('segws-1024', 0) == [0] and D.segments_holding('w4096-step', 4095) == [0, 1]


@pytest.mark.parametrize('form', ['peak', 'iir', 'sensor'])
@pytest.mark.parametrize('bad', sorted(D.BAD))
def test_chain_oracle_state_is_non_finite_from_the_bad_vector_on(form, bad):
    nfft = 256
    x = D.chain_stream(nfft)
    v = D.poisoned(x, D.CHAIN_BAD_VECTOR * nfft + nfft // 2 + 1, D.BAD[bad])
    rows0, state0 = D.chain_reference(form, x, nfft)
    with np.errstate(invalid='ignore'):
        rows, state = D.chain_reference(form, v, nfft)
    assert rows.shape == (D.CHAIN_VECTORS, nfft)
    k = D.CHAIN_BAD_VECTOR
    assert np.array_equal(rows[:k], rows0[:k])
    if form == 'iir':      # the dB rows carry the filter's memory
        assert not np.isfinite(rows[k:]).any()
    else:
        assert not np.isfinite(rows[k]).any() and np.array_equal(rows[k + 1:], rows0[k + 1:])
    if state is not None:
        assert np.array_equal(state[:k], state0[:k]) and not np.isfinite(state[k:]).any()
    if form == 'peak' and bad == 'nan':      # np.maximum keeps the NaN: the specification of the device's peak hold.  (An inf
        assert np.isnan(state[k:]).all()     # sample: np.abs(nan + inf j) = inf in some bins - NaN against inf is not pinned)


def test_chain_oracle_ignores_a_bad_sample_in_a_dropped_vector():
    nfft = 256
    x = D.chain_stream(nfft)
    v = D.poisoned(x, 4 * nfft + 3, float('nan'))      # keep_one_in_n = 2 keeps vectors 1, 3, 5, ...
    for form in D.CHAIN_FORMS:
        a, b = D.chain_reference(form, x, nfft, 2), D.chain_reference(form, v, nfft, 2)
        assert len(a[0]) == D.CHAIN_VECTORS // 2 and np.array_equal(a[0], b[0])
        assert a[1] is None or np.array_equal(a[1], b[1])


@pytest.mark.parametrize('route', ['generic-256', 'any-1000', 'segpad-1024', 'w16384-x1', 'mtm-1024'])
def test_silence_and_a_detrended_constant_are_exact_zeros_in_the_oracle(route):
    r = D.shape(route)
    zeros = np.zeros(r['nsamples'], np.complex64)
    const = np.full(r['nsamples'], D.CONSTANT, np.complex64)
    for detrend in r['detrends']:
        ref = D.reference(route, zeros, detrend)
        assert ref.shape == (r['nfft'],) and np.all(ref == 0)
        with np.errstate(divide='ignore'):
            assert np.all(np.isneginf(10.0 * np.log10(ref)))
    if 'constant' in r['detrends']:
        assert np.all(D.reference(route, const, 'constant') == 0)      # 3 - 2j: the float64 mean is exact
    # ... and without the detrend the line is there: the bound of the fast detrend is a small part of it
    line = D.reference(route, const, 'none')
    assert 0 < D.constant_fast_bound(route) < 1e-12 * line.max() * 10


@pytest.mark.parametrize('route', D.OVERFLOW_ROUTES)
def test_overflow_classes(route):
    nfft = D.ROUTES[route]['nfft']
    detrend = D.shape(route)['detrends'][0]
    g, must_nan, must_right, either = D.overflow_case(route, detrend)
    p = D.segment_powers(route, D.stream(route), detrend)
    assert p.max() * 4.0 ** g < 2.0 ** 134 <= p.max() * 4.0 ** (g + 1)
    assert {256: 58, 4096: 55}.get(nfft, g) == g, (route, g)
    assert np.sqrt(p.max()) * 2.0 ** g < 2.0 ** 67                       # amplitudes: only the squaring overflows
    x = D.gained(D.stream(route), g)
    assert np.isfinite(x.view(np.float32)).all() and np.abs(x.view(np.float32)).max() < 2.0 ** 67
    n_nan, n_either = int(must_nan.sum()), int(either.sum())
    print('overflow classes | %s g %d | must be NaN %d, either %d, must be right %d' % (route, g, n_nan, n_either, int(must_right.sum())))
    assert n_nan >= 1 and n_either <= 0.02 * nfft, (route, n_nan, n_either)
    assert not (must_nan & must_right).any() and (must_nan | must_right | either).all()
    # the bins that must be right are representable: the scaled reference stays below FLT_MAX
    ref = D.clean_reference(route, detrend) * 4.0 ** g
    assert ref[must_right].max() < D.FLT_MAX / 2 and ref[must_right].min() > D.FLT_MIN


@pytest.mark.parametrize('route', sorted(D.ROUTES))
def test_power_of_two_gains_stay_inside_the_normal_range(route):
    for detrend in D.shape(route)['detrends']:
        ref = D.clean_reference(route, detrend)
        for k in (20, -20):
            v = ref * 4.0 ** k
            assert v.min() > D.FLT_MIN * 2.0 ** 24 and v.max() < D.FLT_MAX * 2.0 ** -24, (route, detrend, k)
    x = D.stream(route)
    for k in (20, -20):      # the gain itself is exact
        assert np.array_equal(D.gained(x, k).astype(np.complex128), np.asarray(x, np.complex128) * 2.0 ** k)


def test_route_table_names_the_kernels_the_routing_gives():
    """oth__debug_recipe (pure host logic, csrc/abi_route.hip) for every Welch route and every detrend mode it accepts, at
    nine segments in one stream, under the library's schedule and under the two static ones the GPU file forces: the kernel
    the table names.  One exception, as the routing documents: the role-split 8192-point build walks contiguous runs only and
    hands an interleaved schedule to the one-role kernel."""
    import recipes
    from ofdm_tools import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built yet')
    lib = recipes._lib()
    codes = {'none': 0, 'constant': 1, 'fast': 3}
    kernels = {'auto': 0, 'generic': 1, 'tuned': 2}
    for route in sorted(D.ROUTES):
        r = D.shape(route)
        if r['mtm']:
            continue
        for detrend in r['detrends']:
            for sched in (2, 0, 1):
                rec = recipes.recipe(lib, r['nfft'], r['nperseg'], r['noverlap'], window=0 if r['window'] == 'boxcar' else 1,
                                     detrend=codes[detrend], kernel=kernels[r['kernel']], variant=r['tuning'], sched=sched,
                                     nseg=D.NSEG)
                want = r['recipe']
                if route == 'w8192-split' and sched == 1:
                    want = 'kernel=welch16k1x_half '
                assert rec.startswith(want), (route, detrend, sched, rec)
