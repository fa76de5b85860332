"""CPU checks of the seeded random-shape cases of the core Welch and CSD routes (tests/core_fuzz_cases.py; no GPU, but the
built library: the routes come from oth__debug_recipe_tuned): the list is a function of the seed and pinned by a digest,
every case lies inside the domain the header documents and under the cap, the drawn routes are exactly the routes the
routing has, class A covers the output stages, scalings and detrend modes, class C walks unequal runs under every
schedule a route honours, the oracle alone - under a single-precision transform - meets half of every gate, and the
layout detects a read past a stream's samples and a read from the neighbouring stream."""
import os

import numpy as np
import pytest

from ofdm_tools import _hip

if not os.path.exists(_hip.LIB_PATH):
    pytest.skip('library not built yet', allow_module_level=True)

import core_fuzz_cases as K  # noqa: E402 - after the skip
import fuzz_layout as FL  # noqa: E402

DIGEST = 'd963af54feb67544d3c00b94bddecc3032c73e5a9070ffea244faee502461b91'      # sha256 of repr(all_cases(K.SEED))


@pytest.fixture(scope='module')
def suite():
    return K.all_cases(K.SEED)


# ---- a. determinism ----------------------------------------------------------------------------------------------------------------

def test_the_same_seed_gives_the_same_list_and_the_suites_list_is_pinned(suite):
    assert K.all_cases(K.SEED) == suite and K.all_cases(5) == K.all_cases(5) and K.all_cases(5) != K.all_cases(6)
    assert len(suite) == 3 * len(K.DRAWN) and [c.cls for c in suite] == list(K.CLASSES) * len(K.DRAWN)
    assert K.digest(K.SEED) == DIGEST, 'the case list moved: every change of it shows as a change of this literal'


# ---- b. domain -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [K.SEED, 1, 2, 3, 4, 5])
def test_every_case_lies_inside_the_documented_domain_and_names_its_route(seed, suite):
    lib = K.recipes._lib()
    for c in (suite if seed == K.SEED else K.all_cases(seed)):
        K.check_domain(c)
        for L in c.launches:
            text = K.predicted(c, L, lib)
            assert K.names(text, c.route), (text, K.shape_text(c, L))
        if c.cls == 'A':
            assert c.launches == (K.Launch(c.launches[0].nseg, 1, 0, 0),) and c.launches[0].nseg in K.NSEGS
        if c.cls == 'B':
            L, = c.launches
            assert (L.nstreams == 1 if c.route.two else 2 <= L.nstreams <= 5) and L.sched == -1 and L.nseg in K.NSEGS
            assert c.gap in (0, 1, 67) or (c.gap - 3) % 64 == 0 and 1 <= (c.gap - 3) // 64 <= 4
    # the layout of the suite's small cases: NaN everywhere but the samples each stream's whole segments cover
    if seed == K.SEED:
        for c in suite:
            if c.cls == 'B':
                L = c.launches[0]
                for buf, lead in K.layout(c):
                    lanes = 1 if c.route.two else L.nstreams
                    assert buf.dtype == np.complex64 and len(buf) == lead + (lanes - 1) * K.stride(c, L) + K.nsamples(c, L) + FL.BEHIND
                    finite = np.isfinite(buf.view(np.float32)).reshape(-1, 2).all(axis=1)
                    want = np.zeros(len(buf), bool)
                    for i in range(lanes):
                        want[lead + i * K.stride(c, L):lead + i * K.stride(c, L) + K.owned(c, L)] = True
                    assert np.array_equal(finite, want)


# ---- c. coverage ---------------------------------------------------------------------------------------------------------------------

def test_the_drawn_routes_are_the_routes_the_routing_has(suite):
    """a route resolve_recipe() gains fails here until DRAWN lists it; one struck out of DRAWN fails here too"""
    derived = {K.route_id(r) for r in K.witnesses()}
    assert len(set(K.DRAWN)) == len(K.DRAWN)
    assert derived == set(K.DRAWN), ('not drawn: %s; drawn but not derived: %s' % (sorted(derived - set(K.DRAWN)), sorted(set(K.DRAWN) - derived)))
    assert not any('anyfft' in i for i in K.DRAWN)
    # the kernels the issue names, the words it names
    kernels = {r.kernel for r in K.routes()}
    assert {'welch4096:ws', 'welch4096:pipe', 'welch4096:dpp', 'seg:half', 'seg:full', 'segws', 'seg_padded:half', 'seg_padded:full', 'welch16k',
            'welch16k1x:pipe', 'welch16k1x_half', 'welch16k1x_half:ws', 'csd4096ws', 'csd4096', 'welch_generic'} <= kernels
    assert {r.word for r in K.routes()} == set(K.WORDS) | {''}
    # the suite's seed reaches every route once per class
    reached = {(K.route_id(c.route), c.cls) for c in suite}
    assert reached == {(i, cls) for i in K.DRAWN for cls in K.CLASSES}


def test_class_a_covers_the_output_stages_scalings_and_detrend_modes(suite):
    A = [c for c in suite if c.cls == 'A']
    assert {(c.fftshift, c.trim > 0, c.db) for c in A if not c.route.two} == {(s, t, d) for s in (False, True) for t in (False, True) for d in (False, True)}
    assert {c.scaling for c in A} == set(K.SCALINGS) and {c.detrend for c in A} == set(K.DETREND_CODE)
    assert {c.window for c in suite} == set(K.WINDOWS)
    # both sides of kFdMinSegments, for the routes that exist on both
    for r in K.routes():
        W = K.witnesses()[r]
        if any(w.few for w in W) and any(not w.few for w in W):
            counts = {L.nseg for seed in (K.SEED, 1, 2, 3, 4, 5) for c in K.cases(r, seed)[:2] for L in c.launches}
            assert min(counts) < 8 <= max(counts), (K.route_id(r), counts)
    assert any(c.offset for c in suite) and any(not c.offset and c.detrend == 'constant' for c in suite)


def test_class_c_walks_unequal_runs_under_every_schedule_a_route_honours(suite):
    lib = K.recipes._lib()
    lone, one_sided = [], []
    for c in suite:
        if c.cls != 'C':
            continue
        rid = K.route_id(c.route)
        texts = [K.predicted(c, L, lib) for L in c.launches]
        if rid in K.NO_WALK:
            assert not any(K.walks(t, L) for t, L in zip(texts, c.launches))
            continue
        assert all(K.walks(t, L) for t, L in zip(texts, c.launches)), (rid, texts)                  # W < nseg with a remainder
        scheds = K.schedules(lib, K.shape_of(c), c.route)
        if c.route.kernel == 'welch_generic':
            assert all(L.sched == -1 for L in c.launches)
            assert c.route.two or {L.nstreams > 64 for L in c.launches} == {True, False}
            continue
        # each schedule the route honours (tickets hand more than 64 streams to the interleaved schedule)
        assert [L.sched for L in c.launches] == scheds and scheds, (rid, scheds)
        for t, L in zip(texts, c.launches):
            got = K.fields(t)['sched']
            assert got == K.SCHEDS[L.sched] or (L.sched == 2 and L.nstreams > 64 and got == 'interleaved'), (rid, t)
            assert got != 'dynamic' or K.guided_tail(t, L), (rid, t)                                    # the guided tail under tickets
        # both sides of the ticket words - or no stream count of the missing side walks under the cap (16384 points at eight
        # segments and more; a shape that exists below eight segments only: W <= 6 takes more than 85 streams)
        sides = {L.nstreams > 64 for L in c.launches}
        if not c.route.two and len(scheds) > 1 and sides != {True, False}:
            missing = 0 if sides == {True} else 1
            assert not any(K._find(lib, K.shape_of(c), c.route, None, s, 1, missing, False, None, every=True) for s in scheds), rid
            one_sided.append(rid)
        if not any(K.crosses(t, L) for t, L in zip(texts, c.launches)):
            lone.append(rid)
    # a run that crosses a chunk boundary: every route whose walking launch leaves room for two chunks under the cap
    print('core fuzz class C on one side of 64 streams only: %s' % one_sided)
    print('core fuzz class C without a chunk crossing: %s' % lone)
    assert sorted(lone) == sorted(K.NO_CROSSING)
    # ... and for those the cap rules it out: a run longer than a chunk is two segments and more for every resident workgroup,
    # with a remainder: nstreams x nseg > 2 x 256 bpc, on every shape the route has
    for rid in K.NO_CROSSING:
        route = K.routes()[K.DRAWN.index(rid)]
        for w in K._admitted(route):
            nperseg = K.nperseg_of(w.nfft, w.npk)
            sh = K.Shape(w.nfft, nperseg, K.noverlap_of(nperseg, w.ovk), w.wclass, w.detrend, route.two, route.word)
            bpc = int(K.fields(K.predict(lib, sh, 3 if w.few else 9))['bpc'])
            assert (2 if route.two else 1) * 2 * 256 * bpc * (sh.nperseg - sh.noverlap) >= K.CAP, (rid, w)


# ---- d, e. what the oracle reads; the gates in float32 --------------------------------------------------------------------------

def units_checked(c, L):
    """the streams of a launch the CPU suite runs: all of them up to five, then every 37th (the GPU suite checks every one)"""
    n = K.units(c, L)
    return list(range(n)) if n <= 5 else sorted(set(range(0, n, 37)) | {1, n - 1})


@pytest.mark.parametrize('rid', K.DRAWN)
def test_the_oracle_reads_only_finite_samples_and_float32_holds_half_of_every_gate(rid):
    route = K.routes()[K.DRAWN.index(rid)]
    worst = {}
    for c in K.cases(route, K.SEED):
        for li, L in enumerate(c.launches):
            data = K.lane_data(c, li)
            for i in units_checked(c, L):
                x = K.lane_input(c, li, i)                                     # the lane with its NaN tail
                ref = K.reference(c, x)
                plain = tuple(d[0] for d in data) if c.route.two else data[i]
                again = K.reference(c, plain)                                  # d: bit for bit, and finite
                for a, b in zip(ref if c.route.two else [ref], again if c.route.two else [again]):
                    assert a.tobytes() == b.tobytes() and np.all(np.isfinite(a)), K.shape_text(c, L)
                shares = K.compare(c, K.emulated(c, x), ref, K.shape_text(c, L))      # e: as if these were the GPU's rows
                for k, v in shares.items():
                    if v > worst.get(k, (0.0, ''))[0]:
                        worst[k] = (v, K.shape_text(c, L))
                    assert v <= 0.5, (k, v, K.shape_text(c, L))
    for k, (v, text) in sorted(worst.items()):
        print('core fuzz float32 emulation %s: %s %.3f of its gate [%s]' % (rid, k, v, text))


# ---- f. the layout detects ------------------------------------------------------------------------------------------------------------

def _case_b(suite, pick):
    return next(c for c in suite if c.cls == 'B' and not c.route.two and pick(c))


def test_a_read_one_sample_past_a_streams_samples_yields_nan_rows(suite):
    """the oracle as the kernel, fed from the layout's buffer with one sample too many: the row is NaN, and the gate refuses it"""
    c = _case_b(suite, lambda c: K.tail(c) > 0 or c.gap > 0)
    L = c.launches[0]
    (buf, lead), = K.layout(c)
    for i in range(L.nstreams):
        at = lead + i * K.stride(c, L)
        good = K.reference(c, buf[at:at + K.owned(c, L)])
        assert np.all(np.isfinite(good)) and good.tobytes() == K.reference(c, K.lane_input(c, 0, i)).tobytes()
        past = K.reference(c, buf[at + 1:at + 1 + K.owned(c, L)])             # the window slid one sample on
        assert np.all(np.isnan(past))
        before = K.reference(c, buf[at - 1:at - 1 + K.owned(c, L)])
        assert np.all(np.isnan(before))
        with pytest.raises(AssertionError):
            K.compare(c, 10.0 * np.log10(past) if c.db else past, good)


def _wrong_stream_shares(c, same_offset):
    """every stream's row computed from its neighbour's samples, against its own oracle: the worst reading per stream pair
    as a share of the gate (above 1: the gate refuses it)"""
    L = c.launches[0]
    data = K.lane_data(c, 0, same_offset)
    from test_hip_parity import plan_err
    out = []
    for i in range(L.nstreams):
        own = K.reference(c, FL.nan_tail(data[i], K.owned(c, L)))
        other = K.reference(c, FL.nan_tail(data[(i + 1) % L.nstreams], K.owned(c, L)))
        out.append(plan_err(other, own) / K.RTOL)
    return out


def test_a_read_from_the_neighbouring_stream_exceeds_the_gate(suite):
    """... by the samples themselves (every stream has its own seed); and a MEAN or pilot taken from the neighbour - the
    samples right, the subtracted value wrong - exceeds it because the offset is distinct per stream: with the same offset
    on every stream the wrong stream's mean is the right one to the noise's own mean, and passes."""
    c = _case_b(suite, lambda c: c.offset)
    assert min(_wrong_stream_shares(c, False)) > 1.0
    L = c.launches[0]
    win = K.window_of(c).astype(np.float64)

    def wrong_mean_shares(same):
        """stream i detrended by its neighbour's per-segment mean: the oracle on x_i - mean_j + mean_i-free samples"""
        from oracle import ref_cpu as R
        from test_hip_parity import plan_err
        data = K.lane_data(c, 0, same)
        own_n = K.owned(c, L)
        out = []
        for i in range(L.nstreams):
            j = (i + 1) % L.nstreams
            xi, xj = (np.asarray(data[k][:own_n], np.complex128) for k in (i, j))
            si, sj = R._segments(xi, c.nperseg, c.noverlap), R._segments(xj, c.nperseg, c.noverlap)
            X = np.fft.fft((si - sj.mean(axis=1, keepdims=True)) * win, c.nfft, axis=1)      # the neighbour's mean
            Y = np.fft.fft((si - si.mean(axis=1, keepdims=True)) * win, c.nfft, axis=1)      # its own
            out.append(plan_err((np.abs(X) ** 2).mean(axis=0), (np.abs(Y) ** 2).mean(axis=0)) / K.RTOL)
        return out

    distinct, same = wrong_mean_shares(False), wrong_mean_shares(True)
    print('core fuzz layout: a neighbour\'s mean reads %.3g of the gate at least with distinct offsets, %.3g at most with one offset' % (min(distinct), max(same)))
    assert min(distinct) > 1.0
    assert min(distinct) > 1e3 * max(same)      # what the rule buys: the same offset everywhere hides the wrong mean a thousandfold
