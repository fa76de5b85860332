"""CPU checks of the seeded random-shape cases of the per-bin statistic families (tests/stat_fuzz_cases.py; no GPU): the
list is a function of the seed and pinned by a digest, every case lies inside the domain the header documents, the suite's
seed covers every size, build, output stage, optional-row pattern and edge, the oracles read only what the layout leaves
finite, and every family's gates are reachable in float32 with room - its oracle with a single-precision transform in
np.fft.fft's place (pocketfft on complex64; welch_pfb_oracle.emulate32 and mtm_adaptive_oracle.emulate32 where the family
has the closer emulation) passes the family's own comparison at half of each gate."""
import numpy as np
import pytest

import stat_fuzz_cases as S
from stat_support import POWERS

DIGEST = '80bc2704350a64ad22d97a21a54cc22d50a32dba9333dee5946ba634afe63cf3'      # sha256 of repr(all_cases(S.SEED))


# ---- a. determinism ----------------------------------------------------------------------------------------------------------------

def test_the_same_seed_gives_the_same_list_and_the_suites_list_is_pinned():
    assert S.all_cases(S.SEED) == S.all_cases(S.SEED) and S.all_cases(5) == S.all_cases(5) and S.all_cases(5) != S.all_cases(6)
    for family in S.FAMILIES:
        for nfft in POWERS:
            drawn = S.cases(family, nfft, S.SEED)
            assert [c.cls for c in drawn] == list(S.CLASSES) and all(c.family == family and c.nfft == nfft for c in drawn)
    assert len(S.all_cases()) == 3 * len(POWERS) * len(S.FAMILIES) == 297
    assert S.digest(S.SEED) == DIGEST, 'the case list moved: every change of it shows as a change of this literal'


# ---- b. domain -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [S.SEED, 1, 2, 3, 4, 5])
def test_every_case_lies_inside_the_documented_domain(seed):
    for c in S.all_cases(seed):
        S.check_domain(c)
        F = S.FAMILY[c.family]
        if c.cls == 'A':
            assert c.nperseg == c.nfft and c.noverlap in (0, c.nfft // 2) and c.nstreams == 1
            assert c.nseg in S.segs(F.min_nseg)
        if c.cls == 'B':
            assert c.fftshift and 1 <= c.trim <= c.nfft // 2 - 1 and 1 <= c.noverlap <= c.nperseg - 1
            assert (c.nperseg == c.nfft) if F.full_segments else (max(8, c.nfft // 8) <= c.nperseg <= c.nfft - 1)
            assert c.nseg in S.segs(F.min_nseg)
        if c.cls == 'C' and not F.single:
            assert c.nseg in S.segs_c(F.min_nseg)
            assert S.samples_read(c) + S.nsamples(c) > S.CAP or c.nstreams == 65535      # as many streams as fit
        # the layout: 8-byte alignment only, the gaps of the issue, the tail inside nsamples
        assert c.gap in (0, 1, 67) or (c.gap - 3) % 64 == 0 and 1 <= (c.gap - 3) // 64 <= 4
        for buf, lead in S.layout(c):
            assert buf.dtype == np.complex64 and len(buf) == lead + (S.lanes(c) - 1) * S.stride(c) + S.nsamples(c) + S.BEHIND
            finite = np.isfinite(buf.view(np.float32)).reshape(-1, 2).all(axis=1)
            want = np.zeros(len(buf), bool)
            for i in range(S.lanes(c)):
                want[lead + i * S.stride(c):lead + i * S.stride(c) + S.owned(c)] = True
            assert np.array_equal(finite, want)
        if seed != S.SEED:
            break      # (the layout of one case per further seed: the buffers are the slow part)


# ---- c. coverage ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', S.FAMILIES)
def test_the_suites_seed_covers_every_size_build_stage_row_pattern_and_edge(family):
    F = S.FAMILY[family]
    cs = S.all_cases(S.SEED, (family,))
    assert sorted({c.nfft for c in cs}) == list(POWERS) and all(sorted(c.cls for c in cs if c.nfft == n) == list(S.CLASSES) for n in POWERS)
    stages = {(c.fftshift, c.trim > 0, c.db) for c in cs}
    assert len(stages) == (8 if F.db else 4), stages                       # all eight output stages (four where dB is refused)
    assert {c.rows for c in cs} == set(F.row_patterns)                     # every optional-row pattern
    assert any(c.nseg == F.min_nseg for c in cs)                           # the family's minimum M
    assert any(S.step(c) % 2 for c in cs) and any(S.step(c) % 2 == 0 for c in cs)
    assert F.full_segments or any(c.nperseg < S.PILOT for c in cs)         # shorter than the pilot's 64 samples
    assert any(c.offset for c in cs) and {c.detrend for c in cs} == {True, False}
    assert any(c.nstreams > 1 and not all(c.rows) for c in cs) or F.single or len(F.row_patterns) == 1      # an optional row left NULL on a many-stream launch
    if F.kind != 'welch':
        assert {c.extra[:2] for c in cs} == set(S.NW_K)
    if family in ('mtm', 'mtmcsd'):
        assert {c.extra[2] for c in cs} == {'unity', 'eigen'}
    if family == 'adapt':
        assert {c.extra[2] for c in cs} == {1, 4}
    if family == 'cyc':
        assert {c.extra[1] for c in cs} == {1, 2, 4} and {len(c.extra[0]) for c in cs} == {1, 2, 3, 4, 5}
    if family == 'caf':
        assert {c.extra[1] for c in cs} == {1, 2} and {len(c.extra[0]) for c in cs} == {1, 2, 3, 4, 5}
        assert {0 in c.extra[0] for c in cs} == {True, False}
    if family == 'mat':
        assert {2 if c.extra[0] == 2 else 4 if c.extra[0] <= 4 else 8 for c in cs} == {2, 4, 8} and {c.extra[0] for c in cs} >= {2, 8}
    if family == 'pfb':
        assert min(c.extra[0] for c in cs) == 2 and max(c.extra[0] for c in cs) == 16
    if not F.single:      # class C: hundreds of streams at 64 ... 512 points, a few at 8192 / 16384
        assert all(c.nstreams >= 100 for c in cs if c.cls == 'C' and c.nfft <= 512)
        assert all(c.nstreams >= 2 for c in cs if c.cls == 'C' and c.nfft >= 8192) or family == 'pfb'


# ---- d, e. what the oracle reads; the gates in float32 --------------------------------------------------------------------------

def _same(a, b):
    if isinstance(a, dict):
        return all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return all(_same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes() and bool(np.all(np.isfinite(a)))


def units_checked(c):
    """the units of a case the CPU suite runs: all of them up to five, then every 97th (a class-C case has thousands of
    streams of one shape; the GPU suite checks every one)"""
    n = S.units(c)
    return list(range(n)) if n <= 5 else sorted(set(range(0, n, 97)) | {1, n - 1})


@pytest.mark.parametrize('family', S.FAMILIES)
def test_the_oracle_reads_only_finite_samples_and_float32_holds_half_of_every_gate(family):
    F = S.FAMILY[family]
    worst = {}
    for c in S.all_cases(S.SEED, (family,)):
        data = S.lane_data(c)
        for i in units_checked(c):
            ref = S.reference(c, i)                                            # the lane with its NaN tail
            if isinstance(data, tuple):
                finite = tuple(d[i] for d in data)
            else:
                finite = data if family == 'mat' else data[i]
            assert _same(F.rows_of(c, ref), F.rows_of(c, F.oracle(c, finite))), S.shape_text(c)      # d: bit for bit, and finite
            shares = S.compare(c, S.emulated_rows(c, i), ref, S.shape_text(c))      # e: as if these were the GPU's rows
            for k, v in shares.items():
                if v > worst.get(k, (0.0, ''))[0]:
                    worst[k] = (v, S.shape_text(c))
                assert v <= 0.5, (k, v, S.shape_text(c))
    for k, (v, text) in sorted(worst.items()):
        print('stat fuzz float32 emulation %s: %s %.3f of its gate [%s]' % (family, k, v, text))
