"""What the call-order suite (test_call_order_gpu.py) takes for granted, checked without a GPU: that its op table
(call_order_cases.py) covers every entry point of the ABI that takes a plan, that its inputs hold the segment counts the table
claims, and that the inputs of the ticketed launches are ones on which the project's gate can tell a lost or doubled segment
from rounding."""
import os
import re

import numpy as np
import pytest

import call_order_cases as C
import csd_oracle as O
from oracle import ref_cpu as R
from test_hip_parity import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_entry_points():
    """the names in ofdm_tools._hip.SIGNATURES whose first parameter the public header declares as a plan handle"""
    from ofdm_tools import _hip
    header = open(os.path.join(ROOT, 'include', 'ofdm_tools_hip.h')).read()
    takes_plan = set(re.findall(r'^int (oth_\w+)\((?:const )?oth_plan \*', header, re.M))
    assert takes_plan <= set(_hip.SIGNATURES)      # (test_abi_cpu pins the two lists to each other)
    return {n for n in _hip.SIGNATURES if n in takes_plan}


def test_every_plan_entry_point_has_a_row():
    """A future entry point without a row in the op table - or, for a setter or destructor, a line in NOT_OPS - fails here."""
    names = plan_entry_points()
    assert len(names) > 50
    rows = {e for op in C.OPS for e in op.entries}
    assert not rows & set(C.NOT_OPS)
    missing = names - rows - set(C.NOT_OPS)
    assert not missing, 'no row in call_order_cases.OPS: %s' % sorted(missing)
    unknown = (rows | set(C.NOT_OPS)) - names
    assert not unknown, 'not an entry point that takes a plan: %s' % sorted(unknown)


def test_the_binding_has_every_method_the_table_calls():
    from ofdm_tools import _hip
    for op in C.OPS:
        for e in op.entries:
            assert e in _hip.SIGNATURES
    for name, (_, kinds, readers) in C.SETTERS.items():
        cls = _hip.MtmPlan if 'mtm' in kinds else _hip.WelchPlan
        assert hasattr(cls, name) and all(r in C.BY_NAME for r in readers)


@pytest.mark.parametrize('shape', C.WELCH_SHAPES + C.MTM_SHAPES, ids=C.shape_id)
def test_inputs_hold_the_segment_counts_the_table_claims(shape):
    """3 and 11 segments for every op at every plan shape of sections 1 and 2, under both table sets - and a ragged end, so
    that no call sees a length that is a whole number of steps."""
    names = [op.name for op in C.ops_for(shape)]
    assert len(names) >= 12 and ('csd' in names) == (shape.kind != 'mtm' and not shape.db)
    for tables in (C.TABLES_A, C.TABLES_B):
        for op in C.ops_for(shape):
            for M in C.SIZES:
                inp = C.inputs(op.name, shape, M, tables)
                assert C.segments_of(op, shape, inp, tables) == M, (op.name, M)
                n = inp['n'] if 'buf' in inp else inp['x'].shape[-1]
                assert (n - shape.noverlap) % C.step(shape), (op.name, M)
                for a in inp.values():
                    if isinstance(a, np.ndarray):
                        assert a.dtype == np.complex64 and not a.flags.writeable and np.all(np.isfinite(a.view(np.float32)))
    assert C.SMALL == 3 and C.LARGE == 11


def test_the_orders_run_every_pair():
    for shape in C.WELCH_SHAPES + C.MTM_SHAPES:
        pairs = C.pairs_for(shape)
        assert len(set(pairs)) == len(pairs) == 2 * len(C.ops_for(shape))
        (_, large), (_, small), (_, shuffled) = C.orders(shape, 20260101)
        assert sorted(large) == sorted(small) == sorted(pairs)
        assert large[0][1] == C.LARGE and small[0][1] == C.SMALL
        half = len(shuffled) // 2
        assert shuffled[:half] == shuffled[half:] and sorted(shuffled[:half]) == sorted(pairs) and shuffled[:half] != pairs
        assert C.orders(shape, 20260101)[2] == C.orders(shape, 20260101)[2]      # seeded: the order repeats


def test_the_two_table_sets_differ_in_every_length():
    a, b = C.TABLES_A, C.TABLES_B
    assert len(a.cycles) != len(b.cycles) and len(a.lags) != len(b.lags) and a.ntaps != b.ntaps
    assert a.steer[1] != b.steer[1] and a.steer[0] < 32 < b.steer[0]      # one direction tile of 32, crossed both ways
    assert a.ratio_pow != b.ratio_pow


# ---- the condition on the inputs of the ticketed launches (section 4 of the GPU file) -----------------------------------

def segment_power(x, nfft):
    """|FFT((segment - mean) hann)|^2 per segment, float64 [M, nfft] - the terms of R.welch_np's mean up to its scale"""
    from ofdm_tools import windows
    step = nfft // 2
    M = (len(x) - step) // step
    w = np.asarray(windows.get_window('hann', nfft), np.float64)
    seg = np.stack([np.asarray(x[s * step:s * step + nfft], np.complex128) for s in range(M)])
    seg = seg - seg.mean(axis=1, keepdims=True)
    return np.abs(np.fft.fft(seg * w, axis=1)) ** 2


@pytest.mark.parametrize('nfft', sorted(C.TICKET_M))
def test_a_lost_or_doubled_segment_shows_at_the_gate(nfft):
    """A ticket word that is misread makes a chunk run twice or not at all.  For every input of the ticketed launches: leave
    out the oracle's weakest segment (the one whose removal moves the mean least) and, separately, count it twice; each must
    move at least 90 % of the bins by more than 10 RTOL - with M segments a segment carries 1 / M of a bin, so M <= 200 keeps
    that a multiple of the gate.  The 10 % of the bins left out is a cap, not a measurement."""
    M = C.TICKET_M[nfft]
    assert 40 <= M <= 200
    for k in range(3):
        x = C.ticket_stream(nfft, k)
        P = segment_power(x, nfft)
        assert P.shape == (M, nfft)
        mean = P.mean(axis=0)
        _, ref = R.welch_np(x, fs=1.0, nperseg=nfft, nfft=nfft)
        scale = ref / mean
        assert np.max(scale) / np.min(scale) - 1.0 < 1e-9      # the terms above are the oracle's
        weakest = int(np.argmin(P.sum(axis=1)))
        dropped = (P.sum(axis=0) - P[weakest]) / (M - 1)
        doubled = (P.sum(axis=0) + P[weakest]) / (M + 1)
        for what, other in (('dropped', dropped), ('doubled', doubled)):
            moved = np.abs(other - mean) / mean > 10 * RTOL
            print('%d points, stream %d, weakest segment %s: %.1f %% of the bins move by more than 10 RTOL' % (nfft, k, what, 100 * moved.mean()))
            assert moved.mean() >= 0.9, (nfft, k, what, moved.mean())


def test_a_lost_or_doubled_segment_pair_shows_at_the_coherence_gate():
    """The two-channel launch: the same for Pxx and Pyy at 10 RTOL, and for the coherence at ten times its absolute gate of
    1e-4 on at least 90 % of the bins."""
    x, y = C.ticket_pair()
    nfft, step = 4096, 2048
    M = (len(x) - step) // step
    assert M == C.TICKET_CSD_M and 40 <= M <= 200
    PX, PY = segment_power(x, nfft), segment_power(y, nfft)
    pxx, pyy, pxy, cxy = O.csd(x, y, 1.0, 'hann', nfft, step, nfft, 'constant', 'density')
    assert np.max(np.abs(PX.mean(axis=0) / pxx / (PX.mean(axis=0) / pxx)[0] - 1.0)) < 1e-9
    from ofdm_tools import windows
    w = np.asarray(windows.get_window('hann', nfft), np.float64)

    def spectra(v):
        seg = np.stack([np.asarray(v[s * step:s * step + nfft], np.complex128) for s in range(M)])
        return np.fft.fft((seg - seg.mean(axis=1, keepdims=True)) * w, axis=1)
    X, Y = spectra(x), spectra(y)
    cross = np.conj(X) * Y
    coh = lambda keep: np.abs((cross * keep[:, None]).sum(axis=0)) ** 2 / ((PX * keep[:, None]).sum(axis=0) * (PY * keep[:, None]).sum(axis=0))      # noqa: E731
    ones = np.ones(M)
    assert np.max(np.abs(coh(ones) - cxy)) < 1e-9
    weakest = int(np.argmin(PX.sum(axis=1) + PY.sum(axis=1)))
    for what, weight in (('dropped', 0.0), ('doubled', 2.0)):
        keep = ones.copy()
        keep[weakest] = weight
        for name, P in (('Pxx', PX), ('Pyy', PY)):
            other = (P * keep[:, None]).sum(axis=0) / keep.sum()
            moved = np.abs(other - P.mean(axis=0)) / P.mean(axis=0) > 10 * RTOL
            assert moved.mean() >= 0.9, (what, name, moved.mean())
        moved = np.abs(coh(keep) - cxy) > 10 * 1e-4
        print('segment pair %s: %.1f %% of the coherence bins move by more than 1e-3' % (what, 100 * moved.mean()))
        assert moved.mean() >= 0.9, (what, moved.mean())
