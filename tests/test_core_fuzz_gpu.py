"""GPU tests of the core Welch and CSD routes on seeded random shapes (tests/core_fuzz_cases.py): for every route of
resolve_recipe() - and every build the parity suite forces through set_tuning - three drawn cases through exec_dev /
csd_exec_dev on a buffer that is NaN everywhere but the samples the launch owns, every output row a device block of its own
between guards (core_fuzz_cases.run_case): the return value, last_recipe() equal to the predicted string, every stream
against the float64 oracle of its own samples at the project's gates through the case's fftshift / trim / dB, guards and
spare rows still the sentinel, no sentinel left in a written row, the input read back byte for byte, and for the class-A
case the host form's bits.  The second test reads the DEVICE's recipes of the class-C launches: runs of unequal length
(W < nseg with a remainder), and a run that crosses a chunk boundary wherever the cap leaves room for one.
Measured on an MI355X, worst reading per route as a share of its gate: see MEASURED below (profiles/core_fuzz.txt has seeds
1 ... 5 of tools/core_fuzz.py, NOTES.md section 2 the table)."""
import pytest

import core_fuzz_cases as K
from test_hip_parity import ctx, hip  # noqa: F401 - ctx / hip are fixtures

pytestmark = pytest.mark.gpu

MEASURED = """worst reading per route as a share of its gate, on an MI355X: the suite's seed / seeds 1 ... 5 (1455 cases, none failed)
seg.full-none-none 0.02 / 0.04, seg.full-time-launch 0.06 / 0.03, seg.full-time-none 0.01 / 0.03, seg.half-none-none 0.01
/ 0.03, seg.half-time-launch 0.02 / 0.01, seg.half-time-none 0.02 / 0.02, seg_padded.full-none-none 0.01 / 0.02,
seg_padded.full-time-launch 0.02 / 0.04, seg_padded.full-time-none 0.01 / 0.03, seg_padded.half-none-none 0.01 / 0.03,
seg_padded.half-time-launch 0.03 / 0.02, seg_padded.half-time-none 0.01 / 0.03, segws-freq-launch 0.03 / 0.03,
segws-freq-none 0.03 / 0.04, segws-none-none 0.03 / 0.05, segws-time-launch 0.01 / 0.10, segws-time-none 0.04 / 0.04,
welch16k-freq-launch 0.12 / 0.21, welch16k-freq-none 0.13 / 0.21, welch16k-none-none 0.35 / 0.22, welch16k-time-launch
0.12 / 0.35, welch16k-time-none 0.39 / 0.21, welch16k1x.pipe-none-none 0.37 / 0.39, welch16k1x.plain.window-none-none 0.32
/ 0.65, welch16k1x_half-freq-inline 0.06 / 0.11, welch16k1x_half-freq-none 0.06 / 0.07, welch16k1x_half-none-none 0.16 /
0.21, welch16k1x_half.ws-freq-inline 0.06 / 0.08, welch16k1x_half.ws-freq-none 0.07 / 0.08, welch16k1x_half.ws-none-none
0.10 / 0.28, welch4096.dpp-none-none 0.03 / 0.07, welch4096.dpp-time-launch 0.13 / 0.07, welch4096.dpp-time-none 0.06 /
0.13, welch4096.pipe-time-launch 0.06 / 0.22, welch4096.pipe-time-none 0.12 / 0.18, welch4096.ws-freq-inline 0.07 / 0.10,
welch4096.ws-freq-none 0.10 / 0.06, welch4096.ws-none-none 0.07 / 0.08, welch_generic-none-none 0.02 / 0.09,
welch_generic-time-launch 0.01 / 0.05, welch_generic-time-none 0.04 / 0.05, welch16k-freq-launch+16k4 0.04 / 0.43,
welch16k-freq-none+16k4 0.13 / 0.33, welch16k-none-none+16k4 0.08 / 0.22, welch16k-none-none+16kplain 0.40 / 0.36,
welch16k1x.plain-none-none+16kplain 0.60 / 0.97, welch16k1x_half-freq-inline+8k1role 0.10 / 0.14,
welch16k1x_half-freq-none+8k1role 0.06 / 0.13, welch16k1x_half-none-none+8k1role 0.09 / 0.11, segws-freq-launch+fd 0.04 /
0.11, segws-freq-none+fd 0.06 / 0.10, welch16k-freq-launch+fd 0.15 / 0.47, welch16k-freq-none+fd 0.21 / 0.47,
welch16k1x_half-freq-inline+fd 0.25 / 0.20, welch16k1x_half-freq-none+fd 0.18 / 0.26, welch16k1x_half.ws-freq-inline+fd
0.06 / 0.12, welch16k1x_half.ws-freq-none+fd 0.08 / 0.15, welch4096.ws-freq-inline+fd 0.09 / 0.21,
welch4096.ws-freq-none+fd 0.08 / 0.18, welch16k1x_half-freq-launch+plaunch 0.12 / 0.11,
welch16k1x_half.ws-freq-launch+plaunch 0.06 / 0.09, welch4096.ws-freq-launch+plaunch 0.04 / 0.06, seg.half-none-none+seg3
0.01 / 0.05, seg.half-time-launch+seg3 0.09 / 0.04, seg.half-time-none+seg3 0.03 / 0.04, seg.full.wps4-none-none+seg4 0.03
/ 0.04, seg.full.wps4-time-launch+seg4 0.02 / 0.04, seg.full.wps4-time-none+seg4 0.01 / 0.09, seg.half.wps4-none-none+seg4
0.02 / 0.08, seg.half.wps4-time-launch+seg4 0.01 / 0.03, seg.half.wps4-time-none+seg4 0.01 / 0.04, seg.half-time-launch+td
0.04 / 0.05, seg.half-time-none+td 0.09 / 0.07, welch16k-time-launch+td 0.15 / 0.21, welch16k-time-none+td 0.11 / 0.16,
welch4096.pipe-time-launch+td 0.10 / 0.09, welch4096.pipe-time-none+td 0.10 / 0.14, welch4096.ws-freq-inline+wsgen 0.08 /
0.07, welch4096.ws-freq-none+wsgen 0.08 / 0.11, welch4096.ws-none-none+wsgen 0.05 / 0.10, csd-csd4096-none-none 0.02 /
0.05, csd-csd4096-time-launch 0.03 / 0.07, csd-csd4096-time-none 0.04 / 0.05, csd-csd4096ws-freq-inline 0.01 / 0.04,
csd-csd4096ws-freq-none 0.08 / 0.21, csd-csd4096ws-none-none 0.08 / 0.03, csd-welch_generic-none-none 0.06 / 0.07,
csd-welch_generic-time-launch 0.04 / 0.13, csd-welch_generic-time-none 0.11 / 0.27, csd-csd4096-none-none+csd1 0.04 /
0.03, csd-csd4096-time-launch+csd1 0.04 / 0.07, csd-csd4096-time-none+csd1 0.04 / 0.09, csd-csd4096ws-freq-inline+fd 0.05
/ 0.07, csd-csd4096ws-freq-none+fd 0.10 / 0.16, csd-csd4096ws-freq-launch+plaunch 0.02 / 0.03, csd-csd4096-time-launch+td
0.01 / 0.05, csd-csd4096-time-none+td 0.04 / 0.08
The closest: 0.97, seed 1, welch16k1x:plain under '16kplain' on 40 streams of three 16384-point rectangular segments (the float32
emulation of the same draw class reads 0.31); every route below 8192 points stays under 0.28."""

RAN = {}      # (route id, class) -> run_case's result in this process: the second test reads the first one's class-C launches


def _route(rid):
    return K.routes()[K.DRAWN.index(rid)]


@pytest.mark.parametrize('rid', K.DRAWN)
def test_three_drawn_cases_against_the_float64_oracle(ctx, hip, rid):
    drawn = K.cases(_route(rid), K.SEED)
    assert [c.cls for c in drawn] == list(K.CLASSES)
    for c in drawn:
        K.check_domain(c)
        RAN[(rid, c.cls)] = K.run_case(ctx, hip, c)


@pytest.mark.parametrize('rid', [i for i in K.DRAWN if i not in K.NO_WALK])
def test_the_devices_class_c_recipes_walk_unequal_runs_and_cross_a_chunk_boundary(ctx, hip, rid):
    """the recipe the device recorded, not only the predicted one (run alone, the test launches the case itself, unchecked)"""
    c = K.cases(_route(rid), K.SEED)[2]
    ran = RAN.get((rid, 'C')) or K.run_case(ctx, hip, c, check=False)
    assert len(ran) == len(c.launches)
    for (recipe, _), L in zip(ran, c.launches):
        print('core fuzz class C %s: nseg %d streams %d [%s]%s' % (rid, L.nseg, L.nstreams, recipe, ' <- crosses' if K.crosses(recipe, L) else ''))
        assert K.names(recipe, c.route) and K.walks(recipe, L), (recipe, L)
        assert K.fields(recipe)['sched'] != 'dynamic' or K.guided_tail(recipe, L), (recipe, L)
    if c.route.kernel != 'welch_generic':      # (the coverage kernel takes no schedule and has no chunks: contiguous runs)
        assert rid in K.NO_CROSSING or any(K.crosses(recipe, L) for (recipe, _), L in zip(ran, c.launches)), ran
