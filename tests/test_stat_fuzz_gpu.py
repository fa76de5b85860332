"""GPU tests of the per-bin statistic families on seeded random shapes (tests/stat_fuzz_cases.py): for every family and
size three drawn cases - full segments, awkward segments, many items per workgroup - through the family's _dev call on a
buffer that is NaN everywhere but the samples the launch owns, each output row a device block of its own between guards
(stat_fuzz_cases.run_case): the return value and the recipe (the forced build named), every stream against the float64
oracle of its own samples at the family's own gates through the case's fftshift / trim / dB, guards and spare rows still
the sentinel, the input read back byte for byte, and for the class-A case the host form's bits.
Measured on an MI355X, worst reading per family as a share of its gate - the suite's seed / seeds 1 ... 5 of
tools/stat_fuzz.py (profiles/stat_fuzz.txt; NOTES.md section 2 has the cases): mtm 0.09 / 0.14 (PSD), mtmcsd 0.02 / 0.07
(Pxy / Cxy), ftest 0.12 / 0.12 (sums), jack 0.08 / 0.15 (lnsd), csdjack 0.26 / 0.50 (zsd), adapt 0.18 / 0.65 (dof), sk 0.12 /
0.23 (PSD), cyc 0.05 / 0.28 (scf / PSD), caf 0.12 / 0.28, mat 0.18 / 0.28 (S), pfb 0.13 / 0.42.  No case failed; what the
fuzz found on the way - two inputs float32 does not hold, now bounds of the draw - is in stat_fuzz_cases's docstring.
Class-C recipes of the suite's seed that show W < items with items no multiple of W, one per family:
  mtm      91 items   kernel=mtm nfft=256 ntapers=7 W=14 nseg=13 nstreams=564 bpc=32
  mtmcsd   32760      kernel=mtmcsd nfft=64 ntapers=15 W=8192 nseg=2184 nstreams=1 bpc=32
  ftest    19         kernel=mtmftest nfft=64 ntapers=4 W=5 nseg=19 nstreams=1379 bpc=32
  jack     52         kernel=mtmjack nfft=128 ntapers=4 W=7 nseg=13 nstreams=1083 bpc=32
  csdjack  2045       kernel=mtmcsdjack nfft=1024 ntapers=5 W=1280 nseg=409 nstreams=1 bpc=5
  adapt    13         kernel=mtmadapt nfft=64 ntapers=15 iters=4 W=3 nseg=13 nstreams=2299 bpc=32
  sk       3          kernel=welchsk nfft=64 W=2 nseg=3 nstreams=3495 bpc=32
  cyc      19         kernel=welchcyc nfft=64 W=2 nseg=19 nstreams=1885 ncyc=3 group=2 bpc=32
  caf      19         kernel=welchlag nfft=64 W=10 nseg=19 nstreams=757 nlags=1 group=2 bpc=32
  mat      13094      kernel=welchmat nfft=64 W=8192 nseg=13094 nstreams=1 nchan=4 cap=4 state=regs bpc=32
  pfb      9          kernel=welchpfb nfft=64 ntaps=2 W=6 nseg=9 nstreams=1317 bpc=32
(csdjack walks at 1024 points only: its class C stops at 2500 items, fewer than the device holds workgroups of the smaller
builds.)"""
import pytest

import stat_fuzz_cases as S
from stat_support import POWERS
from test_hip_parity import ctx, hip  # noqa: F401 - ctx / hip are fixtures

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('nfft', POWERS)
@pytest.mark.parametrize('family', S.FAMILIES)
def test_three_drawn_cases_against_the_float64_oracle(ctx, hip, family, nfft):
    drawn = S.cases(family, nfft, S.SEED)
    assert [c.cls for c in drawn] == list(S.CLASSES)
    for c in drawn:
        S.run_case(ctx, hip, c)


@pytest.mark.parametrize('family', S.FAMILIES)
def test_a_class_c_launch_walks_runs_of_unequal_length(ctx, hip, family):
    """over the family's sizes up to 1024 points a class-C recipe shows, at least once, W < items with items no multiple of W"""
    seen = []
    for nfft in POWERS:
        if nfft <= 1024:
            c = S.cases(family, nfft, S.SEED)[2]
            recipe, _ = S.run_case(ctx, hip, c, check=False)
            seen.append((S.items(c), recipe, S.walks(c, recipe)))
            print('stat fuzz class C %s: %d items a stream [%s]%s' % (family, S.items(c), recipe, ' <- walks' if seen[-1][2] else ''))
    assert any(w for _, _, w in seen), seen
