"""GPU tests of the spectral kurtosis of Welch plans (oth_welch_sk / _dev, csrc/welchsk.hip) against the float64 oracle by
the definition (tests/welch_sk_oracle.py).  Gates, on every bin: the PSD row within RTOL = 1e-4 relative of the oracle (the
project's gate), and R = M S2 / S1^2 recovered from the returned SK within 3e-4 relative of the oracle's R - the two sums
each good to 1e-4 give dR / R <= e2 + 2 e1.  Input is unit noise plus tones of amplitude at most 100: the amplitude of each
case is the largest at which float32 arithmetic holds the gates with a margin of four (amp_for: 2 ... 22 for the parity
cases, 100 for a long average).  Measured on an MI355X, worst case of this file: PSD 2.7e-5, R 4.9e-5 (16384 points; the
parity cases up to 2048 points read at most 7.1e-6 and 4.3e-6).  With the strong tone at amplitude 100 in every case the
same kernel reads up to 6.1e-4 (8192 points x 4 segments) - the white rounding floor of a 40 dB tone's own transform
against the shallowest bins of a short average, which no float32 transform holds."""
import os

import numpy as np
import pytest

import median_oracle as MO
import welch_sk_oracle as SO
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from stat_support import FS, welch_plan as make_plan
from test_median_gpu import noise_tones

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
RTOL_R = 3e-4


def tones_for(nfft, amp=100.0):
    """a tone of amplitude `amp` on a bin of the transform, one of 0.5 between bins"""
    return ((amp, round(0.123 * nfft) / float(nfft)), (0.5, -0.31))


def amp_for(M, bins):
    """The strong tone's amplitude for a check of `bins` bins over M segments: the largest, up to 100, at which float32
    arithmetic can hold the gates with a margin of four.  The gates are relative to each bin's own S1.  What a tone of
    amplitude A leaves in every other bin is the rounding of its own samples, window products and butterflies - white, about
    2^-24 sqrt(17 roundings) A of the noise floor in amplitude - so a bin's S1 is off by c A / sqrt(M f) relative, f its
    level over the floor, c = 3e-6 for the worst of 16384 bins (measured at A = 100: 6.1e-4 at 8192 points x 4 segments,
    3.4e-4 at 16384 x 5, 1.1e-4 at 1024 x 5 - over the gate, which no float32 transform holds at 40 dB).  S1 of a noise bin
    is Gamma(M) distributed, a fraction (M f)^M / M! of the bins lies below f times the floor: f is the deepest null
    expected among the bins, bins (M f)^M / M! = 1."""
    import math
    f = (math.factorial(M) / float(bins)) ** (1.0 / M) / M if M < 64 else 1.0
    return min(100.0, RTOL / 4.0 / 3e-6 * math.sqrt(M * f))


def check_rows(sk, psd, ref, ref_psd, fftshift=False, trim=0, db=False, what=''):
    """sk, psd: the returned rows of one stream; ref: the oracle's dict; ref_psd: its linear PSD row.  Asserts the two gates
    of the file header on every bin -> (worst PSD error, worst R error)."""
    M = ref['M']
    R = MO.shift_trim_db(ref['R'], fftshift, trim)
    P = MO.shift_trim_db(ref_psd, fftshift, trim)
    sk, psd = np.asarray(sk, np.float64), np.asarray(psd, np.float64)
    assert sk.shape == R.shape and psd.shape == P.shape and np.all(np.isfinite(sk)) and np.all(np.isfinite(psd))
    lin = 10.0 ** (psd / 10.0) if db else psd
    e_p = float(np.max(np.abs(lin - P) / P))
    e_r = float(np.max(np.abs(SO.r_of_sk(sk, M) - R) / R))
    if what:
        print('sk parity %s: PSD %.2e, R %.2e (SK %.3g ... %.3g)' % (what, e_p, e_r, sk.min(), sk.max()))
    assert e_p <= RTOL and e_r <= RTOL_R, (what, e_p, e_r)
    return e_p, e_r


# ---- 1. parity at every size -----------------------------------------------------------------------------------------------

PARITY_CASES = [  # nfft, nperseg, overlap %, M, detrend, scaling, fftshift, trim, db, offset
    (64, 64, 0, 20, True, 'density', False, 0, False, 0.0),
    (128, 100, 0, 7, True, 'raw', True, 10, False, 0.0),                      # nperseg < nfft, fftshift with trim
    (256, 256, 50, 9, True, 'density', False, 0, True, 0.0),                  # 50 % overlap, dB
    (512, 512, 0, 2, False, 'over_n2', False, 0, False, 0.0),                 # M = 2, detrend off
    (1024, 1024, 50, 5, True, 'density', True, 100, False, 35.0 - 20.0j),     # a 35-sigma complex offset under detrend
    (2048, 1500, 0, 3, True, 'raw', False, 0, False, 0.0),
    (4096, 4096, 50, 9, True, 'over_n2', False, 0, False, 0.0),
    (4096, 4096, 0, 4, False, 'density', True, 0, True, 0.0),
    (8192, 8192, 0, 4, False, 'raw', False, 0, False, 0.0),
    (8192, 5000, 50, 6, True, 'density', True, 1000, False, 35.0 - 20.0j),
    (16384, 16384, 0, 3, True, 'density', False, 0, False, 0.0),
    (16384, 10000, 50, 5, True, 'over_n2', True, 0, True, 35.0 - 20.0j),
    (16384, 16384, 50, 8, False, 'raw', False, 0, False, 0.0),
]


@pytest.mark.parametrize('nfft,nperseg,ov,M,detrend,scaling,fftshift,trim,db,offset', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, nperseg, ov, M, detrend, scaling, fftshift, trim, db, offset):
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    x = (noise_tones(noverlap + M * step + step // 3, 5 * nfft + ov + M, tones_for(nfft, amp_for(M, nfft))) + np.complex64(offset)).astype(np.complex64)
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, db)
    sk, psd = plan.sk(x, return_psd=True)
    assert plan.last_nseg == M and sk.shape == (nfft - 2 * trim,)
    assert plan.last_recipe().startswith('kernel=welchsk nfft=%d W=%d nseg=%d nstreams=1 bpc=' % (nfft, M, M))
    ref = SO.sk(x, nfft, nperseg, noverlap, 'hann', detrend)
    check_rows(sk, psd, ref, SO.psd(ref, 'hann', nperseg, scaling, FS, nfft), fftshift, trim, db,
               what=str((nfft, nperseg, ov, M, detrend, scaling)))
    assert np.array_equal(plan.sk(x).view(np.uint32), sk.view(np.uint32))      # SK alone: the PSD row is optional
    plan.close()


# ---- 2. the PSD row is exec_dev's ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,nperseg,ov,M,scaling,fftshift,trim,db', [
    (256, 200, 0, 24, 'density', True, 20, True), (1024, 1024, 50, 17, 'raw', False, 0, False),
    (4096, 4096, 50, 21, 'density', True, 0, True), (4096, 4096, 0, 16, 'over_n2', False, 0, False),
    (16384, 16384, 0, 32, 'density', False, 0, True), (8192, 8192, 50, 19, 'raw', True, 100, False)])
def test_psd_row_is_the_row_of_exec_dev(ctx, hip, nfft, nperseg, ov, M, scaling, fftshift, trim, db):
    """the same plan on the same input, to 1e-5 relative in linear power (a dB row: |difference| <= 10 log10(1 + 1e-5) dB).
    Two float32 transforms of different build stand against each other here, so the input is unit noise with a weak tone
    and a small offset - nothing whose own rounding stands over the floor's - and the rows average 16 segments or more: no
    bin of a Gamma(16) row lies deep under the floor."""
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    x = noise_tones(noverlap + M * step, 40 + nfft + ov, ((0.5, -0.31),))
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, True, scaling, fftshift, trim, db)
    m = plan.out_len
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * 3 * m)
    try:
        ctx.h2d(d, x)
        assert plan.sk_dev(d, len(x), 1, len(x), out, out + 4 * m) == M
        assert plan.exec_dev(d, len(x), out + 8 * m) == M
        sk, psd, ref = ctx.d2h(out, (3, m), np.float32).astype(np.float64)
    finally:
        ctx.free(d)
        ctx.free(out)
    errs = np.abs(10.0 ** ((psd - ref) / 10.0) - 1.0) if db else np.abs(psd - ref) / ref
    err = float(errs.max())
    print('sk PSD row against exec_dev %s [%s]: %.2e (output bin %d)' % ((nfft, nperseg, ov, M, scaling, db), plan.last_recipe(), err,
                                                                      int(errs.argmax())))
    assert err <= 1e-5
    plan.close()


# ---- 3. several segments per workgroup -------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,M,nstreams,pad', [(64, 16384, 3, 17),        # sums in registers, runs of six and seven
                                                 (4096, 5, 300, 100),      # sums in registers, runs of one and two
                                                 (16384, 5, 100, 64),      # sums in the partial rows, runs of two and three
                                                 (16384, 3, 130, 64)])     # ... one workgroup per stream
def test_a_workgroup_walks_several_segments(ctx, hip, nfft, M, nstreams, pad):
    """More work than the device holds workgroups for, so that W < nseg and a workgroup carries its sums from one segment
    of its run to the next - in registers up to 8192 points, in its own partial rows at 16384 - with runs of unequal length
    and stream_stride > nsamples.  W = max(1, resident / nstreams) with 256 CUs."""
    n = nfft * M
    stride = n + pad
    x = noise_tones(stride * nstreams, 900 + nfft + nstreams, tones_for(nfft, amp_for(M, nfft * nstreams)))
    plan = make_plan(ctx, hip, nfft, scaling='raw')
    m, sentinel = plan.out_len, np.float32(-7.0)
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * 2 * (nstreams + 1) * m)
    try:
        ctx.h2d(d, x)
        ctx.h2d(out, np.full(2 * (nstreams + 1) * m, sentinel, np.float32))
        assert plan.sk_dev(d, n, nstreams, stride, out, out + 4 * (nstreams + 1) * m) == M == plan.last_nseg
        got = ctx.d2h(out, (2, nstreams + 1, m), np.float32)
    finally:
        ctx.free(d)
        ctx.free(out)
    assert np.all(got[:, nstreams] == sentinel)      # nothing behind the rows
    recipe = plan.last_recipe()
    W = int(recipe.split(' W=')[1].split()[0])
    assert 1 <= W < M and 'nstreams=%d ' % nstreams in recipe, recipe
    worst = np.zeros(2)
    for s in range(nstreams):
        ref = SO.sk(x[s * stride:s * stride + n], nfft)
        worst = np.maximum(worst, check_rows(got[0, s], got[1, s], ref, SO.psd(ref, 'hann', nfft, 'raw', FS, nfft)))
    print('sk %d x %d segments of %d (%s): PSD %.2e, R %.2e' % (nstreams, M, nfft, recipe, worst[0], worst[1]))
    plan.close()


# ---- 4. degenerate input ----------------------------------------------------------------------------------------------------

def test_silence_and_a_constant_give_zero_rows(ctx, hip):
    for nfft in (256, 4096, 16384):
        plan = make_plan(ctx, hip, nfft, fftshift=True)
        raw = make_plan(ctx, hip, nfft, detrend=False)
        for p, x in ((plan, np.zeros(3 * nfft, np.complex64)), (raw, np.zeros(3 * nfft, np.complex64)),
                     (plan, np.full(3 * nfft, 3.0 - 2.0j, np.complex64))):
            for row in p.sk(x, return_psd=True):
                assert row.shape == (nfft,) and not row.any()
        plan.close()
        raw.close()


def test_a_line_120_db_over_the_noise_stays_finite(ctx, hip):
    """amplitude 10^6 on unit noise, 16384 points x 4 segments: P^2 of the line's bin stays inside float32 because of g"""
    nfft, M, k = 16384, 4, 2000
    x = noise_tones(nfft * M, 31, ((1e6, k / float(nfft)),))
    plan = make_plan(ctx, hip, nfft)
    sk, psd = plan.sk(x, return_psd=True)
    assert np.all(np.isfinite(sk)) and np.all(np.isfinite(psd)) and np.all(psd >= 0)
    print('sk at a 120 dB line: %.3g' % sk[k])
    assert abs(sk[k]) < 0.01
    plan.close()


def test_identical_segments_read_zero(ctx, hip):
    """a noiseless input whose segments are identical: every P_m of a bin is the same number, R = 1 and |SK| <= 1e-5"""
    for nfft, M in ((512, 5), (4096, 7), (16384, 6)):
        t = np.arange(nfft)
        base = (2.0 * np.exp(2j * np.pi * 0.123 * t) + 0.5 * np.exp(-2j * np.pi * 0.31 * t) + 0.3 - 0.1j).astype(np.complex64)
        plan = make_plan(ctx, hip, nfft)
        sk = plan.sk(np.tile(base, M))
        print('sk of %d identical segments of %d: |SK| <= %.2e' % (M, nfft, np.abs(sk).max()))
        assert plan.last_nseg == M and np.abs(sk).max() <= 1e-5
        plan.close()


# ---- 5. refusals, run-to-run identity -------------------------------------------------------------------------------------------

def test_refusals_leave_the_plan_usable(ctx, hip):
    x = noise_tones(4096, 9)
    d = ctx.alloc(x.nbytes)

    def refused(call, code, word):
        with pytest.raises(hip.HipError) as ei:
            call()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    try:
        ctx.h2d(d, x)
        mtm = ctx.mtm_plan(1024, nw=4.0)
        refused(lambda: mtm.sk(x), UNSUPPORTED, 'multitaper')
        refused(lambda: mtm.sk_dev(d, len(x), 1, len(x), d), UNSUPPORTED, 'multitaper')
        assert mtm.exec(x).shape == (1024,)
        mtm.close()
        med = make_plan(ctx, hip, 1024, average='median')
        refused(lambda: med.sk(x), UNSUPPORTED, 'MEDIAN')
        refused(lambda: med.sk_dev(d, len(x), 1, len(x), d), UNSUPPORTED, 'MEDIAN')
        assert med.exec(x).shape == (1024,)
        med.set_average('mean')
        assert med.sk(x).shape == (1024,)                                          # ... and the mean is served
        med.close()
        for nfft in (100, 32, 32768):
            odd = make_plan(ctx, hip, nfft)
            big = noise_tones(4 * nfft, 3)
            refused(lambda: odd.sk(big), UNSUPPORTED, 'power of two')
            assert odd.exec(big).shape == (nfft,)
            odd.close()
        plan = make_plan(ctx, hip, 1024)
        refused(lambda: plan.sk(x[:2047]), INVALID, 'two segments')                # one segment
        refused(lambda: plan.sk_dev(d, 1024, 1, 1024, d), INVALID, 'two segments')
        refused(lambda: plan.sk(x[:1000]), INVALID, 'nperseg')
        refused(lambda: plan.sk_dev(d, 2048, 2, 2000, d), INVALID, 'stream_stride')
        refused(lambda: plan.sk_dev(d, 2048, 0, 2048, d), INVALID, 'bad argument')
        refused(lambda: plan.sk_dev(0, 2048, 1, 2048, d), INVALID, 'bad argument')
        refused(lambda: plan.sk_dev(d, 2048, 1, 2048, 0), INVALID, 'bad argument')
        refused(lambda: plan.sk_dev(d, 2048, 65536, 2048, d), UNSUPPORTED, '65535')
        ref = SO.sk(x, 1024)
        sk, psd = plan.sk(x, return_psd=True)                                      # ... and the plan still works
        check_rows(sk, psd, ref, SO.psd(ref, 'hann', 1024, 'density', FS, 1024))
        plan.close()
    finally:
        ctx.free(d)


def test_two_calls_are_bit_identical_and_sources_agree(ctx, hip):
    for nfft, ov, M in ((2048, 50, 21), (16384, 0, 5)):
        noverlap = nfft * ov // 100
        x = noise_tones(noverlap + M * (nfft - noverlap), 11 + nfft, tones_for(nfft))
        plan = make_plan(ctx, hip, nfft, noverlap=noverlap)
        a = plan.sk(x, return_psd=True)
        b = plan.sk(x, return_psd=True)
        d = ctx.alloc(x.nbytes)
        try:
            ctx.h2d(d, x)
            c = plan.sk(d, return_psd=True, nsamples=len(x))
        finally:
            ctx.free(d)
        assert plan.last_nseg == M
        for i in range(2):
            assert a[i].tobytes() == b[i].tobytes() == c[i].tobytes()
        plan.close()


# ---- 6. the helper: what the feature exists for ---------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1])
def test_sk_scan_tells_a_carrier_from_a_burst(ctx, hip, seed):
    """unit noise, 256 points, M = 64; an amplitude-1 carrier on bin 40 and an amplitude-3 tone at bin 170.3 that is present
    in the first 16 segments only: the carrier's bins are steady, the burst's intermittent, at most 4 other bins are
    flagged - and the PSD cannot tell the two apart (22 and 25 dB over the floor)."""
    from ofdm_tools import ofdm_cr_tools as T
    n, M = 256, 64
    rng = np.random.default_rng(seed)
    t = np.arange(n * M)
    x = (rng.standard_normal(n * M) + 1j * rng.standard_normal(n * M)) / np.sqrt(2.0)
    x = x + np.exp(2j * np.pi * 40.0 / n * t)
    x[:16 * n] += 3.0 * np.exp(2j * np.pi * 170.3 / n * t[:16 * n])
    x = x.astype(np.complex64)
    sk, axis, steady, burst = T.sk_scan(x, n, float(n), ctx=ctx)                   # fs = n: the axis reads in bins
    assert sk.shape == (n,) and np.array_equal(axis, np.arange(-n // 2, n // 2))
    carrier, hop = np.isin(axis, (39, 40, 41)), np.isin(axis, (169 - n, 170 - n, 171 - n))
    print('sk_scan seed %d: SK %s at the carrier, %s at the burst; %d other bins flagged'
          % (seed, sk[carrier], sk[hop], int(np.sum((steady | burst) & ~carrier & ~hop))))
    assert np.all(steady[carrier]) and not np.any(burst[carrier])
    assert np.all(burst[hop]) and not np.any(steady[hop])
    assert int(np.sum((steady | burst) & ~carrier & ~hop)) <= 4
    lower, upper = T.sk_limits(M, 1e-3)
    assert np.array_equal(steady, sk < lower) and np.array_equal(burst, sk > upper)
    assert np.array_equal(T.sk_scan(x, n, float(n), fc=1000.0, ctx=ctx)[1], axis + 1000.0)


# ---- 7. time --------------------------------------------------------------------------------------------------------------------

def test_fused_call_is_no_slower_than_the_composition(tmp_path):
    """tools/welch_sk_time.py in a child process: whole steps between HIP events, the fused call and the composition a user
    had before it (segments_dev into a rows buffer, sum and sum of squares in torch, the SK formula) alternating on the same
    plan, median of 30, at 2^24 samples x 4096 points and 64 captures of 4 x 16384.  Its gate - fused <= 1.05 x the
    composition at either shape (5 % for box noise) - is its exit status."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / 'welch_sk_time.txt')
    p = subprocess.run([sys.executable, os.path.join(root, 'tools', 'welch_sk_time.py'), '30', '--out', out],
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.count('gate: fused') == 2 and 'FAILED' not in p.stdout and os.path.exists(out)
