"""GPU tests of the spectral matrix and the generalized coherence of Welch plans (oth_welch_matrix / _dev,
csrc/welchmat.hip) against the float64 oracle by the definition (tests/welch_matrix_oracle.py).  Gates on every bin, from the
project's RTOL = 1e-4: |S_ab - oracle| <= RTOL scale sqrt(T_aa T_bb) / M (the size of a fully coherent bin) and
|gcoh - oracle| <= 2 C (C - 1) RTOL - a cofactor of a unit-diagonal positive matrix is at most 1 and each of the C (C - 1)
off-diagonal entries of G carries at most 2 RTOL; at C = 2 this is the 4 RTOL of the cyclic coherence.  Input is unit noise per
channel plus a common band-limited component and tones whose amplitude test_welch_sk_gpu's amp_for sets.
Measured on an MI355X, worst bin of this file (S as a fraction of the gate's size sqrt(S_aa S_bb), gcoh absolute): the 45
parity cases S 5.6e-5 (gate 1e-4), gcoh 1.3e-5 (gates 4e-4 at C = 2 ... 1.12e-2 at C = 8; at most 3 % of a case's gate); the
long runs S 5.5e-7, 4.2e-7 and 1.1e-6 at 64 points, 1.8e-5 at 4096 x 1200 and 2.6e-5 at 16384 x 600, gcoh at most 2.3e-6;
against plan.csd S at most 1.8e-5 (gate 2e-4), C = 2 gcoh against cxy at most 6.7e-6 (gate 8e-4).  multiantenna_scan on the
detection capture: 0.9717 in band, 0.1814 outside, null mean 0.1769 - the oracle's figures to four digits."""
import numpy as np
import pytest

import welch_matrix_oracle as XO
from stat_support import FS, recipe_field, welch_plan as make_plan
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_welch_matrix_cpu import DET_C, DET_M, DET_NFFT, check_detection, detection_capture
from test_welch_sk_gpu import amp_for, tones_for

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
CHANNELS = (2, 3, 4, 5, 8)      # capacity 2 full; 4 partial and full; 8 partial and full


def capture(nchan, n, seed, nfft, M, offset=0.0):
    """unit noise per channel, a common component of unit power in the lowest quarter of the band with a phase per channel,
    and test_welch_sk_gpu's tones (one strong on a bin, one of 0.5 between bins), common too, with a phase per channel"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = (rng.standard_normal((nchan, n)) + 1j * rng.standard_normal((nchan, n))) / np.sqrt(2.0)
    nfast = 1 << (n - 1).bit_length()      # a power of two at least n: the transform behind the band limit stays quick
    spec = np.fft.fft((rng.standard_normal(nfast) + 1j * rng.standard_normal(nfast)))
    spec[~(np.fft.fftfreq(nfast) < -0.25)] = 0.0
    s = np.fft.ifft(spec)[:n]
    s /= np.sqrt(np.mean(np.abs(s) ** 2))
    for a, f in tones_for(nfft, amp_for(M, nfft)):
        s = s + a * np.exp(2j * np.pi * f * t)
    x = x + s[None, :] * np.exp(2j * np.pi * rng.random(nchan))[:, None]
    return (x + offset).astype(np.complex64)


def check_matrix(S, gcoh, ref, fftshift=False, trim=0, what=''):
    """S [C, C, m] and gcoh [m] (or None) against the oracle's dict at the two gates of the file header -> the worst readings"""
    st = lambda r: XO.shape_out(r, fftshift, trim)      # noqa: E731
    C = ref['T'].shape[0]
    d = np.einsum('aaj->aj', ref['T']).real
    size = st(ref['scale'] * np.sqrt(d[:, None, :] * d[None, :, :]) / ref['M'])
    want = st(ref['S'])
    S = np.asarray(S, np.complex128)
    assert S.shape == want.shape and np.all(np.isfinite(S.real)) and np.all(np.isfinite(S.imag))
    assert not S[np.arange(C), np.arange(C)].imag.any()
    e_s = float(np.max(np.abs(S - want) / size))
    e_g = 0.0
    if gcoh is not None:
        g = np.asarray(gcoh, np.float64)
        assert g.shape == st(ref['gcoh']).shape and np.all(np.isfinite(g)) and g.min() >= 0.0 and g.max() <= 1.0
        e_g = float(np.max(np.abs(g - st(ref['gcoh']))))
    if what:
        print('matrix parity %s: S %.2e of the size (gate %.0e), gcoh %.2e (gate %.2e)' % (what, e_s, RTOL, e_g, 2 * C * (C - 1) * RTOL))
    assert e_s <= RTOL and e_g <= 2 * C * (C - 1) * RTOL, (what, e_s, e_g)
    return e_s, e_g


# ---- 1. parity with the oracle: every size x every channel count ---------------------------------------------------------------

OPTIONS = [  # nperseg as a fraction of nfft (x / 16), overlap %, detrend, scaling, fftshift, trim (x nfft / 64), db, offset
    (16, 0, True, 'density', False, 0, False, 0.0),
    (12, 0, True, 'raw', True, 5, False, 0.0),                       # nperseg < nfft, fftshift with trim
    (16, 50, True, 'density', False, 0, True, 0.0),                  # 50 % overlap, dB on the plan
    (16, 0, False, 'over_n2', False, 0, False, 0.0),                 # detrend off
    (16, 50, True, 'spectrum', True, 3, False, 35.0 - 20.0j),        # a 35 - 20j offset under detrend
    (10, 50, False, 'density', True, 0, True, 0.0),
    (16, 0, True, 'spectrum', False, 0, False, 35.0 - 20.0j),
]
PARITY_CASES = [(nfft, C, 1 + (5 * (i * len(CHANNELS) + k) + i) % 12) + OPTIONS[(i * len(CHANNELS) + k) % len(OPTIONS)]
                for i, nfft in enumerate(SIZES) for k, C in enumerate(CHANNELS)]


assert {c[2] for c in PARITY_CASES} == set(range(1, 13)) and {c[3:] for c in PARITY_CASES} == set(OPTIONS)
assert all(sorted(c[1] for c in PARITY_CASES if c[0] == nfft) == list(CHANNELS) for nfft in SIZES)


@pytest.mark.parametrize('nfft,C,M,frac,ov,detrend,scaling,fftshift,trim64,db,offset', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, C, M, frac, ov, detrend, scaling, fftshift, trim64, db, offset):
    nperseg = nfft * frac // 16
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    trim = trim64 * nfft // 64
    x = capture(C, noverlap + M * step + step // 3, 7 * nfft + 13 * C + M, nfft, M, offset)
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, db)
    S, gcoh = plan.matrix(x)
    m = nfft - 2 * trim
    assert plan.last_nseg == M and S.shape == (C, C, m) and gcoh.shape == (m,)
    assert S.dtype == np.complex64 and gcoh.dtype == np.float32
    recipe = plan.last_recipe()
    assert recipe.startswith('kernel=welchmat nfft=%d W=%d nseg=%d nstreams=1 nchan=%d ' % (nfft, M, M, C)), recipe
    assert recipe_field(recipe, 'cap') == (2 if C == 2 else 4 if C <= 4 else 8) and ' bpc=' in recipe
    ref = XO.matrix(x, nfft, nperseg, noverlap, 'hann', detrend, scaling, FS)
    check_matrix(S, gcoh, ref, fftshift, trim, what=str((nfft, C, nperseg, ov, M, detrend, scaling)) + ' ' + recipe)
    for a in range(C):
        for b in range(a + 1, C):
            assert S[b, a].tobytes() == np.conj(S[a, b]).tobytes()
    if M == 1:
        assert np.max(np.abs(gcoh.astype(np.float64) - 1.0)) <= 2 * C * (C - 1) * RTOL      # rank one
    if db:      # the matrix is linear on a dB plan: the linear twin's, bit for bit
        twin = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, False)
        S2, g2 = twin.matrix(x)
        assert S2.tobytes() == S.tobytes() and g2.tobytes() == gcoh.tobytes()
        twin.close()
    only = plan.matrix(x, return_gcoh=False)      # gcoh is optional, and takes no part in the matrix
    assert only.tobytes() == S.tobytes()
    plan.close()


# ---- 2. runs longer than one segment per workgroup ----------------------------------------------------------------------------

# 64 points x 5000 segments at C = 2: an MI355X holds 8192 workgroups of that build (32 per CU), more than the segments, so
# the run there is one segment long; 12000 segments reach the later-add path of the same build.
@pytest.mark.parametrize('nfft,ov,M,C,longer', [(64, 0, 5000, 2, False), (64, 0, 12000, 2, True), (64, 0, 5000, 8, True),
                                                (4096, 0, 1200, 4, True), (16384, 50, 600, 3, True)])
def test_runs_longer_than_one_segment(ctx, hip, nfft, ov, M, C, longer):
    noverlap = nfft * ov // 100
    x = capture(C, noverlap + M * (nfft - noverlap) + 5, nfft + C, nfft, M)
    plan = make_plan(ctx, hip, nfft, nfft, noverlap)
    S, gcoh = plan.matrix(x)
    recipe = plan.last_recipe()
    assert plan.last_nseg == M and (recipe_field(recipe, 'W') < M) == longer, recipe      # the first-store and later-add path
    check_matrix(S, gcoh, XO.matrix(x, nfft, nfft, noverlap, fs=FS), what='long run ' + recipe)
    plan.close()


# ---- 3. exact properties ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,C,M', [(256, 3, 7), (512, 8, 5), (4096, 4, 6), (16384, 2, 3)])
def test_exact_properties(ctx, hip, nfft, C, M):
    x = capture(C, nfft * M + 9, 3 * nfft + C, nfft, M)
    plan = make_plan(ctx, hip, nfft, scaling='raw')
    gate = 2 * C * (C - 1) * RTOL
    S, gcoh = plan.matrix(x)
    S2, g2 = plan.matrix(x)      # two calls: bit-identical
    assert S2.tobytes() == S.tobytes() and g2.tobytes() == gcoh.tobytes()
    # two identical channels
    twin = x.copy()
    twin[C - 1] = twin[0]
    St, gt = plan.matrix(twin)
    assert not St[0, C - 1].imag.any()
    assert St[0, C - 1].real.tobytes() == St[0, 0].real.tobytes() == St[C - 1, C - 1].real.tobytes()
    assert gt.min() >= 1.0 - gate
    # a permutation of the channels: the permuted matrix, bit for bit
    perm = np.roll(np.arange(C), 1) if C > 2 else np.array([1, 0])
    Sp, gp = plan.matrix(x[perm])
    for a in range(C):
        for b in range(C):
            assert Sp[a, b].tobytes() == S[perm[a], perm[b]].tobytes(), (a, b)
            assert a == b or Sp[b, a].tobytes() == np.conj(Sp[a, b]).tobytes()
    assert np.max(np.abs(gp.astype(np.float64) - gcoh)) <= gate
    # a power-of-two gain on one channel scales its row and column exactly
    scaled = x.copy()
    scaled[1] *= np.float32(0.125)
    Sg, gg = plan.matrix(scaled)
    for a in range(C):
        for b in range(C):
            f = np.float32(0.125) ** ((a == 1) + (b == 1))
            assert Sg[a, b].tobytes() == (S[a, b] * f).astype(np.complex64).tobytes(), (a, b)
    assert np.max(np.abs(gg.astype(np.float64) - gcoh)) <= gate
    plan.close()


# ---- 4. against what exists ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,C,M', [(1024, 2, 9), (1024, 4, 6), (4096, 2, 8), (4096, 3, 5)])
def test_against_the_two_channel_plan(ctx, hip, nfft, C, M):
    x = capture(C, nfft * M + 3, 11 * nfft + C, nfft, M)
    plan = make_plan(ctx, hip, nfft)
    S, gcoh = plan.matrix(x)
    worst, worst_c = 0.0, 0.0
    for a in range(C):
        for b in range(a + 1, C):
            pxx, pyy, pxy, cxy = plan.csd(x[a], x[b])
            size = np.sqrt(pxx.astype(np.float64) * pyy)
            for got, want in ((S[a, a].real, pxx), (S[b, b].real, pyy), (S[a, b], pxy)):
                worst = max(worst, float(np.max(np.abs(got.astype(np.complex128) - want) / size)))
            if C == 2:
                worst_c = float(np.max(np.abs(gcoh.astype(np.float64) - cxy)))
    print('matrix against plan.csd, %d points C = %d: S %.2e of the size (gate %.0e), gcoh against cxy %.2e (gate %.0e)'
          % (nfft, C, worst, 2 * RTOL, worst_c, 8 * RTOL))
    assert worst <= 2 * RTOL and worst_c <= 8 * RTOL
    plan.close()


# ---- 5. the _dev form ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,C,M', [(256, 3, 6), (8192, 5, 3)])
def test_dev_form(ctx, hip, nfft, C, M):
    n, stride = nfft * M + 7, nfft * M + 7 + 129
    x = capture(C, n, 5 * nfft + C, nfft, M)
    plan = make_plan(ctx, hip, nfft, fftshift=True, trim=nfft // 16)
    S, gcoh = plan.matrix(x)
    m, pairs = plan.out_len, C * (C + 1) // 2
    padded = np.full((C, stride), np.nan + 1j * np.nan, np.complex64)      # what lies between the channels is never read
    padded[:, :n] = x
    dx, ds, dg = ctx.alloc(padded.nbytes), ctx.alloc(8 * pairs * m), ctx.alloc(4 * m)
    try:
        ctx.h2d(dx, padded)
        for with_s, with_g in ((True, True), (True, False), (False, True)):
            ctx.h2d(ds, np.full(2 * pairs * m, -7.0, np.float32))
            ctx.h2d(dg, np.full(m, -7.0, np.float32))
            assert plan.matrix_dev(dx, n, C, stride, ds if with_s else None, dg if with_g else None) == M
            packed = ctx.d2h(ds, (pairs, m), np.complex64)
            g = ctx.d2h(dg, (m,), np.float32)
            if with_s:
                assert hip.unpack_matrix(packed, C).tobytes() == S.tobytes()
            else:
                assert np.all(packed.view(np.float32) == -7.0)
            if with_g:
                assert g.tobytes() == gcoh.tobytes()
            else:
                assert np.all(g == -7.0)
    finally:
        for d in (dx, ds, dg):
            ctx.free(d)
    plan.close()


# ---- 6. degenerate input ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft', [128, 4096, 16384])
def test_degenerate_input(ctx, hip, nfft):
    C, M = 3, 5
    x = capture(C, nfft * M, nfft + 1, nfft, M)
    plan = make_plan(ctx, hip, nfft)
    clean, gclean = plan.matrix(x)
    ref = XO.matrix(x, nfft, fs=FS)

    def others_untouched(S, a):
        for r in range(C):
            for c in range(C):
                if a not in (r, c):
                    assert S[r, c].tobytes() == clean[r, c].tobytes(), (r, c)

    for kind in ('silent', 'constant'):
        y = x.copy()
        y[1] = 0.0 if kind == 'silent' else np.complex64(35.0 - 20.0j)
        S, g = plan.matrix(y)
        assert not g.any() and not S[1].view(np.float32).any() and not S[:, 1].view(np.float32).any(), kind
        others_untouched(S, 1)
    S, g = plan.matrix(np.zeros_like(x))
    assert not S.view(np.float32).any() and not g.any()
    for bad in (np.nan, np.inf, complex(0.0, -np.inf)):
        y = x.copy()
        y[2, nfft + 17] = bad
        S, g = plan.matrix(y)
        assert np.isnan(g).all(), bad
        for r in range(C):
            part = S[r, 2].view(np.float32) if r != 2 else S[2, 2].real
            assert np.isnan(part).all() and np.isnan(S[2, r].real).all(), (bad, r)
        others_untouched(S, 2)
    x1, x2 = capture(C, nfft, nfft + 2, nfft, 1), capture(C, 2 * nfft, nfft + 3, nfft, 2)      # amp_for's tone for their own M
    one, gone = plan.matrix(x1)      # M = 1: rank one
    assert plan.last_nseg == 1 and np.max(np.abs(gone.astype(np.float64) - 1.0)) <= 2 * C * (C - 1) * RTOL
    check_matrix(one, gone, XO.matrix(x1, nfft, fs=FS))
    few, gfew = plan.matrix(x2)      # M < C: singular
    assert plan.last_nseg == 2 and np.max(np.abs(gfew.astype(np.float64) - 1.0)) <= 2 * C * (C - 1) * RTOL
    check_matrix(few, gfew, XO.matrix(x2, nfft, fs=FS))
    S, g = plan.matrix(x)      # ... and the plan's next call is right
    assert S.tobytes() == clean.tobytes() and g.tobytes() == gclean.tobytes()
    check_matrix(S, g, ref)
    plan.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_plan_usable(ctx, hip):
    C, n = 3, 4096
    x = capture(C, n, 9, 1024, 4)
    d, out = ctx.alloc(x.nbytes), ctx.alloc(8 * 6 * 1024 + 4 * 1024)

    def refused(call, code, word):
        with pytest.raises(hip.HipError) as ei:
            call()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    def host(plan, nchan, src=x, s=True, g=True):
        buf, gb = np.empty(2 * 36 * plan.out_len, np.float32), np.empty(plan.out_len, np.float32)
        src = np.ascontiguousarray(src, np.complex64)
        return ctx.check(ctx.lib.oth_welch_matrix(plan.h, src.ctypes.data_as(hip.C.c_void_p) if src.size else None, src.shape[-1], nchan, 0,
                                                  buf.ctypes.data_as(hip.C.POINTER(hip.C.c_float)) if s else None,
                                                  gb.ctypes.data_as(hip.C.POINTER(hip.C.c_float)) if g else None, None), 'oth_welch_matrix')

    try:
        ctx.h2d(d, x)
        mtm = ctx.mtm_plan(1024, nw=4.0)
        refused(lambda: mtm.matrix(x), UNSUPPORTED, 'multitaper')
        refused(lambda: mtm.matrix_dev(d, n, C, n, out), UNSUPPORTED, 'multitaper')
        assert mtm.exec(x[0]).shape == (1024,)
        mtm.close()
        med = make_plan(ctx, hip, 1024)
        med.set_average('median')
        refused(lambda: med.matrix(x), UNSUPPORTED, 'MEDIAN')
        refused(lambda: med.matrix_dev(d, n, C, n, out), UNSUPPORTED, 'MEDIAN')
        assert med.exec(x[0]).shape == (1024,)
        med.set_average('mean')
        assert med.matrix(x)[0].shape == (C, C, 1024)
        med.close()
        for nfft in (100, 32, 32768):
            odd = make_plan(ctx, hip, nfft)
            big = capture(2, 4 * nfft, 3, nfft, 4)
            refused(lambda: odd.matrix(big), UNSUPPORTED, 'power of two')
            assert odd.exec(big[0]).shape == (nfft,)
            odd.close()
        plan = make_plan(ctx, hip, 1024)
        for nchan in (1, 0, -2, 9):
            refused(lambda: host(plan, nchan), INVALID, 'nchan')
            refused(lambda: plan.matrix_dev(d, 1024, nchan, 1024, out), INVALID, 'nchan')
        refused(lambda: plan.matrix_dev(0, n, C, n, out), INVALID, 'input is NULL')
        refused(lambda: host(plan, C, src=np.empty((C, 0), np.complex64)), INVALID, 'input is NULL')
        refused(lambda: plan.matrix_dev(d, n, C, n, None, None), INVALID, 'both NULL')
        refused(lambda: host(plan, C, s=False, g=False), INVALID, 'both NULL')
        refused(lambda: plan.matrix_dev(d, n, C, n - 1, out), INVALID, 'chan_stride')
        refused(lambda: plan.matrix(x[:, :1000]), INVALID, 'nperseg')
        refused(lambda: plan.matrix_dev(d, 1000, C, n, out), INVALID, 'nperseg')
        with pytest.raises(ValueError):
            plan.matrix(x[0])
        with pytest.raises(ValueError):
            plan.matrix(np.zeros((9, 2048), np.complex64))
        S, gcoh = plan.matrix(x)      # ... and the plan still works
        check_matrix(S, gcoh, XO.matrix(x, 1024, fs=FS))
        ref_row = XO.matrix(x, 1024, fs=FS)['S'][0, 0].real
        assert np.max(np.abs(plan.exec(x[0]) - ref_row) / ref_row) <= RTOL      # no other call of the plan is affected
        plan.close()
    finally:
        ctx.free(d)
        ctx.free(out)


# ---- 8. multiantenna_scan ------------------------------------------------------------------------------------------------------

def test_multiantenna_scan_meets_the_detection_condition(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    x = detection_capture(0)
    freqs, psd, gcoh, null_mean = T.multiantenna_scan(x, DET_NFFT, 20e6, fc=2.4e9, ctx=ctx)
    assert freqs.shape == gcoh.shape == (DET_NFFT,) and psd.shape == (DET_C, DET_NFFT)
    assert null_mean == XO.null_mean(DET_C, DET_M) and abs(null_mean - 0.1769) < 1e-4
    assert np.isclose(freqs[0], 2.4e9 - 10e6, rtol=1e-12) and np.isclose(freqs[DET_NFFT // 2], 2.4e9, rtol=1e-12)
    check_detection(gcoh, null_mean, 'multiantenna_scan')
    ref = XO.matrix(x, DET_NFFT, detrend=True, fs=20e6)
    assert np.max(np.abs(gcoh - np.fft.fftshift(ref['gcoh']))) <= 2 * DET_C * (DET_C - 1) * RTOL
    want = np.fft.fftshift(np.einsum('aaj->aj', ref['S']).real, axes=-1)
    assert np.max(np.abs(psd - want) / want) <= RTOL
    g2 = T.multiantenna_scan(x, DET_NFFT, 20e6, ctx=ctx)[2]      # the cached plan
    assert g2.tobytes() == gcoh.tobytes()
    noise_only = T.multiantenna_scan(detection_capture(0, signal=False), DET_NFFT, 20e6, ctx=ctx)[2]
    assert abs(noise_only.mean() - null_mean) <= 0.25 * null_mean
