"""GPU tests of the eigenvalues and the principal eigenvector of the spectral matrix of Welch plans (oth_welch_matrix_eig /
_dev, csrc/mateig.hip) against the float64 oracle (tests/welch_eig_oracle.py: numpy.linalg.eigh per bin).  The gates follow
from the gates the matrix already meets (tests/test_welch_matrix_gpu.py, RTOL = 1e-4) by Weyl's inequality - an eigenvalue
moves by at most the 2-norm of the perturbation, which is at most its Frobenius norm:
  of S   |l_k - oracle| <= RTOL trace(S_oracle): each S_ab is within RTOL sqrt(S_aa S_bb), and the Frobenius norm of those
         bounds is RTOL trace;
  of G   |l_k - oracle| <= 2 C RTOL: each of the C (C - 1) off-diagonal entries carries at most 2 RTOL, and
         2 RTOL sqrt(C (C - 1)) <= 2 C RTOL.
The vector, every bin: | ||v|| - 1 | <= 1e-6, Im v_0 == 0, Re v_0 >= 0, ||A_oracle v - l_1 v|| <= 2 gates; its direction
(Davis-Kahan) sqrt(1 - |v^H v_oracle|^2) <= 2 gates / (l_1 - l_2) on the bins where the oracle's gap is at least 0.1 l_1, which
at least 75 % of a case's bins must be.
Measured on an MI355X, worst bin of this file: the 45 parity cases of S eigenvalues 0.159 of the gate, residual 0.063 and
direction 0.043 of theirs, at most 2.1 % of a case's bins outside the gap condition; of G 0.042, 0.049, 0.049 and 3.1 %;
| ||v|| - 1 | at most 5.1e-8 (gate 1e-6).  Identities: the trace within 9.6e-8 (gates 4.8e-7 ... 1.9e-6), 1 - prod l(G)
against gcoh within 6.4e-8 (gates 3.6e-7 ... 1.1e-6).  G eigenvalues under gains 2^k: moved by 0 (the sums scale exactly).
Trailing eigenvalues of the singular cases (M = 1 at C = 4, M = 3 at C = 8, two identical channels): at most 0.001 of the gate.
eigen_scan on the detection capture: nsrc = 1 in 98.3 % of the band and 0 in 100 % outside, 0 in 100 % of the bins without
the signal; l_1(G) 3.384 in band against 1.425 outside - the oracle's figures."""
import ctypes as C
import gc

import numpy as np
import pytest

import welch_eig_oracle as EO
import welch_matrix_oracle as XO
from stat_support import FS, welch_plan as make_plan
from test_hip_parity import RTOL, ctx, hip  # noqa: F401 - ctx / hip are fixtures
from test_welch_eig_cpu import check_source_count
from test_welch_matrix_cpu import DET_BAND, DET_C, DET_GUARD, DET_M, DET_NFFT, detection_capture
from test_welch_matrix_gpu import PARITY_CASES, capture

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1


def gate_of(ref, of, fftshift=False, trim=0):
    """the eigenvalue gate per output bin from the matrix oracle's dict"""
    C_ = ref['T'].shape[0]
    if of == 'G':
        return np.full(ref['T'].shape[2] - 2 * trim, 2 * C_ * RTOL)
    return RTOL * XO.shape_out(np.einsum('aaj->j', ref['S']).real, fftshift, trim)


def check_eig(eig, vec, ref, of, fftshift=False, trim=0, what=''):
    """eig [C, m] and vec [C, m] (or None) of the device against the oracle at the gates of the file header -> the worst
    readings as fractions of their gates, and the share of bins outside the gap condition"""
    want = EO.eig(None, ref['T'].shape[2], of=of, ref=ref)
    st = lambda r: XO.shape_out(r, fftshift, trim)      # noqa: E731
    gate = gate_of(ref, of, fftshift, trim)
    lam, lam_ref = np.asarray(eig, np.float64), st(want['eig'])
    assert eig.dtype == np.float32 and lam.shape == lam_ref.shape
    assert np.all(np.isfinite(lam)) and lam.min() >= 0.0 and np.all(np.diff(lam, axis=0) <= 0)
    e_l = float(np.max(np.abs(lam - lam_ref) / gate))
    e_n = e_r = e_d = share = 0.0
    if vec is not None:
        assert vec.dtype == np.complex64 and vec.shape == lam.shape
        v = np.asarray(vec, np.complex128).T                                   # [m, C]
        A = np.moveaxis(st(np.moveaxis(want['A'], 0, 2)), 2, 0)                # [m, C, C]
        e_n = float(np.max(np.abs(np.linalg.norm(v, axis=1) - 1.0)))
        assert not vec[0].imag.any() and np.all(vec[0].real >= 0)
        resid = np.linalg.norm(np.einsum('jac,jc->ja', A, v) - lam[0][:, None] * v, axis=1)
        e_r = float(np.max(resid / (2 * gate)))
        gap = lam_ref[0] - lam_ref[1]
        wide = gap >= 0.1 * lam_ref[0]
        share = float(np.mean(~wide))
        # sqrt(1 - |v^H v_ref|^2) as the norm of v's part orthogonal to v_ref: the same number, without the cancellation
        vr = st(want['vec']).T
        inner = np.einsum('jc,jc->j', np.conj(vr), v)
        sine = np.linalg.norm(v - inner[:, None] * vr, axis=1) / np.linalg.norm(v, axis=1)
        e_d = float(np.max((sine * gap / (2 * gate))[wide])) if wide.any() else 0.0
    if what:
        print('eig parity %s of %s: eigenvalues %.3f of the gate, | |v| - 1 | %.1e (gate 1e-6), residual %.3f of its gate, direction %.3f '
              'of its gate, %.1f %% of the bins outside the gap condition' % (what, of, e_l, e_n, e_r, e_d, 100 * share))
    assert e_l <= 1.0 and e_n <= 1e-6 and e_r <= 1.0 and e_d <= 1.0 and share <= 0.25, (what, of, e_l, e_n, e_r, e_d, share)
    return e_l, e_n, e_r, e_d, share


# ---- 1. parity with the oracle: every size x every channel count, both matrices ------------------------------------------------

@pytest.mark.parametrize('nfft,C_,M,frac,ov,detrend,scaling,fftshift,trim64,db,offset', PARITY_CASES)
def test_parity_with_the_float64_oracle(ctx, hip, nfft, C_, M, frac, ov, detrend, scaling, fftshift, trim64, db, offset):
    nperseg = nfft * frac // 16
    noverlap = nperseg * ov // 100
    step = nperseg - noverlap
    trim = trim64 * nfft // 64
    x = capture(C_, noverlap + M * step + step // 3, 7 * nfft + 13 * C_ + M, nfft, M, offset)
    plan = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, db)
    ref = XO.matrix(x, nfft, nperseg, noverlap, 'hann', detrend, scaling, FS)
    m = nfft - 2 * trim
    for of in 'SG':
        eig, vec = plan.matrix_eig(x, of=of)
        assert plan.last_nseg == M and eig.shape == vec.shape == (C_, m)
        recipe = plan.last_recipe()
        assert recipe.startswith('kernel=welchmat nfft=%d W=%d nseg=%d nstreams=1 nchan=%d ' % (nfft, M, M, C_)), recipe
        assert recipe.endswith(' eig=%s vec=1' % of), recipe
        check_eig(eig, vec, ref, of, fftshift, trim, what=str((nfft, C_, nperseg, ov, M, detrend, scaling)))
        only = plan.matrix_eig(x, of=of, return_vector=False)      # the vector is optional, and takes no part in the eigenvalues
        assert only.tobytes() == eig.tobytes() and plan.last_recipe().endswith(' eig=%s' % of)
        if db:      # always linear: the linear twin's rows, bit for bit
            twin = make_plan(ctx, hip, nfft, nperseg, noverlap, detrend, scaling, fftshift, trim, False)
            e2, v2 = twin.matrix_eig(x, of=of)
            assert e2.tobytes() == eig.tobytes() and v2.tobytes() == vec.tobytes()
            twin.close()
    plan.close()


# ---- 2. identities on the device's own rows --------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,C_,M,db', [(64, 2, 3, False), (256, 5, 7, True), (4096, 8, 12, False), (16384, 3, 2, True)])
def test_identities_and_bit_equal_forms(ctx, hip, nfft, C_, M, db):
    n, stride = nfft * M + 5, nfft * M + 5 + 77
    x = capture(C_, n, 3 * nfft + C_, nfft, M)
    plan = make_plan(ctx, hip, nfft, fftshift=True, trim=nfft // 32, db=db)
    m = plan.out_len
    S, gcoh = plan.matrix(x)
    ls, vs = plan.matrix_eig(x, of='S')
    lg, vg = plan.matrix_eig(x, of='G')
    trace = np.einsum('aaj->j', S.astype(np.complex128)).real
    e_t = float(np.max(np.abs(ls.astype(np.float64).sum(axis=0) - trace) / trace))
    e_g = float(np.max(np.abs((1.0 - np.prod(lg.astype(np.float64), axis=0)) - gcoh)))
    print('identities, %d points C = %d M = %d: trace %.2e (gate %.2e), 1 - prod l(G) against gcoh %.2e (gate %.2e)'
          % (nfft, C_, M, e_t, 4 * C_ * 2.0 ** -24, e_g, (C_ + 1) * 2.0 ** -23))
    assert e_t <= 4 * C_ * 2.0 ** -24 and e_g <= (C_ + 1) * 2.0 ** -23
    padded = np.full((C_, stride), np.nan + 1j * np.nan, np.complex64)      # what lies between the channels is never read
    padded[:, :n] = x
    dx, de, dv = ctx.alloc(padded.nbytes), ctx.alloc(4 * C_ * m), ctx.alloc(8 * C_ * m)
    twin = make_plan(ctx, hip, nfft, fftshift=True, trim=nfft // 32, db=not db)
    try:
        ctx.h2d(dx, padded)
        for of, lam, vec in (('S', ls, vs), ('G', lg, vg)):
            assert plan.matrix_eig(x, of=of, return_vector=False).tobytes() == lam.tobytes()      # with and without vec_out
            again = plan.matrix_eig(x, of=of)                                                     # two runs
            assert again[0].tobytes() == lam.tobytes() and again[1].tobytes() == vec.tobytes()
            other = twin.matrix_eig(x, of=of)                                                     # dB plan against linear plan
            assert other[0].tobytes() == lam.tobytes() and other[1].tobytes() == vec.tobytes()
            for with_e, with_v in ((True, True), (True, False), (False, True)):                   # host form against _dev form
                ctx.h2d(de, np.full(C_ * m, -7.0, np.float32))
                ctx.h2d(dv, np.full(2 * C_ * m, -7.0, np.float32))
                assert plan.matrix_eig_dev(dx, n, C_, stride, of, de if with_e else None, dv if with_v else None) == M
                e, v = ctx.d2h(de, (C_, m), np.float32), ctx.d2h(dv, (C_, m), np.complex64)
                assert e.tobytes() == lam.tobytes() if with_e else np.all(e == -7.0)
                assert v.tobytes() == vec.tobytes() if with_v else np.all(v.view(np.float32) == -7.0)
    finally:
        for d in (dx, de, dv):
            ctx.free(d)
    twin.close()
    plan.close()


# ---- 3. gain invariance ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,C_,M', [(128, 3, 5), (2048, 8, 9)])
def test_coherence_eigenvalues_ignore_power_of_two_gains(ctx, hip, nfft, C_, M):
    x = capture(C_, nfft * M, nfft + 5 * C_, nfft, M)
    k = np.random.default_rng(C_).integers(-8, 9, C_)
    k[0], k[1] = -8, 8
    plan = make_plan(ctx, hip, nfft)
    base = plan.matrix_eig(x, of='G', return_vector=False)
    scaled = plan.matrix_eig((x * (2.0 ** k)[:, None]).astype(np.complex64), of='G', return_vector=False)
    err = float(np.max(np.abs(scaled.astype(np.float64) - base)))
    print('G eigenvalues under gains 2^k, %d points C = %d: moved by %.2e (gate %.2e)' % (nfft, C_, err, C_ * 2.0 ** -22))
    assert err <= C_ * 2.0 ** -22
    plan.close()


# ---- 4. degenerate input ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nfft', [64, 4096])
def test_degenerate_input(ctx, hip, nfft):
    C_, M = 3, 5
    x = capture(C_, nfft * M, nfft + 1, nfft, M)
    plan = make_plan(ctx, hip, nfft)
    clean = {of: plan.matrix_eig(x, of=of) for of in 'SG'}
    e0 = np.zeros((C_, nfft), np.complex64)
    e0[0] = 1.0
    for kind in ('silent', 'constant'):      # a silent channel, a constant under detrend
        y = x.copy()
        y[1] = 0.0 if kind == 'silent' else np.complex64(35.0 - 20.0j)
        eig, vec = plan.matrix_eig(y, of='S')
        assert not eig[2].any() and np.all(eig[1] > 0) and not vec[1].view(np.float32).any(), kind
        eig, vec = plan.matrix_eig(y, of='G')
        assert np.all(eig == 1.0) and vec.tobytes() == e0.tobytes(), kind
    eig, vec = plan.matrix_eig(np.zeros_like(x), of='S')      # all channels silent
    assert not eig.any() and vec.tobytes() == e0.tobytes()
    eig, vec = plan.matrix_eig(np.zeros_like(x), of='G')
    assert np.all(eig == 1.0) and vec.tobytes() == e0.tobytes()
    for bad in (np.nan, np.inf):
        for of in 'SG':
            y = x.copy()
            y[2, nfft + 17] = bad
            eig, vec = plan.matrix_eig(y, of=of)
            assert np.isnan(eig).all() and np.isnan(vec.real).all() and np.isnan(vec.imag).all(), (bad, of)
            eig, vec = plan.matrix_eig(x, of=of)      # ... and the next call on clean input is the one before, bit for bit
            assert eig.tobytes() == clean[of][0].tobytes() and vec.tobytes() == clean[of][1].tobytes()
    # M = 1 at C = 4: rank one; M = 3 at C = 8: singular; two identical channels at C = 3
    for C2, M2, twin, zeros in ((4, 1, False, 3), (8, 3, False, 5), (3, 5, True, 1)):
        y = capture(C2, nfft * M2, nfft + 7 + C2, nfft, M2)
        if twin:
            y[2] = y[0]
        ref = XO.matrix(y, nfft, fs=FS)
        for of in 'SG':
            eig, vec = plan.matrix_eig(y, of=of)
            assert plan.last_nseg == M2
            check_eig(eig, vec, ref, of, what='degenerate %s' % str((nfft, C2, M2, twin)))
            gate = gate_of(ref, of)
            worst = float(np.max(eig[C2 - zeros:].astype(np.float64) / gate))
            print('  trailing %d eigenvalues: at most %.3f of the gate' % (zeros, worst))
            assert worst <= 1.0
            if M2 == 1:
                tr = np.einsum('aaj->j', ref['S']).real if of == 'S' else np.full(nfft, float(C2))
                assert np.max(np.abs(eig[0] - tr) / gate) <= 1.0
    plan.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------

N5, C5 = 64, 3
WHAT = 'the eigenvalues of the spectral matrix'
TEXT_MTM = WHAT + " is not available on a multitaper plan: its segments' transforms are Welch's (oth_welch_plan)"
TEXT_MEDIAN = WHAT + ' is not available with OTH_AVERAGE_MEDIAN: its rows are means over segments (oth_plan_set_average(OTH_AVERAGE_MEAN) first)'
TEXT_SIZE = WHAT + ' takes a transform length that is a power of two from 64 to 16384, not 32'
TEXT_NCHAN = 'nchan must lie in 2 ... 8'
TEXT_OF = 'of must be OTH_EIG_OF_S or OTH_EIG_OF_G'
TEXT_INPUT = 'the input is NULL'
TEXT_ROWS = 'eig_out and vec_out are both NULL'
TEXT_STRIDE = 'chan_stride < nsamples'
TEXT_SHORT = 'input shorter than nperseg'


def test_refusals_in_order_leave_the_plan_usable(ctx, hip):
    n = 4 * N5
    x = capture(C5, n, 9, N5, 4)
    d, out = ctx.alloc(x.nbytes), ctx.alloc(4 * 3 * 8 * N5)
    host_e, host_v = np.empty(8 * N5, np.float32), np.empty(16 * N5, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    welch = make_plan(ctx, hip, N5)
    mtm = ctx.mtm_plan(N5, nw=2.0, ntapers=3)
    med = make_plan(ctx, hip, N5)
    med.set_average('median')
    small = make_plan(ctx, hip, 32)
    want = plan_rows = welch.matrix_eig(x, of='S')

    def call(dev, plan, nchan=C5, of=0, src=True, e=True, v=True, nsamples=n, stride=n):
        nseg = C.c_uint64()
        gc.collect()
        before = hip.live_resources()
        if dev:
            rc = ctx.lib.oth_welch_matrix_eig_dev(plan.h, C.c_void_p(d) if src else None, nsamples, nchan, stride, of,
                                                  C.c_void_p(out) if e else None, C.c_void_p(out + 4 * 8 * N5) if v else None, C.byref(nseg))
        else:
            rc = ctx.lib.oth_welch_matrix_eig(plan.h, x.ctypes.data_as(C.c_void_p) if src else None, nsamples, nchan, 0, of,
                                              fp(host_e) if e else None, fp(host_v) if v else None, C.byref(nseg))
        return rc, ctx.lib.oth_last_error(ctx.h).decode(), hip.live_resources() == before

    table = [  # the header's seven in order, then two at once: which goes first
        (dict(plan=mtm), UNSUPPORTED, TEXT_MTM), (dict(plan=med), UNSUPPORTED, TEXT_MEDIAN), (dict(plan=small), UNSUPPORTED, TEXT_SIZE),
        (dict(nchan=1), INVALID, TEXT_NCHAN), (dict(nchan=9), INVALID, TEXT_NCHAN),
        (dict(of=2), INVALID, TEXT_OF), (dict(of=-1), INVALID, TEXT_OF),
        (dict(src=False), INVALID, TEXT_INPUT),
        (dict(e=False, v=False), INVALID, TEXT_ROWS),
        (dict(stride=n - 1), INVALID, TEXT_STRIDE),
        (dict(nsamples=N5 - 1, stride=N5 - 1), INVALID, TEXT_SHORT),
        (dict(plan=mtm, nchan=9), UNSUPPORTED, TEXT_MTM),
        (dict(nchan=9, of=2), INVALID, TEXT_NCHAN), (dict(of=2, src=False), INVALID, TEXT_OF),
        (dict(src=False, e=False, v=False), INVALID, TEXT_INPUT), (dict(e=False, v=False, nsamples=N5 - 1, stride=N5 - 1), INVALID, TEXT_ROWS),
    ]
    try:
        ctx.h2d(d, x)
        ctx.sync()
        for dev in (False, True):
            for kw, code, text in table:
                if not dev and 'stride' in kw and 'nsamples' not in kw:
                    continue      # the host form has no stride of its own
                kw = dict(kw)
                plan = kw.pop('plan', welch)
                rc, said, untouched = call(dev, plan, **kw)
                print('dev' if dev else 'host', kw, rc, repr(said))
                assert (rc, said) == (code, text)
                assert untouched      # refused before anything is allocated or staged
                got = welch.matrix_eig(x, of='S')      # ... and the plan goes on working
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert mtm.exec(x[0]).shape == (N5,) and med.exec(x[0]).shape == (N5,) and small.exec(x[0]).shape == (32,)
        with pytest.raises(ValueError):
            welch.matrix_eig(x[0])
        with pytest.raises(ValueError):
            welch.matrix_eig(np.zeros((9, 256), np.complex64))
        with pytest.raises(KeyError):
            welch.matrix_eig(x, of='T')
        check_eig(plan_rows[0], plan_rows[1], XO.matrix(x, N5, fs=FS), 'S')
    finally:
        ctx.free(d)
        ctx.free(out)
        for p in (welch, mtm, med, small):
            p.close()


# ---- 6. eigen_scan -------------------------------------------------------------------------------------------------------------

def test_eigen_scan_on_the_detection_capture(ctx, hip):
    from ofdm_tools import ofdm_cr_tools as T
    x = detection_capture(0)
    freqs, eig, vec, stats = T.eigen_scan(x, DET_NFFT, 20e6, fc=2.4e9, ctx=ctx)
    assert freqs.shape == (DET_NFFT,) and eig.shape == vec.shape == (DET_C, DET_NFFT)
    assert np.isclose(freqs[0], 2.4e9 - 10e6, rtol=1e-12) and np.isclose(freqs[DET_NFFT // 2], 2.4e9, rtol=1e-12)
    check_eig(eig, vec, XO.matrix(x, DET_NFFT, detrend=True, fs=20e6), 'S', fftshift=True, what='eigen_scan')
    check_source_count(stats['nsrc'], True, 'eigen_scan')
    assert np.all(np.isfinite(stats['mme'])) and np.all(stats['agm'] >= 1.0 - 1e-6)
    quiet = T.eigen_scan(detection_capture(0, signal=False), DET_NFFT, 20e6, ctx=ctx)
    check_source_count(quiet[3]['nsrc'], False, 'eigen_scan, no signal')
    top = T.eigen_scan(x, DET_NFFT, 20e6, of='G', ctx=ctx)[1][0].astype(np.float64)
    inband, outband = top[DET_GUARD:DET_BAND - DET_GUARD].mean(), top[DET_BAND + DET_GUARD:DET_NFFT - DET_GUARD].mean()
    print('l_1(G), eigen_scan: in band %.3f, outside %.3f' % (inband, outband))
    assert inband - 1.0 >= 2.0 * (outband - 1.0)
    gcoh = T.multiantenna_scan(x, DET_NFFT, 20e6, ctx=ctx)[2]      # the same cached plan serves both helpers
    lg = T.eigen_scan(x, DET_NFFT, 20e6, of='G', ctx=ctx)[1].astype(np.float64)
    assert np.max(np.abs((1.0 - np.prod(lg, axis=0)) - gcoh)) <= (DET_C + 1) * 2.0 ** -23
