"""GPU tests of the two-channel path (oth_csd_exec / _exec_dev / _partial_dev / _scale_dev, coherence_estimator): Pxx, Pyy, Pxy
and Cxy against the float64 oracle (tests/csd_oracle.py) with two DIFFERENT channels - y = 0.7 x delayed by five samples plus
half a unit of independent noise, so that coherence spans about 0.3 ... 1 and the phase of Pxy has a slope: a swapped
conjugate, a wrong sign on Im Pxy or swapped sums show in every bin.  Gates, each on every bin, all RTOL = 1e-4:
relerr(Pxx), relerr(Pyy), |dPxy| / sqrt(Pxx Pyy), |d Im Pxy| / sqrt(Pxx Pyy) on its own, |dCxy|.

  1. every power-of-two size 64 ... 16384 on the generic instance (and 4096 as the plan routes it) x 3 / 40 / 70 segment pairs -
     the three finalize routes, read back from the recipe - x four shapes;
  2. the tuned 4096-point kernels (csd4096, csd4096ws) at every step, window and detrend mode, and the refusals of
     OTH_KERNEL_TUNED;
  3. scalings, fs, fftshift + trim (odd lengths included) through every entry point, NULL outputs, the time-sharded form;
  4. degenerate inputs: a silent channel, one NaN / inf sample, gains of 2^+-40, identical channels;
  5. one plan across shrinking and regrowing segment counts;
  6. coherence_estimator -> coherence_detector at 1024 and 1000 points.

A float32 emulation of section 1 on the CPU (pocketfft on complex64, float32 accumulators; every size but 4096) read at most
1.8e-5 (Pxx / Pyy), 1.7e-5 (Pxy) and 1.0e-5 (Cxy).  Worst readings on an MI355X (Pxx or Pyy / Pxy / Im Pxy / Cxy):
  1. 1.2e-5 / 8.4e-6 / 7.6e-6 / 7.9e-6 (16384 and 8192 points, 3 segment pairs);
  2. 4.9e-6 / 8.7e-6 / 8.4e-6 / 3.9e-6 (fast detrend, 9 pairs); the few-pair fast-detrend cases 1.3e-5 outside bins 0, +-1
     and 7.4e-6 in them; bin 0 of the rectangular detrended cases 7e-11 against a bound of 1.5e-7;
  3. 1.0e-5 / 7.1e-6 / 4.3e-6 / 3.3e-6 (32768 points, 7 pairs); time-sharded against one-shot 9.3e-7 (gate 2e-6);
  4. gains 2.9e-6, Cxy bit-identical on every route; identical channels |Cxy - 1| = 0 and Im Pxy = 0 at every size; an inf
     sample: NaN in every bin on every route (before csd_store in kernels_misc.hip the 4096-point tuned route left inf in
     56 Pyy bins);
  5. 3.8e-5 / 1.9e-5 / 1.4e-5 / 1.6e-6 (the single segment pair; 1.2e-5 for the others);
  6. 1.1e-6 / 9.3e-7 / 7.4e-7 / 4.4e-7."""
import functools

import numpy as np
import pytest

import csd_oracle as O
from oracle import ref_cpu as R
from test_hip_parity import DC_BINS, RTOL, _dc_bins_gate, _f32_mean_bound, ctx, hip, relerr  # noqa: F401 - ctx / hip are fixtures
from test_median_gpu import SCALINGS, window

pytestmark = pytest.mark.gpu

POW2 = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
UNSUPPORTED = -3
SENTINEL = np.float32(-7.0)
NAMES = ('pxx', 'pyy', 'pxy', 'cxy')


@functools.lru_cache(maxsize=4)
def _pair(n, seed):
    x = R.synth_iq(n, seed, dc=2 - 1j)
    y = (0.7 * np.roll(x, 5) + 0.5 * R.synth_iq(n, seed + 1000, tones=(), dc=0.5 + 0.25j)).astype(np.complex64)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def pair(nperseg, noverlap, nseg, seed):
    """The issue's inputs: exactly nseg segments and a third of a step left over."""
    step = nperseg - noverlap
    return _pair(noverlap + nseg * step + step // 3, seed)


def oracle(x, y, nfft, nperseg=None, noverlap=None, win='hann', detrend=True, scaling='density', fs=1.0, fftshift=False, trim=0):
    nperseg = nfft if nperseg is None else nperseg
    ref = O.csd(x, y, fs, win, nperseg, noverlap, nfft, 'constant' if detrend else False, scaling)
    return [O.shift_trim(v, fftshift, trim) for v in ref]


def errors(got, ref):
    """-> relerr(Pxx), relerr(Pyy), max |dPxy| / sqrt(Pxx Pyy), max |d Im Pxy| / sqrt(Pxx Pyy), max |dCxy|"""
    (gxx, gyy, gxy, gc), (pxx, pyy, pxy, cxy) = got, ref
    norm = np.sqrt(pxx * pyy)
    d = np.asarray(gxy).astype(np.complex128) - pxy
    return (relerr(gxx, pxx), relerr(gyy, pyy), float(np.max(np.abs(d) / norm)), float(np.max(np.abs(d.imag) / norm)),
            float(np.max(np.abs(np.asarray(gc, np.float64) - cxy))))


def gate(section, label, got, ref, bound=RTOL):
    e = errors(got, ref)
    print('csd %s | %s | Pxx %.2e Pyy %.2e Pxy %.2e ImPxy %.2e Cxy %.2e' % ((section, label) + e))
    assert max(e) < bound, (section, label, e)


def recipe_W(rec):
    return int(rec.split(' W=')[1].split()[0])


def finalize_route(W, nfft):
    """launch_finalize (kernels_misc.hip) for four channels"""
    if W >= 64 and nfft % 16 == 0:
        return 'wide'                   # finalize_wide_kernel<16, 4>
    if W > 32 and nfft % 256 == 0:
        return 'two-stage'              # reduce_partials_kernel + finalize_kernel
    return 'one-stage'                  # finalize_kernel


def detrend_code(hip, name):
    return {'constant': hip.DETREND_CONSTANT, 'fast': hip.DETREND_CONSTANT_FAST, 'none': hip.DETREND_NONE}[name]


# ---- 1. every power-of-two size, every finalize route ---------------------------------------------------------------------

def shape(nfft, which):
    """-> nperseg, noverlap, window, detrend"""
    odd = 3 * nfft // 4 - 1
    return {'full': (nfft, nfft // 2, 'hann', True),
            'padded': (odd, odd // 3, 'flattop', True),
            'rect': (nfft, 0, 'boxcar', False),
            'quarter': (nfft // 4, nfft // 8, 'hann', True)}[which]


@pytest.mark.parametrize('which', ['full', 'padded', 'rect', 'quarter'])
@pytest.mark.parametrize('nfft,kernel', [(n, 'generic') for n in POW2] + [(4096, 'auto')])
def test_parity_matrix_over_sizes_and_finalize_routes(ctx, hip, nfft, kernel, which):
    nperseg, noverlap, wname, detrend = shape(nfft, which)
    plan = ctx.welch_plan(nfft, nperseg=nperseg, noverlap=noverlap, window=window(wname, nperseg),
                          detrend=hip.DETREND_CONSTANT if detrend else hip.DETREND_NONE,
                          kernel=hip.KERNEL_GENERIC if kernel == 'generic' else hip.KERNEL_AUTO)
    routes = {}
    for nseg in (3, 40, 70):
        x, y = pair(nperseg, noverlap, nseg, nfft + nseg)
        got = plan.csd(x, y)
        rec = plan.last_recipe()
        assert plan.last_nseg == nseg and ' nch=4 ' in rec
        if kernel == 'auto' and nperseg == nfft:
            assert rec.split()[0] in ('kernel=csd4096', 'kernel=csd4096ws') and rec.endswith(' layout=1'), rec
        else:      # the instance welch_generic_kernel<nfft, T, true>
            assert rec.startswith('kernel=welch_generic nfft=%d ' % nfft) and rec.endswith(' layout=0'), rec
        routes[nseg] = finalize_route(recipe_W(rec), nfft)
        gate('matrix', '%d %s %s nseg %d (%s)' % (nfft, kernel, which, nseg, routes[nseg]), got,
             oracle(x, y, nfft, nperseg, noverlap, wname, detrend))
    plan.close()
    # 64 and 128 points have no two-stage route (nfft % 256 != 0): 40 rows go through finalize_kernel there
    want = {'one-stage', 'two-stage', 'wide'} if nfft % 256 == 0 else {'one-stage', 'wide'}
    assert set(routes.values()) == want and routes[3] == 'one-stage' and routes[70] == 'wide', routes


# ---- 2. the tuned 4096-point kernels away from their default shape ------------------------------------------------------------

@pytest.mark.parametrize('detrend', ['constant', 'fast', 'none'])
@pytest.mark.parametrize('wname', ['hann', 'flattop', 'boxcar'])
@pytest.mark.parametrize('noverlap', [0, 3072, 1000, 2048])
def test_tuned_4096_every_step_window_and_detrend(ctx, hip, noverlap, wname, detrend):
    """One exclusion: a rectangular window with a constant detrend leaves sum(x - mean) in bin 0 - identically 0, so both
    sides hold rounding noise only there (SciPy on complex64 input - the float32 emulation of this case - reads 2e-11 where
    the float64 oracle reads 5e-30 and the neighbouring bins 1: a relative error of 4e18 in the reference's own arithmetic;
    its other bins read 2e-6).  Bin 0 of those cases is held to what float32 can leave of a sum that cancels:
    |X[0]| <= N max |x| (log2 N + 2) 2^-24 per segment - one rounding per transform stage, one for the mean, one for the
    subtraction, each of the running magnitude N max |x| at most - and its Cxy (0 / 0) is not read; every other bin takes
    the gates."""
    N, step = 4096, 4096 - noverlap
    zero_bin = wname == 'boxcar' and detrend != 'none'
    for nseg in (9, 70):
        x, y = pair(N, noverlap, nseg, N + noverlap + nseg)
        ref = oracle(x, y, N, N, noverlap, wname, detrend != 'none')
        for force in ((None, 'csd1') if step == 2048 else (None,)):
            plan = ctx.welch_plan(N, noverlap=noverlap, window=window(wname, N), detrend=detrend_code(hip, detrend),
                                  kernel=hip.KERNEL_TUNED)
            plan.set_tuning(force)
            got = plan.csd(x, y)
            kern = plan.last_recipe().split()[0]
            assert plan.last_nseg == nseg
            plan.close()
            if step != 2048 or force:
                assert kern == 'kernel=csd4096', (kern, force)
            elif wname == 'hann':
                assert kern == 'kernel=csd4096ws', kern
            else:
                assert kern in ('kernel=csd4096', 'kernel=csd4096ws'), kern
            label = 'noverlap %d %s %s nseg %d %s' % (noverlap, wname, detrend, nseg, kern[7:])
            if zero_bin:
                k = 1.0 / N                                                        # density, fs = 1: 1 / sum(w^2)
                ax, ay = (N * np.abs(sig).max() * 14 * 2.0 ** -24 for sig in (x, y))
                print('csd tuned4096 | %s | bin 0: Pxx %.2e (bound %.2e) Pyy %.2e (bound %.2e) |Pxy| %.2e'
                      % (label, got[0][0], k * ax * ax, got[1][0], k * ay * ay, abs(got[2][0])))
                assert 0.0 <= got[0][0] <= k * ax * ax and 0.0 <= got[1][0] <= k * ay * ay, label
                assert abs(got[2][0]) <= k * ax * ay, (label, got[2][0])
                got, ref_ = [v[1:] for v in got], [v[1:] for v in ref]
            else:
                ref_ = ref
            gate('tuned4096', label, got, ref_)


@pytest.mark.parametrize('noverlap', [0, 3072, 1000, 2048])
def test_tuned_4096_fast_detrend_few_segments(ctx, hip, noverlap):
    """OTH_DETREND_CONSTANT_FAST below 8 segment pairs: bins 0 and +-1 by the float32-mean bound of
    test_hip_parity.test_csd_few_segments_with_dc (its helpers: max(RTOL, bound)); every other bin by RTOL.  2, 3 and 7
    pairs; ONE pair is not gated per bin: a single periodogram of these inputs has nulls 4.5e-5 of its median (noverlap
    3072, bin 3187), where SciPy on complex64 input - the float32 emulation - is itself 6.6e-5 off the float64 oracle and
    the kernel read 1.4e-4; with two pairs and more the emulation reads at most 1.0e-5."""
    N = 4096
    dc = DC_BINS(N)
    mx, my = abs(2 - 1j), abs(0.7 * (2 - 1j) + 0.5 * (0.5 + 0.25j))
    for nseg in (2, 3, 7):
        x, y = pair(N, noverlap, nseg, 300 + noverlap + nseg)
        pxx, pyy, pxy, cxy = oracle(x, y, N, N, noverlap)
        plan = ctx.welch_plan(N, noverlap=noverlap, window=window('hann', N), detrend=hip.DETREND_CONSTANT_FAST,
                              kernel=hip.KERNEL_TUNED)
        gxx, gyy, gxy, gc = plan.csd(x, y)
        assert plan.last_nseg == nseg and plan.last_recipe().startswith('kernel=csd4096 ')
        plan.close()
        for got, ref, sig, m_abs in ((gxx, pxx, x, mx), (gyy, pyy, y, my)):
            rest, e_dc, e32, ok = _dc_bins_gate(got, ref, R.welch_c64(sig, nperseg=N, noverlap=noverlap, nfft=N), N, m_abs)
            print('csd tuned4096-few | noverlap %d nseg %d | k=0,+-1 %.2e (reference float32 %.2e) other bins %.2e'
                  % (noverlap, nseg, e_dc, e32, rest))
            assert rest < RTOL and ok, (nseg, rest, e_dc, e32)
        e = np.abs(gxy - pxy) / np.sqrt(pxx * pyy)
        bound = np.maximum(RTOL, _f32_mean_bound(pxx, mx, N) + _f32_mean_bound(pyy, my, N))
        assert np.delete(e, dc).max() < RTOL and np.all(e[dc] <= bound), (nseg, e.max(), e[dc], bound)
        assert np.max(np.abs(np.delete(gc - cxy, dc))) < RTOL


@pytest.mark.parametrize('nfft,nperseg', [(4096, 1024), (4096, 3071), (1024, 1024), (16384, 16384), (1000, 1000)])
def test_tuned_is_refused_where_no_tuned_two_channel_kernel_exists(ctx, hip, nfft, nperseg):
    x, y = pair(nperseg, nperseg // 2, 9, 5 + nfft)
    plan = ctx.welch_plan(nfft, nperseg=nperseg, window=window('hann', nperseg), kernel=hip.KERNEL_TUNED)
    with pytest.raises(hip.HipError) as ei:
        plan.csd(x, y)
    assert ei.value.code == UNSUPPORTED and 'tuned kernel does not cover this plan' in str(ei.value), str(ei.value)
    plan.set_kernel(hip.KERNEL_AUTO)                                               # ... and the plan still works
    gate('refused', '%d/%d under AUTO' % (nfft, nperseg), plan.csd(x, y), oracle(x, y, nfft, nperseg))
    assert plan.last_nseg == 9
    plan.close()


# ---- 3. plan options through every entry point ----------------------------------------------------------------------------------

def near(a, b, tol=2e-6):
    """Two runs of the same sums (another entry point, or halves added on the host): Pxx, Pyy relative, Pxy over
    sqrt(Pxx Pyy), Cxy absolute."""
    norm = np.sqrt(b['pxx'].astype(np.float64) * b['pyy'])
    e = (relerr(a['pxx'], b['pxx']), relerr(a['pyy'], b['pyy']),
         float(np.max(np.abs(a['pxy'].astype(np.complex128) - b['pxy']) / norm)),
         float(np.max(np.abs(a['cxy'].astype(np.float64) - b['cxy']))))
    print('csd options | two runs of the same sums | Pxx %.2e Pyy %.2e Pxy %.2e Cxy %.2e (gate %.0e)' % (e + (tol,)))
    return max(e) < tol


class DeviceOutputs(object):
    """Four device outputs of m bins with a sentinel row of m floats behind each:
    [pxx m | s m | pyy m | s m | pxy 2 m | s m | cxy m | s m]."""

    def __init__(self, ctx, m):
        self.ctx, self.m = ctx, m
        self.off = {'pxx': 0, 'pyy': 2 * m, 'pxy': 4 * m, 'cxy': 7 * m}
        self.len = {'pxx': m, 'pyy': m, 'pxy': 2 * m, 'cxy': m}
        self.d = ctx.alloc(4 * 9 * m)

    def run(self, names, call):
        """call(pxx=..., ...) with device pointers for `names` only -> their contents; everything else still the sentinel"""
        self.ctx.h2d(self.d, np.full(9 * self.m, SENTINEL, np.float32))
        call(**{k: self.d + 4 * self.off[k] for k in names})
        buf = self.ctx.d2h(self.d, (9 * self.m,), np.float32)
        untouched = np.ones(9 * self.m, bool)
        out = {}
        for k in names:
            out[k] = buf[self.off[k]:self.off[k] + self.len[k]].copy()
            untouched[self.off[k]:self.off[k] + self.len[k]] = False
        assert np.all(buf[untouched] == SENTINEL), (names, int(np.sum(buf[untouched] != SENTINEL)))
        if 'pxy' in out:
            out['pxy'] = out['pxy'].view(np.complex64)
        return out

    def free(self):
        self.ctx.free(self.d)


OPTION_SIZES = {1024: 'kernel=welch_generic ', 4096: 'kernel=csd4096ws ', 1000: 'kernel=anyfft:', 4099: 'kernel=anyfft:',
                32768: 'kernel=anyfft:twolevel'}


@pytest.mark.parametrize('trim', [0, 37])
@pytest.mark.parametrize('scaling', ['density', 'spectrum', 'raw', 'over_n2'])
@pytest.mark.parametrize('nfft', sorted(OPTION_SIZES))
def test_plan_options_on_every_entry_point(ctx, hip, nfft, scaling, trim):
    fs, noverlap = 2.5e6, nfft // 2
    step = nfft - noverlap
    # 4096 tuned: 17 pairs, so that both halves of the time-sharded form (9 + 8) stay on the role-split kernel the whole
    # takes - below 8 pairs the plan detrends in the time domain, another arithmetic: RTOL against the oracle, but not the
    # 2e-6 of one sum added in another order
    nseg = {32768: 7, 4096: 17}.get(nfft, 9)
    x, y = pair(nfft, noverlap, nseg, 40 + nfft)
    plan = ctx.welch_plan(nfft, noverlap=noverlap, window=window('hann', nfft), scaling=SCALINGS[scaling], fs=fs, fftshift=True,
                          trim_bins=trim, kernel=hip.KERNEL_TUNED if nfft == 4096 else hip.KERNEL_AUTO)
    m = plan.out_len
    assert m == nfft - 2 * trim
    ref = oracle(x, y, nfft, nfft, noverlap, 'hann', True, scaling, fs, True, trim)
    label = '%d %s trim %d' % (nfft, scaling, trim)
    host = dict(zip(NAMES, plan.csd(x, y)))
    rec = plan.last_recipe()
    assert plan.last_nseg == nseg and rec.startswith(OPTION_SIZES[nfft]) and (nfft != 32768 or rec.endswith(' layout=6')), rec
    gate('options', label + ' csd', [host[k] for k in NAMES], ref)
    dx, dy, sums = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes), ctx.alloc(4 * 2 * 4 * nfft)
    out = DeviceOutputs(ctx, m)
    try:
        ctx.h2d(dx, x)
        ctx.h2d(dy, y)

        def exec_dev(**ptrs):
            assert plan.csd_exec_dev(dx, dy, len(x), **ptrs) == nseg
        dev = out.run(NAMES, exec_dev)
        gate('options', label + ' csd_exec_dev', [dev[k] for k in NAMES], ref)
        assert near(dev, host)
        for k in NAMES:                                                            # three NULLs: no fault, no stray store
            one = out.run((k,), exec_dev)
            assert near(dict(dev, **one), dev, 1e-6), k
        # time-sharded: two halves that share the overlap halo, raw sums added on the host, then the scale stage
        ka = (nseg + 1) // 2
        assert plan.csd_partial_dev(dx, dy, ka * step + noverlap, sums) == ka
        assert plan.csd_partial_dev(dx + 8 * ka * step, dy + 8 * ka * step, len(x) - ka * step, sums + 16 * nfft) == nseg - ka
        both = ctx.d2h(sums, (2, 4 * nfft), np.float32).astype(np.float64)
        tot = both[0] + both[1]
        sxx, syy, sxy, n_ref = O.csd_sums(x, y, 'hann', nfft, noverlap, nfft)
        assert n_ref == nseg
        gxy = tot[2 * nfft::2] + 1j * tot[2 * nfft + 1::2]
        raw = [tot[:nfft], tot[nfft:2 * nfft], gxy, np.abs(gxy) ** 2 / (tot[:nfft] * tot[nfft:2 * nfft])]
        gate('options', label + ' raw sums', raw, [sxx, syy, sxy, np.abs(sxy) ** 2 / (sxx * syy)])
        ctx.h2d(sums, tot.astype(np.float32))
        sharded = out.run(NAMES, lambda **ptrs: plan.csd_scale_dev(sums, nseg, **ptrs))
        gate('options', label + ' csd_scale_dev', [sharded[k] for k in NAMES], ref)
        assert near(sharded, host)
        one = out.run(('cxy',), lambda **ptrs: plan.csd_scale_dev(sums, nseg, **ptrs))
        assert np.array_equal(one['cxy'].view(np.uint32), sharded['cxy'].view(np.uint32))
    finally:
        out.free()
        for p in (dx, dy, sums):
            ctx.free(p)
    plan.close()


def test_db_plans_refuse_every_csd_call(ctx, hip):
    """dB is not defined for a complex cross spectrum: oth_csd_exec, _exec_dev, _partial_dev and _scale_dev all refuse a
    plan with dB output (the raw sums and the scale stage included: one rule for the section), and plan and context go on."""
    nfft = 1024
    x, y = pair(nfft, nfft // 2, 9, 77)
    plan = ctx.welch_plan(nfft, window=window('hann', nfft), db=True)
    dx, dy, out = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes), ctx.alloc(4 * 5 * nfft)
    try:
        ctx.h2d(dx, x)
        ctx.h2d(dy, y)
        ctx.h2d(out, np.full(5 * nfft, SENTINEL, np.float32))
        for call in (lambda: plan.csd(x, y),
                     lambda: plan.csd_device_src(dx, dy, len(x)),
                     lambda: plan.csd_exec_dev(dx, dy, len(x), out, out + 4 * nfft, out + 8 * nfft, out + 16 * nfft),
                     lambda: plan.csd_partial_dev(dx, dy, len(x), out),
                     lambda: plan.csd_scale_dev(out, 9, out, out + 4 * nfft, out + 8 * nfft, out + 16 * nfft)):
            with pytest.raises(hip.HipError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED and 'not defined for the cross spectrum' in str(ei.value), str(ei.value)
        assert np.all(ctx.d2h(out, (5 * nfft,), np.float32) == SENTINEL)              # nothing was launched
        got = plan.exec(x)                                                         # the plan still serves its own output
        _, ref = R.welch_np(x, nperseg=nfft, nfft=nfft)
        assert relerr(10.0 ** (got.astype(np.float64) / 10.0), ref) < RTOL
    finally:
        for p in (dx, dy, out):
            ctx.free(p)
    plan.close()
    lin = ctx.welch_plan(nfft, window=window('hann', nfft))
    gate('options', 'context after the dB refusals', lin.csd(x, y), oracle(x, y, nfft))
    lin.close()


# ---- 4. degenerate inputs -----------------------------------------------------------------------------------------------------------

ROUTES = {  # name: nfft, segment pairs, kernel, through oth_csd_partial_dev + oth_csd_scale_dev, what the recipe must say
    'generic-256': (256, 9, 'auto', False, ('kernel=welch_generic ', 'one-stage')),
    'generic-1024-two-stage': (1024, 40, 'auto', False, ('kernel=welch_generic ', 'two-stage')),
    'generic-1024-wide': (1024, 70, 'auto', False, ('kernel=welch_generic ', 'wide')),
    'tuned-4096': (4096, 9, 'tuned', False, ('kernel=csd4096ws ', 'one-stage')),
    'any-4099': (4099, 9, 'auto', False, ('kernel=anyfft:', 'one-stage')),
    'scale-dev-1024': (1024, 9, 'auto', True, ('kernel=welch_generic ', 'one-stage')),
}


def run_route(ctx, hip, route, x, y, detrend=True, check_route=True):
    nfft, nseg, kernel, via_scale, (kern, fin) = ROUTES[route]
    plan = ctx.welch_plan(nfft, window=window('hann', nfft), detrend=hip.DETREND_CONSTANT if detrend else hip.DETREND_NONE,
                          kernel=hip.KERNEL_TUNED if kernel == 'tuned' else hip.KERNEL_AUTO)
    if not via_scale:
        got = plan.csd(x, y)
        assert plan.last_nseg == nseg
    else:
        dx, dy, sums, out = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes), ctx.alloc(4 * 4 * nfft), ctx.alloc(4 * 5 * nfft)
        try:
            ctx.h2d(dx, x)
            ctx.h2d(dy, y)
            assert plan.csd_partial_dev(dx, dy, len(x), sums) == nseg
            plan.csd_scale_dev(sums, nseg, out, out + 4 * nfft, out + 8 * nfft, out + 16 * nfft)
            buf = ctx.d2h(out, (5 * nfft,), np.float32)
            got = (buf[:nfft], buf[nfft:2 * nfft], buf[2 * nfft:4 * nfft].view(np.complex64), buf[4 * nfft:])
        finally:
            for p in (dx, dy, sums, out):
                ctx.free(p)
    rec = plan.last_recipe()
    plan.close()
    if check_route:      # (a NaN in a launch's pilot does not change the route; checked where the input is finite)
        assert rec.startswith(kern) and finalize_route(recipe_W(rec), nfft) == fin, rec
    return got


def route_pair(route):
    nfft, nseg = ROUTES[route][:2]
    return pair(nfft, nfft // 2, nseg, 70 + nfft)


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_a_silent_channel_gives_zero_power_and_nan_coherence(ctx, hip, route):
    """y = 0: Pyy and Pxy are exactly 0 and Cxy is 0 / 0 = NaN in every bin, as scipy.signal.coherence gives."""
    nfft = ROUTES[route][0]
    x, _ = route_pair(route)
    zero = np.zeros_like(x)
    pxx = oracle(x, zero, nfft)[0]
    for order in ('xy', 'yx'):
        gxx, gyy, gxy, gc = run_route(ctx, hip, route, *((x, zero) if order == 'xy' else (zero, x)))
        live, dead = (gxx, gyy) if order == 'xy' else (gyy, gxx)
        print('csd degenerate | %s silent %s | live channel %.2e' % (route, order[1], relerr(live, pxx)))
        assert relerr(live, pxx) < RTOL
        assert np.all(dead == 0) and np.all(gxy.real == 0) and np.all(gxy.imag == 0) and np.all(np.isnan(gc)), route


def census(v):
    v = np.asarray(v)
    v = v.view(np.float32) if np.iscomplexobj(v) else v
    return 'nan %d inf %d finite %d' % (np.isnan(v).sum(), np.isinf(v).sum(), np.isfinite(v).sum())


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('route', sorted(ROUTES))
def test_one_bad_sample_in_one_channel_stays_in_that_channel(ctx, hip, route, bad):
    """One NaN / +inf sample (real part) in one channel: the other channel's spectrum stays finite and within RTOL - the
    channels share no state in LDS, the pilot or the mean - and the bad channel's power, Pxy and Cxy are NaN in every bin,
    with and without the detrend, as SciPy's are (its transform turns an inf into NaN in every bin too)."""
    nfft = ROUTES[route][0]
    x, y = route_pair(route)
    pos = len(x) // 2 + 1
    clean = oracle(x, y, nfft)[:2], oracle(x, y, nfft, detrend=False)[:2]
    for which in ('y', 'x'):
        for detrend in (False, True):
            v = [x.copy(), y.copy()]
            v[which == 'y'][pos] = np.complex64(complex(bad, 0.0))
            got = run_route(ctx, hip, route, v[0], v[1], detrend, check_route=False)
            good, spoiled = (got[0], got[1]) if which == 'y' else (got[1], got[0])
            e = relerr(good, clean[0 if detrend else 1][0 if which == 'y' else 1])
            print('csd degenerate | %s %s in %s detrend %d | clean channel %.2e; bad channel %s; Pxy %s; Cxy %s'
                  % (route, bad, which, detrend, e, census(spoiled), census(got[2]), census(got[3])))
            assert np.all(np.isfinite(good)) and e < RTOL, (route, which, detrend, e)
            assert np.all(np.isnan(spoiled)), (route, which, detrend, census(spoiled))
            assert np.all(np.isnan(got[2].real)) and np.all(np.isnan(got[2].imag)), (route, which, detrend, census(got[2]))
            assert np.all(np.isnan(got[3])), (route, which, detrend, census(got[3]))


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_gains_of_2_to_the_40_leave_the_coherence_alone(ctx, hip, route):
    """x * 2^40 and y * 2^-40: powers of two are exact in every float32 operation of the path."""
    nfft = ROUTES[route][0]
    x, y = route_pair(route)
    base = run_route(ctx, hip, route, x, y)
    xs, ys = (x * np.float32(2.0 ** 40)).astype(np.complex64), (y * np.float32(2.0 ** -40)).astype(np.complex64)
    got = run_route(ctx, hip, route, xs, ys)
    d = float(np.max(np.abs(got[3].astype(np.float64) - base[3])))
    print('csd degenerate | %s gains | Cxy moved by %.2e, bit-identical: %s' % (route, d, np.array_equal(got[3].view(np.uint32), base[3].view(np.uint32))))
    assert d < 1e-6
    gate('degenerate', route + ' gains', got, oracle(xs, ys, nfft))
    ref = oracle(x, y, nfft)
    assert relerr(got[0].astype(np.float64) * 2.0 ** -80, ref[0]) < RTOL and relerr(got[1].astype(np.float64) * 2.0 ** 80, ref[1]) < RTOL


@pytest.mark.parametrize('nfft,kernel', [(n, 'generic') for n in POW2] + [(4096, 'tuned'), (4099, 'auto')])
def test_identical_channels(ctx, hip, nfft, kernel):
    """x against itself: Cxy = 1 (1e-5, as test_hip_parity's 1024-point case) and Im Pxy = 0 EXACTLY - Im(conj(X) X) =
    Xr Xi - Xi Xr is formed from two rounded products (cross_im in fft_lds.hip.h), not from an fma that leaves one
    product's rounding error behind."""
    code = {'generic': hip.KERNEL_GENERIC, 'tuned': hip.KERNEL_TUNED, 'auto': hip.KERNEL_AUTO}[kernel]
    for nseg in (1, 9, 70):
        x, _ = pair(nfft, nfft // 2, nseg, 9 + nfft)
        plan = ctx.welch_plan(nfft, window=window('hann', nfft), kernel=code)
        pxx, pyy, pxy, cxy = plan.csd(x, x)
        plan.close()
        print('csd degenerate | identical %d %s nseg %d | max |Cxy - 1| %.2e, max |Im Pxy| / Pxx %.2e'
              % (nfft, kernel, nseg, np.max(np.abs(cxy - 1.0)), np.max(np.abs(pxy.imag) / pxx)))
        assert np.max(np.abs(cxy - 1.0)) < 1e-5
        assert np.all(pxy.imag == 0), float(np.max(np.abs(pxy.imag) / pxx))
        assert np.array_equal(pxx, pyy) and relerr(pxy.real, pxx) < 1e-6
        assert nseg == 1 or relerr(pxx, oracle(x, x, nfft)[0]) < RTOL      # (one periodogram has nulls: not gated per bin)


# ---- 5. one plan, shrinking and regrowing segment counts --------------------------------------------------------------------------

@pytest.mark.parametrize('nfft,kernel', [(1024, 'auto'), (4096, 'tuned')])
def test_one_plan_across_shrinking_segment_counts(ctx, hip, nfft, kernel):
    """70, 3, 40, 1 and 70 segment pairs on ONE plan: the partial buffer keeps its widest size, so a finalize that read
    rows of an earlier, wider launch would show in the narrow ones; the last run equals the first bit for bit."""
    plan = ctx.welch_plan(nfft, window=window('hann', nfft), kernel=hip.KERNEL_TUNED if kernel == 'tuned' else hip.KERNEL_AUTO)
    first = None
    for i, nseg in enumerate((70, 3, 40, 1, 70)):
        x, y = pair(nfft, nfft // 2, nseg, 600 + nfft + nseg)
        got = plan.csd(x, y)
        assert plan.last_nseg == nseg and recipe_W(plan.last_recipe()) == nseg
        gate('reuse', '%d %s call %d nseg %d' % (nfft, kernel, i, nseg), got, oracle(x, y, nfft))
        if first is None:
            first = [v.copy() for v in got]
    for a, b in zip(first, got):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    plan.close()


# ---- 6. the block on top ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', [1024, 1000])
def test_coherence_estimator_block(ctx, hip, N):
    import ofdm_tools
    Sf, tune, block_len = 2000000, 433000000, 10 * N
    x, y = _pair(2 * block_len, 31 + N)
    est = ofdm_tools.coherence_estimator(N, Sf, block_len=block_len, ctx=ctx)
    msgs = []
    est.msg_connect('coherence', msgs.append)
    for call in range(2):
        xs, ys = x[call * block_len:(call + 1) * block_len], y[call * block_len:(call + 1) * block_len]
        assert est.work([xs, ys], []) == block_len
        ref = oracle(xs, ys, N, fs=float(Sf), fftshift=True)
        gate('block', 'N %d call %d' % (N, call), (est.pxx, est.pyy, est.pxy, est.cxy), ref)
        assert len(msgs) == call + 1 and msgs[-1][0] == 'coherence' and np.array_equal(np.asarray(msgs[-1][1]), est.cxy)
    assert est._plan.last_recipe().startswith('kernel=welch_generic ' if N == 1024 else 'kernel=anyfft:')
    calls = []
    det = ofdm_tools.coherence_detector(N, Sf, threshold=1.2, threshold_mtm=0.2, tune_freq=tune,
                                        subject_channels=[tune + 0.1234 * Sf, tune - 0.31 * Sf, tune + 0.25 * Sf],
                                        valve_callback=calls.append)
    quiet = np.zeros(N, np.float32)
    det.work([est.cxy.reshape(1, N), quiet.reshape(1, N), quiet.reshape(1, N)], [])
    coh, outcome, valve = R.coherence_scanner(ref[3], quiet, quiet, det.idx_subject_channels, 1.2, 0.2)
    assert det.get_subject_channels_outcome() == outcome and calls == valve
    assert np.allclose(det.subject_channels_coherence, coh, atol=2 * RTOL)
