"""Spectrum-scanner helpers of ``ofdm_tools.ofdm_cr_tools`` with the reference's
names, argument order and return values (python/ofdm_cr_tools.py:136-250,
:321-345, :471-537), computing on the MI355X through libofdmtools_hip.so.

Host code here is limited to what the reference also does in Python around the
arithmetic: ``frange`` lists, slice bounds with ``int()`` truncation, threshold
bookkeeping.  The FFTs, the Welch averaging, the moving average and the channel
sums run in HIP kernels; nothing here falls back to NumPy/SciPy for them.
"""
import math
import threading

import numpy as np

from . import _hip
from . import windows


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _py2div(a, b):
    """The reference is Python 2: ``/`` between two ints floors."""
    if _is_int(a) and _is_int(b):
        return a // b
    return a / b


def _welch_plan(ctx, nfft, window_name, Sf, npts=None, use='exec', average='mean'):
    """The reference's `sg.welch(x, Sf, window, nperseg=nfft, nfft=nfft)` + fftshift (ofdm_cr_tools.py:214,322,342).
    SciPy shortens nperseg to the input length when the vector is shorter than nfft ("nperseg = N is greater than input
    length", one zero-padded segment) - which fast_spectrum_scan(n_fft=0) always hits, its nFFT being the next power of
    two above len(vct_sample) (ofdm_cr_tools.py:474-475).  average: 'mean' (the reference's call) or 'median'
    (sg.welch(..., average='median')).  -> (cache key, factory) with use='async', else the plan."""
    nperseg = nfft if npts is None else min(int(nfft), int(npts))
    code = _hip.average_code(average)
    key = ('welch', use, nfft, nperseg, window_name, float(Sf), code)
    extra = {} if code == _hip.AVERAGE_MEAN else {'average': code}
    make = lambda: ctx.welch_plan(nfft, nperseg=nperseg, window=windows.get_window(window_name, nperseg), fs=float(Sf),
                                  fftshift=True, **extra)
    # `use`: the ticket callers (SpectrumScan: exec_async / poll from work()) do not share plans with the blocking helpers,
    # whose calls could push an uncollected ticket out of a plan's output ring; among themselves they share a pool
    # (_exec_async_pooled)
    return (key, make) if use == 'async' else ctx.cached_plan(key, make)


def _mtm_plan(ctx, nfft, Sf, npts=None, NW=4.0, K=None, use='exec'):
    """The multitaper estimate of one capture: Slepian tapers of half-bandwidth NW over nperseg = min(nfft, len) samples (the
    nperseg rule of _welch_plan: a vector shorter than nfft is one zero-padded segment), K = int(2 NW) - 1 of them by
    default, unit weights, density scaling, no overlap, fftshift.  -> (cache key, factory) with use='async', else the plan."""
    nperseg = nfft if npts is None else min(int(nfft), int(npts))
    K = int(2 * NW) - 1 if K is None else int(K)
    key = ('mtm', use, nfft, nperseg, float(NW), K, float(Sf))
    make = lambda: ctx.mtm_plan(nfft, nperseg=nperseg, noverlap=0, nw=float(NW), ntapers=K, fs=float(Sf), fftshift=True)
    return (key, make) if use == 'async' else ctx.cached_plan(key, make)


def _exec_async_pooled(ctx, key, make, vector):
    """exec_async() on the first plan of the shape's pool (cache keys key + (0,), key + (1,), ...) whose next ticket lands
    in an output-ring slot no uncollected ticket holds (WelchPlan.next_ticket_slot_free: the library keeps launch t in
    slot t % 4, so a plan owing fewer than four tickets can still be unsafe when they are collected out of order); a new
    plan joins the pool when none is free.  Several scans of one shape in flight - SpectrumScans of several blocks on the
    default context, collected in any order - then never lose a ticket to each other, and Context.cached_plan keeps every
    plan that still owes one.  Pool plans serve exec_async() only.  -> (plan, ticket)."""
    with ctx.__dict__.setdefault('_async_pool_lock', threading.Lock()):      # one free slot cannot go to two threads
        i = 0
        while True:
            plan = ctx.cached_plan(key + (i,), make)
            if plan.next_ticket_slot_free():
                return plan, plan.exec_async(vector)
            i += 1


def frange(x, y, jump):
    """ofdm_cr_tools.py:136-141."""
    out = []
    while x < y:
        out.append(x)
        x += jump
    return out


def _slice_bounds(n, Fr, Sf, bb_freqs, srch_bins):
    """Start/stop of every channel slice exactly as Python evaluates
    ``psd[0:int(b+sb/2)]`` / ``psd[int(b-sb/2):int(b+sb/2)]`` (ofdm_cr_tools.py:239-248)."""
    half = _py2div(Sf, 2)
    lo, hi = [], []
    for i, f in enumerate(bb_freqs):
        bin_n = (f + half) / Fr
        sl = slice(0, int(bin_n + srch_bins / 2)) if i == 0 else \
            slice(int(bin_n - srch_bins / 2), int(bin_n + srch_bins / 2))
        a, b, _ = sl.indices(n)
        lo.append(a)
        hi.append(max(a, b))
    return lo, hi


def movingaverage(interval, window_size, ctx=None):
    """ofdm_cr_tools.py:168-170 on the device."""
    ctx = ctx or _hip.default_context()
    _, ma = ctx.channel_power(interval, float(window_size), [0], [0], want_movavg=True)
    return ma


def src_power(psd, nFFT, Fr, Sf, bb_freqs, srch_bins, ctx=None):
    """ofdm_cr_tools.py:232-249: moving average, then per-channel sums."""
    ctx = ctx or _hip.default_context()
    lo, hi = _slice_bounds(len(psd), Fr, Sf, bb_freqs, srch_bins)
    return [float(v) for v in ctx.channel_power(psd, float(srch_bins), lo, hi)]


def _plain_channel_sums(psd, Fr, Sf, bb_freqs, srch_bins, ctx):
    # channel sums without the moving average (src_power_welch / src_power_fft): a 1-tap average
    lo, hi = _slice_bounds(len(psd), Fr, Sf, bb_freqs, srch_bins)
    return [float(v) for v in ctx.channel_power(psd, 1.0, lo, hi)]


def _enqueue_welch(vector, nFFT, Sf, ctx, average='mean'):
    """src_power_welch's PSD (flattop, nperseg = nfft, ofdm_cr_tools.py:213-216) as a ticket: -> (plan, ticket, post)."""
    plan, ticket = _exec_async_pooled(ctx, *_welch_plan(ctx, nFFT, 'flattop', Sf, len(vector), use='async', average=average),
                                      vector=vector)
    return plan, ticket, None


def _enqueue_fft(vector, nFFT, Sf, ctx):
    """src_power_fft's single flat-top periodogram |FFT(x w, nFFT)|^2 / nFFT (ofdm_cr_tools.py:173-178) as a ticket."""
    vector = np.asarray(vector)
    total = len(vector)                   # the reference windows ALL len(vector) samples, then np.fft.fft(., nFFT) keeps the first nFFT
    vector = vector[:nFFT]
    npts = len(vector)
    plan, ticket = _exec_async_pooled(
        ctx, ('fft', nFFT, total, npts),
        lambda: ctx.welch_plan(nFFT, nperseg=npts, noverlap=0, window=windows.flattop(total)[:nFFT],
                               detrend=_hip.DETREND_NONE, scaling=_hip.SCALE_RAW, fftshift=True), vector)
    return plan, ticket, (lambda psd: psd / np.float32(nFFT))


def _enqueue_mtm(vector, nFFT, Sf, ctx, NW=4.0, K=7):
    """The scan's PSD as a multitaper estimate (NW 4, K 7) as a ticket: -> (plan, ticket, post)."""
    plan, ticket = _exec_async_pooled(ctx, *_mtm_plan(ctx, nFFT, Sf, len(vector), NW, K, use='async'), vector=vector)
    return plan, ticket, None


def src_power_mtm(vector, npts, nFFT, Fr, Sf, bb_freqs, srch_bins, NW=4.0, K=None, ctx=None):
    """src_power_welch with the multitaper estimate in place of the flat-top Welch PSD: -> (psd, axis, channel sums)."""
    ctx = ctx or _hip.default_context()
    plan, ticket, _ = _enqueue_mtm(vector, nFFT, Sf, ctx, NW, K)
    psd = plan.wait(ticket)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf))
    return psd, axis, _plain_channel_sums(psd, Fr, Sf, bb_freqs, srch_bins, ctx)


def src_power_welch(vector, npts, nFFT, Fr, Sf, bb_freqs, srch_bins, ctx=None, average='mean'):
    """ofdm_cr_tools.py:213-230 (average='median': the same with sg.welch(..., average='median'))."""
    ctx = ctx or _hip.default_context()
    plan, ticket, _ = _enqueue_welch(vector, nFFT, Sf, ctx, average)
    psd = plan.wait(ticket)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf))
    return psd, axis, _plain_channel_sums(psd, Fr, Sf, bb_freqs, srch_bins, ctx)


def src_power_fft(vector, npts, nFFT, Fr, Sf, bb_freqs, srch_bins, ctx=None):
    """ofdm_cr_tools.py:173-192: one flat-top periodogram |FFT(x w, nFFT)|^2 / nFFT, shifted."""
    ctx = ctx or _hip.default_context()
    plan, ticket, post = _enqueue_fft(vector, nFFT, Sf, ctx)
    psd = post(plan.wait(ticket))
    axis = _py2div(Sf, 2) * np.linspace(-1, 1, nFFT)
    return psd, axis, _plain_channel_sums(psd, Fr, Sf, bb_freqs, srch_bins, ctx)


def clc_power_freq(vector, nFFT, Sf, ctx=None):
    """ofdm_cr_tools.py:149-153."""
    n = len(vector)                       # normalisation uses the full length even when fft() truncates
    return float((_raw_periodogram(vector, nFFT, ctx or _hip.default_context(), False) / n / Sf).sum())


def _raw_periodogram(vector, nFFT, ctx, fftshift):
    """|FFT(vector, nFFT)|^2 on the device - np.fft.fft(v, n) truncates a longer vector and zero-pads a shorter one."""
    vector = np.asarray(vector)[:nFFT]
    plan = ctx.welch_plan(nFFT, nperseg=len(vector), noverlap=0, window=None, detrend=_hip.DETREND_NONE,
                          scaling=_hip.SCALE_RAW, fftshift=fftshift)
    psd = plan.exec(vector).astype(np.float64)
    plan.close()
    return psd


def clc_power_time(vector, ctx=None):
    """ofdm_cr_tools.py:144-146: mean |x|^2 (one reduction on the device)."""
    ctx = ctx or _hip.default_context()
    v = np.ascontiguousarray(vector, np.complex64)
    d = ctx.alloc(v.nbytes)
    try:
        ctx.h2d(d, v)
        mean, var = ctx.iq_power(d, len(v))
    finally:
        ctx.free(d)
    return float(var + abs(mean) ** 2)


def td_power_estimate(vector, Sf, ctx=None):
    """ofdm_cr_tools.py:337-339: sum |x|^2 / Sf."""
    return clc_power_time(vector, ctx) * len(vector) / Sf


def fft_plot_dB(data, Sf, fc, nfft, ctx=None):
    """ofdm_cr_tools.py:312-319: one rectangular periodogram / (npts Sf), shifted, in dB over the shifted axis."""
    psd = _raw_periodogram(data, nfft, ctx or _hip.default_context(), True) / (len(data) * Sf)
    fft_axis = _py2div(Sf, 2) * np.linspace(-1, 1, nfft)
    return [item + fc for item in fft_axis], [10 * math.log10(item + 1e-20) for item in psd]


def fft_plot_lin(data, Sf, fc, nfft, ctx=None):
    """ofdm_cr_tools.py:328-335: the same periodogram, linear."""
    psd = _raw_periodogram(data, nfft, ctx or _hip.default_context(), True) / len(data) / Sf
    fft_axis = _py2div(Sf, 2) * np.linspace(-1, 1, nfft)
    return [item + fc for item in fft_axis], psd


def xcorr(a, b, length, ctx=None):
    """ofdm_cr_tools.py:155-161."""
    return (ctx or _hip.default_context()).xcorr(a, b, length)


def fac(data, length, ctx=None):
    """ofdm_cr_tools.py:163-166."""
    return (ctx or _hip.default_context()).fac(data, length)


def welch_plot_dB(data, Sf, fc, nfft, ctx=None, average='mean'):
    """ofdm_cr_tools.py:321-326 (default Hann window, 50 % overlap)."""
    ctx = ctx or _hip.default_context()
    psd = _welch_plan(ctx, nfft, 'hann', Sf, len(data), average=average).exec(data)
    axis = np.fft.fftshift(np.fft.fftfreq(nfft, 1.0 / Sf))
    return [item + fc for item in axis], [10 * math.log10(item + 1e-20) for item in psd]


def welch_power_estimate(vector, nFFT, Sf, ctx=None, average='mean'):
    """ofdm_cr_tools.py:341-345."""
    ctx = ctx or _hip.default_context()
    return float(np.sum(_welch_plan(ctx, nFFT, 'hann', Sf, len(vector), average=average).exec(vector), dtype=np.float64))


def mtm_plot_dB(data, Sf, fc, nfft, NW=4.0, K=None, ctx=None):
    """welch_plot_dB with the multitaper estimate (Slepian tapers, half-bandwidth NW, K tapers)."""
    ctx = ctx or _hip.default_context()
    psd = _mtm_plan(ctx, nfft, Sf, len(data), NW, K).exec(data)
    axis = np.fft.fftshift(np.fft.fftfreq(nfft, 1.0 / Sf))
    return [item + fc for item in axis], [10 * math.log10(item + 1e-20) for item in psd]


def mtm_power_estimate(vector, nFFT, Sf, NW=4.0, K=None, ctx=None):
    """welch_power_estimate with the multitaper estimate: the sum over bins of the density."""
    ctx = ctx or _hip.default_context()
    return float(np.sum(_mtm_plan(ctx, nFFT, Sf, len(vector), NW, K).exec(vector), dtype=np.float64))


def _pfb_plan(ctx, nfft, ntaps, Sf, npts):
    """The filter-bank estimate of one capture: windows.pfb_prototype(nfft, ntaps) folded onto nfft points, critically
    sampled (hop nfft), constant detrend per frame, density scaling, fftshift.  Refuses in Python what the library would
    refuse: a size outside the powers of two 64 ... 16384, ntaps outside 2 ... 16, a capture shorter than one frame."""
    if not _is_int(nfft) or nfft < 64 or nfft > 16384 or nfft & (nfft - 1):
        raise ValueError('the filter-bank PSD needs nFFT a power of two from 64 to 16384, not %r' % (nfft,))
    if not _is_int(ntaps) or not 2 <= ntaps <= 16:
        raise ValueError('the filter-bank PSD needs ntaps in 2 ... 16, not %r' % (ntaps,))
    if npts < ntaps * nfft:
        raise ValueError('the filter-bank PSD needs at least ntaps * nFFT = %d samples, not %d' % (ntaps * nfft, npts))
    nfft, ntaps = int(nfft), int(ntaps)
    ctx = ctx or _hip.default_context()

    def make():
        plan = ctx.welch_plan(nfft, nperseg=nfft, noverlap=0, window=None, fs=float(Sf), fftshift=True)
        plan.set_prototype(windows.pfb_prototype(nfft, ntaps), ntaps)
        return plan
    return ctx.cached_plan(('pfb', nfft, ntaps, float(Sf)), make)


def src_power_pfb(vector, npts, nFFT, Fr, Sf, bb_freqs, srch_bins, ntaps=8, ctx=None):
    """src_power_welch with the polyphase filter-bank estimate (a Kaiser-windowed sinc of ntaps * nFFT taps folded in front
    of the transform) in place of the flat-top Welch PSD: a strong neighbour does not leak into an empty channel's sum.
    Blocking.  -> (psd, axis, channel sums)."""
    plan = _pfb_plan(ctx, nFFT, ntaps, Sf, len(vector))
    psd = plan.pfb(vector)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf))
    return psd, axis, _plain_channel_sums(psd, Fr, Sf, bb_freqs, srch_bins, plan.ctx)


def pfb_plot_dB(data, Sf, fc, nfft, ntaps=8, ctx=None):
    """welch_plot_dB with the polyphase filter-bank estimate (ntaps taps per branch)."""
    psd = _pfb_plan(ctx, nfft, ntaps, Sf, len(data)).pfb(data)
    axis = np.fft.fftshift(np.fft.fftfreq(nfft, 1.0 / Sf))
    return [item + fc for item in axis], [10 * math.log10(item + 1e-20) for item in psd]


def pfb_power_estimate(vector, nFFT, Sf, ntaps=8, ctx=None):
    """welch_power_estimate with the polyphase filter-bank estimate: the sum over bins of the density."""
    return float(np.sum(_pfb_plan(ctx, nFFT, ntaps, Sf, len(vector)).pfb(vector), dtype=np.float64))


def _ftest_log_sf(f, a, b, logc):
    """log P(F > f) for F(2 a, 2 b), a and b integers: with x = a f / (a f + b) the survival function is the binomial sum
    sum_{i < a} C(a + b - 1, i) x^i (1 - x)^(a + b - 1 - i); logc[i] = log C(a + b - 1, i)."""
    n = a + b - 1
    i = np.arange(a, dtype=np.float64)
    lden = math.log(a * f + b)
    terms = logc + i * (math.log(a * f) - lden) + (n - i) * (math.log(b) - lden)
    top = float(np.max(terms))
    return top + math.log(float(np.sum(np.exp(terms - top))))


def ftest_threshold(p_false, nseg, K):
    """The value the harmonic F-test (MtmPlan.ftest) exceeds with probability p_false in a bin without a line: the upper
    p_false quantile of F(2 nseg, 2 nseg (K - 1)).  Both half-degrees of freedom are integers, so the survival function is a
    finite binomial sum (evaluated in log space) and the quantile its inversion by bisection on log f."""
    nseg, K = int(nseg), int(K)
    if not 0.0 < p_false < 1.0 or nseg < 1 or K < 2:
        raise ValueError('need 0 < p_false < 1, nseg >= 1 and K >= 2')
    a, b = nseg, nseg * (K - 1)
    n = a + b - 1
    logc = np.array([math.lgamma(n + 1) - math.lgamma(i + 1) - math.lgamma(n - i + 1) for i in range(a)])
    want = math.log(p_false)
    lo, hi = -700.0, 700.0      # log f: the survival function falls from 1 to 0 between
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        if _ftest_log_sf(math.exp(mid), a, b, logc) > want:
            lo = mid
        else:
            hi = mid
    return math.exp(0.5 * (lo + hi))


def _betacf(a, b, x):
    """The continued fraction of the incomplete beta function (modified Lentz), for x < (a + 1) / (a + b + 2)."""
    tiny = 1e-300
    c, d = 1.0, 1.0 - (a + b) * x / (a + 1.0)
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 100000):
        m2 = 2 * m
        for num in (m * (b - m) * x / ((a + m2 - 1.0) * (a + m2)), -(a + m) * (a + b + m) * x / ((a + m2) * (a + m2 + 1.0))):
            d = 1.0 + num * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + num / c
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return h


def _betainc(a, b, x, xc):
    """Regularised incomplete beta I_x(a, b); xc = 1 - x, handed in so that neither end loses digits."""
    if x <= 0.0:
        return 0.0
    if xc <= 0.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(xc))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, xc) / b


def _student_t_sf(t, dof):
    """P(T > t), t >= 0, for Student's t with dof degrees of freedom: I_x(dof / 2, 1 / 2) / 2 at x = dof / (dof + t^2)."""
    t2 = t * t
    return 0.5 * _betainc(0.5 * dof, 0.5, dof / (dof + t2), t2 / (dof + t2))


def student_t_quantile(p, dof):
    """The value Student's t with dof degrees of freedom exceeds with probability p (the upper-p quantile,
    scipy.stats.t.isf): the survival function through the regularised incomplete beta function (continued fraction),
    inverted by bisection on log t.  The jackknife intervals take it at M - 1 degrees of freedom."""
    p, dof = float(p), float(dof)
    if not 0.0 < p < 1.0 or not dof >= 1.0:
        raise ValueError('need 0 < p < 1 and dof >= 1')
    if p == 0.5:
        return 0.0
    if p > 0.5:
        return -student_t_quantile(1.0 - p, dof)
    lo, hi = -100.0, 100.0      # log t: the survival function falls from 1 / 2 to 0 between
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        if _student_t_sf(math.exp(mid), dof) > p:
            lo = mid
        else:
            hi = mid
    return math.exp(0.5 * (lo + hi))


def _gamma_pq(a, x, lga):
    """Regularised incomplete gamma functions (P, Q)(a, x) of float64 arrays a > 0, x > 0 (lga = lgamma(a)): the series for
    P where x < a + 1, the continued fraction for Q (modified Lentz) elsewhere, the other as the complement - which loses
    nothing there: the complement is the larger of the two."""
    front = np.exp(a * np.log(x) - x - lga)
    P = np.empty_like(x)
    low = x < a + 1.0
    if np.any(low):
        al, xl = a[low], x[low]
        term = 1.0 / al
        total = term.copy()
        for n in range(1, 100000):
            term = term * xl / (al + n)
            total += term
            if np.all(term <= 1e-17 * total):
                break
        P[low] = front[low] * total
    high = ~low
    if np.any(high):
        ah, xh = a[high], x[high]
        tiny = 1e-300
        b = xh + 1.0 - ah
        c = np.full_like(xh, 1.0 / tiny)
        d = 1.0 / np.where(np.abs(b) > tiny, b, tiny)
        h = d.copy()
        for i in range(1, 100000):
            an = -i * (i - ah)
            b = b + 2.0
            d = an * d + b
            d = 1.0 / np.where(np.abs(d) > tiny, d, tiny)
            c = b + an / c
            c = np.where(np.abs(c) > tiny, c, tiny)
            delta = d * c
            h = h * delta
            if np.all(np.abs(delta - 1.0) < 4e-16):
                break
        P[high] = 1.0 - front[high] * h
    Q = 1.0 - P
    Q[high] = front[high] * h if np.any(high) else Q[high]
    return P, Q


def chi2_quantile(p, nu):
    """The p-quantile of chi-square with nu degrees of freedom, any real nu > 0 (scipy.stats.chi2.ppf): the regularised
    incomplete gamma function at a = nu / 2 by its series or continued fraction, inverted by bisection on log x - against
    the lower tail for p <= 1 / 2 and the upper one above, so that neither end loses digits.  p and nu may be arrays (they
    broadcast); two scalars give a float.  The adaptive estimate's per-bin degrees of freedom are not integers."""
    scalar = np.ndim(p) == 0 and np.ndim(nu) == 0
    pa, na = np.broadcast_arrays(np.asarray(p, np.float64), np.asarray(nu, np.float64))
    shape = pa.shape
    pa, na = pa.ravel().copy(), na.ravel().copy()
    if not (np.all(pa > 0.0) and np.all(pa < 1.0) and np.all(na > 0.0) and np.all(np.isfinite(na))):
        raise ValueError('need 0 < p < 1 and nu > 0')
    a = 0.5 * na
    lga = np.array([math.lgamma(v) for v in a])
    upper = pa > 0.5
    want = np.where(upper, 1.0 - pa, pa)
    lo = np.full_like(a, -745.0)      # log (x / 2): the distribution function rises from 0 to 1 between
    hi = np.log(a + 40.0 * np.sqrt(a) + 800.0)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not np.any((lo < mid) & (mid < hi)):
            break
        P, Q = _gamma_pq(a, np.exp(mid), lga)
        below = np.where(upper, Q > want, P < want)      # mid lies below the quantile
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    out = (2.0 * np.exp(0.5 * (lo + hi))).reshape(shape)
    return float(out) if scalar else out


def mtm_adaptive_estimate(vector, nFFT, Sf, NW=4.0, K=None, iters=4, ctx=None):
    """mtm_power_estimate's plan with Thomson's adaptive weights (MtmPlan.adaptive) -> (psd, dof): the density, fftshifted,
    in which an empty channel next to an occupied one is not lifted by the high-order tapers' leakage (fixed weights see
    no floor more than about 34 dB under a neighbouring band at NW 4, K 7), and the per-bin equivalent degrees of freedom
    a chi-square threshold or interval needs (mtm_adaptive_interval)."""
    ctx = ctx or _hip.default_context()
    return _mtm_plan(ctx, nFFT, Sf, len(vector), NW, K).adaptive(vector, iters=iters, return_dof=True)


def mtm_adaptive_interval(psd, dof, nseg, confidence=0.95):
    """The chi-square interval of an adaptive estimate: with nu' = nseg dof per bin and alpha = 1 - confidence,
    (lo, hi) = psd nu' / chi2_{nu'}(1 - alpha / 2), psd nu' / chi2_{nu'}(alpha / 2).  psd linear (not dB), dof as
    MtmPlan.adaptive returns it, nseg the plan's last_nseg.  nu' = nseg dof takes the segments for independent: it holds
    for segments that do not overlap and overstates the degrees of freedom of overlapping ones.  A bin without degrees of
    freedom (dof = 0: silence) gets lo = hi = psd."""
    if not 0.0 < confidence < 1.0:
        raise ValueError('confidence must lie in (0, 1)')
    psd = np.asarray(psd, np.float64)
    nu = float(nseg) * np.asarray(dof, np.float64)
    live = nu > 0.0
    lo, hi = psd.copy(), psd.copy()
    if np.any(live):
        alpha = 1.0 - confidence
        lo[live] = psd[live] * nu[live] / chi2_quantile(1.0 - 0.5 * alpha, nu[live])
        hi[live] = psd[live] * nu[live] / chi2_quantile(0.5 * alpha, nu[live])
    return lo, hi


def mtm_psd_interval(vector, nFFT, Sf, fc=0.0, NW=4.0, K=None, confidence=0.95, ctx=None):
    """mtm_plot_dB with a confidence band: the multitaper PSD of one capture on the plan of the other mtm_* helpers and its
    jackknife interval over the M = K nseg (segment, taper) items (MtmPlan.jackknife) - psd exp(-+ q lnsd) with q the
    Student-t quantile at (1 - confidence) / 2 and M - 1 degrees of freedom.  -> (axis, lo_dB, psd_dB, hi_dB), arrays."""
    if not 0.0 < confidence < 1.0:
        raise ValueError('confidence must lie in (0, 1)')
    ctx = ctx or _hip.default_context()
    plan = _mtm_plan(ctx, nFFT, Sf, len(vector), NW, K)
    lnsd, psd = plan.jackknife(vector, return_psd=True)
    M = plan.last_nseg * plan.ntapers
    q = student_t_quantile(0.5 * (1.0 - confidence), M - 1)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf)) + fc
    psd_dB = 10.0 * np.log10(psd.astype(np.float64) + 1e-20)
    half = (10.0 / math.log(10.0)) * q * lnsd.astype(np.float64)
    return axis, psd_dB - half, psd_dB, psd_dB + half


def _mtm_csd_plan(ctx, nfft, Sf, npts=None, NW=4.0, K=None):
    """_mtm_plan's shape with the two-channel calls open."""
    nperseg = nfft if npts is None else min(int(nfft), int(npts))
    K = int(2 * NW) - 1 if K is None else int(K)
    key = ('mtmcsd', 'exec', nfft, nperseg, float(NW), K, float(Sf))
    return ctx.cached_plan(key, lambda: ctx.mtm_csd_plan(nfft, nperseg=nperseg, noverlap=0, nw=float(NW), ntapers=K,
                                                         fs=float(Sf), fftshift=True))


def coherence_bounds(cxy, zsd, q_lo, q_hi):
    """tanh(max(0, z - q_lo zsd))^2 and tanh(z + q_hi zsd)^2 at z = atanh(sqrt(cxy)), clamped as the library clamps it."""
    z = np.arctanh(np.minimum(np.sqrt(np.asarray(cxy, np.float64)), 1.0 - 2.0 ** -24))
    zsd, c = np.asarray(zsd, np.float64), np.asarray(cxy, np.float64)
    # (the estimate itself bounds both: tanh(atanh(s))^2 is s^2 to rounding only, and the clamp sits below a coherence of 1)
    return np.minimum(np.tanh(np.maximum(0.0, z - q_lo * zsd)) ** 2, c), np.maximum(np.tanh(z + q_hi * zsd) ** 2, c)


def mtm_coherence_interval(x, y, nFFT, Sf, NW=4.0, K=None, confidence=0.95, ctx=None):
    """The multitaper magnitude-squared coherence of a capture pair and its jackknife interval (MtmCsdPlan.csd_jackknife):
    tanh(max(0, z -+ q zsd))^2 around z = atanh(sqrt(cxy)), q the Student-t quantile at (1 - confidence) / 2 and M - 1
    degrees of freedom.  A true coherence of 0 is not covered at the nominal rate: the estimate is biased upwards there.
    -> (axis, cxy_lo, cxy, cxy_hi), fftshifted arrays."""
    if not 0.0 < confidence < 1.0:
        raise ValueError('confidence must lie in (0, 1)')
    ctx = ctx or _hip.default_context()
    plan = _mtm_csd_plan(ctx, nFFT, Sf, min(len(x), len(y)), NW, K)
    cxy, zsd, _, _ = plan.csd_jackknife(x, y)
    q = student_t_quantile(0.5 * (1.0 - confidence), plan.last_nseg * plan.ntapers - 1)
    lo, hi = coherence_bounds(cxy, zsd, q, q)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf))
    return axis, lo, cxy.astype(np.float64), hi


def mtm_line_scan(vector, nFFT, Sf, fc=0.0, NW=4.0, K=None, p_false=None, ctx=None):
    """Coherent lines (pilots, carriers, narrowband interferers) of one capture by Thomson's harmonic F-test on the plan of
    the other mtm_* helpers: nperseg = min(nFFT, len), one pass without overlap.  A line is a bin whose F exceeds
    ftest_threshold(p_false, nseg, K) - p_false = 1e-3 / nFFT by default: one false line in a thousand scans - and is the
    largest within the main lobe, +-ceil(NW nFFT / nperseg) bins.  -> (F fftshifted, frequency axis, line frequencies)."""
    ctx = ctx or _hip.default_context()
    plan = _mtm_plan(ctx, nFFT, Sf, len(vector), NW, K)
    F = plan.ftest(vector)
    nseg = plan.last_nseg
    p_false = 1e-3 / nFFT if p_false is None else p_false
    thr = ftest_threshold(p_false, nseg, plan.ntapers)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf)) + fc
    half = int(math.ceil(float(NW) * nFFT / plan.nperseg))
    lines = []
    for i in np.flatnonzero(F > thr):
        lobe = F[np.arange(i - half, i + half + 1) % nFFT]      # (the spectrum is periodic)
        if int(np.argmax(lobe)) == half:
            lines.append(float(axis[i]))
    return F, axis, lines


SK_SIZES = tuple(2 ** i for i in range(6, 15))      # the transform lengths WelchPlan.sk takes


def sk_null_moments(M):
    """Exact moments of the spectral kurtosis estimator over M independent segments of Gaussian noise (Nita & Gary): the
    mean is 1; -> (mu2, beta1, beta2), the variance, the squared skewness and the kurtosis."""
    M = float(M)
    mu2 = 4.0 * M * M / ((M - 1.0) * (M + 2.0) * (M + 3.0))
    beta1 = 4.0 * (M + 2.0) * (M + 3.0) * (5.0 * M - 7.0) ** 2 / ((M - 1.0) * (M + 4.0) ** 2 * (M + 5.0) ** 2)
    beta2 = (3.0 * (M + 2.0) * (M + 3.0) * (M ** 3 + 98.0 * M * M - 185.0 * M + 78.0) /
             ((M - 1.0) * (M + 4.0) * (M + 5.0) * (M + 6.0) * (M + 7.0)))
    return mu2, beta1, beta2


def sk_limits(M, p_false):
    """(lower, upper): the values the spectral kurtosis of a noise-only bin (WelchPlan.sk over M segments) falls below,
    respectively exceeds, with probability p_false each.  A Pearson type IV density fitted to the exact null moments of the
    estimator (sk_null_moments), normalised numerically on [0, 1 + 60 sqrt(mu2)] - SK is never negative - and inverted on
    that grid; no SciPy.  The moments call for type IV from M = 24 on, and a type III fit misses the lower tail by a factor
    of 40 at M = 16: M < 32 is a ValueError.  The limits assume independent segments, that is no overlap; against a Monte
    Carlo of the null the fit's rates lie within 0.6 ... 1.1 of p_false down to 1e-3, and below 1e-4 the tails are
    extrapolated, not checked."""
    if isinstance(M, bool) or int(M) != M:
        raise ValueError('M must be an integer segment count, not %r' % (M,))
    M = int(M)
    if M < 32:
        raise ValueError('sk_limits needs M >= 32 segments (the Pearson type IV fit of the null does not hold below), not %d' % M)
    if not 0.0 < p_false < 1.0:
        raise ValueError('need 0 < p_false < 1')
    mu2, beta1, beta2 = sk_null_moments(M)
    r = 6.0 * (beta2 - beta1 - 1.0) / (2.0 * beta2 - 3.0 * beta1 - 6.0)
    m = 0.5 * (r + 2.0)
    d = 16.0 * (r - 1.0) - beta1 * (r - 2.0) ** 2
    nu = -r * (r - 2.0) * math.sqrt(beta1) / math.sqrt(d)
    a = math.sqrt(mu2 * d) / 4.0
    lam = 1.0 - (r - 2.0) * math.sqrt(beta1 * mu2) / 4.0
    x = np.linspace(0.0, 1.0 + 60.0 * math.sqrt(mu2), (1 << 20) + 1)
    t = (x - lam) / a
    logpdf = -m * np.log1p(t * t) - nu * np.arctan(t)
    pdf = np.exp(logpdf - np.max(logpdf))
    cell = 0.5 * (pdf[1:] + pdf[:-1])                        # trapezoids (the grid step cancels in the ratios)
    below = np.concatenate(([0.0], np.cumsum(cell)))           # mass in [0, x]
    above = np.concatenate((np.cumsum(cell[::-1])[::-1], [0.0]))      # mass in [x, end], summed from the far tail
    total = below[-1]
    lower = float(np.interp(p_false * total, below, x))
    upper = float(np.interp(p_false * total, above[::-1], x[::-1]))
    return lower, upper


def sk_scan(vector, nFFT, Sf, fc=0.0, p_false=None, ctx=None):
    """What occupies each bin of one capture, by the spectral kurtosis of its nFFT-point periodograms (WelchPlan.sk; Hann
    window, nperseg = nFFT, no overlap): noise-like - OFDM, the thermal floor - inside sk_limits(M, p_false), steady - a
    carrier - below the lower limit, intermittent - a burst, a radar, a hopping interferer - above the upper one; none of
    it depends on the noise floor.  p_false = 1e-3 per side by default.
    -> (SK fftshifted, frequency axis, steady mask, intermittent mask).
    The limits assume independent segments, that is no overlap - which is why the scan uses none.  Below p_false = 1e-4
    the tails of the fitted null density are extrapolated, not checked.  Needs M = len(vector) // nFFT >= 32 segments and
    nFFT a power of two from 64 to 16384 (ValueError otherwise, before anything runs)."""
    if nFFT not in SK_SIZES:
        raise ValueError('sk_scan needs nFFT a power of two from 64 to 16384, not %r' % (nFFT,))
    p_false = 1e-3 if p_false is None else p_false
    lower, upper = sk_limits(len(vector) // int(nFFT), p_false)
    ctx = ctx or _hip.default_context()
    key = ('sk', nFFT, float(Sf))
    plan = ctx.cached_plan(key, lambda: ctx.welch_plan(nFFT, nperseg=nFFT, noverlap=0, window=windows.get_window('hann', nFFT),
                                                       fs=float(Sf), fftshift=True))
    sk = plan.sk(vector)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf)) + fc
    return sk, axis, sk < lower, sk > upper


def channelized_scan(vector, nchan, nFFT, Sf, fc=0.0, decim=None, taps=8, p_false=None, ctx=None):
    """sk_scan per channel of a wide band: the capture goes through a polyphase channelizer (Context.channelizer: nchan
    channels, hop decim = nchan // 2 by default, a prototype of taps * nchan taps), and the nchan baseband rows - rate
    Sf / decim each - go as they lie on the device into WelchPlan.sk_dev (Hann window, nperseg = nFFT, no overlap): a fine
    PSD and the spectral kurtosis of every channel from one upload and two launches; nothing but the two result arrays
    comes back.  p_false = 1e-3 per side by default.
    -> (channel centres [nchan] in Hz, fftshifted; offsets [nFFT] in Hz from a channel's centre at rate Sf / decim,
    fftshifted; psd [nchan, nFFT]; sk [nchan, nFFT]; steady mask; intermittent mask; M), rows in the order of the centres,
    M the fine segments per channel.
    Needs nFFT a power of two from 64 to 16384 and M = frames // nFFT >= 32 with frames = (len(vector) - taps nchan) //
    decim + 1 (ValueError otherwise, before anything runs); the limits are sk_limits(M, p_false)."""
    nchan, decim, taps, h = _hip.channelizer_args(nchan, decim, taps)
    if nFFT not in SK_SIZES:
        raise ValueError('channelized_scan needs nFFT a power of two from 64 to 16384, not %r' % (nFFT,))
    nFFT = int(nFFT)
    x = _hip._c64(vector)
    L = taps * nchan
    frames = (len(x) - L) // decim + 1 if len(x) >= L else 0
    M = frames // nFFT
    if M < 32:
        raise ValueError('channelized_scan needs at least 32 fine segments per channel: %d samples give %d frames of %d channels, '
                         '%d segments of %d points' % (len(x), frames, nchan, M, nFFT))
    p_false = 1e-3 if p_false is None else p_false
    lower, upper = sk_limits(M, p_false)
    ctx = ctx or _hip.default_context()
    rate = float(Sf) / decim
    chan = ctx.cached_plan(('chan', nchan, decim, taps), lambda: ctx.channelizer(nchan, decim, taps, h))
    plan = ctx.cached_plan(('sk', nFFT, rate), lambda: ctx.welch_plan(nFFT, nperseg=nFFT, noverlap=0, window=windows.get_window('hann', nFFT),
                                                                     fs=rate, fftshift=True))
    bufs = []
    try:
        for nbytes in (8 * len(x), 8 * nchan * frames, 4 * nchan * nFFT, 4 * nchan * nFFT):
            bufs.append(ctx.alloc(nbytes))
        d_x, d_rows, d_sk, d_psd = bufs
        ctx.h2d(d_x, x)
        chan.reset()
        got = chan.push_dev(d_x, len(x), d_rows, frames)
        assert got == frames
        segs = plan.sk_dev(d_rows, frames, nchan, frames, d_sk, d_psd)
        assert segs == M
        sk = ctx.d2h(d_sk, (nchan, nFFT), np.float32)
        psd = ctx.d2h(d_psd, (nchan, nFFT), np.float32)
    finally:
        ctx.sync()
        for b in bufs:
            ctx.free(b)
    sk, psd = np.fft.fftshift(sk, axes=0), np.fft.fftshift(psd, axes=0)
    centres = np.fft.fftshift(chan.channel_freqs(Sf, fc))
    offsets = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / rate))
    return centres, offsets, psd, sk, sk < lower, sk > upper, M


def ofdm_cycle_frequencies(fft_len, cp_len, Sf, harmonics=2):
    """The cycle frequencies of a cyclic-prefix OFDM signal of fft_len useful and cp_len prefix samples per symbol at
    sample rate Sf: +-k Sf / (fft_len + cp_len) in Hz for k = 1 ... harmonics, ordered +1, -1, +2, -2, ...  The prefix
    repeats the symbol's tail, so the signal is correlated with itself at lag +-fft_len with the symbol period."""
    fft_len, cp_len, harmonics = int(fft_len), int(cp_len), int(harmonics)
    if fft_len < 1 or cp_len < 1 or harmonics < 1 or not Sf > 0:
        raise ValueError('ofdm_cycle_frequencies needs fft_len, cp_len, harmonics >= 1 and Sf > 0')
    base = float(Sf) / float(fft_len + cp_len)
    return np.array([sign * k * base for k in range(1, harmonics + 1) for sign in (1.0, -1.0)], np.float64)


def cyclic_scan(vector, nFFT, Sf, cycles_hz, fc=0.0, ctx=None):
    """Is the thing in this band cyclostationary at the given cycle frequencies - a CP-OFDM signal of known symbol period
    (ofdm_cycle_frequencies) - or just noise of unknown level and colour?  The cyclic coherence of one capture
    (WelchPlan.cyclic; Hann window, nperseg = nFFT, no overlap) at each of the A cycle frequencies cycles_hz [Hz].
    -> (profile[A]: the mean over bins of each coherence row, the coherence rows [A, nFFT] fftshifted, frequency axis,
    null level 1 / M).  Stationary noise reads about 1 / M in every entry of the profile, M = len(vector) // nFFT, whatever
    its level; that null mean assumes independent segments, that is no overlap - which is why the scan uses none.
    Row a, bin j compares the spectrum at axis[j] and at axis[j] + cycles_hz[a].  Needs nFFT a power of two from 64 to
    16384, 1 ... 64 cycle frequencies with |cycle| <= Sf / 2 and at least one segment (ValueError otherwise, before
    anything runs)."""
    if nFFT not in SK_SIZES:
        raise ValueError('cyclic_scan needs nFFT a power of two from 64 to 16384, not %r' % (nFFT,))
    if not Sf > 0:
        raise ValueError('cyclic_scan needs a sample rate Sf > 0')
    cycles = np.atleast_1d(np.asarray(cycles_hz, np.float64))
    if cycles.ndim != 1 or not 1 <= len(cycles) <= 64:
        raise ValueError('cyclic_scan needs 1 ... 64 cycle frequencies, not %d' % cycles.size)
    if not np.all(np.isfinite(cycles)) or np.any(np.abs(cycles) > 0.5 * float(Sf)):
        raise ValueError('every cycle frequency must be finite with |cycle| <= Sf / 2')
    M = len(vector) // int(nFFT)
    if M < 1:
        raise ValueError('cyclic_scan needs at least nFFT = %d samples' % nFFT)
    alphas = cycles / float(Sf)
    ctx = ctx or _hip.default_context()
    key = ('cyclic', nFFT, float(Sf), alphas.tobytes())

    def make():
        plan = ctx.welch_plan(nFFT, nperseg=nFFT, noverlap=0, window=windows.get_window('hann', nFFT), fs=float(Sf), fftshift=True)
        plan.set_cycles(alphas)
        return plan

    coh = ctx.cached_plan(key, make).cyclic(vector)[1]
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf)) + fc
    return coh.mean(axis=1, dtype=np.float64), coh, axis, 1.0 / M


def caf_scan(vector, nFFT, Sf, lags, fc=0.0, ctx=None):
    """Which lags of this capture carry a cyclic autocorrelation, with no prior knowledge of the signal: the Welch PSD of the
    lag product x[n + tau] conj(x[n]) (WelchPlan.caf; Hann window, nperseg = nFFT, no overlap, the segment mean taken off,
    density scaling) at each of the L lags [samples].
    -> (alpha axis [Hz] fftshifted, caf rows [L, nFFT] fftshifted, r [L] complex - the mean lag product R(tau) - and the
    segment count M = (len(vector) - max(lags)) // nFFT).  A CP-OFDM signal shows lines at k Sf / (Tu + Tcp) in the row of
    tau = Tu and |r| well above the other lags'; stationary noise shows a flat row at every lag.  The lag product of a
    signal does not move with the tuner, so fc does not enter the alpha axis; it is accepted as the other scans do.
    Needs nFFT a power of two from 64 to 16384, 1 ... 64 integer lags in 0 ... 65535 and at least max(lags) + nFFT samples
    (ValueError otherwise, before anything runs)."""
    if nFFT not in SK_SIZES:
        raise ValueError('caf_scan needs nFFT a power of two from 64 to 16384, not %r' % (nFFT,))
    if not Sf > 0:
        raise ValueError('caf_scan needs a sample rate Sf > 0')
    taus = np.atleast_1d(np.asarray(lags))
    if taus.ndim != 1 or not 1 <= len(taus) <= 64:
        raise ValueError('caf_scan needs 1 ... 64 lags, not %d' % taus.size)
    if not np.issubdtype(taus.dtype, np.integer) or np.any(taus < 0) or np.any(taus > 65535):
        raise ValueError('every lag must be an integer in 0 ... 65535 samples')
    taus = taus.astype(np.intc)
    if len(vector) < int(taus.max()) + int(nFFT):
        raise ValueError('caf_scan needs at least max(lags) + nFFT = %d samples' % (int(taus.max()) + int(nFFT)))
    ctx = ctx or _hip.default_context()
    key = ('caf', nFFT, float(Sf), taus.tobytes())

    def make():
        plan = ctx.welch_plan(nFFT, nperseg=nFFT, noverlap=0, window=windows.get_window('hann', nFFT), fs=float(Sf), fftshift=True)
        plan.set_lags(taus)
        return plan

    plan = ctx.cached_plan(key, make)
    caf, r = plan.caf(vector, return_r=True)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf))
    return axis, caf, r, int(plan.last_nseg)


def multiantenna_null_mean(nchan, M):
    """E[1 - det G] of nchan channels of independent noise over M independent segments: 1 - prod_{k=1}^{C-1} (M - k) / M
    (the determinant of a complex Wishart sample coherence matrix; 1 / M at two channels).  1 where M < nchan."""
    prod = 1.0
    for k in range(1, int(nchan)):
        prod *= max(M - k, 0) / float(M)
    return 1.0 - prod


def multiantenna_scan(vectors, nFFT, Sf, fc=0.0, ctx=None):
    """Do these C coherent channels (antennas of one receiver, 2 <= C <= 8) share a signal, with no knowledge of any
    channel's gain or noise floor?  The spectral matrix of one capture (WelchPlan.matrix; Hann window, nperseg = nFFT, no
    overlap, density scaling) and its generalized coherence 1 - det G per bin, the GLRT for a common signal in uncalibrated
    receivers.  vectors: (C, n) complex array.
    -> (frequency axis [Hz] fftshifted, psd [C, nFFT]: each channel's Welch PSD fftshifted, gcoh [nFFT] fftshifted in [0, 1],
    null_mean).  Independent noise reads about null_mean = 1 - prod_{k=1}^{C-1} (M - k) / M in every bin, M = n // nFFT,
    whatever its level per channel; that expectation assumes independent segments, that is no overlap - which is why the scan
    uses none.  A bin where the channels share a signal reads near 1.  With M < C every bin reads 1: the matrix is singular.
    Needs nFFT a power of two from 64 to 16384, 2 ... 8 channels and at least one segment (ValueError otherwise, before
    anything runs)."""
    if nFFT not in SK_SIZES:
        raise ValueError('multiantenna_scan needs nFFT a power of two from 64 to 16384, not %r' % (nFFT,))
    if not Sf > 0:
        raise ValueError('multiantenna_scan needs a sample rate Sf > 0')
    x = np.asarray(vectors)
    if x.ndim != 2 or not 2 <= x.shape[0] <= 8:
        raise ValueError('multiantenna_scan needs a (C, n) array of 2 ... 8 channels, not shape %r' % (x.shape,))
    M = x.shape[1] // int(nFFT)
    if M < 1:
        raise ValueError('multiantenna_scan needs at least nFFT = %d samples per channel' % nFFT)
    ctx = ctx or _hip.default_context()
    key = ('matrix', nFFT, float(Sf))

    def make():
        return ctx.welch_plan(nFFT, nperseg=nFFT, noverlap=0, window=windows.get_window('hann', nFFT), fs=float(Sf), fftshift=True)

    S, gcoh = ctx.cached_plan(key, make).matrix(x)
    psd = np.ascontiguousarray(S[np.arange(x.shape[0]), np.arange(x.shape[0])].real)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf)) + fc
    return axis, psd, gcoh, multiantenna_null_mean(x.shape[0], M)


def eigenvalue_stats(eig, M):
    """The blind multi-antenna detection statistics of the eigenvalues of a spectral (or coherence) matrix of C channels
    averaged over M segments, in float64.  eig: [C, m], the rows descending (WelchPlan.matrix_eig).  -> dict of rows [m]:
    'mme'   l_1 / l_C, the maximum-minimum eigenvalue ratio; inf where l_C == 0 < l_1, NaN where l_1 is 0 or NaN.
    'agm'   the arithmetic over the geometric mean of all C eigenvalues (the sphericity test); inf where the geometric mean
            is 0 (an eigenvalue is 0), NaN where an eigenvalue is NaN.
    'nsrc'  int: the Wax-Kailath MDL source count, the k in 0 ... C - 1 that minimises
            MDL(k) = -M (C - k) ln(g_k / a_k) + k (2 C - k) ln(M) / 2, a_k and g_k the arithmetic and the geometric mean of
            l_{k+1} ... l_C (the lowest k on ties); -1 where M < C or an eigenvalue is <= 0 or not finite."""
    l = np.asarray(eig, np.float64)
    if l.ndim != 2:
        raise ValueError('eigenvalue_stats takes the eigenvalue rows [C, m]')
    C, m = l.shape
    M = int(M)
    with np.errstate(all='ignore'):
        top, low = l[0], l[C - 1]
        mme = np.where(top > 0, np.where(low == 0, np.inf, top / low), np.nan)
        mme = np.where(np.isnan(l).any(axis=0), np.nan, mme)
        am = l.mean(axis=0)
        gm = np.exp(np.log(l).mean(axis=0))
        gm = np.where((l == 0).any(axis=0), 0.0, gm)
        agm = np.where(gm == 0, np.inf, am / gm)
        agm = np.where(np.isnan(l).any(axis=0), np.nan, agm)
        usable = np.all(np.isfinite(l) & (l > 0), axis=0) & (M >= C)
        nsrc = np.full(m, -1, np.int64)
        if usable.any():
            lu = l[:, usable]
            mdl = np.empty((C, lu.shape[1]))
            for k in range(C):
                tail = lu[k:]
                a_k, lng_k = tail.mean(axis=0), np.log(tail).mean(axis=0)
                mdl[k] = -M * (C - k) * (lng_k - np.log(a_k)) + 0.5 * k * (2 * C - k) * np.log(M)
            nsrc[usable] = np.argmin(mdl, axis=0)
    return {'mme': mme, 'agm': agm, 'nsrc': nsrc}


def eigen_scan(vectors, nFFT, Sf, fc=0.0, of='S', ctx=None):
    """Eigenvalues and the principal eigenvector per bin of the spectral matrix (of='S') or of the coherence matrix (of='G')
    of C coherent channels, 2 <= C <= 8, on the plan multiantenna_scan makes (WelchPlan.matrix_eig; Hann window,
    nperseg = nFFT, no overlap, density scaling), and the detection statistics that follow from the eigenvalues.
    vectors: (C, n) complex array.
    -> (frequency axis [Hz] fftshifted, eig [C, nFFT] float32 descending rows, fftshifted, vec [C, nFFT] complex64: the unit
    eigenvector of the largest eigenvalue, the array response of the strongest emitter in the bin, stats: eigenvalue_stats(eig,
    M) with M = n // nFFT).  Needs nFFT a power of two from 64 to 16384, 2 ... 8 channels and at least one segment (ValueError
    otherwise, before anything runs)."""
    if nFFT not in SK_SIZES:
        raise ValueError('eigen_scan needs nFFT a power of two from 64 to 16384, not %r' % (nFFT,))
    if not Sf > 0:
        raise ValueError('eigen_scan needs a sample rate Sf > 0')
    x = np.asarray(vectors)
    if x.ndim != 2 or not 2 <= x.shape[0] <= 8:
        raise ValueError('eigen_scan needs a (C, n) array of 2 ... 8 channels, not shape %r' % (x.shape,))
    M = x.shape[1] // int(nFFT)
    if M < 1:
        raise ValueError('eigen_scan needs at least nFFT = %d samples per channel' % nFFT)
    ctx = ctx or _hip.default_context()
    key = ('matrix', nFFT, float(Sf))      # multiantenna_scan's plan

    def make():
        return ctx.welch_plan(nFFT, nperseg=nFFT, noverlap=0, window=windows.get_window('hann', nFFT), fs=float(Sf), fftshift=True)

    eig, vec = ctx.cached_plan(key, make).matrix_eig(x, of=of)
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf)) + fc
    return axis, eig, vec, eigenvalue_stats(eig, M)


def ula_delays(nchan, angles_deg, spacing_wavelengths, fc_cycles):
    """The steering table of a uniform line array for WelchPlan.set_steering / doa_scan: element c of nchan sits c spacings
    along the line, a spacing is spacing_wavelengths wavelengths of the carrier, the carrier is fc_cycles cycles per sample,
    and a plane wave from angle theta off broadside reaches element c later by c spacing sin(theta) carrier periods.
    -> float64 [len(angles_deg), nchan] delays in samples, tau[d, c] = c spacing_wavelengths sin(theta_d) / fc_cycles."""
    if not _is_int(nchan) or not 2 <= nchan <= 8:
        raise ValueError('ula_delays needs 2 ... 8 channels, not %r' % (nchan,))
    if not (np.isfinite(fc_cycles) and fc_cycles > 0):
        raise ValueError('ula_delays needs a carrier fc_cycles > 0 in cycles per sample')
    if not (np.isfinite(spacing_wavelengths) and spacing_wavelengths > 0):
        raise ValueError('ula_delays needs a spacing > 0 in wavelengths')
    theta = np.atleast_1d(np.asarray(angles_deg, np.float64))
    if theta.ndim != 1 or theta.size < 1 or not np.all(np.abs(theta) <= 90.0):
        raise ValueError('ula_delays needs a list of angles from -90 to 90 degrees')
    return np.arange(int(nchan))[None, :] * (float(spacing_wavelengths) * np.sin(np.deg2rad(theta)) / float(fc_cycles))[:, None]


def doa_band_combine(rows, band=None):
    """The band-combined spectrum of doa_scan, in float64, over the bins band = (lo, hi) of the rows' last axis (hi excluded;
    None: every bin): rows: dict method -> [D, m].  -> dict method -> [D]: the mean over the band for 'bartlett',
    1 / mean(1 / P) - the bins' null spectra added - for 'capon' and 'music'."""
    out = {}
    for name, r in rows.items():
        r = np.asarray(r, np.float64)
        r = r if band is None else r[:, band[0]:band[1]]
        with np.errstate(all='ignore'):
            out[name] = r.mean(axis=1) if name == 'bartlett' else 1.0 / (1.0 / r).mean(axis=1)
    return out


def doa_scan(vectors, nFFT, Sf, delays, fc, nsrc, loading=1e-2, band=None, ctx=None):
    """Where is the emitter?  The Bartlett, Capon (MVDR) and MUSIC spectra per bin and per direction of the spectral matrix
    of C coherent channels, 2 <= C <= 8, on the plan multiantenna_scan makes (WelchPlan.matrix_doa; Hann window,
    nperseg = nFFT, no overlap, density scaling), and their combination over a band.  vectors: (C, n) complex array.
    delays: [D, C] in samples, channel c of direction d carries s(t - delays[d, c]) (ula_delays gives a uniform line array's),
    1 <= D <= 1024.  fc: the carrier in cycles per sample.  nsrc: the number of sources MUSIC takes, 1 ... C - 1.  loading:
    Capon's diagonal loading as a fraction of the mean eigenvalue.  band: (lo, hi) bins of the fftshifted axis, hi excluded;
    None for all of them.
    -> (frequency axis [Hz] fftshifted around fc Sf, bartlett, capon, music: float32 [D, nFFT] each, fftshifted, combined:
    doa_band_combine of the three over band, float64 [D] each).  Needs nFFT a power of two from 64 to 16384, 2 ... 8 channels
    and at least one segment (ValueError otherwise, before anything runs)."""
    if nFFT not in SK_SIZES:
        raise ValueError('doa_scan needs nFFT a power of two from 64 to 16384, not %r' % (nFFT,))
    if not Sf > 0:
        raise ValueError('doa_scan needs a sample rate Sf > 0')
    x = np.asarray(vectors)
    if x.ndim != 2 or not 2 <= x.shape[0] <= 8:
        raise ValueError('doa_scan needs a (C, n) array of 2 ... 8 channels, not shape %r' % (x.shape,))
    if x.shape[1] // int(nFFT) < 1:
        raise ValueError('doa_scan needs at least nFFT = %d samples per channel' % nFFT)
    tab = np.asarray(delays, np.float64)
    if tab.ndim != 2 or tab.shape[1] != x.shape[0] or not 1 <= tab.shape[0] <= 1024 or not np.all(np.isfinite(tab)):
        raise ValueError('doa_scan needs finite delays of shape (D, %d), 1 <= D <= 1024, not shape %r' % (x.shape[0], tab.shape))
    if not np.isfinite(fc):
        raise ValueError('doa_scan needs a finite carrier fc in cycles per sample')
    if not _is_int(nsrc) or not 1 <= nsrc <= x.shape[0] - 1:
        raise ValueError('doa_scan needs nsrc in 1 ... %d, not %r' % (x.shape[0] - 1, nsrc))
    if not (np.isfinite(loading) and loading >= 0):
        raise ValueError('doa_scan needs a finite loading >= 0')
    if band is not None and not (len(band) == 2 and _is_int(band[0]) and _is_int(band[1]) and 0 <= band[0] < band[1] <= nFFT):
        raise ValueError('doa_scan needs band = (lo, hi) with 0 <= lo < hi <= nFFT = %d' % nFFT)
    ctx = ctx or _hip.default_context()
    key = ('matrix', nFFT, float(Sf))      # multiantenna_scan's plan

    def make():
        return ctx.welch_plan(nFFT, nperseg=nFFT, noverlap=0, window=windows.get_window('hann', nFFT), fs=float(Sf), fftshift=True)

    plan = ctx.cached_plan(key, make)
    plan.set_steering(tab, fc)
    rows = plan.matrix_doa(x, of='S', nsrc=int(nsrc), loading=float(loading))
    axis = np.fft.fftshift(np.fft.fftfreq(nFFT, 1.0 / Sf)) + fc * Sf
    return axis, rows['bartlett'], rows['capon'], rows['music'], doa_band_combine(rows, band)


GCC_WEIGHTINGS = ('plain', 'phat', 'scot')


def tdoa_scan(vectors, nFFT, Sf, weighting='phat', band=None, upsample=1, maxlag=None, ctx=None):
    """What are the delays between these C coherent channels, 2 <= C <= 8?  The generalized cross-correlation of every pair
    (WelchPlan.matrix_gcc: 'phat', 'scot' or 'plain') on the plan multiantenna_scan makes (Hann window, nperseg = nFFT, no
    overlap) and the delay at its peak - what a steering table has to be calibrated with, and the TDOA of separated
    receivers.  vectors: (C, n) complex array.  band: (f_lo, f_hi) in Hz of the baseband axis, -Sf / 2 <= f_lo <= f_hi
    < Sf / 2, both inclusive: the bins ceil(f_lo nFFT / Sf) ... floor(f_hi nFFT / Sf), of which there must be one; None for
    every bin.  upsample U: 1, 2, 4 or 8 with U nFFT <= 16384; the lags count 1 / (U Sf) seconds.  maxlag: the largest lag
    in seconds, floor(maxlag U Sf) lags to either side, at most U nFFT / 2 - 1; None for that most.
    -> (delays float64 [C, C] in seconds, delays[a][b] = tau_b - tau_a where channel c carries s(t - tau_c), antisymmetric;
    peaks float32 [C, C], |R_ab| at the peak; phases float32 [C, C], arg R_ab at the peak in radians; the lag axis in
    seconds, float64 [2 L + 1]; rows complex64 [C (C - 1) / 2, 2 L + 1], R_ab over the axis, pairs (0,1), (0,2), ...,
    (C-2,C-1)).  channel_delays turns the pair matrix into per-channel delays.  Needs nFFT a power of two from 64 to 16384,
    2 ... 8 channels and at least one segment (ValueError otherwise, before anything runs)."""
    if nFFT not in SK_SIZES:
        raise ValueError('tdoa_scan needs nFFT a power of two from 64 to 16384, not %r' % (nFFT,))
    if not Sf > 0:
        raise ValueError('tdoa_scan needs a sample rate Sf > 0')
    x = np.asarray(vectors)
    if x.ndim != 2 or not 2 <= x.shape[0] <= 8:
        raise ValueError('tdoa_scan needs a (C, n) array of 2 ... 8 channels, not shape %r' % (x.shape,))
    if x.shape[1] // int(nFFT) < 1:
        raise ValueError('tdoa_scan needs at least nFFT = %d samples per channel' % nFFT)
    if weighting not in GCC_WEIGHTINGS:
        raise ValueError("tdoa_scan needs weighting 'plain', 'phat' or 'scot', not %r" % (weighting,))
    if not _is_int(upsample) or upsample not in (1, 2, 4, 8) or upsample * nFFT > _hip.GCC_POINTS_MAX:
        raise ValueError('tdoa_scan needs upsample 1, 2, 4 or 8 with upsample * nFFT <= %d, not %r' % (_hip.GCC_POINTS_MAX, upsample))
    half, ni = nFFT // 2, int(upsample) * nFFT
    bins = None
    if band is not None:
        if not (len(band) == 2 and np.all(np.isfinite(band)) and -0.5 * Sf <= band[0] <= band[1] < 0.5 * Sf):
            raise ValueError('tdoa_scan needs band = (f_lo, f_hi) in Hz with -Sf / 2 <= f_lo <= f_hi < Sf / 2')
        bins = (max(int(math.ceil(band[0] * nFFT / float(Sf))), -half), min(int(math.floor(band[1] * nFFT / float(Sf))), half - 1))
        if bins[0] > bins[1]:
            raise ValueError('tdoa_scan: the band %r Hz holds no bin of width %g Hz' % (tuple(band), Sf / float(nFFT)))
    lags = ni // 2 - 1
    if maxlag is not None:
        if not (np.isfinite(maxlag) and maxlag >= 0):
            raise ValueError('tdoa_scan needs maxlag >= 0 in seconds')
        lags = int(math.floor(maxlag * upsample * float(Sf)))
        if lags > ni // 2 - 1:
            raise ValueError('tdoa_scan: maxlag is %d lags of 1 / (upsample Sf); upsample * nFFT / 2 - 1 = %d at most' % (lags, ni // 2 - 1))
    ctx = ctx or _hip.default_context()
    key = ('matrix', nFFT, float(Sf))      # multiantenna_scan's plan

    def make():
        return ctx.welch_plan(nFFT, nperseg=nFFT, noverlap=0, window=windows.get_window('hann', nFFT), fs=float(Sf), fftshift=True)

    delays, peaks, phases, rows = ctx.cached_plan(key, make).matrix_gcc(x, weighting=weighting, band=bins, upsample=int(upsample), maxlag=lags)
    axis = np.arange(-lags, lags + 1) / (float(upsample) * float(Sf))
    return delays.astype(np.float64) / float(Sf), peaks, phases, axis, rows


def channel_delays(pair_delays, weights=None):
    """Per-channel delays from the antisymmetric pair matrix of tdoa_scan / WelchPlan.matrix_gcc, pair_delays[a][b] =
    tau_b - tau_a: the tau with tau_0 = 0 that minimises sum_{a < b} weights[a][b] (tau_b - tau_a - pair_delays[a][b])^2, in
    float64.  weights: [C, C] >= 0, read above the diagonal (the pairs' peaks, say: a pair without a common signal counts
    less); None for equal weights.  Every channel must hang on channel 0 through pairs of weight > 0 (ValueError otherwise).
    -> float64 [C], in the unit of pair_delays.  Cable and front-end delays measured this way, added to a geometry's
    (ula_delays), are the rows WelchPlan.set_steering takes."""
    d = np.asarray(pair_delays, np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1] or d.shape[0] < 2 or not np.all(np.isfinite(d)):
        raise ValueError('channel_delays needs a finite (C, C) matrix of pair delays, C >= 2')
    nchan = d.shape[0]
    w = np.ones((nchan, nchan)) if weights is None else np.asarray(weights, np.float64)
    if w.shape != d.shape or not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError('channel_delays needs finite weights >= 0 of the shape of pair_delays')
    pairs = [(a, b) for a in range(nchan) for b in range(a + 1, nchan) if w[a, b] > 0]
    A = np.zeros((len(pairs), nchan))
    for r, (a, b) in enumerate(pairs):
        A[r, a], A[r, b] = -1.0, 1.0
    root = np.sqrt(np.array([w[a, b] for a, b in pairs]))
    A = A[:, 1:] * root[:, None]      # tau_0 = 0
    if not pairs or np.linalg.matrix_rank(A) < nchan - 1:
        raise ValueError('channel_delays: a channel is not tied to channel 0 by pairs of weight > 0')
    rhs = np.array([d[a, b] for a, b in pairs]) * root
    return np.concatenate(([0.0], np.linalg.lstsq(A, rhs, rcond=None)[0]))


def ofdm_blind_hypotheses(fft_lens, cp_fractions, nFFT):
    """The (Tu, cp = Tu // f, bin) triples ofdm_blind_parameters tests, bin = round(nFFT / (Tu + cp)): where the symbol
    rate of the hypothesis falls in a caf row of nFFT points.  ValueError when two of them fall on the same bin or one on a
    bin below 4 - nFFT is too small to tell these candidates apart, or from the row's DC."""
    hyp = []
    for tu in fft_lens:
        for f in cp_fractions:
            tu, f = int(tu), int(f)
            if tu < 1 or f < 1 or tu // f < 1:
                raise ValueError('ofdm_blind_parameters needs fft_lens >= 1 and cp_fractions that leave a prefix of a sample at least')
            cp = tu // f
            hyp.append((tu, cp, int(round(float(nFFT) / float(tu + cp)))))
    bins = [q for _, _, q in hyp]
    if not hyp or len(set(bins)) != len(bins) or min(bins) < 4:
        raise ValueError('nFFT = %d is too small for these candidates: their symbol rates fall on bins %s, which must differ and '
                         'be 4 at least' % (nFFT, bins))
    return hyp


def ofdm_blind_threshold(nseg, nhyp, p_false=1e-3):
    """What the statistic of ofdm_blind_decision exceeds with probability p_false over all nhyp hypotheses on a flat floor:
    the mean of two bins of an M-segment average is chi-square with 4 M degrees of freedom over 4 M, the row's median that of
    2 M over 2 M; Bonferroni over the hypotheses."""
    M = float(nseg)
    return (chi2_quantile(1.0 - float(p_false) / float(nhyp), 4.0 * M) / (4.0 * M)) / (chi2_quantile(0.5, 2.0 * M) / (2.0 * M))


def ofdm_blind_decision(rows, r, nseg, Sf, fft_lens, cp_fractions=(4, 8, 16, 32), p_false=1e-3):
    """The decision of ofdm_blind_parameters on caf rows in natural bin order: rows [1 + len(fft_lens), nFFT] and r for the
    lags (0,) + fft_lens, nseg the segment count behind them.  -> the dict ofdm_blind_parameters returns."""
    rows = np.asarray(rows, np.float64)
    nFFT = rows.shape[-1]
    fft_lens = [int(t) for t in fft_lens]
    if rows.shape[0] != 1 + len(fft_lens) or len(r) != rows.shape[0]:
        raise ValueError('rows and r must hold lag 0 and one lag per entry of fft_lens')
    hyp = ofdm_blind_hypotheses(fft_lens, cp_fractions, nFFT)
    floors = {tu: float(np.median(rows[1 + i, 1:])) for i, tu in enumerate(fft_lens)}
    best = None
    for tu, cp, q in hyp:
        row = rows[1 + fft_lens.index(tu)]
        stat = float(row[q] + row[nFFT - q]) / (2.0 * floors[tu]) if floors[tu] > 0.0 else 0.0
        if best is None or stat > best[0]:
            best = (stat, tu, cp)
    stat, tu, cp = best
    threshold = float(ofdm_blind_threshold(nseg, len(hyp), p_false))
    r0 = float(np.real(r[0]))
    rho = float(abs(r[1 + fft_lens.index(tu)]) / r0) if r0 > 0.0 else 0.0
    return {'detected': bool(stat >= threshold), 'fft_len': tu, 'cp_len': cp, 'rho': rho, 'stat': stat, 'threshold': threshold,
            'nseg': int(nseg), 'cycles_hz': ofdm_cycle_frequencies(tu, cp, Sf)}


def ofdm_blind_parameters(vector, Sf, fft_lens=(64, 128, 256, 512), cp_fractions=(4, 8, 16, 32), nFFT=4096, p_false=1e-3, ctx=None):
    """The useful length and the prefix length of an unknown CP-OFDM signal in this capture, by its cyclic autocorrelation:
    one WelchPlan.caf call (caf_scan) with the lags (0,) + fft_lens.  For every hypothesis (Tu, cp = Tu // f) the statistic
    is (row_Tu[q] + row_Tu[nFFT - q]) / (2 median(row_Tu[1:])) at q = round(nFFT / (Tu + cp)) - the line at the symbol rate
    over the row's floor; the largest wins, and `detected` says that it reaches ofdm_blind_threshold (p_false over all
    hypotheses).  -> dict: detected, fft_len, cp_len, rho = |r_Tu| / r_0 (the correlation coefficient at lag Tu, about
    cp / (Tu + cp) times the signal's share of the power), stat, threshold, nseg, cycles_hz =
    ofdm_cycle_frequencies(fft_len, cp_len, Sf) - what cyclic_scan takes.
    Assumes that the floor of the lag product is flat over the row, which holds for receiver noise that is white over the
    capture band.  ValueError when two hypotheses fall on the same bin or one on a bin below 4: nFFT is too small for
    these candidates (fft_lens up to 512 with a prefix of 1/32 need nFFT = 8192)."""
    fft_lens = tuple(int(t) for t in fft_lens)
    ofdm_blind_hypotheses(fft_lens, cp_fractions, nFFT)      # the refusals, before anything runs
    _, caf, r, nseg = caf_scan(vector, nFFT, Sf, (0,) + fft_lens, ctx=ctx)
    return ofdm_blind_decision(np.fft.ifftshift(caf, axes=-1), r, nseg, Sf, fft_lens, cp_fractions, p_false)


def ofdm_sync_scan(vector, fft_len, cp_len, Sf, rho=1.0, ctx=None):
    """Where a symbol of a CP-OFDM signal of known lengths starts and how far its carrier is off, by the cyclic-prefix
    correlator folded over all symbols of the capture (Context.cp_sync, one hypothesis): Lambda[t] = |gamma[t]| - rho phi[t]
    over t < fft_len + cp_len, `rho` the weight of the energy term (1: the likelihood at high SNR, 0: the correlation alone).
    -> dict: timing = theta, the samples from the capture's first to the first sample of a cyclic prefix modulo
    fft_len + cp_len; eps, the carrier offset in subcarrier spacings (|eps| <= 1/2: the fractional part only);
    cfo_hz = eps * Sf / fft_len; rho = rho_hat = |gamma[theta]| / phi[theta], about SNR / (SNR + 1);
    snr_db = 10 log10(rho / (1 - rho)), inf at rho >= 1 and -inf at rho <= 0; nsym, the symbols folded; gamma complex64 and phi
    float32 [fft_len + cp_len].  A capture with a NaN or inf sample gives NaN timing, eps, rho and snr_db."""
    ctx = ctx or _hip.default_context()
    gamma, phi, est, nsym = ctx.cp_sync(vector, [(int(fft_len), int(cp_len))], rho=rho)
    theta, eps, rho_hat = float(est[0, 0]), float(est[0, 1]), float(est[0, 2])
    if not rho_hat == rho_hat:
        snr_db = float('nan')
    elif rho_hat >= 1.0:
        snr_db = float('inf')
    elif rho_hat <= 0.0:
        snr_db = float('-inf')
    else:
        snr_db = 10.0 * math.log10(rho_hat / (1.0 - rho_hat))
    return {'timing': int(theta) if theta == theta else theta, 'eps': eps, 'cfo_hz': eps * float(Sf) / float(fft_len), 'rho': rho_hat,
            'snr_db': snr_db, 'nsym': int(nsym[0]), 'gamma': gamma[0], 'phi': phi[0]}


def ofdm_blind_sync(vector, Sf, rho=1.0, ctx=None, **kw):
    """ofdm_blind_parameters(vector, Sf, **kw), and on a detected signal ofdm_sync_scan at the lengths it found.  -> the two
    dicts merged; both name a `rho`, so the correlation coefficient at lag Tu of ofdm_blind_parameters is `caf_rho` here and
    `rho` the synchroniser's rho_hat.  Not detected: the dict of ofdm_blind_parameters as it is."""
    found = ofdm_blind_parameters(vector, Sf, ctx=ctx, **kw)
    if not found['detected']:
        return found
    out = dict(found, caf_rho=found['rho'])
    out.update(ofdm_sync_scan(vector, found['fft_len'], found['cp_len'], Sf, rho=rho, ctx=ctx))
    return out


class SpectrumScan(object):
    """The legacy sensor's scan (reference: ofdm_cr_tools.py:471-537; its matplotlib branch is not carried over), split
    where the GPU works: the constructor enqueues the PSD of the chosen method ('welch': flat-top Welch, 'fft': one
    flat-top periodogram, 'mtm': the multitaper estimate with NW 4 and 7 Slepian tapers) through ``oth_welch_exec_async`` and returns at once - the sample buffer may be reused;
    ``poll(noise_estimate)`` returns None while the launch is running, ``wait(noise_estimate)`` blocks.  Both finish with
    the channel sums on the device, the noise estimate ``ne <- (1 - a) ne + a min(p)``, the threshold ``ne * thr_leveler``
    and the channel frequencies whose power exceeds it: -> (threshold, channel powers, noise estimate, occupied [Hz])."""
    _ENQUEUE = {'welch': _enqueue_welch, 'fft': _enqueue_fft, 'mtm': _enqueue_mtm}

    def __init__(self, vct_sample, fc, channel_rate, srch_bw, n_fft, samp_rate, method, thr_leveler, alpha_avg, ctx=None):
        try:
            enqueue = self._ENQUEUE[method]
        except KeyError:
            raise ValueError("method must be 'welch', 'fft' or 'mtm'")
        self.ctx = ctx or _hip.default_context()
        self.nfft = n_fft or int(2 ** math.ceil(math.log(len(vct_sample), 2)))
        self.samp_rate, self.thr_leveler, self.alpha_avg = samp_rate, thr_leveler, alpha_avg
        self.resolution = float(samp_rate) / float(self.nfft)
        half = _py2div(samp_rate, 2)
        self.bb_freqs = frange(_py2div(-samp_rate, 2), half, channel_rate)
        self.srch_bins = srch_bw / self.resolution
        self.channel_hz = frange(fc - half, fc + half, channel_rate)
        self._plan, self._ticket, self._post = enqueue(vct_sample, self.nfft, samp_rate, self.ctx)
        self._result = None

    def _finish(self, psd, noise_estimate):
        if self._post is not None:
            psd = self._post(psd)
        power = _plain_channel_sums(psd, self.resolution, self.samp_rate, self.bb_freqs, self.srch_bins, self.ctx)
        noise_estimate = (1 - self.alpha_avg) * noise_estimate + self.alpha_avg * np.amin(power)
        threshold = noise_estimate * self.thr_leveler
        occupied = [self.channel_hz[i] for i in np.flatnonzero(np.asarray(power) > threshold)]
        self._result = (threshold, power, noise_estimate, occupied)
        return self._result

    def poll(self, noise_estimate):
        if self._result is None:
            psd = self._plan.poll(self._ticket)
            if psd is None:
                return None
            self._finish(psd, noise_estimate)
        return self._result

    def wait(self, noise_estimate):
        if self._result is None:
            self._finish(self._plan.wait(self._ticket), noise_estimate)
        return self._result


def fast_spectrum_scan(vct_sample, fc, channel_rate, srch_bw, n_fft, samp_rate, method, thr_leveler,
                       noise_estimate, alpha_avg, show_plot=False, ctx=None):
    """ofdm_cr_tools.py:471-537 with the reference's arguments and return value: SpectrumScan, waited for."""
    return SpectrumScan(vct_sample, fc, channel_rate, srch_bw, n_fft, samp_rate, method, thr_leveler, alpha_avg,
                        ctx).wait(noise_estimate)


# the reference keeps its file logger next to the numeric helpers (ofdm_cr_tools.py:1850-2107): same import path here
from .sensing_log import logger  # noqa: E402,F401
