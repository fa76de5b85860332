// C ABI, host side: Welch and CSD plans - the window-spectrum tables, the averaging launch (run_average) and the
// median average, the exec / async / poll / wait forms with their pinned output ring, the streaming form
// (accumulate / finalize / reset), the partial / scale forms and the cross spectrum.
#include "abi_state.h"

#include <sched.h>
#include <time.h>

namespace {
// The transform of the n-point window (host_fft_pow2) into re / im -> true when it is negligible outside the bins
// [0, band) and [n - band, n) that a frequency-domain detrend corrects: |W[k]|^2 <= 1e-10 sum(w^2) (see below).
// (band_neg: the bins [n - band_neg, n) instead, for a correction that reaches further down than up)
bool window_spectrum(const std::vector<float> &w, int n, int band, std::vector<double> &re, std::vector<double> &im, int band_neg = 0) {
    if (!band_neg) band_neg = band;
    re.assign(n, 0.0);
    im.assign(n, 0.0);
    double s2 = 0.0;
    for (int i = 0; i < n; ++i) {
        re[i] = (double)w[i];
        s2 += (double)w[i] * (double)w[i];
    }
    host_fft_pow2(re, im);
    for (int k = band; k < n - band_neg; ++k)
        if (re[k] * re[k] + im[k] * im[k] > 1e-10 * s2) return false;
    return true;
}

// Window spectrum table for welch4096ws (WelchArgs.fd).  FFT((x - m) w) = FFT(x w) - m FFT(w): the kernel
// corrects only bins [0, 256) and [3840, 4096), so the table exists only when FFT(w) is negligible elsewhere:
// |W[k]|^2 <= 1e-10 sum(w^2) there bounds the uncorrected term by 1e-10 |m|^2 / sigma^2 of a white-noise
// bin's level.  True for boxcar and the periodic cosine-sum windows (hann, blackman-harris, flattop, ...).
bool window_spectrum_table(const std::vector<float> &w, std::vector<float> &fd) {
    std::vector<double> re, im;
    if (!window_spectrum(w, 4096, 256, re, im)) return false;
    fd.resize(4 * 256);
    for (int t = 0; t < 256; ++t) {
        const int k = (t >> 4) + 16 * (t & 15);
        fd[4 * t] = (float)re[k];
        fd[4 * t + 1] = (float)im[k];
        fd[4 * t + 2] = (float)re[k + 3840];
        fd[4 * t + 3] = (float)im[k + 3840];
    }
    return true;
}

// The table of welch4096ws's complementary-window build (WelchArgs.fd_sym).  That build runs its three passes on signed digits
// around the time origin n' = n - 136: register mu of consumer thread t = 16 k0 + k1 holds
//     (-1)^(lambda + mu) e^(+2 pi i 136 k / 4096) X[k],   k = kappa + 16 lambda + 256 mu,  kappa = sym16(k0), lambda = sym16(k1),
// so the registers mu = 0 are exactly the bins [-136, 120) and each thread corrects that one bin with FFT(w)[k] carrying the
// same phase and sign, formed here in double.  The table exists when FFT(w) is negligible outside those bins, by the
// criterion of window_spectrum_table (every periodic cosine-sum window: Hann reaches +-1, flattop +-4).
bool window_spectrum_table_sym(const std::vector<float> &w, std::vector<float2> &fd) {
    std::vector<double> re, im;
    if (!window_spectrum(w, 4096, 120, re, im, kSymShift)) return false;
    fd.resize(256);
    for (int t = 0; t < 256; ++t) {
        const int k0 = t >> 4, k1 = t & 15;
        const int lambda = k1 < 8 ? k1 : k1 - 16;
        const int k = (k0 < 8 ? k0 : k0 - 16) + 16 * lambda;
        const double a = 2.0 * M_PI * (double)((kSymShift * k) % 4096) / 4096.0, sg = (lambda & 1) ? -1.0 : 1.0;
        const double fr = re[(k + 4096) & 4095], fi = im[(k + 4096) & 4095];
        fd[t] = make_float2((float)(sg * (fr * std::cos(a) - fi * std::sin(a))), (float)(sg * (fr * std::sin(a) + fi * std::cos(a))));
    }
    return true;
}

// The same table for the role-split 1024 / 2048 kernel (segfft.hip, segws_kernel<R, 2>): consumer thread
// t = R k0 + j corrects, for k1 = j + R m (m < 16 / R), the bins k0 + 16 k1 (k2 = 0) and k0 + 16 k1 + 256 (R - 1).
bool window_spectrum_table_seg(const std::vector<float> &w, int n, std::vector<float> &fd) {
    const int R = n / 256, Q = 16 / R;
    std::vector<double> re, im;
    if (!window_spectrum(w, n, 256, re, im)) return false;
    fd.assign((size_t)4 * (n / 16) * Q, 0.f);
    for (int t = 0; t < n / 16; ++t) {
        const int k0 = t / R, j = t % R;
        for (int m = 0; m < Q; ++m) {
            const int lo = k0 + 16 * (j + R * m), hi = lo + 256 * (R - 1);
            float *o = &fd[4 * ((size_t)Q * t + m)];
            o[0] = (float)re[lo];
            o[1] = (float)im[lo];
            o[2] = (float)re[hi];
            o[3] = (float)im[hi];
        }
    }
    return true;
}

// The same table for welch16k.hip (N = 4096 F, F = 2 or 4): thread tid = 256 k' + 16 k0 + k1 holds, after pass 3, the bins
// k' + F (k0 + 16 k1 + 256 k2); it corrects k2 = 0 and k2 = 15, i.e. the table exists when the window's spectrum is
// confined to [0, 256 F) U [N - 256 F, N).
bool window_spectrum_table_16k(const std::vector<float> &w, int n, std::vector<float> &fd) {
    const int F = n / 4096;
    std::vector<double> re, im;
    if (!window_spectrum(w, n, 256 * F, re, im)) return false;
    fd.assign((size_t)4 * 256 * F, 0.f);
    for (int tid = 0; tid < 256 * F; ++tid) {
        const int kp = tid >> 8, k0 = (tid >> 4) & 15, k1 = tid & 15;
        const int lo = kp + F * (k0 + 16 * k1), hi = kp + F * (k0 + 16 * k1 + 3840);
        fd[4 * tid] = (float)re[lo];
        fd[4 * tid + 1] = (float)im[lo];
        fd[4 * tid + 2] = (float)re[hi];
        fd[4 * tid + 3] = (float)im[hi];
    }
    return true;
}

// The table for welch16k1x_half_kernel.  N = 16384: thread tid = 64 k0 + 4 k1 + q corrects register k2 = 0 - bin k0 when
// k1 = 0, q = 0 - and register k2 = 15 - bin N - 16 + k0 when k1 = 15, q = 3, where the quad butterfly leaves i X.
// N = 8192 (the 8-wave form, round 5): wave k0' holds k0 = 2 k0' + h; register k2 = 0 of lane 32 h is bin k0, register
// k2 = 15 of lane 32 h + 31 (k1 = 7, q = 3) is bin N - 16 + k0.  Either way the table exists when the window's spectrum is
// confined to |k| < 16 (all periodic cosine-sum windows; boxcar).
bool window_spectrum_table_1x(const std::vector<float> &w, int n, std::vector<float> &fd) {
    std::vector<double> re, im;
    if (!window_spectrum(w, n, 16, re, im)) return false;
    fd.assign((size_t)4 * (n / 16), 0.f);
    for (int k0 = 0; k0 < 16; ++k0) {
        const int lo = n == 16384 ? 64 * k0 : 64 * (k0 >> 1) + 32 * (k0 & 1);
        const int hi = n == 16384 ? 64 * k0 + 63 : 64 * (k0 >> 1) + 32 * (k0 & 1) + 31;
        fd[4 * lo] = (float)re[k0];
        fd[4 * lo + 1] = (float)im[k0];
        const int kh = n - 16 + k0;                       // i (re + i im) = -im + i re
        fd[4 * hi + 2] = (float)(-im[kh]);
        fd[4 * hi + 3] = (float)re[kh];
    }
    return true;
}

// Acceptance test of welch4096ws's complementary-window producer (WelchArgs.compl_win): in double, on the float window
// the plan was given, |w[n] + w[n + N / 2] - 1| <= 2^-23 for every n - one float32 ulp at 1.  SciPy's default periodic Hann
// measures 3.0e-8, a quarter of it; flattop, Blackman-Harris and boxcar miss by 0.5 ... 1.1 and keep the general build.
bool window_is_complementary(const std::vector<float> &w, int n) {
    for (int i = 0; i < n / 2; ++i)
        if (!(std::fabs((double)w[i] + (double)w[i + n / 2] - 1.0) <= 1.1920928955078125e-07)) return false;
    return true;
}

int segments(const oth_plan *p, size_t nsamples, long long *nseg) {
    if (nsamples < (size_t)p->nperseg) return OTH_ERR_INVALID;
    *nseg = (long long)((nsamples - (size_t)p->noverlap) / (size_t)p->step);
    return OTH_OK;
}

// What an averaging launch leaves in plan->d_partial: W rows in `layout` per stream (and channel), sums over nseg segments.
struct Averaged {
    int rc = OTH_OK;      // or the refusal / error (run_average's `return fail(...)` and HIPCHK): nothing was left
    long long nseg = 0;
    int W = 0;
    RowLayout layout = ROW_NATURAL;
    Averaged() = default;
    Averaged(int code) : rc(code) {}
};

// Launch the averaging kernel: partial sums land in plan->d_partial.
Averaged run_average(oth_plan *p, const float2 *x, const float2 *y, size_t nsamples, int nstreams, size_t stride) {
    oth_ctx *c = p->ctx;
    Averaged av;
    long long &nseg = av.nseg;
    if (segments(p, nsamples, &nseg) != OTH_OK)
        return fail(c, OTH_ERR_INVALID, "input shorter than nperseg");
    const bool csd = (y != nullptr);
    if (p->ntapers) {      // multitaper plans: mtm.hip, before any routing
        if (csd)      // (the oth_csd_* entry points have asked already)
            if (int rc = mtm_csd_gate(p, "the cross spectrum")) return rc;
        if (int rc = mtm_run(p, x, y, nseg, nstreams, stride, &av.W)) return rc;
        return av;
    }
    LaunchRecipe r;
    const char *why = "";
    if (int rrc = resolve_recipe(shape_of(p), csd, nseg, nstreams, c->cu_count, runtime_bpc, &r, &why))
        return fail(c, rrc, why);
    p->last_recipe = recipe_text(r, p->nfft);
    int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)nstreams * r.W * r.nch * p->nfft);
    {
        const int groups = std::max(kReduceGroups, finalize_row_groups(p->nfft, r.W, r.nch));
        if (!rc) rc = p->d_reduce.ensure(c, sizeof(float) * (size_t)nstreams * groups * r.nch * p->nfft);
    }
    if (rc) return rc;
    const float4 *fd_tab = r.form == 2 ? (r.use_fd1x ? p->d_fd1x.get() : p->d_fd.get()) : nullptr;
    // the pilot of every stream (WelchArgs.pilot): from its own launch, or formed in the kernel's prologue
    const float2 *pilot = nullptr;
    if (r.pilot == 1) {
        rc = p->d_pilot.ensure(c, sizeof(float2) * 2 * kPilotProbes * (size_t)nstreams);
        if (rc) return rc;
        HIPCHK(c, launch_pilot_mean(x, csd ? y : nullptr, stride, p->nperseg, p->step, nseg, nstreams, p->d_pilot.get(), c->stream));
        pilot = p->d_pilot.get();
    }
    unsigned *queue = nullptr;
    if (r.tickets) {
        queue = c->queue.get();
        if (!c->queue_clean) HIPCHK(c, hipMemsetAsync(c->queue.get(), 0, sizeof(unsigned) * 64, c->stream));
        c->queue_clean = false;      // until the finalize launch that follows has re-zeroed them
        c->queue_used = nstreams;
    }
    if (r.kern == RK_ANY && r.any_onewg) {
        Timed tm(c);
        for (int st = 0; st < nstreams; ++st) {
            W32kArgs a{};
            a.x = x + (size_t)st * stride;
            a.first = 0, a.step = p->step, a.nseg = nseg;
            a.win = p->d_win.get(), a.tw = p->any.tw;
            a.partial = p->d_partial.get() + (size_t)st * r.W * p->nfft;
            a.detrend = p->detrend != OTH_DETREND_NONE;
            a.front = p->nfft == 65536, a.wpm = p->d_wpm.get();
            HIPCHK(c, launch_welch32k(a, r.W, c->stream));
        }
    } else if (r.kern == RK_ANY) {
        Timed tm(c);
        for (int st = 0; st < nstreams; ++st) {
            rc = any_run(c, p->any, x + (size_t)st * stride, csd ? y + (size_t)st * stride : nullptr, 0, p->step, p->nperseg, p->d_win.get(),
                         p->detrend != OTH_DETREND_NONE, nseg, p->d_partial.get() + (size_t)st * r.W * r.nch * p->nfft, r.W, nullptr, 0,
                         1.0f, 0, p->tune_variant == "anycov");
            if (rc) return rc;
        }
    } else if (r.kern == RK_SEG || r.kern == RK_SEGWS || r.kern == RK_SEGPAD) {
        SegArgs g{};
        g.x = x;
        g.stream_stride = stride;
        g.nstreams = nstreams;
        g.win = p->d_win.get();
        g.tw = p->d_tw;
        g.first = 0;
        g.step = p->step;
        g.nseg = nseg;
        g.detrend = p->detrend;
        g.chain = 0;
        g.partial = p->d_partial.get();
        g.wg_per_stream = r.W;
        g.sched = r.sched;
        g.chunk = r.chunk;
        g.tail_chunk = r.tail_chunk;
        g.nbig = r.nbig;
        g.queue = queue;
        g.fd = fd_tab;
        g.pilot = pilot;
        Timed tm(c);
        switch (r.kern) {
            case RK_SEGPAD: HIPCHK(c, launch_seg_padded(p->nfft, p->nperseg, g, r.seg_kind, c->stream)); break;
            case RK_SEGWS: HIPCHK(c, launch_segws(p->nfft, g, r.seg_det, c->stream)); break;
            default: HIPCHK(c, launch_seg(p->nfft, g, r.seg_kind, r.seg_wps4, c->stream)); break;
        }
    } else {
        WelchArgs a;
        a.x = x;
        a.y = y;
        a.win = p->d_win.get();
        a.tw = p->d_tw;
        a.partial = p->d_partial.get();
        a.nseg = nseg;
        a.stream_stride = stride;
        a.nperseg = p->nperseg;
        a.step = p->step;
        a.detrend = p->detrend;
        a.wg_per_stream = r.W;
        a.nstreams = nstreams;
        a.sched = r.sched;
        a.chunk = r.chunk;
        a.tail_chunk = r.tail_chunk;
        a.nbig = r.nbig;
        a.queue = queue;
        a.fd = fd_tab;
        a.pilot = pilot;
        a.pilot_inline = r.pilot == 2 ? 1 : 0;
        // (read by launch_welch_tuned4096_ws only; the tuning word "wsgen" keeps the general build: the A/B and the parity tests)
        a.compl_win = p->compl_window && p->tune_variant != "wsgen" ? 1 : 0;
        a.symtw = p->d_symtw.get();
        a.fd_sym = p->d_fd_sym.get();
        Timed tm(c);
        switch (r.kern) {
            case RK_W4096: HIPCHK(c, r.variant->launch(a, c->stream)); break;
            case RK_CSD4096WS: HIPCHK(c, launch_csd_tuned4096ws(a, c->stream)); break;
            case RK_CSD4096: HIPCHK(c, launch_csd_tuned4096(a, c->stream)); break;
            case RK_W16K1X_HALF:
                HIPCHK(c, r.half_ws ? launch_welch_tuned8kws(a, c->stream) : launch_welch_tuned16k1x_half(p->nfft, a, c->stream));
                break;
            case RK_W16K1X: HIPCHK(c, launch_welch_tuned16k1x(p->nfft, a, r.x1_window, r.x1_plain, c->stream)); break;
            case RK_W16K: HIPCHK(c, launch_welch_tuned16k(p->nfft, a, c->stream)); break;
            default: HIPCHK(c, launch_welch_generic(p->nfft, a, c->stream)); break;
        }
    }
    av.W = r.W;
    av.layout = r.layout;
    return av;
}

// finalize_kernel zeroes the ticket counters the averaging launch before it used (saves a memset per call)
int finalize_and_rearm(oth_ctx *c, FinalizeArgs &f, int nstreams) {
    f.queue_reset = nullptr;
    f.queue_n = 0;
    if (!c->queue_clean && c->queue_used > 0) {
        f.queue_reset = c->queue.get();
        f.queue_n = c->queue_used;
    }
    HIPCHK(c, launch_finalize(f, nstreams, c->stream));
    if (f.queue_reset) {
        c->queue_clean = true;
        c->queue_used = 0;
    }
    return OTH_OK;
}

// ---- median average (OTH_AVERAGE_MEDIAN) --------------------------------------------------------------------------------
// scipy.signal._spectral_helper's _median_bias(n): 1 + sum_{i=1}^{(n-1)//2} (1 / (2 i + 1) - 1 / (2 i)), in double
double median_bias(long long n) {
    double b = 1.0;
    for (long long i = 1; i <= (n - 1) / 2; ++i) b += 1.0 / (double)(2 * i + 1) - 1.0 / (double)(2 * i);
    return b;
}

int refuse_median(oth_plan *p, const char *what) {
    return fail(p->ctx, OTH_ERR_UNSUPPORTED, std::string(what) + " is not available with OTH_AVERAGE_MEDIAN: a median is not a "
                "sum of partials (the median runs through oth_welch_exec, _exec_async and _exec_dev)");
}

// Rows producer: nseg raw |X|^2 rows per stream, [stream][segment][nfft] in natural bin order, into p->d_rows.  256 ... 4096
// points with nperseg = nfft: the chain build of seg_kernel (segfft.hip launch_seg_rows); every other shape: any_run's rows.
int median_rows(oth_plan *p, const float2 *x, int nstreams, size_t stride, long long nseg, const char **route) {
    oth_ctx *c = p->ctx;
    const int N = p->nfft;
    const size_t need = sizeof(float) * (size_t)nstreams * (size_t)nseg * (size_t)N;
    if (int rc = p->d_rows.ensure(c, need)) {
        if (rc != OTH_ERR_NOMEM) return rc;
        return fail(c, rc, "per-segment rows workspace of " + std::to_string(need) +
                               " bytes (nstreams x nseg x nfft x 4 B) could not be allocated (" + c->err + ")");
    }
    const bool det = p->detrend != OTH_DETREND_NONE;
    if (seg_supported(N) && p->nperseg == N) {
        SegArgs a{};
        a.x = x;
        a.stream_stride = stride;
        a.nstreams = nstreams;
        a.win = p->d_win.get();
        a.tw = p->d_tw;
        a.first = 0;
        a.step = p->step;
        a.nseg = nseg;
        a.detrend = det ? 1 : 0;
        a.chain = 1;
        a.acc_mode = 3;      // rows only
        a.rows = p->d_rows.get();
        a.store_from = 0;
        a.epilogue = OTH_EPI_MAG2;
        a.scale = 1.0f;
        interleaved_chunks(a, (long long)c->cu_count * seg_rows_teams_per_cu(N));      // as the chain's fused launch
        HIPCHK(c, launch_seg_rows(N, a, c->stream));
        *route = "seg";
        return OTH_OK;
    }
    AnyTables *t = &p->any;
    if (t->sh.kind == ANY_NONE) {      // power-of-two plans: tables of their own (any_describe: "direct" up to 16384)
        t = &p->rows_any;
        if (t->sh.kind == ANY_NONE)
            if (int rc = any_tables_init(c, N, t)) return rc;
    }
    for (int st = 0; st < nstreams; ++st)
        if (int rc = any_run(c, *t, x + (size_t)st * stride, nullptr, 0, p->step, p->nperseg, p->d_win.get(), det, nseg, nullptr, 0,
                             p->d_rows.get() + (size_t)st * nseg * N, OTH_EPI_MAG2, 1.0f, 0))
            return rc;
    *route = kAnyKindName[t->sh.kind];
    return OTH_OK;
}

// rows + radix select: the medians of every bin of every stream land in p->d_med.get() ([stream][nfft], unscaled)
int median_run(oth_plan *p, const float2 *x, size_t nsamples, int nstreams, size_t stride, long long *nseg_out) {
    oth_ctx *c = p->ctx;
    long long nseg = 0;
    if (segments(p, nsamples, &nseg) != OTH_OK) return fail(c, OTH_ERR_INVALID, "input shorter than nperseg");
    if (nseg >= (1LL << 31)) return fail(c, OTH_ERR_UNSUPPORTED, "median average: more than 2^31 segments per stream");
    const int N = p->nfft;
    MedianArgs m{};
    m.nseg = nseg;
    m.nfft = N;
    m.nstreams = nstreams;
    m.seg_per_wg = median_seg_per_wg(nseg, N, nstreams, c->cu_count);
    const char *route = "";
    {
        Timed tm(c);      // rows producer + selection
        // the rows workspace first: it is the one a large request is refused on, and the plan then holds what it held before
        int rc = median_rows(p, x, nstreams, stride, nseg, &route);
        if (!rc) rc = p->d_med.ensure(c, sizeof(float) * (size_t)nstreams * N);
        if (!rc) rc = p->d_msel.ensure(c, sizeof(unsigned) * median_scratch_words(N, nstreams));
        if (rc) return rc;
        median_bind_scratch(m, p->d_msel.get());
        m.med = p->d_med.get();
        m.rows = reinterpret_cast<const unsigned *>(p->d_rows.get());
        HIPCHK(c, launch_median_select(m, c->stream));
    }
    p->last_recipe = std::string("kernel=median rows=") + route + " nfft=" + std::to_string(N) + " nseg=" + std::to_string(nseg) +
                     " nstreams=" + std::to_string(nstreams) + " select=radix8x4 seg_per_wg=" + std::to_string(m.seg_per_wg);
    if (p->bias_nseg != nseg) {
        p->bias = median_bias(nseg);
        p->bias_nseg = nseg;
    }
    *nseg_out = nseg;
    return OTH_OK;
}
}  // namespace

namespace oth {
int plan_begin(oth_ctx *c, int nfft, int nperseg, int noverlap, int detrend, int scaling, double fs, int fftshift, int trim_bins,
               std::unique_ptr<oth_plan> *out) {
    if (nfft < 1) return fail(c, OTH_ERR_INVALID, "nfft must be positive");
    if (nperseg < 1 || nperseg > nfft) return fail(c, OTH_ERR_INVALID, "need 1 <= nperseg <= nfft");
    if (noverlap < 0 || noverlap >= nperseg) return fail(c, OTH_ERR_INVALID, "need 0 <= noverlap < nperseg");
    if (detrend != OTH_DETREND_NONE && detrend != OTH_DETREND_CONSTANT && detrend != OTH_DETREND_CONSTANT_EXACT &&
        detrend != OTH_DETREND_CONSTANT_FAST)
        return fail(c, OTH_ERR_INVALID, "unknown detrend");
    if (scaling < OTH_SCALE_RAW || scaling > OTH_SCALE_SPECTRUM) return fail(c, OTH_ERR_INVALID, "unknown scaling");
    if (trim_bins < 0 || 2 * trim_bins >= nfft) return fail(c, OTH_ERR_INVALID, "trim_bins out of range");
    if (!(fs > 0.0)) return fail(c, OTH_ERR_INVALID, "fs must be positive");
    if (use_device(c)) return OTH_ERR_HIP;
    std::unique_ptr<oth_plan> p(new (std::nothrow) oth_plan());
    if (!p) return fail(c, OTH_ERR_NOMEM, "host allocation failed");
    p->ctx = c;
    p->nfft = nfft;
    p->nperseg = nperseg;
    p->noverlap = noverlap;
    p->step = nperseg - noverlap;
    p->fast_detrend = detrend == OTH_DETREND_CONSTANT_FAST;
    p->detrend = detrend != OTH_DETREND_NONE ? OTH_DETREND_CONSTANT : OTH_DETREND_NONE;      // one operation: forms and builds
                                                                                              // are run_average's choice
    p->scaling = scaling;
    p->fs = fs;
    p->fftshift = fftshift != 0;
    p->trim = trim_bins;
    if (const char *e = getenv("OTH_HOSTWAIT")) p->hostwait = !strcmp(e, "sync") ? 1 : 0;      // initial value of oth_plan_set_hostwait
    *out = std::move(p);
    return OTH_OK;
}
}  // namespace oth

extern "C" {
/* ---- Welch ---------------------------------------------------------------- */

int oth_welch_plan(oth_ctx *c, int nfft, int nperseg, int noverlap, const float *window, int detrend, int scaling,
                   double fs, int fftshift, int trim_bins, oth_plan **out) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !out) return fail(c, OTH_ERR_INVALID, "ctx/out is NULL");
    *out = nullptr;
    std::unique_ptr<oth_plan> p;
    if (int rc = plan_begin(c, nfft, nperseg, noverlap, detrend, scaling, fs, fftshift, trim_bins, &p)) return rc;
    const bool any_route = !generic_supported(nfft);      // not a power of two in [64, 16384]: fft_any.hip
    const bool det = p->detrend == OTH_DETREND_CONSTANT;
    if (const char *e = getenv("OTH_W4096_VARIANT")) p->tune_variant = e;      // read once, here
    if (const char *e = getenv("OTH_W4096_SCHED")) p->tune_sched = atoi(e);
    if (const char *e = getenv("OTH_W4096_CHUNK")) p->tune_chunk = atoi(e);
    if (const char *e = getenv("OTH_W4096_TAIL")) p->tune_tail = atoi(e);
    if (const char *e = getenv("OTH_PILOT_LAUNCH")) p->pilot_launch = atoi(e) != 0;
    std::vector<float> w(nfft, 0.f);   // zero-extended so that kernels may index [0, nfft)
    double s1 = 0.0, s2 = 0.0;
    p->rect_window = true;
    for (int i = 0; i < nperseg; ++i) {
        w[i] = window ? window[i] : 1.0f;
        if (w[i] != 1.0f) p->rect_window = false;
        s1 += (double)w[i];
        s2 += (double)w[i] * (double)w[i];
    }
    switch (scaling) {
        case OTH_SCALE_DENSITY: p->scale = 1.0 / (fs * s2); break;
        case OTH_SCALE_OVER_N2: p->scale = 1.0 / ((double)nfft * (double)nfft); break;
        case OTH_SCALE_SPECTRUM: p->scale = 1.0 / (s1 * s1); break;
        default: p->scale = 1.0;
    }
    p->sk_g = s2 > 0.0 && std::isfinite(1.0 / s2) ? 1.0 / s2 : 1.0;      // oth_welch_sk's periodogram scale
    p->win_host.assign(w.begin(), w.begin() + nperseg);                   // oth_welch_set_cycles' complex tapers
    if (const char *e = getenv("OTH_CYC_GROUP")) p->tune_cyc_group = atoi(e);
    if (const char *e = getenv("OTH_LAG_GROUP")) p->tune_lag_group = atoi(e);
    // the welch4096ws route's shape; its complementary-window build detrends one bin per thread and needs its own table
    std::vector<float2> fd_sym, symtw;
    p->compl_window = nfft == 4096 && nperseg == 4096 && window_is_complementary(w, nfft) && (!det || window_spectrum_table_sym(w, fd_sym));
    if (p->compl_window) symtw = symtw_table();
    // the host tables first, then the uploads: nothing between the first asynchronous copy and the synchronise can throw
    std::vector<float> fd, fd1x, wpm;
    const bool have_fd = det && ((nfft == 4096 && nperseg == 4096 && window_spectrum_table(w, fd)) ||
                                 (nfft == 2048 && nperseg == 2048 && window_spectrum_table_seg(w, nfft, fd)) ||
                                 ((nfft == 8192 || nfft == 16384) && nperseg == nfft && window_spectrum_table_16k(w, nfft, fd)));
    const bool have_fd1x = det && (nfft == 16384 || nfft == 8192) && nperseg == nfft && window_spectrum_table_1x(w, nfft, fd1x);
    if (any_route && nfft == 65536 && nperseg == 65536) {
        wpm.resize(65536);
        for (int n = 0; n < 32768; ++n) {
            wpm[n] = (float)((double)w[n] + (double)w[n + 32768]);
            wpm[32768 + n] = (float)((double)w[n] - (double)w[n + 32768]);
        }
    }
    if (int rc = any_route ? any_tables_init(c, nfft, &p->any) : get_twiddles(c, nfft, &p->d_tw)) return rc;
    hipError_t e = p->d_win.upload(c, w.data(), sizeof(float) * nfft);
    if (e == hipSuccess) e = p->d_sum.alloc(sizeof(float) * nfft);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_sum.get(), 0, sizeof(float) * nfft, c->stream);
    if (e == hipSuccess && have_fd) e = p->d_fd.upload(c, fd.data(), sizeof(float) * fd.size());
    if (e == hipSuccess && !symtw.empty()) e = p->d_symtw.upload(c, symtw.data(), sizeof(float2) * symtw.size());
    if (e == hipSuccess && !fd_sym.empty()) e = p->d_fd_sym.upload(c, fd_sym.data(), sizeof(float2) * fd_sym.size());
    if (e == hipSuccess && have_fd1x) e = p->d_fd1x.upload(c, fd1x.data(), sizeof(float) * fd1x.size());
    if (e == hipSuccess && !wpm.empty()) e = p->d_wpm.upload(c, wpm.data(), sizeof(float) * wpm.size());
    const hipError_t es = hipStreamSynchronize(c->stream);      // also after a failure: the host tables die here
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string("plan setup: ") + hipGetErrorString(e));
    *out = p.release();
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_plan_destroy(oth_plan *p) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return OTH_OK;
    oth_ctx *c = p->ctx;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    delete p;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_plan_set_output_db(oth_plan *p, int enable) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    p->db = enable != 0;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_plan_set_kernel(oth_plan *p, int which) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (which < OTH_KERNEL_AUTO || which > OTH_KERNEL_TUNED) return fail(p->ctx, OTH_ERR_INVALID, "unknown kernel id");
    if (p->ntapers && which == OTH_KERNEL_TUNED) return refuse_mtm(p, "OTH_KERNEL_TUNED", "no tuned kernel carries the taper loop");
    p->kernel = which;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_plan_set_schedule(oth_plan *p, int which) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (which < OTH_SCHED_CONTIGUOUS || which > OTH_SCHED_DYNAMIC) return fail(p->ctx, OTH_ERR_INVALID, "unknown schedule");
    p->sched = which;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_plan_set_tuning(oth_plan *p, const char *variant, int sched, int chunk, int tail_chunk) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (sched < -1 || sched > OTH_SCHED_DYNAMIC || chunk < 0 || tail_chunk < 0)
        return fail(p->ctx, OTH_ERR_INVALID, "bad tuning value");
    if (p->ntapers && variant && *variant) return refuse_mtm(p, "a kernel build variant", "mtm_kernel has one build per size");
    if (variant && *variant) {
        bool known = !strcmp(variant, "seg3") || !strcmp(variant, "seg4") || !strcmp(variant, "segws") ||   // 1024 / 2048
                     !strcmp(variant, "csd1") ||                                // the one-role two-channel kernel
                     !strcmp(variant, "fd") || !strcmp(variant, "td") ||        // detrend form only (run_average)
                     !strcmp(variant, "plaunch") ||                             // pilot from its own launch (run_average)
                     !strcmp(variant, "wsgen") ||                               // "ws" with the general-window producer also where the
                                                                                // window is complementary (the A/B of WelchArgs.compl_win)
                     !strcmp(variant, "16k4") || !strcmp(variant, "16kplain") ||  // 16384 points: the 4 x 4096 build / the
                                                                                // un-pipelined one-exchange build
                     !strcmp(variant, "8kws") || !strcmp(variant, "8k1role") ||  // 8192 points, 50 % overlap: role-split / one-role
                     !strcmp(variant, "anycov") ||                              // 32768 / 65536 points: fft_any.hip's coverage kernels
                                                                                // instead of fft_tl.hip's
                     !strcmp(variant, "r16");                                   // 32768 points: fft_tl.hip's four-step route instead
                                                                                // of welch32k.hip
        known = known || w4096_variant_known(variant);
        if (!known) return fail(p->ctx, OTH_ERR_UNSUPPORTED, std::string("unknown kernel build: ") + variant);
    }
    p->tune_variant = variant ? variant : "";
    p->tune_sched = sched;
    p->tune_chunk = chunk;
    p->tune_tail = tail_chunk;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_plan_set_hostwait(oth_plan *p, int mode) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (mode != OTH_HOSTWAIT_POLL && mode != OTH_HOSTWAIT_SYNC) return fail(p->ctx, OTH_ERR_INVALID, "unknown host-wait mode");
    p->hostwait = mode;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_plan_out_len(oth_plan *p, int *n) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p || !n) return fail(p ? p->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    *n = p->nfft - 2 * p->trim;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_plan_set_average(oth_plan *p, int mode) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (mode != OTH_AVERAGE_MEAN && mode != OTH_AVERAGE_MEDIAN) return fail(p->ctx, OTH_ERR_INVALID, "unknown average mode");
    if (p->ntapers && mode == OTH_AVERAGE_MEDIAN)
        return refuse_mtm(p, "OTH_AVERAGE_MEDIAN", "the taper loop sums the segments' estimates and keeps no per-segment rows");
    if (p->nseg_total || p->carry)
        return fail(p->ctx, OTH_ERR_STATE, "an accumulation is in progress (oth_welch_finalize or oth_welch_reset first)");
    p->average = mode;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_segments_dev(oth_plan *p, const void *iq_dev, size_t nsamples, float *rows_dev, uint64_t capacity_rows,
                           uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    oth_ctx *c = p->ctx;
    if (p->ntapers) return refuse_mtm(p, "oth_welch_segments_dev", "the taper loop sums the segments' estimates and keeps no per-segment rows");
    if (!iq_dev || !rows_dev) return fail(c, OTH_ERR_INVALID, "bad argument");
    long long nseg = 0;
    if (segments(p, nsamples, &nseg) != OTH_OK) return fail(c, OTH_ERR_INVALID, "input shorter than nperseg");
    if ((uint64_t)nseg > capacity_rows)
        return fail(c, OTH_ERR_INVALID, "capacity_rows " + std::to_string(capacity_rows) + " < nseg " + std::to_string(nseg));
    if (use_device(c)) return OTH_ERR_HIP;
    const char *route = "";
    if (int rc = median_rows(p, (const float2 *)iq_dev, 1, nsamples, nseg, &route)) return rc;
    // (a launch of its own: without this line oth__debug_last_recipe went on naming the call before this one)
    p->last_recipe = std::string("kernel=segments rows=") + route + " nfft=" + std::to_string(p->nfft) + " nseg=" + std::to_string(nseg);
    // the plan's scaling, fftshift, trim and dB per row: finalize_kernel with one "stream" per segment (grid.y <= 65535)
    FinalizeArgs f = finalize_args(p, 1, ROW_NATURAL, 1, out_stage(p));
    f.scratch = nullptr;
    f.scale = p->scale;
    for (long long s0 = 0; s0 < nseg; s0 += 65535) {
        const long long nb = std::min(65535LL, nseg - s0);
        f.partial = p->d_rows.get() + (size_t)s0 * p->nfft;
        f.out0 = rows_dev + (size_t)s0 * f.out.nout;
        HIPCHK(c, launch_finalize(f, (int)nb, c->stream));
    }
    if (nseg_out) *nseg_out = (uint64_t)nseg;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

// averaging launch + finalize into psd_out (device memory, or a pinned host row when host_seq is given: the finalize
// launch then also publishes seq_value there once the row is complete)
static int welch_exec_dev_impl(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                               float *psd_out_dev, uint64_t *nseg_out, unsigned *host_seq, unsigned seq_value) {
    oth_ctx *c = p->ctx;
    if (!iq_dev || !psd_out_dev || nstreams < 1) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (nstreams > 1 && stream_stride < nsamples) return fail(c, OTH_ERR_INVALID, "stream_stride < nsamples");
    if (use_device(c)) return OTH_ERR_HIP;
    long long nseg = 0;
    FinalizeArgs f;
    if (p->average == OTH_AVERAGE_MEDIAN) {
        // one row of medians per stream: finalize_kernel applies scale / bias, fftshift, trim and dB
        if (int rc = median_run(p, (const float2 *)iq_dev, nsamples, nstreams, stream_stride, &nseg)) return rc;
        f = finalize_args(p, 1, ROW_NATURAL, 1, out_stage(p));
        f.partial = p->d_med.get();
        f.scratch = nullptr;
        f.scale = p->scale / p->bias;
    } else {
        const Averaged av = run_average(p, (const float2 *)iq_dev, nullptr, nsamples, nstreams, stream_stride);
        if (av.rc) return av.rc;
        nseg = av.nseg;
        f = finalize_args(p, av.W, av.layout, 1, out_stage(p));
        f.scale = p->scale / (double)nseg;
    }
    f.out0 = psd_out_dev;
    if (host_seq) {
        f.done_count = c->done_count;
        f.host_seq = host_seq;
        f.seq_value = seq_value;
    }
    if (int frc = finalize_and_rearm(c, f, nstreams)) return frc;
    if (nseg_out) *nseg_out = (uint64_t)nseg;
    return OTH_OK;
}

int oth_welch_exec_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                       float *psd_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    return welch_exec_dev_impl(p, iq_dev, nsamples, nstreams, stream_stride, psd_out_dev, nseg_out, nullptr, 0u);
    OTH_CATCH((p ? p->ctx : nullptr))
}

static int stage_host(oth_plan *p, const void *x, const void *y, size_t nsamples, const float2 **dx, const float2 **dy) {
    oth_ctx *c = p->ctx;
    const size_t bytes = nsamples * sizeof(float2);
    int rc = p->d_stage.ensure(c, bytes * (y ? 2 : 1));
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(p->d_stage.get(), x, bytes, hipMemcpyHostToDevice, c->stream));
    *dx = p->d_stage.get();
    if (y) {
        HIPCHK(c, hipMemcpyAsync(p->d_stage.get() + nsamples, y, bytes, hipMemcpyHostToDevice, c->stream));
        *dy = p->d_stage.get() + nsamples;
    }
    return OTH_OK;
}

// ---- host-output forms: oth_welch_exec (blocking), oth_welch_exec_async / _poll / _wait (tickets) --------------------
// SURVEY 8d ends the metric at "PSD available on host".  Round 4: three launches, then hipStreamSynchronize - an
// interrupt wake-up whose latency differs by 100 us between hosts of the same pool.  Now the finalize launch writes the
// row into pinned host memory and a completion word behind it (kernels_misc.hip finalize_signal), and the host polls
// that word: first in a tight loop, then yielding the CPU between looks, and only after kPollFallbackMs through
// hipStreamSynchronize (which also turns a faulted launch into an error code instead of an endless wait).
// OTH_HOSTWAIT=sync restores the wait of round 4 for the A/B.
namespace {
constexpr double kPollSpinUs = 2000.0;         // tight polling (pause instructions only): covers a 2^28-sample launch; with
                                               // sched_yield() from 200 us on, a process with other runnable threads (bench.py
                                               // under torch) came back 30 us late (0.6256 against 0.595 ms per step)
constexpr double kPollFallbackMs = 20.0;       // then yield between looks; past this, hipStreamSynchronize (round 5: 200 ms -
                                               // a core per blocked caller for that long; OTH_HOSTWAIT_SYNC / oth_plan_set_hostwait
                                               // is the mode for flowgraphs with many blocking sensors)

inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#endif
}

inline double now_us() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3;
}

// The word of a slot only ever grows (tickets t, t + 4, t + 8, ... of that slot, low 32 bits): "reached" is >= in
// wrap-safe arithmetic, so a waiter whose ticket was overtaken by a newer launch on the slot leaves its loop too (and is
// then told OTH_ERR_STATE, not that the word was never written).
inline bool seq_reached(const unsigned *word, unsigned want) {
    return (int)(__atomic_load_n(word, __ATOMIC_ACQUIRE) - want) >= 0;
}

// -> true when the word shows `want` (the row behind it is then visible to this thread)
bool poll_seq(const unsigned *word, unsigned want, double budget_ms) {
    if (seq_reached(word, want)) return true;
    const double t0 = now_us();
    for (;;) {
        for (int i = 0; i < 32; ++i) {
            if (seq_reached(word, want)) return true;
            cpu_relax();
        }
        const double dt = now_us() - t0;
        if (dt > budget_ms * 1e3) return false;
        if (dt > kPollSpinUs) sched_yield();
    }
}

int out_ring_init(oth_plan *p) {
    oth_ctx *c = p->ctx;
    if (p->h_out) return OTH_OK;
    PinnedBuf<float> rows;
    PinnedBuf<unsigned> seq;
    if (rows.alloc(sizeof(float) * p->nfft * oth_plan::kOutRing) != hipSuccess ||
        seq.alloc(sizeof(unsigned) * 16 * oth_plan::kOutRing) != hipSuccess)
        return fail(c, OTH_ERR_NOMEM, "pinned host allocation failed");
    memset(seq.get(), 0, sizeof(unsigned) * 16 * oth_plan::kOutRing);      // one word per 64-byte line
    p->h_out = std::move(rows);
    p->h_seq = std::move(seq);
    return OTH_OK;
}

// The caller's buffer is copied into the next slot of the plan's pinned ring, the H2D copy to dst is enqueued from there
// and the call returns without waiting for the GPU (a slot is reused four calls later; only then, if the GPU is still
// that far behind, does the call wait)
int ring_upload(oth_plan *p, void *dst, const void *src, size_t bytes) {
    oth_ctx *c = p->ctx;
    const unsigned slot = p->h_ring_next++ & 3u;
    if (!p->h_ring_ev[slot]) HIPCHK(c, p->h_ring_ev[slot].create());
    else HIPCHK(c, hipEventSynchronize(p->h_ring_ev[slot].get()));
    if (int rc = p->h_ring[slot].grow(c, bytes)) return rc;
    memcpy(p->h_ring[slot].get(), src, bytes);
    HIPCHK(c, hipMemcpyAsync(dst, p->h_ring[slot].get(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(p->h_ring_ev[slot].get(), c->stream));
    return OTH_OK;
}

// Enqueue one host-output launch; the caller holds the context lock.
int welch_enqueue(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, bool caller_blocks, uint64_t *ticket_out) {
    oth_ctx *c = p->ctx;
    if (!iq) return fail(c, OTH_ERR_INVALID, "iq is NULL");
    if (nsamples < (size_t)p->nperseg) return fail(c, OTH_ERR_INVALID, "input shorter than nperseg");
    if (use_device(c)) return OTH_ERR_HIP;
    int rc = out_ring_init(p);
    if (rc) return rc;
    const uint64_t ticket = p->next_out_ticket;
    const int slot = (int)(ticket % oth_plan::kOutRing);
    unsigned *word = p->h_seq.get() + 16 * slot;
    // the slot's previous launch (kOutRing tickets ago) must have delivered before its row is written again
    if (p->out_ticket[slot] && !seq_reached(word, (unsigned)p->out_ticket[slot])) {
        if (!poll_seq(word, (unsigned)p->out_ticket[slot], kPollFallbackMs)) HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const float2 *dx = (const float2 *)iq, *dy = nullptr;
    if (!src_is_device) {
        // the caller's buffer is valid during the call only (sync_block.work()): pageable memory is staged by the
        // runtime before hipMemcpyAsync returns; a pinned / registered source would be read asynchronously, so that
        // copy is awaited (the one case in which the asynchronous form waits for the stream)
        const size_t bytes = nsamples * sizeof(float2);
        if (!caller_blocks && bytes <= kPinnedStageMax) {
            // work()-sized buffers: through a pinned slot (as oth_welch_accumulate), so that the call returns at once -
            // from pageable memory hipMemcpyAsync may hold the host until the stream has drained
            if ((rc = p->d_stage.ensure(c, bytes))) return rc;
            if ((rc = ring_upload(p, p->d_stage.get(), iq, bytes))) return rc;
            dx = p->d_stage.get();
        } else if (!caller_blocks && host_ptr_is_pinned(iq)) {
            if ((rc = p->d_stage.ensure(c, bytes))) return rc;
            if ((rc = copy_in_and_wait(c, p->d_stage.get(), iq, bytes))) return rc;
            dx = p->d_stage.get();
        } else if ((rc = stage_host(p, iq, nullptr, nsamples, &dx, &dy))) {
            return rc;
        }
    }
    uint64_t nseg = 0;
    if ((rc = welch_exec_dev_impl(p, dx, nsamples, 1, nsamples, p->h_out.get() + (size_t)slot * p->nfft, &nseg, word,
                                  (unsigned)ticket)))
        return rc;
    p->out_ticket[slot] = ticket;
    p->out_nseg[slot] = nseg;
    p->next_out_ticket = ticket + 1;
    *ticket_out = ticket;
    return OTH_OK;
}

// Collect a ticket: wait == 0 looks once, wait == 1 polls (outside the context lock) and falls back to the stream.
int welch_collect(oth_plan *p, uint64_t ticket, float *psd_out, uint64_t *nseg_out, int *ready, bool wait) {
    oth_ctx *c = p->ctx;
    const int slot = (int)(ticket % oth_plan::kOutRing);
    const unsigned *word;
    uint64_t nseg;
    {
        CtxGuard guard_(c);
        if (!ticket || !p->h_out.get() || p->out_ticket[slot] != ticket)
            return fail(c, OTH_ERR_STATE, "ticket unknown or overwritten (the ring keeps the last 4 launches)");
        word = p->h_seq.get() + 16 * slot;
        nseg = p->out_nseg[slot];
    }
    bool done = seq_reached(word, (unsigned)ticket);
    if (!done && wait) {
        if (p->hostwait == 0) done = poll_seq(word, (unsigned)ticket, kPollFallbackMs);
        if (!done) {
            CtxGuard guard_(c);
            if (use_device(c)) return OTH_ERR_HIP;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            done = seq_reached(word, (unsigned)ticket);
            if (!done) return fail(c, OTH_ERR_INTERNAL, "stream idle but the completion word was never written");
        }
    }
    if (ready) *ready = done ? 1 : 0;
    if (!done) return OTH_OK;
    {
        CtxGuard guard_(c);      // (a newer launch may have taken the slot while this thread was polling)
        if (p->out_ticket[slot] != ticket)
            return fail(c, OTH_ERR_STATE, "ticket overwritten while waiting (the ring keeps the last 4 launches)");
        if (psd_out) memcpy(psd_out, p->h_out.get() + (size_t)slot * p->nfft, sizeof(float) * (p->nfft - 2 * p->trim));
    }
    if (nseg_out) *nseg_out = nseg;
    return OTH_OK;
}
}  // namespace

int oth_welch_exec_async(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, uint64_t *ticket_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (!ticket_out) return fail(p->ctx, OTH_ERR_INVALID, "ticket_out is NULL");
    *ticket_out = 0;
    return welch_enqueue(p, iq, nsamples, src_is_device, false, ticket_out);
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_poll(oth_plan *p, uint64_t ticket, float *psd_out, uint64_t *nseg_out, int *ready) {
    OTH_TRY
    if (!p || !ready) return fail(p ? p->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    *ready = 0;
    return welch_collect(p, ticket, psd_out, nseg_out, ready, false);
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_wait(oth_plan *p, uint64_t ticket, float *psd_out, uint64_t *nseg_out) {
    OTH_TRY
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    return welch_collect(p, ticket, psd_out, nseg_out, nullptr, true);
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_exec(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, float *psd_out,
                   uint64_t *nseg_out) {
    OTH_TRY
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (!iq || !psd_out) return fail(p->ctx, OTH_ERR_INVALID, "bad argument");
    uint64_t ticket = 0;
    std::lock_guard<std::mutex> one_at_a_time(p->exec_mu);      // blocking callers of ONE plan, any number of threads
    {
        CtxGuard guard_(p->ctx);
        if (int rc = welch_enqueue(p, iq, nsamples, src_is_device, true, &ticket)) return rc;
    }
    return welch_collect(p, ticket, psd_out, nseg_out, nullptr, true);      // polls outside the context lock
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_partial_dev(oth_plan *p, const void *iq_dev, size_t nsamples, float *sum_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (p->average == OTH_AVERAGE_MEDIAN) return refuse_median(p, "oth_welch_partial_dev");
    oth_ctx *c = p->ctx;
    if (!iq_dev || !sum_out_dev) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (use_device(c)) return OTH_ERR_HIP;
    const Averaged av = run_average(p, (const float2 *)iq_dev, nullptr, nsamples, 1, nsamples);
    if (av.rc) return av.rc;
    FinalizeArgs f = finalize_args(p, av.W, av.layout, 1, raw_stage(p));
    f.out0 = sum_out_dev;
    f.scale = 1.0;
    f.accumulate = 2;      // raw sums, non-finite or not: the rule for them applies where sums are scaled (oth_welch_scale_dev)
    if (int frc = finalize_and_rearm(c, f, 1)) return frc;
    if (nseg_out) *nseg_out = (uint64_t)av.nseg;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_scale_dev(oth_plan *p, const float *sum_dev, uint64_t nseg_total, float *psd_out_dev) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (p->average == OTH_AVERAGE_MEDIAN) return refuse_median(p, "oth_welch_scale_dev");
    oth_ctx *c = p->ctx;
    if (!sum_dev || !psd_out_dev || !nseg_total) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (use_device(c)) return OTH_ERR_HIP;
    HIPCHK(c, launch_scale(sum_dev, psd_out_dev, p->nfft, p->scale / (double)nseg_total, out_stage(p), c->stream));
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_reset(oth_plan *p) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    HIPCHK(c, hipMemsetAsync(p->d_sum.get(), 0, sizeof(float) * p->nfft, c->stream));
    p->nseg_total = 0;
    p->carry = 0;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_accumulate(oth_plan *p, const void *iq_host, size_t nsamples) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (p->average == OTH_AVERAGE_MEDIAN) return refuse_median(p, "oth_welch_accumulate");
    oth_ctx *c = p->ctx;
    if (!iq_host && nsamples) return fail(c, OTH_ERR_INVALID, "iq is NULL");
    if (!nsamples) return OTH_OK;
    if (use_device(c)) return OTH_ERR_HIP;
    const size_t total = p->carry + nsamples;
    int rc = p->d_stream.ensure_keep(c, total * sizeof(float2), p->carry * sizeof(float2));
    if (rc) return rc;
    const bool pinned_src = nsamples * sizeof(float2) > kPinnedStageMax && host_ptr_is_pinned(iq_host);
    if (pinned_src && nsamples * sizeof(float2) > kPinnedRingMax) {
        if ((rc = copy_in_and_wait(c, p->d_stream.get() + p->carry, iq_host, nsamples * sizeof(float2)))) return rc;
    } else if (nsamples * sizeof(float2) > kPinnedStageMax && !pinned_src) {
        // large chunks: the runtime's own staged copy from pageable memory is faster than a host memcpy into a pinned
        // slot (55 against 33 GB/s at 32 MiB); it returns once the caller's buffer has been read.  (A pinned /
        // registered source would be read asynchronously: it takes the ring below whatever its size.)
        HIPCHK(c, hipMemcpyAsync(p->d_stream.get() + p->carry, iq_host, nsamples * sizeof(float2), hipMemcpyHostToDevice,
                                 c->stream));
    } else {
        // the caller's buffer is only valid during the call (sync_block.work contract): through the plan's pinned ring
        if ((rc = ring_upload(p, p->d_stream.get() + p->carry, iq_host, nsamples * sizeof(float2)))) return rc;
    }
    if (total < (size_t)p->nperseg) {
        p->carry = total;
        return OTH_OK;
    }
    const Averaged av = run_average(p, p->d_stream.get(), nullptr, total, 1, total);
    if (av.rc) return av.rc;
    FinalizeArgs f = finalize_args(p, av.W, av.layout, 1, raw_stage(p));
    f.out0 = p->d_sum.get();
    f.scale = 1.0;
    f.accumulate = 1;
    if (int frc = finalize_and_rearm(c, f, 1)) return frc;
    p->nseg_total += (uint64_t)av.nseg;
    // keep the samples the next segment still needs
    const size_t consumed = (size_t)av.nseg * (size_t)p->step;
    const size_t keep = total - consumed;
    if (keep) {
        // regions may overlap when keep > consumed: bounce through the partial-free tail of d_stage
        if (keep <= consumed) {
            HIPCHK(c, hipMemcpyAsync(p->d_stream.get(), p->d_stream.get() + consumed, keep * sizeof(float2),
                                     hipMemcpyDeviceToDevice, c->stream));
        } else {
            if ((rc = p->d_stage.ensure(c, keep * sizeof(float2)))) return rc;
            HIPCHK(c, hipMemcpyAsync(p->d_stage.get(), p->d_stream.get() + consumed, keep * sizeof(float2),
                                     hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(p->d_stream.get(), p->d_stage.get(), keep * sizeof(float2), hipMemcpyDeviceToDevice,
                                     c->stream));
        }
    }
    p->carry = keep;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_finalize(oth_plan *p, float *psd_out, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (p->average == OTH_AVERAGE_MEDIAN) return refuse_median(p, "oth_welch_finalize");
    oth_ctx *c = p->ctx;
    if (!psd_out) return fail(c, OTH_ERR_INVALID, "psd_out is NULL");
    if (!p->nseg_total) return fail(c, OTH_ERR_STATE, "no complete segment accumulated yet");
    if (use_device(c)) return OTH_ERR_HIP;
    int rc = p->d_out.ensure(c, sizeof(float) * 5 * p->nfft);
    if (rc) return rc;
    const OutStage stage = out_stage(p);
    HIPCHK(c, launch_scale(p->d_sum.get(), p->d_out.get(), p->nfft, p->scale / (double)p->nseg_total, stage, c->stream));
    HIPCHK(c, hipMemcpyAsync(psd_out, p->d_out.get(), sizeof(float) * stage.nout, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nseg_out) *nseg_out = p->nseg_total;
    return oth_welch_reset(p);
    OTH_CATCH((p ? p->ctx : nullptr))
}

// Averaging launch + cross-workgroup reduction of the two-channel path.  raw: unscaled sums in natural
// order (no shift / trim), the time-sharded form; else the plan's scale, shift and trim.
static int csd_run(oth_plan *p, const float2 *dx, const float2 *dy, size_t nsamples, bool raw, float *o_xx,
                   float *o_yy, float *o_xy, float *o_c, uint64_t *nseg_out) {
    oth_ctx *c = p->ctx;
    const Averaged av = run_average(p, dx, dy, nsamples, 1, nsamples);
    if (av.rc) return av.rc;
    FinalizeArgs f = finalize_args(p, av.W, av.layout, 4, raw ? raw_stage(p) : out_stage(p));      // (dB: refused by every caller)
    f.out0 = o_xx;
    f.out1 = o_yy;
    f.out2 = o_xy;
    f.out3 = o_c;
    f.scale = raw ? 1.0 : p->scale / (double)av.nseg;
    if (int frc = finalize_and_rearm(c, f, 1)) return frc;
    if (nseg_out) *nseg_out = (uint64_t)av.nseg;
    return OTH_OK;
}

int oth_csd_exec_dev(oth_plan *p, const void *x_dev, const void *y_dev, size_t nsamples, float *pxx_dev,
                     float *pyy_dev, float *pxy_dev, float *cxy_dev, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (p->average == OTH_AVERAGE_MEDIAN) return refuse_median(p, "oth_csd_exec_dev");
    if (int rc = mtm_csd_gate(p, "oth_csd_exec_dev")) return rc;
    oth_ctx *c = p->ctx;
    if (!x_dev || !y_dev) return fail(c, OTH_ERR_INVALID, "x/y is NULL");
    if (p->db) return fail(c, OTH_ERR_UNSUPPORTED, "dB output is not defined for the cross spectrum");
    if (nsamples < (size_t)p->nperseg) return fail(c, OTH_ERR_INVALID, "input shorter than nperseg");
    if (use_device(c)) return OTH_ERR_HIP;
    return csd_run(p, (const float2 *)x_dev, (const float2 *)y_dev, nsamples, false, pxx_dev, pyy_dev, pxy_dev,
                   cxy_dev, nseg_out);
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_csd_partial_dev(oth_plan *p, const void *x_dev, const void *y_dev, size_t nsamples, float *sums_out_dev,
                        uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (p->average == OTH_AVERAGE_MEDIAN) return refuse_median(p, "oth_csd_partial_dev");
    if (int rc = mtm_csd_gate(p, "oth_csd_partial_dev")) return rc;
    oth_ctx *c = p->ctx;
    if (!x_dev || !y_dev || !sums_out_dev) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (p->db) return fail(c, OTH_ERR_UNSUPPORTED, "dB output is not defined for the cross spectrum");
    if (nsamples < (size_t)p->nperseg) return fail(c, OTH_ERR_INVALID, "input shorter than nperseg");
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft;
    return csd_run(p, (const float2 *)x_dev, (const float2 *)y_dev, nsamples, true, sums_out_dev, sums_out_dev + N,
                   sums_out_dev + 2 * N, nullptr, nseg_out);
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_csd_scale_dev(oth_plan *p, const float *sums_dev, uint64_t nseg_total, float *pxx_dev, float *pyy_dev,
                      float *pxy_dev, float *cxy_dev) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (p->average == OTH_AVERAGE_MEDIAN) return refuse_median(p, "oth_csd_scale_dev");
    if (int rc = mtm_csd_gate(p, "oth_csd_scale_dev")) return rc;
    oth_ctx *c = p->ctx;
    if (!sums_dev || !nseg_total) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (p->db) return fail(c, OTH_ERR_UNSUPPORTED, "dB output is not defined for the cross spectrum");
    if (use_device(c)) return OTH_ERR_HIP;
    HIPCHK(c, launch_csd_scale(sums_dev, p->nfft, p->scale / (double)nseg_total, out_stage(p), pxx_dev, pyy_dev, pxy_dev, cxy_dev,
                               c->stream));
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_csd_exec(oth_plan *p, const void *x, const void *y, size_t nsamples, int src_is_device, float *pxx,
                 float *pyy, float *pxy, float *cxy, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (p->average == OTH_AVERAGE_MEDIAN) return refuse_median(p, "oth_csd_exec");
    if (int rc = mtm_csd_gate(p, "oth_csd_exec")) return rc;
    oth_ctx *c = p->ctx;
    if (!x || !y) return fail(c, OTH_ERR_INVALID, "x/y is NULL");
    if (p->db) return fail(c, OTH_ERR_UNSUPPORTED, "dB output is not defined for the cross spectrum");
    if (nsamples < (size_t)p->nperseg) return fail(c, OTH_ERR_INVALID, "input shorter than nperseg");
    if (use_device(c)) return OTH_ERR_HIP;
    const float2 *dx = (const float2 *)x, *dy = (const float2 *)y;
    int rc;
    if (!src_is_device && (rc = stage_host(p, x, y, nsamples, &dx, &dy))) return rc;
    if ((rc = p->d_out.ensure(c, sizeof(float) * 5 * p->nfft))) return rc;
    const int nout = p->nfft - 2 * p->trim;
    float *o0 = p->d_out.get(), *o1 = p->d_out.get() + p->nfft, *o2 = p->d_out.get() + 2 * p->nfft, *o3 = p->d_out.get() + 4 * p->nfft;
    if ((rc = csd_run(p, dx, dy, nsamples, false, o0, o1, o2, o3, nseg_out))) return rc;
    if (pxx) HIPCHK(c, hipMemcpyAsync(pxx, o0, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
    if (pyy) HIPCHK(c, hipMemcpyAsync(pyy, o1, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
    if (pxy) HIPCHK(c, hipMemcpyAsync(pxy, o2, sizeof(float) * 2 * nout, hipMemcpyDeviceToHost, c->stream));
    if (cxy) HIPCHK(c, hipMemcpyAsync(cxy, o3, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

// recipe of the plan's last averaging launch ("" before the first)
int oth__debug_last_recipe(oth_plan *p, char *buf, size_t buflen) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p || !buf || !buflen) return fail(p ? p->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    snprintf(buf, buflen, "%s", p->last_recipe.c_str());
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
