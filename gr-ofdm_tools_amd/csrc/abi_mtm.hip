// C ABI, host side: multitaper (Thomson) PSD plans - the Slepian tapers (oth_dpss: host only, double), the plan
// (oth_mtm_plan: an ordinary oth_plan whose averaging launch is mtm.hip's taper loop; oth_mtm_csd_plan: the same plan with
// the two-channel calls open, on mtmcsd.hip) and that launch (mtm_run, which run_average branches to before any routing).
#include "abi_stat.h"

namespace {
// ---- Slepian tapers ---------------------------------------------------------------------------------------------------------
// The symmetric tridiagonal matrix that commutes with the sinc kernel (Slepian 1978): diagonal d, off-diagonal e.  Its
// eigenvalues are simple and - at the top, where the tapers live - far apart, so each wanted pair comes from a Sturm
// bisection (the eigenvalue to an ulp of the matrix norm) and inverse iteration (the vector), n operations a step.

// eigenvalues below x: the negative terms of the Sturm sequence q_i = d_i - x - e_{i-1}^2 / q_{i-1}
int sturm_below(const std::vector<double> &d, const std::vector<double> &e2, double x, double tiny) {
    int count = 0;
    double q = 1.0;
    for (size_t i = 0; i < d.size(); ++i) {
        q = d[i] - x - (i ? e2[i - 1] / q : 0.0);
        if (std::fabs(q) < tiny) q = -tiny;
        if (q < 0.0) ++count;
    }
    return count;
}

// the eigenvalue of ascending index j
double bisect_eigenvalue(const std::vector<double> &d, const std::vector<double> &e2, int j, double lo, double hi, double tiny) {
    for (int it = 0; it < 400; ++it) {
        const double mid = lo + 0.5 * (hi - lo);
        if (!(mid > lo && mid < hi)) break;
        if (sturm_below(d, e2, mid, tiny) >= j + 1) hi = mid;
        else lo = mid;
    }
    return lo + 0.5 * (hi - lo);
}

// LU with partial pivoting of the tridiagonal T - lambda I (LAPACK's dgttrf / dgttrs shape), then inverse iteration from a
// fixed pseudo-random start; v comes back with unit L2 norm.  The matrix is persymmetric, so the vector of order k is even
// (k even) or odd about the middle: every iterate is projected onto that symmetry and taken off the k vectors already
// found (`found`, [k][n]): at n = 16384 the vectors of plain inverse iteration were orthogonal to 2e-10 only, with the two
// projections the Gram matrix is within 2e-14 of the identity (LAPACK's: 5e-15).
void inverse_iteration(const std::vector<double> &d, const std::vector<double> &e, double lambda, double norm, const double *found,
                       int k, std::vector<double> &v) {
    const int n = (int)d.size();
    std::vector<double> dl(e), dd(n), du(e), du2(n > 2 ? n - 2 : 0, 0.0);
    std::vector<char> piv(n > 1 ? n - 1 : 0, 0);
    for (int i = 0; i < n; ++i) dd[i] = d[i] - lambda;
    const double floor_ = norm * 2.220446049250313e-16;
    for (int i = 0; i < n - 1; ++i) {
        if (std::fabs(dd[i]) >= std::fabs(dl[i])) {
            if (std::fabs(dd[i]) < floor_) dd[i] = floor_;
            const double m = dl[i] / dd[i];
            dl[i] = m;
            dd[i + 1] -= m * du[i];
        } else {                                  // rows i and i + 1 change places
            const double m = dd[i] / dl[i];
            dd[i] = dl[i];
            dl[i] = m;
            const double t = du[i];
            du[i] = dd[i + 1];
            dd[i + 1] = t - m * dd[i + 1];
            if (i < n - 2) {
                du2[i] = du[i + 1];
                du[i + 1] = -m * du[i + 1];
            }
            piv[i] = 1;
        }
    }
    if (std::fabs(dd[n - 1]) < floor_) dd[n - 1] = floor_;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    v.resize(n);
    for (int i = 0; i < n; ++i) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        v[i] = 0.5 + (double)(rng >> 11) * (1.0 / 9007199254740992.0);      // (0.5, 1.5): no symmetry of its own
    }
    for (int it = 0; it < 5; ++it) {
        for (int i = 0; i < n - 1; ++i) {
            if (piv[i]) {
                const double t = v[i] - dl[i] * v[i + 1];
                v[i] = v[i + 1];
                v[i + 1] = t;
            } else {
                v[i + 1] -= dl[i] * v[i];
            }
        }
        v[n - 1] /= dd[n - 1];
        if (n > 1) v[n - 2] = (v[n - 2] - du[n - 2] * v[n - 1]) / dd[n - 2];
        for (int i = n - 3; i >= 0; --i) v[i] = (v[i] - du[i] * v[i + 1] - du2[i] * v[i + 2]) / dd[i];
        double big = 0.0;
        for (int i = 0; i < n; ++i) big = std::max(big, std::fabs(v[i]));
        for (int i = 0; i < n; ++i) v[i] /= big;      // (the solve of a nearly singular system is huge: scale before squaring)
        const double sgn = (k & 1) ? -1.0 : 1.0;
        for (int i = 0; i < (n + 1) / 2; ++i) {
            const double a = 0.5 * (v[i] + sgn * v[n - 1 - i]);
            v[i] = a;
            v[n - 1 - i] = sgn * a;
        }
        for (int j = k & 1; j < k; j += 2) {          // the other parity is orthogonal already
            const double *u = found + (size_t)j * n;
            double dot = 0.0;
            for (int i = 0; i < n; ++i) dot += v[i] * u[i];
            for (int i = 0; i < n; ++i) v[i] -= dot * u[i];
        }
        double s2 = 0.0;
        for (int i = 0; i < n; ++i) s2 += v[i] * v[i];
        const double inv = 1.0 / std::sqrt(s2);
        for (int i = 0; i < n; ++i) v[i] *= inv;
    }
}

// sum_{m,n} v[m] A[m - n] v[n] = A[0] r[0] + 2 sum_{d >= 1} A[d] r[d] with the autocorrelation r of v through one
// zero-padded transform (|V|^2 is real and even, so its forward transform is M r)
double concentration(const std::vector<double> &v, double W) {
    const int n = (int)v.size();
    size_t M = 2;
    while (M < 2 * (size_t)n) M <<= 1;
    std::vector<double> re(M, 0.0), im(M, 0.0);
    for (int i = 0; i < n; ++i) re[i] = v[i];
    host_fft_pow2(re, im);
    std::vector<double> pr(M), pi(M, 0.0);      // (squared in place, the -O3 host build lost the loop between the two calls)
    for (size_t i = 0; i < M; ++i) pr[i] = re[i] * re[i] + im[i] * im[i];
    host_fft_pow2(pr, pi);
    re.swap(pr);
    double acc = 0.0;
    for (int dgt = n - 1; dgt >= 1; --dgt)
        acc += std::sin(2.0 * M_PI * W * (double)dgt) / (M_PI * (double)dgt) * (re[dgt] / (double)M);
    return 2.0 * W * (re[0] / (double)M) + 2.0 * acc;
}

}  // namespace

namespace oth {
int refuse_mtm(oth_plan *p, const char *what, const char *why) {
    return fail(p->ctx, OTH_ERR_UNSUPPORTED, std::string(what) + " is not available on a multitaper plan: " + why);
}

int mtm_csd_gate(oth_plan *p, const char *what) {
    if (!p->ntapers || p->mtm_csd) return OTH_OK;
    return refuse_mtm(p, what, "the taper loop holds one channel");
}

MtmArgs mtm_args(const oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, int W) {
    MtmArgs a{};
    a.x = x;
    a.tapers = p->d_tapers.get();
    a.coef = p->d_coef.get();
    a.tw = p->d_tw;
    a.partial = p->d_partial.get();
    a.nseg = nseg;
    a.stream_stride = stride;
    a.nperseg = p->nperseg;
    a.step = p->step;
    a.detrend = p->detrend != OTH_DETREND_NONE;
    a.ntapers = p->ntapers;
    a.wg_per_stream = W;
    a.nstreams = nstreams;
    return a;
}

int mtm_run(oth_plan *p, const float2 *x, const float2 *y, long long nseg, int nstreams, size_t stride, int *W_out) {
    oth_ctx *c = p->ctx;
    const int N = p->nfft, K = p->ntapers;
    const bool csd = y != nullptr;
    const int nch = csd ? 4 : 1;
    if (nstreams > 65535) return fail(c, OTH_ERR_UNSUPPORTED, kMtmTooMany);
    // the (segment, taper) items of a stream go to W workgroups in contiguous runs: one workgroup per taper at least (a
    // single segment spreads over K of them), and for long launches what the device holds at once
    const int bpc = std::max(1, csd ? mtmcsd_blocks_per_cu(N) : mtm_blocks_per_cu(N));
    const int W = segment_workgroups(c, nseg * K, K, nstreams, bpc);
    int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)nstreams * W * nch * N);
    {
        const int groups = std::max(kReduceGroups, finalize_row_groups(N, W, nch));
        if (!rc) rc = p->d_reduce.ensure(c, sizeof(float) * (size_t)nstreams * groups * nch * N);
    }
    const size_t ws_points = csd ? mtmcsd_ws_points(N) : 0;
    if (!rc && ws_points) rc = p->d_mtm_ws.ensure(c, sizeof(float2) * (size_t)nstreams * W * ws_points);
    if (rc) return rc;
    MtmCsdArgs g{};
    MtmArgs &a = g.m;
    a = mtm_args(p, x, nseg, nstreams, stride, W);
    g.y = y;
    g.ws = ws_points ? p->d_mtm_ws.get() : nullptr;
    TIMED_LAUNCH(c, csd ? launch_mtmcsd(N, g, c->stream) : launch_mtm(N, a, c->stream));
    p->last_recipe = stat_recipe(csd ? "mtmcsd" : "mtm", p, " ntapers=" + std::to_string(K), W, nseg, nstreams, "", bpc);
    *W_out = W;
    return OTH_OK;
}
}  // namespace oth

namespace {
// oth_mtm_plan and oth_mtm_csd_plan inside their barrier and context lock: one body; two_channel opens the oth_csd_* calls on
// the plan (oth_plan::mtm_csd)
int mtm_plan_create(oth_ctx *c, int nfft, int nperseg, int noverlap, int ntapers, const float *tapers, const float *weights,
                    int detrend, int scaling, double fs, int fftshift, int trim_bins, bool two_channel, oth_plan **out) {
    if (!c || !out) return fail(c, OTH_ERR_INVALID, "ctx/out is NULL");
    *out = nullptr;
    // the refusals of its own in front of the shared checks (OTH_SCALE_SPECTRUM before the range check of plan_begin)
    if (nfft >= 1 && !stat_size(nfft))
        return fail(c, OTH_ERR_UNSUPPORTED, "multitaper plans take a transform length that is a power of two from 64 to 16384, not " +
                                                std::to_string(nfft));
    if (scaling == OTH_SCALE_SPECTRUM)
        return fail(c, OTH_ERR_UNSUPPORTED, "OTH_SCALE_SPECTRUM is not defined for multitaper plans: an odd taper sums to zero");
    std::unique_ptr<oth_plan> p;
    if (int rc = plan_begin(c, nfft, nperseg, noverlap, detrend, scaling, fs, fftshift, trim_bins, &p)) return rc;
    p->fast_detrend = false;      // every mode: each segment's own mean
    if (ntapers < 1 || ntapers > 64) return fail(c, OTH_ERR_INVALID, "need 1 <= ntapers <= 64");
    if (!tapers) return fail(c, OTH_ERR_INVALID, "tapers is NULL");
    double wsum = 0.0;
    for (int k = 0; k < ntapers; ++k) {
        const double w = weights ? (double)weights[k] : 1.0;
        if (!std::isfinite(w) || w < 0.0) return fail(c, OTH_ERR_INVALID, "weights must be finite and non-negative");
        wsum += w;
    }
    if (!(wsum > 0.0) || !std::isfinite(wsum)) return fail(c, OTH_ERR_INVALID, "weights must have a positive sum");
    std::vector<float> tab((size_t)ntapers * nfft, 0.f), coef(ntapers);      // zero-extended: the kernel indexes [0, nfft)
    std::vector<float> usum(ntapers);                                        // U_k, the F-test's (oth_mtm_ftest_dev)
    std::vector<float> inv_g(ntapers);                                       // 1 / g_k, the adaptive weighting's (oth_mtm_adaptive_dev)
    double usq = 0.0;
    for (int k = 0; k < ntapers; ++k) {
        double s2 = 0.0, s1 = 0.0;
        for (int i = 0; i < nperseg; ++i) {
            const float t = tapers[(size_t)k * nperseg + i];
            if (!std::isfinite(t)) return fail(c, OTH_ERR_INVALID, "taper values must be finite");
            tab[(size_t)k * nfft + i] = t;
            s2 += (double)t * (double)t;
            s1 += (double)t;
        }
        usum[k] = (float)s1;
        inv_g[k] = s2 > 0.0 ? (float)(1.0 / s2) : 0.f;
        usq += (double)usum[k] * (double)usum[k];
        double ck = (weights ? (double)weights[k] : 1.0) / wsum;
        if (scaling == OTH_SCALE_DENSITY) {
            if (!(s2 > 0.0)) return fail(c, OTH_ERR_INVALID, "taper " + std::to_string(k) + " is all zero");
            ck /= s2;
        }
        coef[k] = (float)ck;
    }
    p->ntapers = ntapers;
    p->mtm_csd = two_channel;
    for (int k = 1; weights && k < ntapers; ++k) p->mtm_uniform = p->mtm_uniform && weights[k] == weights[0];
    p->mtm_s = std::isfinite(usq) ? usq : 0.0;
    p->mtm_inv_g = std::move(inv_g);
    switch (scaling) {
        case OTH_SCALE_DENSITY: p->scale = 1.0 / fs; break;      // the tapers' energies are in c_k
        case OTH_SCALE_OVER_N2: p->scale = 1.0 / ((double)nfft * (double)nfft); break;
        default: p->scale = 1.0;
    }
    if (int rc = get_twiddles(c, nfft, &p->d_tw)) return rc;
    hipError_t e = p->d_tapers.upload(c, tab.data(), sizeof(float) * tab.size());
    if (e == hipSuccess) e = p->d_coef.upload(c, coef.data(), sizeof(float) * coef.size());
    if (e == hipSuccess) e = p->d_mtm_u.upload(c, usum.data(), sizeof(float) * usum.size());
    if (e == hipSuccess) e = p->d_sum.alloc(sizeof(float) * nfft);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_sum.get(), 0, sizeof(float) * nfft, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);      // also after a failure: the host tables die here
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string("plan setup: ") + hipGetErrorString(e));
    *out = p.release();
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_dpss(int n, double nw, int kmax, double *tapers, double *ratios) {
    OTH_TRY
    if (n < 2 || !(nw > 0.0) || !(nw < 0.5 * (double)n) || kmax < 1 || kmax > n || !tapers)
        return fail(nullptr, OTH_ERR_INVALID, "oth_dpss: need n >= 2, 0 < nw < n / 2, 1 <= kmax <= n and a tapers buffer");
    const double W = nw / (double)n;
    std::vector<double> d(n), e(n - 1), e2(n - 1);
    const double cw = std::cos(2.0 * M_PI * W);
    for (int i = 0; i < n; ++i) {
        const double h = 0.5 * (double)(n - 1 - 2 * i);
        d[i] = h * h * cw;
    }
    for (int i = 1; i < n; ++i) {
        e[i - 1] = 0.5 * (double)i * (double)(n - i);
        e2[i - 1] = e[i - 1] * e[i - 1];
    }
    double lo = d[0], hi = d[0], norm = 0.0;      // Gershgorin
    for (int i = 0; i < n; ++i) {
        const double r = (i ? e[i - 1] : 0.0) + (i < n - 1 ? e[i] : 0.0);
        lo = std::min(lo, d[i] - r);
        hi = std::max(hi, d[i] + r);
        norm = std::max(norm, std::fabs(d[i]) + r);
    }
    const double tiny = norm * 1e-300 + 1e-300;
    const double thresh = std::max(1e-7, 1.0 / (double)n);
    std::vector<double> v;
    for (int k = 0; k < kmax; ++k) {
        const double lambda = bisect_eigenvalue(d, e2, n - 1 - k, lo, hi, tiny);
        inverse_iteration(d, e, lambda, norm, tapers, k, v);
        // SciPy's signs: even orders sum to a positive value; odd orders start (first entry whose square exceeds
        // max(1e-7, 1 / n)) with a positive lobe
        bool flip = false;
        if (k % 2 == 0) {
            double s = 0.0;
            for (int i = 0; i < n; ++i) s += v[i];
            flip = s < 0.0;
        } else {
            for (int i = 0; i < n; ++i)
                if (v[i] * v[i] > thresh) {
                    flip = v[i] < 0.0;
                    break;
                }
        }
        double *out = tapers + (size_t)k * n;
        for (int i = 0; i < n; ++i) out[i] = flip ? -v[i] : v[i];
        if (ratios) ratios[k] = concentration(v, W);
    }
    return OTH_OK;
    OTH_CATCH((oth_ctx *)nullptr)
}

int oth_mtm_plan(oth_ctx *c, int nfft, int nperseg, int noverlap, int ntapers, const float *tapers, const float *weights,
                 int detrend, int scaling, double fs, int fftshift, int trim_bins, oth_plan **out) {
    OTH_TRY
    CtxGuard guard_(c);
    return mtm_plan_create(c, nfft, nperseg, noverlap, ntapers, tapers, weights, detrend, scaling, fs, fftshift, trim_bins, false, out);
    OTH_CATCH(c)
}

int oth_mtm_csd_plan(oth_ctx *c, int nfft, int nperseg, int noverlap, int ntapers, const float *tapers, const float *weights,
                     int detrend, int scaling, double fs, int fftshift, int trim_bins, oth_plan **out) {
    OTH_TRY
    CtxGuard guard_(c);
    return mtm_plan_create(c, nfft, nperseg, noverlap, ntapers, tapers, weights, detrend, scaling, fs, fftshift, trim_bins, true, out);
    OTH_CATCH(c)
}
}  // extern "C"
