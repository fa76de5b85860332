// C ABI, host side: cyclic autocorrelation of a Welch plan (oth_welch_set_lags, oth_welch_caf / _dev) - the lag table, the
// checks, the (W, nstreams, groups) launch of welchlag.hip and its finalize launch into the caf rows and r.
#include "abi_stat.h"

namespace {
// What kind of plan takes lags: shared by set_lags and the exec entry points, in the header's order.
int lag_plan_check(oth_plan *p) { return welch_stat_plan(p, "the cyclic autocorrelation"); }

// Every refusal of the two exec entry points, before anything is allocated, staged or launched.  The segments are counted on
// nsamples - T, T the largest lag: every lagged sample a segment reads then lies inside the stream's own nsamples.
int lag_check(oth_plan *p, const void *x, size_t nsamples, int nstreams, size_t stride, const float *caf_out, long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (int rc = lag_plan_check(p)) return rc;
    if (!p->nlags) return fail(c, OTH_ERR_UNSUPPORTED, "the cyclic autocorrelation needs its lags: call oth_welch_set_lags on this plan");
    const std::string too_short =
        "input shorter than the largest lag + nperseg (" + std::to_string(p->lag_max) + " + " + std::to_string(p->nperseg) + " samples)";
    return stream_shape(p, x && caf_out, nsamples, nstreams, stride, "the cyclic autocorrelation takes at most 65535 streams per launch", nseg_out,
                        (size_t)p->lag_max, too_short.c_str());
}

// Lags per workgroup: welchlag.hip's two builds (GL = 1, 2).  The grouped build loads the base segment once for two lags; the
// transforms per lag - what the launch spends its time on - are the same, so all it can save is one 8-byte read per sample
// out of L2.  It pays in registers (at 4096 points two workgroups per CU against four; at 16384 points its sums live in
// memory), and the partial rows the finalize launch reads grow with GL.  Measured (profiles/welch_caf_ab.txt, DESIGN.md 4.16;
// ms of GL = 2 over GL = 1, 64 streams of 8 segments / one capture of 2^24 samples, L = 2, 4, 5, 16):
//   256 points     x1.03 ... 1.26 / x0.99 ... 1.66        1024 points    x0.98 ... 1.13 / x0.97 ... 1.19
//   4096 points    x1.07 ... 1.24 / x1.13 ... 1.39        8192 points    x0.97 ... 1.03 / x0.99 ... 1.19
//   16384 points   x1.04 ... 1.12 / x1.09 ... 1.29
// and a GL = 4 build, measured in an earlier session next to these two and not shipped, read x0.98 ... 1.59
// (profiles/welch_caf_ab_three_builds.txt).  The grouped builds are ahead nowhere by more than 3 % and behind by up to 66 %, so the library runs GL = 1 at every size
// and L; GL = 2 stays for OTH_LAG_GROUP.  64, 128, 512 and 2048 points were not measured and go with their neighbours.
int lag_group(const oth_plan *p) {
    if (p->tune_lag_group == 1 || p->tune_lag_group == kLagGroup) return p->tune_lag_group;
    return 1;
}

// after lag_check: device in, device out
int lag_run(oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, float *caf_out, float *r_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft, L = p->nlags;
    const int gl = lag_group(p), G = (L + gl - 1) / gl;
    // whole segments go to W workgroups per stream and group in contiguous runs: what the device holds at once, a segment at least
    const int bpc = std::max(1, welch_lag_blocks_per_cu(N, gl));
    const int W = segment_workgroups(c, nseg, 1, (long long)nstreams * G, bpc);
    const size_t slots = (size_t)nstreams * G * W;
    if (int rc = p->d_partial.ensure(c, sizeof(float) * slots * gl * N)) return rc;
    if (int rc = p->d_lag_means.ensure(c, sizeof(double) * slots * gl * 2)) return rc;
    WelchLagArgs a = welch_stat_args<WelchLagArgs>(p, x, nseg, nstreams, stride, W);
    a.lags = p->d_lags.get();
    a.means = p->d_lag_means.get();
    a.nlags = L;
    LagFinalizeArgs f{};
    f.partial = p->d_partial.get();
    f.means = p->d_lag_means.get();
    f.caf_out = caf_out;
    f.r_out = r_out;
    f.scale = p->scale / (double)nseg;
    f.inv_m = 1.0 / (double)nseg;
    f.W = W;
    f.G = G;
    f.gl = gl;
    f.nlags = L;
    f.nfft = N;
    f.out = out_stage(p);
    TIMED_LAUNCH(c, launch_welch_lag(N, gl, G, a, c->stream));
    TIMED_LAUNCH(c, launch_lag_finalize(f, nstreams, c->stream));
    p->last_recipe = stat_recipe("welchlag", p, "", W, nseg, nstreams, " nlags=" + std::to_string(L) + " group=" + std::to_string(gl), bpc);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_welch_set_lags(oth_plan *p, int nlags, const int *lags) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    oth_ctx *c = p->ctx;
    if (int rc = lag_plan_check(p)) return rc;
    if (nlags < 1 || nlags > kLagMax) return fail(c, OTH_ERR_INVALID, "nlags must lie in 1 ... " + std::to_string(kLagMax));
    if (!lags) return fail(c, OTH_ERR_INVALID, "lags is NULL");
    int top = 0;
    for (int l = 0; l < nlags; ++l) {
        if (lags[l] < 0 || lags[l] > kLagTauMax) return fail(c, OTH_ERR_INVALID, "every lag must lie in 0 ... " + std::to_string(kLagTauMax) + " samples");
        top = std::max(top, lags[l]);
    }
    DevBuf<int> tab;
    if (int rc = upload_tables(c, "oth_welch_set_lags", [&] { return tab.upload(c, lags, sizeof(int) * nlags); })) return rc;
    p->d_lags = std::move(tab);
    p->nlags = nlags;
    p->lag_max = top;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_caf_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, float *caf_out_dev,
                      float *r_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out, [&](long long *nseg) { return lag_check(p, iq_dev, nsamples, nstreams, stream_stride, caf_out_dev, nseg); },
        [&](long long nseg) { return lag_run(p, (const float2 *)iq_dev, nseg, nstreams, stream_stride, caf_out_dev, r_out_dev); });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_caf(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, float *caf_out, float *r_out, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = lag_check(p, iq, nsamples, 1, nsamples, caf_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim);
    const HostRow rows[] = {{caf_out, (size_t)p->nlags * nout}, {r_out, 2 * (size_t)p->nlags}};      // [L][nout] caf, [L] r pairs
    return host_form(p, iq, nullptr, nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) { return lag_run(p, dx, nseg, 1, nsamples, dev[0], dev[1]); });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
