// C ABI, host side: Thomson's harmonic F-test (oth_mtm_ftest / _dev) on any plan of oth_mtm_plan / oth_mtm_csd_plan - the
// checks, the segment-per-workgroup launch of mtmftest.hip and its finalize launch into the three output rows.
#include "abi_stat.h"

namespace {
// Every refusal of the two entry points, before anything is allocated, staged or launched.
int ftest_check(oth_plan *p, const void *x, size_t nsamples, int nstreams, size_t stride, const float *f_out, long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (!p->ntapers) return fail(c, OTH_ERR_UNSUPPORTED, "the harmonic F-test needs a multitaper plan (oth_mtm_plan): this plan has no tapers");
    if (p->ntapers < 2) return fail(c, OTH_ERR_UNSUPPORTED, "the harmonic F-test needs at least two tapers");
    if (!(p->mtm_s > 0.0)) return fail(c, OTH_ERR_UNSUPPORTED, "the harmonic F-test needs tapers with a non-zero sum: every U_k of this plan is zero");
    return stream_shape(p, x && f_out, nsamples, nstreams, stride, kMtmTooMany, nseg_out);
}

// after ftest_check: device in, device out (line / resid may be null)
int ftest_run(oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, float *f_out, float *line_out, float *resid_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft, K = p->ntapers;
    // whole segments go to W workgroups per stream in contiguous runs: what the device holds at once, a segment at least
    const int bpc = std::max(1, mtm_ftest_blocks_per_cu(N));
    const int W = segment_workgroups(c, nseg, 1, nstreams, bpc);
    int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)nstreams * W * 2 * N);
    const size_t ws_floats = mtm_ftest_ws_floats(N);
    if (!rc && ws_floats) rc = p->d_ftest_ws.ensure(c, sizeof(float) * (size_t)nstreams * W * ws_floats);
    if (rc) return rc;
    MtmFtestArgs g{};
    g.m = mtm_args(p, x, nseg, nstreams, stride, W);
    g.u = p->d_mtm_u.get();
    g.inv_s = (float)(1.0 / p->mtm_s);
    g.ws = ws_floats ? p->d_ftest_ws.get() : nullptr;
    FtestFinalizeArgs f{};
    f.partial = p->d_partial.get();
    f.f_out = f_out;
    f.line_out = line_out;
    f.resid_out = resid_out;
    f.km1 = (double)(K - 1);
    f.line_scale = 1.0 / (p->mtm_s * (double)nseg);
    f.resid_scale = p->scale / ((double)(K - 1) * (double)nseg);
    f.W = W;
    f.nfft = N;
    f.out = out_stage(p);
    TIMED_LAUNCH(c, launch_mtm_ftest(N, g, c->stream));
    TIMED_LAUNCH(c, launch_ftest_finalize(f, nstreams, c->stream));
    p->last_recipe = stat_recipe("mtmftest", p, " ntapers=" + std::to_string(K), W, nseg, nstreams, "", bpc);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_mtm_ftest_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, float *f_out_dev,
                      float *line_out_dev, float *resid_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(p, nseg_out, [&](long long *nseg) { return ftest_check(p, iq_dev, nsamples, nstreams, stream_stride, f_out_dev, nseg); },
                    [&](long long nseg) {
                        return ftest_run(p, (const float2 *)iq_dev, nseg, nstreams, stream_stride, f_out_dev, line_out_dev, resid_out_dev);
                    });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_mtm_ftest(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, float *f_out, float *line_out, float *resid_out,
                  uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (!iq || !f_out) return fail(p->ctx, OTH_ERR_INVALID, "bad argument");      // this form: in front of the plan's refusals
    long long nseg = 0;
    if (int rc = ftest_check(p, iq, nsamples, 1, nsamples, f_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim);
    const HostRow rows[] = {{f_out, nout}, {line_out, nout}, {resid_out, nout}};
    return host_form(p, iq, nullptr, nsamples, src_is_device, rows, nseg, nseg_out, [&](const float2 *dx, const float2 *, float *const *dev) {
        return ftest_run(p, dx, nseg, 1, nsamples, dev[0], dev[1], dev[2]);
    });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
