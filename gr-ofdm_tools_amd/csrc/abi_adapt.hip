// C ABI, host side: Thomson's adaptive-weight multitaper PSD with per-bin degrees of freedom (oth_mtm_set_ratios,
// oth_mtm_adaptive / _dev) on any plan of oth_mtm_plan / oth_mtm_csd_plan - the checks, the segment-per-workgroup launch
// of mtmadapt.hip and its finalize launch into the two output rows.
#include "abi_stat.h"

namespace {
// Every refusal of the entry points, before anything is allocated, staged or launched.
int adapt_check(oth_plan *p, const void *x, size_t nsamples, int nstreams, size_t stride, int iters, const float *psd_out,
                long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (!p->ntapers)
        return fail(c, OTH_ERR_UNSUPPORTED, "the adaptive estimate needs a multitaper plan (oth_mtm_plan): this plan has no tapers");
    if (p->ntapers < 2) return fail(c, OTH_ERR_UNSUPPORTED, "the adaptive estimate needs at least two tapers");
    if (!p->d_mtm_lam)
        return fail(c, OTH_ERR_UNSUPPORTED, "the adaptive estimate needs the tapers' concentration ratios: call oth_mtm_set_ratios on this plan");
    if (!x || !psd_out || nstreams < 1) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (iters < 1 || iters > 64) return fail(c, OTH_ERR_INVALID, "need 1 <= iters <= 64");
    return stream_shape(p, true, nsamples, nstreams, stride, kMtmTooMany, nseg_out);      // (iters goes before the stride)
}

// after adapt_check: psd_out / dof_out are device memory (dof_out may be null)
int adapt_run(oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, int iters, float *psd_out, float *dof_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft, K = p->ntapers;
    // whole segments go to W workgroups per stream in contiguous runs: what the device holds at once, a segment at least
    const int bpc = std::max(1, mtm_adapt_blocks_per_cu(N, K));
    const int W = segment_workgroups(c, nseg, 1, nstreams, bpc);
    int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)nstreams * W * 2 * N);
    const size_t ws_floats = mtm_adapt_ws_floats(N, K);
    if (!rc && ws_floats) rc = p->d_adapt_ws.ensure(c, sizeof(float) * (size_t)nstreams * W * ws_floats);
    if (rc) return rc;
    MtmAdaptArgs g{};
    g.m = mtm_args(p, x, nseg, nstreams, stride, W);
    g.lam = p->d_mtm_lam.get();
    g.ws = ws_floats ? p->d_adapt_ws.get() : nullptr;
    g.iters = iters;
    AdaptFinalizeArgs f{};
    f.partial = p->d_partial.get();
    f.psd_out = psd_out;
    f.dof_out = dof_out;
    f.psd_scale = p->scale / (double)nseg;
    f.inv_nseg = 1.0 / (double)nseg;
    f.W = W;
    f.nfft = N;
    f.out = out_stage(p);
    TIMED_LAUNCH(c, launch_mtm_adapt(N, g, c->stream));
    TIMED_LAUNCH(c, launch_adapt_finalize(f, nstreams, c->stream));
    p->last_recipe = stat_recipe("mtmadapt", p, " ntapers=" + std::to_string(K) + " iters=" + std::to_string(iters), W, nseg, nstreams, "", bpc);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_mtm_set_ratios(oth_plan *p, const double *ratios) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    oth_ctx *c = p->ctx;
    if (!p->ntapers) return fail(c, OTH_ERR_UNSUPPORTED, "concentration ratios belong to a multitaper plan (oth_mtm_plan): this plan has no tapers");
    if (!ratios) return fail(c, OTH_ERR_INVALID, "ratios is NULL");
    const int K = p->ntapers;
    std::vector<float> tab(3 * (size_t)K);
    for (int k = 0; k < K; ++k) {
        const double l = ratios[k];
        if (!(l > 0.0 && l <= 1.0)) return fail(c, OTH_ERR_INVALID, "every concentration ratio must lie in (0, 1]");
        tab[k] = (float)l;
        tab[K + k] = (float)std::max(1.0 - l, 0.0);      // in double: 1 - lambda_0 is 3e-10 at NW 4, below float's spacing at 1
        tab[2 * (size_t)K + k] = p->mtm_inv_g[k];
    }
    DevBuf<float> fresh;
    if (int rc = upload_tables(c, "oth_mtm_set_ratios", [&] { return fresh.upload(c, tab.data(), sizeof(float) * tab.size()); })) return rc;
    p->d_mtm_lam = std::move(fresh);
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_mtm_adaptive_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, int iters,
                         float *psd_out_dev, float *dof_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out, [&](long long *nseg) { return adapt_check(p, iq_dev, nsamples, nstreams, stream_stride, iters, psd_out_dev, nseg); },
        [&](long long nseg) { return adapt_run(p, (const float2 *)iq_dev, nseg, nstreams, stream_stride, iters, psd_out_dev, dof_out_dev); });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_mtm_adaptive(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, int iters, float *psd_out, float *dof_out,
                     uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = adapt_check(p, iq, nsamples, 1, nsamples, iters, psd_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim);
    const HostRow rows[] = {{psd_out, nout}, {dof_out, nout}};
    return host_form(p, iq, nullptr, nsamples, src_is_device, rows, nseg, nseg_out, [&](const float2 *dx, const float2 *, float *const *dev) {
        return adapt_run(p, dx, nseg, 1, nsamples, iters, dev[0], dev[1]);
    });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
