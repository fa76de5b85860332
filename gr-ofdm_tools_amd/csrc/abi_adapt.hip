// C ABI, host side: Thomson's adaptive-weight multitaper PSD with per-bin degrees of freedom (oth_mtm_set_ratios,
// oth_mtm_adaptive / _dev) on any plan of oth_mtm_plan / oth_mtm_csd_plan - the checks, the segment-per-workgroup launch
// of mtmadapt.hip and its finalize launch into the two output rows.
#include "abi_state.h"

namespace {
// Every refusal of the entry points, before anything is allocated, staged or launched.
int adapt_check(oth_plan *p, const void *x, size_t nsamples, int nstreams, size_t stride, int iters, const float *psd_out) {
    oth_ctx *c = p->ctx;
    if (!p->ntapers)
        return fail(c, OTH_ERR_UNSUPPORTED, "the adaptive estimate needs a multitaper plan (oth_mtm_plan): this plan has no tapers");
    if (p->ntapers < 2) return fail(c, OTH_ERR_UNSUPPORTED, "the adaptive estimate needs at least two tapers");
    if (!p->d_mtm_lam)
        return fail(c, OTH_ERR_UNSUPPORTED, "the adaptive estimate needs the tapers' concentration ratios: call oth_mtm_set_ratios on this plan");
    if (!x || !psd_out || nstreams < 1) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (iters < 1 || iters > 64) return fail(c, OTH_ERR_INVALID, "need 1 <= iters <= 64");
    if (nstreams > 1 && stride < nsamples) return fail(c, OTH_ERR_INVALID, "stream_stride < nsamples");
    if (nsamples < (size_t)p->nperseg) return fail(c, OTH_ERR_INVALID, "input shorter than nperseg");
    if (nstreams > 65535) return fail(c, OTH_ERR_UNSUPPORTED, "multitaper plans take at most 65535 streams per launch");
    return OTH_OK;
}

// after adapt_check: psd_out / dof_out are device memory (dof_out may be null)
int adapt_run(oth_plan *p, const float2 *x, size_t nsamples, int nstreams, size_t stride, int iters, float *psd_out, float *dof_out,
              uint64_t *nseg_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft, K = p->ntapers;
    const long long nseg = (long long)((nsamples - (size_t)p->noverlap) / (size_t)p->step);
    // whole segments go to W workgroups per stream in contiguous runs: what the device holds at once, a segment at least
    const int bpc = std::max(1, mtm_adapt_blocks_per_cu(N, K));
    const long long resident = (long long)c->cu_count * bpc;
    const int W = (int)std::min(nseg, std::max<long long>(1, resident / nstreams));
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
    f.fftshift = p->fftshift;
    f.trim = p->trim;
    f.db = p->db;
    f.nout = N - 2 * p->trim;
    {
        Timed tm(c);
        HIPCHK(c, launch_mtm_adapt(N, g, c->stream));
    }
    {
        Timed tm(c);
        HIPCHK(c, launch_adapt_finalize(f, nstreams, c->stream));
    }
    p->last_recipe = "kernel=mtmadapt nfft=" + std::to_string(N) + " ntapers=" + std::to_string(K) + " iters=" + std::to_string(iters) +
                     " W=" + std::to_string(W) + " nseg=" + std::to_string(nseg) + " nstreams=" + std::to_string(nstreams) +
                     " bpc=" + std::to_string(bpc);
    if (nseg_out) *nseg_out = (uint64_t)nseg;
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
    if (use_device(c)) return OTH_ERR_HIP;
    // a fresh table takes the place of an earlier one only when it is complete: launches queued on the old one drain first
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DevBuf<float> fresh;
    hipError_t e = fresh.upload(c, tab.data(), sizeof(float) * tab.size());
    const hipError_t es = hipStreamSynchronize(c->stream);      // also after a failure: the host table dies here
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string("oth_mtm_set_ratios: ") + hipGetErrorString(e));
    p->d_mtm_lam = std::move(fresh);
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_mtm_adaptive_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, int iters,
                         float *psd_out_dev, float *dof_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    if (int rc = adapt_check(p, iq_dev, nsamples, nstreams, stream_stride, iters, psd_out_dev)) return rc;
    return adapt_run(p, (const float2 *)iq_dev, nsamples, nstreams, stream_stride, iters, psd_out_dev, dof_out_dev, nseg_out);
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_mtm_adaptive(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, int iters, float *psd_out, float *dof_out,
                     uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    oth_ctx *c = p->ctx;
    if (int rc = adapt_check(p, iq, nsamples, 1, nsamples, iters, psd_out)) return rc;      // refused before anything is staged
    if (use_device(c)) return OTH_ERR_HIP;
    const float2 *dx = (const float2 *)iq;
    int rc;
    if (!src_is_device) {
        if ((rc = p->d_stage.ensure(c, nsamples * sizeof(float2)))) return rc;
        HIPCHK(c, hipMemcpyAsync(p->d_stage.get(), iq, nsamples * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        dx = p->d_stage.get();
    }
    if ((rc = p->d_out.ensure(c, sizeof(float) * 5 * p->nfft))) return rc;
    const int N = p->nfft, nout = N - 2 * p->trim;
    float *o = p->d_out.get();
    if ((rc = adapt_run(p, dx, nsamples, 1, nsamples, iters, o, dof_out ? o + N : nullptr, nseg_out))) return rc;
    HIPCHK(c, hipMemcpyAsync(psd_out, o, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
    if (dof_out) HIPCHK(c, hipMemcpyAsync(dof_out, o + N, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
