// C ABI, host side: polyphase filter-bank (WOLA) PSD of a Welch plan (oth_welch_set_prototype, oth_welch_pfb / _dev) - the
// prototype's tables and sums, the checks, the frame-per-workgroup launch of welchpfb.hip and the finalize launch into the row.
#include "abi_stat.h"

namespace {
// What kind of plan takes a prototype: shared by set_prototype and the run entry points, in the header's order.
int pfb_plan_check(oth_plan *p) {
    if (int rc = welch_stat_plan(p, "the filter-bank PSD")) return rc;
    if (p->nperseg != p->nfft)
        return fail(p->ctx, OTH_ERR_UNSUPPORTED, "the filter-bank PSD folds whole transform lengths: it takes a plan with nperseg == nfft, not " +
                                                     std::to_string(p->nperseg) + " and " + std::to_string(p->nfft));
    return OTH_OK;
}

// Every refusal of the two run entry points, before anything is allocated, staged or launched.  The frames are counted with a
// reach of (P - 1) nfft samples behind the plan's segment: M = (nsamples - P nfft) / step + 1, and every sample a frame reads
// lies inside the stream's own nsamples.
int pfb_check(oth_plan *p, const void *x, size_t nsamples, int nstreams, size_t stride, const float *pfb_out, long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (int rc = pfb_plan_check(p)) return rc;
    if (!p->pfb_taps) return fail(c, OTH_ERR_UNSUPPORTED, "the filter-bank PSD needs its prototype: call oth_welch_set_prototype on this plan");
    const std::string too_short = "input shorter than ntaps * nfft (" + std::to_string(p->pfb_taps) + " * " + std::to_string(p->nfft) + " samples)";
    return stream_shape(p, x && pfb_out, nsamples, nstreams, stride, "the filter-bank PSD takes at most 65535 streams per launch", nseg_out,
                        (size_t)(p->pfb_taps - 1) * (size_t)p->nfft, too_short.c_str());
}

// after pfb_check: device in, device out
int pfb_run(oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, float *pfb_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft;
    // whole frames go to W workgroups per stream in contiguous runs: what the device holds at once, a frame at least
    const int bpc = std::max(1, welch_pfb_blocks_per_cu(N));
    const int W = segment_workgroups(c, nseg, 1, nstreams, bpc);
    if (int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)nstreams * W * N)) return rc;
    WelchPfbArgs a = welch_stat_args<WelchPfbArgs>(p, x, nseg, nstreams, stride, W);
    a.win = p->d_pfb_h.get();      // the prototype in the window's place
    a.hfold = p->d_pfb_fold.get();
    a.ntaps = p->pfb_taps;
    // welchlag.hip's finalize launch on one lag, one group and one row per workgroup: partial[stream][wg][nfft], no means
    LagFinalizeArgs f{};
    f.partial = p->d_partial.get();
    f.caf_out = pfb_out;
    f.scale = p->pfb_scale / (double)nseg;
    f.W = W;
    f.G = 1;
    f.gl = 1;
    f.nlags = 1;
    f.nfft = N;
    f.out = out_stage(p);
    TIMED_LAUNCH(c, launch_welch_pfb(N, a, c->stream));
    TIMED_LAUNCH(c, launch_lag_finalize(f, nstreams, c->stream));
    p->last_recipe = stat_recipe("welchpfb", p, " ntaps=" + std::to_string(p->pfb_taps), W, nseg, nstreams, "", bpc);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_welch_set_prototype(oth_plan *p, int ntaps, const float *h) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    oth_ctx *c = p->ctx;
    if (int rc = pfb_plan_check(p)) return rc;
    if (ntaps < kPfbTapsMin || ntaps > kPfbTapsMax)
        return fail(c, OTH_ERR_INVALID, "ntaps must lie in " + std::to_string(kPfbTapsMin) + " ... " + std::to_string(kPfbTapsMax));
    if (!h) return fail(c, OTH_ERR_INVALID, "h is NULL");
    const size_t N = (size_t)p->nfft, L = (size_t)ntaps * N;
    double s1 = 0.0, s2 = 0.0;
    for (size_t i = 0; i < L; ++i) {
        if (!std::isfinite(h[i])) return fail(c, OTH_ERR_INVALID, "every tap of the prototype must be finite");
        s1 += (double)h[i];
        s2 += (double)h[i] * (double)h[i];
    }
    if (!(s2 > 0.0)) return fail(c, OTH_ERR_INVALID, "the prototype is all zero");
    if (p->scaling == OTH_SCALE_SPECTRUM && s1 == 0.0)
        return fail(c, OTH_ERR_INVALID, "OTH_SCALE_SPECTRUM needs a prototype with a non-zero sum");
    std::vector<float> fold(N);
    for (size_t n = 0; n < N; ++n) {
        double t = 0.0;
        for (int t0 = 0; t0 < ntaps; ++t0) t += (double)h[n + (size_t)t0 * N];
        fold[n] = (float)t;
    }
    DevBuf<float> taps, folded;
    if (int rc = upload_tables(c, "oth_welch_set_prototype", [&] {
            const hipError_t e = taps.upload(c, h, sizeof(float) * L);
            return e != hipSuccess ? e : folded.upload(c, fold.data(), sizeof(float) * N);
        }))
        return rc;
    p->d_pfb_h = std::move(taps);
    p->d_pfb_fold = std::move(folded);
    p->pfb_taps = ntaps;
    p->pfb_sum = s1;
    p->pfb_sum2 = s2;
    switch (p->scaling) {      // the plan's scaling with h in the window's place
        case OTH_SCALE_DENSITY: p->pfb_scale = 1.0 / (p->fs * s2); break;
        case OTH_SCALE_OVER_N2: p->pfb_scale = 1.0 / ((double)N * (double)N); break;
        case OTH_SCALE_SPECTRUM: p->pfb_scale = 1.0 / (s1 * s1); break;
        default: p->pfb_scale = 1.0;
    }
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_pfb_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, float *pfb_out_dev,
                      uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out, [&](long long *nseg) { return pfb_check(p, iq_dev, nsamples, nstreams, stream_stride, pfb_out_dev, nseg); },
        [&](long long nseg) { return pfb_run(p, (const float2 *)iq_dev, nseg, nstreams, stream_stride, pfb_out_dev); });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_pfb(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, float *pfb_out, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = pfb_check(p, iq, nsamples, 1, nsamples, pfb_out, &nseg)) return rc;
    const HostRow rows[] = {{pfb_out, (size_t)(p->nfft - 2 * p->trim)}};
    return host_form(p, iq, nullptr, nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) { return pfb_run(p, dx, nseg, 1, nsamples, dev[0]); });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
