// C ABI, host side: the jackknife over the (segment, taper) items of a multitaper plan (oth_mtm_jackknife / _dev: ln PSD;
// oth_mtm_csd_jackknife / _dev: the coherence's z = atanh|gamma| and ln PSD of both channels) - the checks, the first pass
// (the plan's own averaging launch, mtm_run, and its reduction, launch_finalize, into the totals buffer), the second pass
// on mtmjack.hip and its finalize launch.
//
// The optional PSD row of the one-channel form is a second finalize launch of the first pass with the plan's scale, shift,
// trim and dB: the launch oth_welch_exec_dev makes, on the same partial rows, so the same bits.  From the float32 totals
// the row would be rounded twice.  The Cxy row does not depend on the scale: the reduction that leaves the totals forms
// it from its double sums in natural order, and the jackknife's finalize launch moves it to the plan's shift and trim.
#include "abi_stat.h"

namespace {
// Every refusal of the entry points, in the header's order, before anything is allocated, staged or launched.  `two`: the
// two-channel forms (y and the mtm_csd_gate checked too, three items at least instead of two).
int jack_check(oth_plan *p, bool two, const void *x, const void *y, size_t nsamples, int nstreams, size_t stride, const float *need_out,
               long long *nseg_out) {
    oth_ctx *c = p->ctx;
    const char *what = two ? "the coherence jackknife" : "the jackknife";
    if (!p->ntapers)
        return fail(c, OTH_ERR_UNSUPPORTED, std::string(what) + " needs a multitaper plan (oth_mtm_plan): this plan has no tapers");
    if (two)
        if (int rc = mtm_csd_gate(p, "oth_mtm_csd_jackknife")) return rc;
    if (!p->mtm_uniform)
        return fail(c, OTH_ERR_UNSUPPORTED, std::string(what) + " needs exchangeable items: the weights of this plan are not all equal");
    if (nstreams > 65535) return fail(c, OTH_ERR_UNSUPPORTED, kMtmTooMany);      // (in front of "bad argument" here)
    if (int rc = stream_shape(p, x && (!two || y) && need_out, nsamples, nstreams, stride, nullptr, nseg_out)) return rc;
    const long long items = *nseg_out * p->ntapers, min_items = two ? 3 : 2;
    if (items < min_items)
        return fail(c, OTH_ERR_INVALID, std::string(what) + " needs at least " + std::to_string(min_items) +
                                            " (segment, taper) items: this input holds " + std::to_string(items));
    return OTH_OK;
}

// the reduction of the first pass: W1 natural-order partial rows per stream (mtm_run) through launch_finalize, raw sums
FinalizeArgs pass1_finalize(const oth_plan *p, int W1, int nch) {
    FinalizeArgs f = finalize_args(p, W1, ROW_NATURAL, nch, raw_stage(p));
    f.scale = 1.0;
    if (nch == 1) f.accumulate = 2;      // raw totals as they are (the two-channel form has its own store, csd_store)
    return f;
}

// after jack_check: device in, device out
int jack_run(oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, float *lnsd_out, float *psd_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft;
    // every buffer of both passes is sized before the first launch: ensure() drains the stream when it has to replace one,
    // and between the passes that would make the asynchronous forms wait
    const int bpc = std::max(1, mtm_jack_blocks_per_cu(N));
    const int W = segment_workgroups(c, nseg * p->ntapers, p->ntapers, nstreams, bpc);      // the items as mtm_run splits them
    if (int rc = p->d_jack_tot.ensure(c, sizeof(float) * (size_t)nstreams * N)) return rc;
    if (int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)nstreams * W * 2 * N)) return rc;
    int W1 = 0;
    if (int rc = mtm_run(p, x, nullptr, nseg, nstreams, stride, &W1)) return rc;
    FinalizeArgs f = pass1_finalize(p, W1, 1);
    f.out0 = p->d_jack_tot.get();
    HIPCHK(c, launch_finalize(f, nstreams, c->stream));
    if (psd_out) {      // oth_welch_exec_dev's finalize launch
        f.out0 = psd_out;
        f.scale = p->scale / (double)nseg;
        f.out = out_stage(p);
        f.accumulate = 0;      // the plan's scaled output
        HIPCHK(c, launch_finalize(f, nstreams, c->stream));
    }
    MtmJackArgs a{};
    a.m = mtm_args(p, x, nseg, nstreams, stride, W);
    a.totals = p->d_jack_tot.get();
    const double m = (double)(nseg * p->ntapers);
    JackFinalizeArgs j{};
    j.partial = p->d_partial.get();
    j.sd_out[0] = lnsd_out;
    j.m = m;
    j.mm1_over_m = (m - 1.0) / m;
    j.npairs = 1;
    j.W = W;
    j.nfft = N;
    j.out = out_stage(p);
    TIMED_LAUNCH(c, launch_mtm_jack(N, a, c->stream));
    TIMED_LAUNCH(c, launch_jack_finalize(j, nstreams, c->stream));
    p->last_recipe = stat_recipe("mtmjack", p, " ntapers=" + std::to_string(p->ntapers), W, nseg, nstreams, "", bpc);
    return OTH_OK;
}

int jackcsd_run(oth_plan *p, const float2 *x, const float2 *y, size_t nsamples, long long nseg, float *cxy_out, float *zsd_out,
                float *lnsdx_out, float *lnsdy_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft;
    const int bpc = std::max(1, mtmcsd_jack_blocks_per_cu(N));      // (both passes' buffers before the first launch, as jack_run)
    const int W = segment_workgroups(c, nseg * p->ntapers, p->ntapers, 1, bpc);
    const size_t ws_points = mtmcsd_jack_ws_points(N);
    if (int rc = p->d_jack_tot.ensure(c, sizeof(float) * 5 * (size_t)N)) return rc;
    if (int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)W * 6 * N)) return rc;
    if (ws_points)
        if (int rc = p->d_mtm_ws.ensure(c, sizeof(float2) * (size_t)W * ws_points)) return rc;
    int W1 = 0;
    if (int rc = mtm_run(p, x, y, nseg, 1, nsamples, &W1)) return rc;
    float *tot = p->d_jack_tot.get();
    FinalizeArgs f = pass1_finalize(p, W1, 4);
    f.out0 = tot;
    f.out1 = tot + N;
    f.out2 = tot + 2 * N;
    f.out3 = tot + 4 * N;
    HIPCHK(c, launch_finalize(f, 1, c->stream));
    MtmCsdJackArgs a{};
    a.c.m = mtm_args(p, x, nseg, 1, nsamples, W);
    a.c.y = y;
    a.c.ws = ws_points ? p->d_mtm_ws.get() : nullptr;
    a.totals = tot;
    const double m = (double)(nseg * p->ntapers);
    JackFinalizeArgs j{};
    j.partial = p->d_partial.get();
    j.sd_out[0] = lnsdx_out;
    j.sd_out[1] = lnsdy_out;
    j.sd_out[2] = zsd_out;
    j.cxy_nat = tot + 4 * N;
    j.cxy_out = cxy_out;
    j.m = m;
    j.mm1_over_m = (m - 1.0) / m;
    j.npairs = 3;
    j.W = W;
    j.nfft = N;
    j.out = out_stage(p);
    TIMED_LAUNCH(c, launch_mtmcsd_jack(N, a, c->stream));
    TIMED_LAUNCH(c, launch_jack_finalize(j, 1, c->stream));
    p->last_recipe = stat_recipe("mtmcsdjack", p, " ntapers=" + std::to_string(p->ntapers), W, nseg, 1, "", bpc);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_mtm_jackknife_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, float *lnsd_out_dev,
                          float *psd_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out, [&](long long *nseg) { return jack_check(p, false, iq_dev, nullptr, nsamples, nstreams, stream_stride, lnsd_out_dev, nseg); },
        [&](long long nseg) { return jack_run(p, (const float2 *)iq_dev, nseg, nstreams, stream_stride, lnsd_out_dev, psd_out_dev); });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_mtm_jackknife(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, float *lnsd_out, float *psd_out, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = jack_check(p, false, iq, nullptr, nsamples, 1, nsamples, lnsd_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim);
    const HostRow rows[] = {{lnsd_out, nout}, {psd_out, nout}};
    return host_form(p, iq, nullptr, nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) { return jack_run(p, dx, nseg, 1, nsamples, dev[0], dev[1]); });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_mtm_csd_jackknife_dev(oth_plan *p, const void *x_dev, const void *y_dev, size_t nsamples, float *cxy_out_dev, float *zsd_out_dev,
                              float *lnsdx_out_dev, float *lnsdy_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(p, nseg_out, [&](long long *nseg) { return jack_check(p, true, x_dev, y_dev, nsamples, 1, nsamples, zsd_out_dev, nseg); },
                    [&](long long nseg) {
                        return jackcsd_run(p, (const float2 *)x_dev, (const float2 *)y_dev, nsamples, nseg, cxy_out_dev, zsd_out_dev,
                                           lnsdx_out_dev, lnsdy_out_dev);
                    });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_mtm_csd_jackknife(oth_plan *p, const void *x, const void *y, size_t nsamples, int src_is_device, float *cxy_out, float *zsd_out,
                          float *lnsdx_out, float *lnsdy_out, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = jack_check(p, true, x, y, nsamples, 1, nsamples, zsd_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim);
    const HostRow rows[] = {{cxy_out, nout}, {zsd_out, nout}, {lnsdx_out, nout}, {lnsdy_out, nout}};
    return host_form(p, x, y, nsamples, src_is_device, rows, nseg, nseg_out, [&](const float2 *dx, const float2 *dy, float *const *dev) {
        return jackcsd_run(p, dx, dy, nsamples, nseg, dev[0], dev[1], dev[2], dev[3]);
    });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
