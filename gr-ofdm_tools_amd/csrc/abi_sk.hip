// C ABI, host side: spectral kurtosis of a Welch plan (oth_welch_sk / _dev) - the checks, the segment-per-workgroup launch
// of welchsk.hip and its finalize launch into the SK row and, where asked for, the PSD row.
#include "abi_stat.h"

namespace {
// Every refusal of the two entry points, in the header's order, before anything is allocated, staged or launched.
int sk_check(oth_plan *p, const void *x, size_t nsamples, int nstreams, size_t stride, const float *sk_out, long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (int rc = welch_stat_plan(p, "the spectral kurtosis", "periodograms", "its PSD row is the mean")) return rc;
    if (int rc = stream_shape(p, x && sk_out, nsamples, nstreams, stride, "the spectral kurtosis takes at most 65535 streams per launch", nseg_out))
        return rc;
    if (*nseg_out < 2) return fail(c, OTH_ERR_INVALID, "the spectral kurtosis needs at least two segments: this input holds one");
    return OTH_OK;
}

// after sk_check: device in, device out
int sk_run(oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, float *sk_out, float *psd_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft;
    // whole segments go to W workgroups per stream in contiguous runs: what the device holds at once, a segment at least
    const int bpc = std::max(1, welch_sk_blocks_per_cu(N));
    const int W = segment_workgroups(c, nseg, 1, nstreams, bpc);
    if (int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)nstreams * W * 2 * N)) return rc;
    WelchSkArgs a = welch_stat_args<WelchSkArgs>(p, x, nseg, nstreams, stride, W);
    a.g = (float)p->sk_g;
    SkFinalizeArgs f{};
    f.partial = p->d_partial.get();
    f.sk_out = sk_out;
    f.psd_out = psd_out;
    f.m = (double)nseg;
    f.mp1_over_mm1 = ((double)nseg + 1.0) / ((double)nseg - 1.0);
    f.psd_scale = p->scale / ((double)a.g * (double)nseg);      // the float the kernel multiplied by: it cancels
    f.W = W;
    f.nfft = N;
    f.out = out_stage(p);
    TIMED_LAUNCH(c, launch_welch_sk(N, a, c->stream));
    TIMED_LAUNCH(c, launch_sk_finalize(f, nstreams, c->stream));
    p->last_recipe = stat_recipe("welchsk", p, "", W, nseg, nstreams, "", bpc);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_welch_sk_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, float *sk_out_dev,
                     float *psd_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out, [&](long long *nseg) { return sk_check(p, iq_dev, nsamples, nstreams, stream_stride, sk_out_dev, nseg); },
        [&](long long nseg) { return sk_run(p, (const float2 *)iq_dev, nseg, nstreams, stream_stride, sk_out_dev, psd_out_dev); });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_sk(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, float *sk_out, float *psd_out, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = sk_check(p, iq, nsamples, 1, nsamples, sk_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim);
    const HostRow rows[] = {{sk_out, nout}, {psd_out, nout}};
    return host_form(p, iq, nullptr, nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) { return sk_run(p, dx, nseg, 1, nsamples, dev[0], dev[1]); });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
