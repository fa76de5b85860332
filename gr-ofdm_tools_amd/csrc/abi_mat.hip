// C ABI, host side: spectral matrix and generalized coherence of C coherent channels on a Welch plan (oth_welch_matrix /
// _dev) - the checks, the segment-per-workgroup launch of welchmat.hip at the channel capacity that takes nchan, and its two
// finalize launches into the packed matrix rows and the gcoh row.
#include "abi_stat.h"

namespace oth {
// The averaging launch of the matrix family after its check (oth_welch_matrix*, oth_welch_matrix_eig*): the workspaces, the
// segment-per-workgroup launch of welchmat.hip at the channel capacity that takes nchan, the arguments of the finalize
// launches (rows left NULL for the caller) and the recipe text.
int welch_mat_sums(oth_plan *p, const float2 *x, long long nseg, int nchan, size_t stride, MatFinalizeArgs &f, std::string &recipe) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft, C = nchan, cc = welch_mat_capacity(C);
    // whole segments (all channels of each) go to W workgroups in contiguous runs: what the device holds at once, a segment at least
    const int bpc = std::max(1, welch_mat_blocks_per_cu(N, cc));
    const int W = segment_workgroups(c, nseg, 1, 1, bpc);
    if (int rc = p->d_partial.ensure(c, sizeof(float) * (size_t)W * C * C * N)) return rc;
    if (int rc = p->d_mat_totals.ensure(c, sizeof(double) * (size_t)C * C * N)) return rc;
    const size_t pts = welch_mat_ws_points(N, cc);
    if (pts)
        if (int rc = p->d_mat_ws.ensure(c, sizeof(float2) * (size_t)W * C * pts)) return rc;
    WelchMatArgs a{};
    a.x = x;
    a.win = p->d_win.get();
    a.tw = p->d_tw;
    a.partial = p->d_partial.get();
    a.ws = p->d_mat_ws.get();
    a.nseg = nseg;
    a.chan_stride = stride;
    a.nperseg = p->nperseg;
    a.step = p->step;
    a.detrend = p->detrend != OTH_DETREND_NONE;
    a.wg_count = W;
    a.nchan = C;
    f = MatFinalizeArgs{};
    f.partial = p->d_partial.get();
    f.totals = p->d_mat_totals.get();
    f.s_scale = p->scale / (double)nseg;
    f.W = W;
    f.nchan = C;
    f.nfft = N;
    f.out = out_stage(p);
    TIMED_LAUNCH(c, launch_welch_mat(N, cc, a, c->stream));
    recipe = stat_recipe("welchmat", p, "", W, nseg, 1,
                         " nchan=" + std::to_string(C) + " cap=" + std::to_string(cc) + (pts ? " state=rows" : " state=regs"), bpc);
    return OTH_OK;
}
}  // namespace oth

namespace {
// Every refusal of the two entry points, in the header's order, before anything is allocated, staged or launched.
int mat_check(oth_plan *p, const void *x, size_t nsamples, int nchan, size_t stride, const float *s_out, const float *gcoh_out,
              long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (int rc = welch_stat_plan(p, "the spectral matrix")) return rc;
    if (nchan < 2 || nchan > kMatChanMax) return fail(c, OTH_ERR_INVALID, "nchan must lie in 2 ... " + std::to_string(kMatChanMax));
    if (!x) return fail(c, OTH_ERR_INVALID, "the input is NULL");
    if (!s_out && !gcoh_out) return fail(c, OTH_ERR_INVALID, "s_out and gcoh_out are both NULL");
    if (stride < nsamples) return fail(c, OTH_ERR_INVALID, "chan_stride < nsamples");
    return stream_shape(p, true, nsamples, nchan, stride, nullptr, nseg_out);
}

// after mat_check: device in, device out
int mat_run(oth_plan *p, const float2 *x, long long nseg, int nchan, size_t stride, float *s_out, float *gcoh_out) {
    oth_ctx *c = p->ctx;
    MatFinalizeArgs f{};
    std::string recipe;
    if (int rc = welch_mat_sums(p, x, nseg, nchan, stride, f, recipe)) return rc;
    f.s_out = s_out;
    f.gcoh_out = gcoh_out;
    TIMED_LAUNCH(c, launch_mat_finalize(f, c->stream));
    p->last_recipe = recipe;
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_welch_matrix_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nchan, size_t chan_stride, float *s_out_dev,
                         float *gcoh_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out, [&](long long *nseg) { return mat_check(p, iq_dev, nsamples, nchan, chan_stride, s_out_dev, gcoh_out_dev, nseg); },
        [&](long long nseg) { return mat_run(p, (const float2 *)iq_dev, nseg, nchan, chan_stride, s_out_dev, gcoh_out_dev); });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_matrix(oth_plan *p, const void *iq, size_t nsamples, int nchan, int src_is_device, float *s_out, float *gcoh_out,
                     uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = mat_check(p, iq, nsamples, nchan, nsamples, s_out, gcoh_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim), pairs = (size_t)nchan * (nchan + 1) / 2;
    const HostRow rows[] = {{s_out, 2 * pairs * nout}, {gcoh_out, nout}};
    // the channels lie one behind the other: staged as one block of nchan nsamples
    return host_form(p, iq, nullptr, (size_t)nchan * nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) { return mat_run(p, dx, nseg, nchan, nsamples, dev[0], dev[1]); });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
