// C ABI, host side: eigenvalues and the principal eigenvector of the spectral matrix or of the coherence matrix of C coherent
// channels on a Welch plan (oth_welch_matrix_eig / _dev) - the checks in the matrix family's order, its averaging launch and
// totals launch (welch_mat_sums, launch_mat_totals: shared with oth_welch_matrix), then mateig.hip's per-bin Jacobi.
#include "abi_stat.h"

namespace {
// Every refusal of the two entry points, in the header's order, before anything is allocated, staged or launched.
int eig_check(oth_plan *p, const void *x, size_t nsamples, int nchan, size_t stride, int of, const float *eig_out, const float *vec_out,
              long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (int rc = welch_stat_plan(p, "the eigenvalues of the spectral matrix")) return rc;
    if (nchan < 2 || nchan > kMatChanMax) return fail(c, OTH_ERR_INVALID, "nchan must lie in 2 ... " + std::to_string(kMatChanMax));
    if (of != OTH_EIG_OF_S && of != OTH_EIG_OF_G) return fail(c, OTH_ERR_INVALID, "of must be OTH_EIG_OF_S or OTH_EIG_OF_G");
    if (!x) return fail(c, OTH_ERR_INVALID, "the input is NULL");
    if (!eig_out && !vec_out) return fail(c, OTH_ERR_INVALID, "eig_out and vec_out are both NULL");
    if (stride < nsamples) return fail(c, OTH_ERR_INVALID, "chan_stride < nsamples");
    return stream_shape(p, true, nsamples, nchan, stride, nullptr, nseg_out);
}

// after eig_check: device in, device out
int eig_run(oth_plan *p, const float2 *x, long long nseg, int nchan, size_t stride, int of, float *eig_out, float *vec_out) {
    oth_ctx *c = p->ctx;
    MatFinalizeArgs f{};
    std::string recipe;
    if (int rc = welch_mat_sums(p, x, nseg, nchan, stride, f, recipe)) return rc;
    MatEigArgs e{};
    e.totals = f.totals;
    e.eig_out = eig_out;
    e.vec_out = vec_out;
    e.s_scale = f.s_scale;
    e.of = of;
    e.nchan = nchan;
    e.nfft = f.nfft;
    e.out = f.out;
    TIMED_LAUNCH(c, launch_mat_totals(f, c->stream));
    TIMED_LAUNCH(c, launch_mat_eig(welch_mat_capacity(nchan), e, c->stream));
    p->last_recipe = recipe + (of == OTH_EIG_OF_G ? " eig=G" : " eig=S") + (vec_out ? " vec=1" : "");
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_welch_matrix_eig_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nchan, size_t chan_stride, int of, float *eig_out_dev,
                             float *vec_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out, [&](long long *nseg) { return eig_check(p, iq_dev, nsamples, nchan, chan_stride, of, eig_out_dev, vec_out_dev, nseg); },
        [&](long long nseg) { return eig_run(p, (const float2 *)iq_dev, nseg, nchan, chan_stride, of, eig_out_dev, vec_out_dev); });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_matrix_eig(oth_plan *p, const void *iq, size_t nsamples, int nchan, int src_is_device, int of, float *eig_out, float *vec_out,
                         uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = eig_check(p, iq, nsamples, nchan, nsamples, of, eig_out, vec_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim);
    const HostRow rows[] = {{eig_out, (size_t)nchan * nout}, {vec_out, 2 * (size_t)nchan * nout}};
    // the channels lie one behind the other: staged as one block of nchan nsamples
    return host_form(p, iq, nullptr, (size_t)nchan * nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) { return eig_run(p, dx, nseg, nchan, nsamples, of, dev[0], dev[1]); });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
