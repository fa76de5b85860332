// C ABI, host side: Bartlett, Capon and MUSIC direction spectra of the spectral matrix or of the coherence matrix of C
// coherent channels on a Welch plan (oth_welch_set_steering, oth_welch_matrix_doa / _dev) - the steering table, the checks in
// the matrix family's order, its averaging launch and totals launch (welch_mat_sums, launch_mat_totals: shared with
// oth_welch_matrix), mateig.hip's basis build, then matdoa.hip's per-bin, per-direction stage.
#include "abi_stat.h"

namespace {
constexpr const char *kDoaWhat = "the direction spectra of the spectral matrix";

// Every refusal of the two entry points, in the header's order, before anything is allocated, staged or launched.
int doa_check(oth_plan *p, const void *x, size_t nsamples, int nchan, size_t stride, int of, int nsrc, double loading, const float *bartlett,
              const float *capon, const float *music, long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (int rc = welch_stat_plan(p, kDoaWhat)) return rc;
    if (nchan < 2 || nchan > kMatChanMax) return fail(c, OTH_ERR_INVALID, "nchan must lie in 2 ... " + std::to_string(kMatChanMax));
    if (of != OTH_EIG_OF_S && of != OTH_EIG_OF_G) return fail(c, OTH_ERR_INVALID, "of must be OTH_EIG_OF_S or OTH_EIG_OF_G");
    if (!x) return fail(c, OTH_ERR_INVALID, "the input is NULL");
    if (!bartlett && !capon && !music) return fail(c, OTH_ERR_INVALID, "bartlett_out, capon_out and music_out are all NULL");
    if (!p->doa_ndir)
        return fail(c, OTH_ERR_UNSUPPORTED, "the direction spectra need a steering table: call oth_welch_set_steering on this plan");
    if (nchan != p->doa_nchan)
        return fail(c, OTH_ERR_INVALID, "nchan is " + std::to_string(nchan) + " and the steering table holds " + std::to_string(p->doa_nchan) + " channels");
    if (music && (nsrc < 1 || nsrc > nchan - 1)) return fail(c, OTH_ERR_INVALID, "nsrc must lie in 1 ... nchan - 1 for the MUSIC spectrum");
    if (!std::isfinite(loading) || loading < 0.0) return fail(c, OTH_ERR_INVALID, "loading must be finite and >= 0");
    if (stride < nsamples) return fail(c, OTH_ERR_INVALID, "chan_stride < nsamples");
    return stream_shape(p, true, nsamples, nchan, stride, nullptr, nseg_out);
}

// after doa_check: device in, device out
int doa_run(oth_plan *p, const float2 *x, long long nseg, int nchan, size_t stride, int of, int nsrc, double loading, float *bartlett,
            float *capon, float *music) {
    oth_ctx *c = p->ctx;
    MatFinalizeArgs f{};
    std::string recipe;
    if (int rc = welch_mat_sums(p, x, nseg, nchan, stride, f, recipe)) return rc;
    const int cc = welch_mat_capacity(nchan);
    if (int rc = p->d_doa_basis.ensure(c, sizeof(double) * mat_eig_basis_entries(cc) * (size_t)f.nfft)) return rc;
    MatEigArgs e{};
    e.totals = f.totals;
    e.s_scale = f.s_scale;
    e.of = of;
    e.nchan = nchan;
    e.nfft = f.nfft;
    e.out = f.out;
    MatDoaArgs d{};
    d.basis = p->d_doa_basis.get();
    d.tau = p->d_doa_steer.get();
    d.frac = d.tau + (size_t)p->doa_ndir * nchan;
    d.bartlett_out = bartlett;
    d.capon_out = capon;
    d.music_out = music;
    d.loading = loading;
    d.nsrc = music ? nsrc : nchan;
    d.ndir = p->doa_ndir;
    d.nchan = nchan;
    d.nfft = f.nfft;
    d.out = f.out;
    TIMED_LAUNCH(c, launch_mat_totals(f, c->stream));
    TIMED_LAUNCH(c, launch_mat_eig_basis(cc, e, p->d_doa_basis.get(), c->stream));
    TIMED_LAUNCH(c, launch_mat_doa(cc, d, c->stream));
    p->last_recipe = recipe + (of == OTH_EIG_OF_G ? " doa=G" : " doa=S") + " ndir=" + std::to_string(p->doa_ndir);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_welch_set_steering(oth_plan *p, int ndir, int nchan, const double *delays, double fc) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    oth_ctx *c = p->ctx;
    if (int rc = welch_stat_plan(p, kDoaWhat)) return rc;
    if (ndir == 0) {      // launches queued on the table drain first
        if (use_device(c)) return OTH_ERR_HIP;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        p->d_doa_steer.reset();
        p->doa_ndir = p->doa_nchan = 0;
        return OTH_OK;
    }
    if (ndir < 1 || ndir > kDoaDirsMax) return fail(c, OTH_ERR_INVALID, "ndir must lie in 0 ... " + std::to_string(kDoaDirsMax));
    if (nchan < 2 || nchan > kMatChanMax) return fail(c, OTH_ERR_INVALID, "nchan must lie in 2 ... " + std::to_string(kMatChanMax));
    if (!delays) return fail(c, OTH_ERR_INVALID, "delays is NULL");
    if (!std::isfinite(fc)) return fail(c, OTH_ERR_INVALID, "fc must be finite");
    const size_t count = (size_t)ndir * nchan;
    std::vector<double> tab(2 * count);      // tau, then frac(fc tau)
    for (size_t j = 0; j < count; ++j) {
        const double tau = delays[j], cycles = fc * tau;
        if (!std::isfinite(tau) || !std::isfinite(cycles)) return fail(c, OTH_ERR_INVALID, "every delay, and fc times it, must be finite");
        tab[j] = tau;
        // fc tau may be 10^6 cycles: the whole cycles come off the rounded product, then the product's own rounding error goes back in
        tab[count + j] = (cycles - std::nearbyint(cycles)) + std::fma(fc, tau, -cycles);
    }
    DevBuf<double> dev;
    if (int rc = upload_tables(c, "oth_welch_set_steering", [&] { return dev.upload(c, tab.data(), sizeof(double) * tab.size()); })) return rc;
    p->d_doa_steer = std::move(dev);
    p->doa_ndir = ndir;
    p->doa_nchan = nchan;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_matrix_doa_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nchan, size_t chan_stride, int of, int nsrc, double loading,
                             float *bartlett_out_dev, float *capon_out_dev, float *music_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out,
        [&](long long *nseg) {
            return doa_check(p, iq_dev, nsamples, nchan, chan_stride, of, nsrc, loading, bartlett_out_dev, capon_out_dev, music_out_dev, nseg);
        },
        [&](long long nseg) {
            return doa_run(p, (const float2 *)iq_dev, nseg, nchan, chan_stride, of, nsrc, loading, bartlett_out_dev, capon_out_dev, music_out_dev);
        });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_matrix_doa(oth_plan *p, const void *iq, size_t nsamples, int nchan, int src_is_device, int of, int nsrc, double loading,
                         float *bartlett_out, float *capon_out, float *music_out, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = doa_check(p, iq, nsamples, nchan, nsamples, of, nsrc, loading, bartlett_out, capon_out, music_out, &nseg)) return rc;
    const size_t row = (size_t)p->doa_ndir * (size_t)(p->nfft - 2 * p->trim);
    // a row that is not asked for takes no room on the device either: at 1024 directions of 16384 bins one is 64 MiB
    const HostRow rows[] = {{bartlett_out, bartlett_out ? row : 0}, {capon_out, capon_out ? row : 0}, {music_out, music_out ? row : 0}};
    // the channels lie one behind the other: staged as one block of nchan nsamples
    return host_form(p, iq, nullptr, (size_t)nchan * nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) {
                         return doa_run(p, dx, nseg, nchan, nsamples, of, nsrc, loading, dev[0], dev[1], dev[2]);
                     });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
