// C ABI, host side: generalized cross-correlation and the delay of every channel pair of C coherent channels on a Welch plan
// (oth_welch_matrix_gcc / _dev) - the checks in the matrix family's order, its averaging launch and totals launch
// (welch_mat_sums, launch_mat_totals: shared with oth_welch_matrix, here over every bin whatever the plan trims), then
// matgcc.hip's weighting, inverse transform and peak, one workgroup per pair.
#include "abi_stat.h"

namespace {
const char *const kGccNames[] = {"plain", "phat", "scot"};

// Every refusal of the two entry points, in the header's order, before anything is allocated, staged or launched.
int gcc_check(oth_plan *p, const void *x, size_t nsamples, int nchan, size_t stride, int weighting, int lo, int hi, int upsample, int maxlag,
              const float *gcc_out, const float *peak_out, long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (int rc = welch_stat_plan(p, "the generalized cross-correlation of the spectral matrix")) return rc;
    if (nchan < 2 || nchan > kMatChanMax) return fail(c, OTH_ERR_INVALID, "nchan must lie in 2 ... " + std::to_string(kMatChanMax));
    if (!x) return fail(c, OTH_ERR_INVALID, "the input is NULL");
    if (stride < nsamples) return fail(c, OTH_ERR_INVALID, "chan_stride < nsamples");
    if (int rc = stream_shape(p, true, nsamples, nchan, stride, nullptr, nseg_out)) return rc;
    if (weighting != OTH_GCC_PLAIN && weighting != OTH_GCC_PHAT && weighting != OTH_GCC_SCOT)
        return fail(c, OTH_ERR_INVALID, "weighting must be OTH_GCC_PLAIN, OTH_GCC_PHAT or OTH_GCC_SCOT");
    const int half = p->nfft / 2;
    if (lo < -half || hi > half - 1 || lo > hi)
        return fail(c, OTH_ERR_INVALID, "band_lo <= band_hi must lie in -nfft / 2 ... nfft / 2 - 1 = " + std::to_string(-half) + " ... " + std::to_string(half - 1));
    if (upsample != 1 && upsample != 2 && upsample != 4 && upsample != 8) return fail(c, OTH_ERR_INVALID, "upsample must be 1, 2, 4 or 8");
    const long long ni = (long long)upsample * p->nfft;
    if (ni > kGccPointsMax)
        return fail(c, OTH_ERR_UNSUPPORTED, "upsample times the transform length is " + std::to_string(ni) + ": the interpolated transform takes " +
                                                std::to_string(kGccPointsMax) + " points at most");
    if (maxlag < 0 || maxlag > ni / 2 - 1)
        return fail(c, OTH_ERR_INVALID, "maxlag must lie in 0 ... upsample nfft / 2 - 1 = " + std::to_string(ni / 2 - 1));
    if (!gcc_out && !peak_out) return fail(c, OTH_ERR_INVALID, "gcc_out and peak_out are both NULL");
    return OTH_OK;
}

// after gcc_check: device in, device out
int gcc_run(oth_plan *p, const float2 *x, long long nseg, int nchan, size_t stride, int weighting, int lo, int hi, int upsample, int maxlag,
            float *gcc_out, float *peak_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int ni = upsample * p->nfft;
    MatGccArgs g{};
    if (int rc = get_twiddles(c, ni, &g.tw)) return rc;      // the context's table of NI entries: the plan's own where upsample = 1
    MatFinalizeArgs f{};
    std::string recipe;
    if (int rc = welch_mat_sums(p, x, nseg, nchan, stride, f, recipe)) return rc;
    f.out = raw_stage(p);      // every bin's totals: the plan's shift and trim take no part
    g.totals = f.totals;
    g.gcc_out = gcc_out;
    g.peak_out = peak_out;
    g.weighting = weighting;
    g.band_lo = lo;
    g.band_hi = hi;
    g.maxlag = maxlag;
    g.nchan = nchan;
    g.nfft = f.nfft;
    TIMED_LAUNCH(c, launch_mat_totals(f, c->stream));
    TIMED_LAUNCH(c, launch_mat_gcc(ni, g, c->stream));
    p->last_recipe = recipe + " gcc=" + kGccNames[weighting] + " ni=" + std::to_string(ni) + " band=" + std::to_string(lo) + ":" +
                     std::to_string(hi) + " maxlag=" + std::to_string(maxlag);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_welch_matrix_gcc_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nchan, size_t chan_stride, int weighting, int band_lo,
                             int band_hi, int upsample, int maxlag, float *gcc_out_dev, float *peak_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(
        p, nseg_out,
        [&](long long *nseg) {
            return gcc_check(p, iq_dev, nsamples, nchan, chan_stride, weighting, band_lo, band_hi, upsample, maxlag, gcc_out_dev, peak_out_dev, nseg);
        },
        [&](long long nseg) {
            return gcc_run(p, (const float2 *)iq_dev, nseg, nchan, chan_stride, weighting, band_lo, band_hi, upsample, maxlag, gcc_out_dev,
                           peak_out_dev);
        });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_matrix_gcc(oth_plan *p, const void *iq, size_t nsamples, int nchan, int src_is_device, int weighting, int band_lo, int band_hi,
                         int upsample, int maxlag, float *gcc_out, float *peak_out, uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = gcc_check(p, iq, nsamples, nchan, nsamples, weighting, band_lo, band_hi, upsample, maxlag, gcc_out, peak_out, &nseg)) return rc;
    const size_t pairs = (size_t)nchan * (nchan - 1) / 2;
    const HostRow rows[] = {{gcc_out, 2 * pairs * (2 * (size_t)maxlag + 1)}, {peak_out, 3 * pairs}};
    // the channels lie one behind the other: staged as one block of nchan nsamples
    return host_form(p, iq, nullptr, (size_t)nchan * nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) {
                         return gcc_run(p, dx, nseg, nchan, nsamples, weighting, band_lo, band_hi, upsample, maxlag, dev[0], dev[1]);
                     });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
