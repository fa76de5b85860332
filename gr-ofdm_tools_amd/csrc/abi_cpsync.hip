// C ABI, host side: cyclic-prefix symbol timing and carrier offset (oth_cp_sync / _dev) - the checks, the work split, the
// partial and total rows in the context's scratch, the three launches of cpsync.hip and the host-output form around them.
#include "abi_stat.h"

namespace {
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// Every refusal of the two entry points, before anything is allocated, staged or launched; then S per hypothesis.
int cps_check(oth_ctx *c, const void *x, size_t nsamples, int nstreams, size_t stride, int nhyp, const int *tu, const int *cp, float rho,
              size_t row_stride, const float *est, uint64_t *nsym_out) {
    if (!x || !tu || !cp || !est || !nsym_out || nstreams < 1) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (nhyp < 1 || nhyp > kCpsHypMax) return fail(c, OTH_ERR_INVALID, "nhyp must lie in 1 ... " + std::to_string(kCpsHypMax));
    int ts_max = 0;
    for (int h = 0; h < nhyp; ++h) {
        nsym_out[h] = 0;
        if (tu[h] < kCpsTuMin || tu[h] > kCpsTuMax)
            return fail(c, OTH_ERR_INVALID, "Tu must lie in " + std::to_string(kCpsTuMin) + " ... " + std::to_string(kCpsTuMax) + ", not " + std::to_string(tu[h]));
    }
    for (int h = 0; h < nhyp; ++h) {
        if (cp[h] < 1 || cp[h] > tu[h]) return fail(c, OTH_ERR_INVALID, "cp must lie in 1 ... Tu, not " + std::to_string(cp[h]));
        ts_max = std::max(ts_max, tu[h] + cp[h]);
    }
    if (!(rho >= 0.f && rho <= 1.f)) return fail(c, OTH_ERR_INVALID, "rho must be a finite value in 0 ... 1");
    if (stride < nsamples) return fail(c, OTH_ERR_INVALID, "stream_stride < nsamples");
    if (nstreams > 65535) return fail(c, OTH_ERR_UNSUPPORTED, "cp_sync takes at most 65535 streams per launch");
    if (row_stride < (size_t)ts_max) return fail(c, OTH_ERR_INVALID, "row_stride below the largest Tu + cp (" + std::to_string(ts_max) + ")");
    for (int h = 0; h < nhyp; ++h)
        if (nsamples < 2 * (size_t)tu[h] + (size_t)cp[h])
            return fail(c, OTH_ERR_INVALID, "input shorter than one symbol and its lag (2 Tu + cp = " + std::to_string(2 * tu[h] + cp[h]) + " samples)");
    for (int h = 0; h < nhyp; ++h) nsym_out[h] = (uint64_t)((nsamples - (size_t)tu[h]) / (size_t)(tu[h] + cp[h]));
    return OTH_OK;
}

// The work split and the scratch layout of a call after cps_check: a (hypotheses, sizes, offsets) and the bytes of the partial
// and total rows at the front of the scratch (the host form puts its staged input and device rows behind them).
int cps_prepare(oth_ctx *c, int nstreams, int nhyp, const int *tu, const int *cp, const uint64_t *nsym, CpsArgs &a, int *threads_out,
                size_t *rows_bytes) {
    int ts_max = 0;
    for (int h = 0; h < nhyp; ++h) ts_max = std::max(ts_max, tu[h] + cp[h]);
    const int threads = cps_fold_threads(ts_max), tile = 4 * threads;
    const int bpc = std::max(1, cps_fold_blocks_per_cu(threads));
    const char *e = getenv("OTH_CPS_WG");      // read per call: at most that many runs of symbols (A/B tools and the parity suite)
    const long long cap = e ? atoll(e) : 0;
    a.nstreams = nstreams;
    a.nhyp = nhyp;
    a.tiles_max = a.w_max = a.nb_max = a.ng_max = 0;
    size_t part = 0, grp = 0, tot = 0;
    for (int h = 0; h < nhyp; ++h) {
        const int ts = tu[h] + cp[h], tiles = (ts + tile - 1) / tile, nb = (ts + kCpsBlock - 1) / kCpsBlock;
        // whole symbols go to W workgroups per stream, hypothesis and tile in contiguous runs: what the device holds at once, a
        // symbol at least
        long long W = segment_workgroups(c, (long long)nsym[h], 1, (long long)nstreams * nhyp * tiles, bpc);
        if (cap > 0) W = std::min(W, cap);
        a.tu[h] = tu[h];
        a.cp[h] = cp[h];
        a.w[h] = (int)W;
        a.ng[h] = (int)std::min((long long)kCpsGroupMax, (W + kCpsGroupRows - 1) / kCpsGroupRows);
        a.nsym[h] = (long long)nsym[h];
        a.part_off[h] = part;
        a.grp_off[h] = grp;
        a.tot_off[h] = tot;
        part += (size_t)nstreams * (size_t)W * 3 * (size_t)ts;
        grp += (size_t)nstreams * (size_t)a.ng[h] * 3 * (size_t)ts;
        tot += (size_t)nstreams * 3 * ((size_t)ts + nb);
        a.tiles_max = std::max(a.tiles_max, tiles);
        a.w_max = std::max(a.w_max, (int)W);
        a.nb_max = std::max(a.nb_max, nb);
        a.ng_max = std::max(a.ng_max, a.ng[h]);
    }
    *threads_out = threads;
    *rows_bytes = up16(sizeof(double) * (part + grp + tot));
    for (int h = 0; h < nhyp; ++h) {      // the groups' rows lie behind all partial rows, the totals behind those
        a.grp_off[h] += part;
        a.tot_off[h] += part + grp;
    }
    return OTH_OK;
}

// after cps_prepare and the scratch: device in, device out, asynchronous
int cps_run(oth_ctx *c, CpsArgs &a, int threads, const float2 *x, size_t stride, float rho, size_t row_stride, float *gamma, float *phi,
            float *est) {
    a.x = x;
    a.rows = (double *)c->scratch.get();
    a.gamma = (float2 *)gamma;
    a.phi = phi;
    a.est = est;
    a.stream_stride = stride;
    a.row_stride = row_stride;
    a.rho = (double)rho;
    TIMED_LAUNCH(c, launch_cps_fold(threads, a, c->stream));
    TIMED_LAUNCH(c, launch_cps_finalize(a, c->stream));
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_cp_sync_dev(oth_ctx *c, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, int nhyp, const int *tu,
                    const int *cp, float rho, size_t row_stride, float *gamma_out_dev, float *phi_out_dev, float *est_out_dev,
                    uint64_t *nsym_out) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c) return fail(nullptr, OTH_ERR_INVALID, "ctx is NULL");
    if (int rc = cps_check(c, iq_dev, nsamples, nstreams, stream_stride, nhyp, tu, cp, rho, row_stride, est_out_dev, nsym_out)) return rc;
    if (use_device(c)) return OTH_ERR_HIP;
    CpsArgs a{};
    int threads = 0;
    size_t rows_bytes = 0;
    if (int rc = cps_prepare(c, nstreams, nhyp, tu, cp, nsym_out, a, &threads, &rows_bytes)) return rc;
    if (int rc = c->scratch.ensure(c, rows_bytes)) return rc;
    return cps_run(c, a, threads, (const float2 *)iq_dev, stream_stride, rho, row_stride, gamma_out_dev, phi_out_dev, est_out_dev);
    OTH_CATCH(c)
}

int oth_cp_sync(oth_ctx *c, const void *iq, size_t nsamples, int src_is_device, int nhyp, const int *tu, const int *cp, float rho,
                size_t row_stride, float *gamma_out, float *phi_out, float *est_out, uint64_t *nsym_out) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c) return fail(nullptr, OTH_ERR_INVALID, "ctx is NULL");
    if (int rc = cps_check(c, iq, nsamples, 1, nsamples, nhyp, tu, cp, rho, row_stride, est_out, nsym_out)) return rc;
    if (use_device(c)) return OTH_ERR_HIP;
    CpsArgs a{};
    int threads = 0;
    size_t rows_bytes = 0;
    if (int rc = cps_prepare(c, 1, nhyp, tu, cp, nsym_out, a, &threads, &rows_bytes)) return rc;
    // behind the rows: the staged input, then gamma, phi (rows of the largest Ts) and est on the device
    size_t ts_max = 0;
    for (int h = 0; h < nhyp; ++h) ts_max = std::max(ts_max, (size_t)(tu[h] + cp[h]));
    const size_t o_x = rows_bytes, o_gamma = up16(o_x + (src_is_device ? 0 : sizeof(float2) * nsamples)),
                 o_phi = up16(o_gamma + (gamma_out ? sizeof(float2) * nhyp * ts_max : 0)),
                 o_est = up16(o_phi + (phi_out ? sizeof(float) * nhyp * ts_max : 0)), bytes = up16(o_est + sizeof(float) * 4 * nhyp);
    if (int rc = c->scratch.ensure(c, bytes)) return rc;
    unsigned char *d = c->scratch.get();
    const float2 *src = (const float2 *)iq;
    if (!src_is_device) {
        HIPCHK(c, hipMemcpyAsync(d + o_x, iq, sizeof(float2) * nsamples, hipMemcpyHostToDevice, c->stream));
        src = (const float2 *)(d + o_x);
    }
    float *d_gamma = gamma_out ? (float *)(d + o_gamma) : nullptr, *d_phi = phi_out ? (float *)(d + o_phi) : nullptr;
    float *d_est = (float *)(d + o_est);
    if (int rc = cps_run(c, a, threads, src, nsamples, rho, ts_max, d_gamma, d_phi, d_est)) return rc;
    for (int h = 0; h < nhyp; ++h) {      // the columns 0 ... Ts_h - 1 of each row and nothing behind them
        const size_t ts = (size_t)(tu[h] + cp[h]);
        if (gamma_out)
            HIPCHK(c, hipMemcpyAsync(gamma_out + 2 * h * row_stride, d_gamma + 2 * h * ts_max, sizeof(float2) * ts, hipMemcpyDeviceToHost, c->stream));
        if (phi_out) HIPCHK(c, hipMemcpyAsync(phi_out + h * row_stride, d_phi + h * ts_max, sizeof(float) * ts, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(est_out, d_est, sizeof(float) * 4 * nhyp, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the caller's buffers are the caller's again
    return OTH_OK;
    OTH_CATCH(c)
}
}  // extern "C"
