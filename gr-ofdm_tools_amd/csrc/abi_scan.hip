// C ABI, host side: the scanner's small ops (group mean, channel power, bin threshold, the decision stage) and
// xcorr / fac.
#include "abi_state.h"

extern "C" {
int oth_rows_group_mean(oth_ctx *c, const float *rows_host, size_t nrows, int nfft, int group, float *out_host) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !rows_host || !out_host || nfft < 1 || group < 1 || nrows < (size_t)group)
        return fail(c, OTH_ERR_INVALID, "bad argument");
    if (use_device(c)) return OTH_ERR_HIP;
    const size_t ngroups = nrows / group;
    const size_t in_bytes = sizeof(float) * ngroups * group * nfft, out_bytes = sizeof(float) * ngroups * nfft;
    int rc = c->scratch.ensure(c, in_bytes + out_bytes);
    if (rc) return rc;
    float *d_in = (float *)c->scratch.get(), *d_out = (float *)(c->scratch.get() + in_bytes);
    HIPCHK(c, hipMemcpyAsync(d_in, rows_host, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_group_mean(d_in, (long long)ngroups, nfft, group, d_out, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_host, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// movingaverage() takes 1 <= int(srch_bins) <= nfft: with a longer window np.convolve swaps its arguments and the
// reference returns int(srch_bins) values - another length and centring, which no nfft-long answer reproduces
static const char *srch_bins_error(double srch_bins, int nfft) {
    if (!(srch_bins >= 1.0)) return "bad argument (srch_bins must be >= 1)";
    if (srch_bins >= (double)nfft + 1.0) return "int(srch_bins) must not exceed nfft (the reference's moving average changes length there)";
    return nullptr;
}

// -> device pointers to the channel slice bounds, uploading them only when they differ from the cached copy
static int channel_bounds_dev(oth_ctx *c, int nch, const int *lo, const int *hi, const int **dlo, const int **dhi) {
    *dlo = *dhi = nullptr;
    if (nch <= 0) return OTH_OK;
    const size_t n = 2 * (size_t)nch;
    bool same = c->d_bounds.get() && c->bounds_host.size() == n;
    for (int i = 0; same && i < nch; ++i) same = c->bounds_host[i] == lo[i] && c->bounds_host[nch + i] == hi[i];
    if (!same) {
        c->bounds_host.clear();      // nothing is cached until the new upload is enqueued
        if (!c->bounds_ev) HIPCHK(c, c->bounds_ev.create());
        else HIPCHK(c, hipEventSynchronize(c->bounds_ev.get()));      // the previous upload has read the pinned words
        // (a longer list: ensure() drains the stream before it frees - kernels may still read the old device copy)
        if (int rc = c->d_bounds.ensure(c, sizeof(int) * n)) return rc;
        if (int rc = c->h_bounds.grow(c, sizeof(int) * n)) return rc;
        memcpy(c->h_bounds.get(), lo, sizeof(int) * nch);
        memcpy(c->h_bounds.get() + nch, hi, sizeof(int) * nch);
        HIPCHK(c, hipMemcpyAsync(c->d_bounds.get(), c->h_bounds.get(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->bounds_ev.get(), c->stream));
        c->bounds_host.assign(c->h_bounds.get(), c->h_bounds.get() + n);
    }
    *dlo = c->d_bounds.get();
    *dhi = c->d_bounds.get() + nch;
    return OTH_OK;
}

int oth_channel_power(oth_ctx *c, const float *psd_host, int nfft, double srch_bins, int nch, const int *lo,
                      const int *hi, float *power_out, float *movavg_out) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !psd_host || !lo || !hi || !power_out || nfft < 1 || nch < 1) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (const char *why = srch_bins_error(srch_bins, nfft)) return fail(c, OTH_ERR_INVALID, why);
    for (int i = 0; i < nch; ++i)
        if (lo[i] < 0 || hi[i] > nfft) return fail(c, OTH_ERR_INVALID, "channel slice outside [0, nfft]");
    if (use_device(c)) return OTH_ERR_HIP;
    const size_t o_psd = 0, o_ma = up16(o_psd + sizeof(float) * nfft), o_maf = up16(o_ma + sizeof(double) * nfft),
                 o_lo = up16(o_maf + sizeof(float) * nfft), o_hi = up16(o_lo + sizeof(int) * nch),
                 o_pw = up16(o_hi + sizeof(int) * nch), bytes = up16(o_pw + sizeof(float) * nch);
    int rc = c->scratch.ensure(c, bytes);
    if (rc) return rc;
    unsigned char *d = c->scratch.get();
    HIPCHK(c, hipMemcpyAsync(d + o_psd, psd_host, sizeof(float) * nfft, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_lo, lo, sizeof(int) * nch, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_hi, hi, sizeof(int) * nch, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_channel_power((const float *)(d + o_psd), 1, nfft, srch_bins, nch, (const int *)(d + o_lo),
                                   (const int *)(d + o_hi), (double *)(d + o_ma), (float *)(d + o_pw),
                                   (float *)(d + o_maf), c->stream));
    HIPCHK(c, hipMemcpyAsync(power_out, d + o_pw, sizeof(float) * nch, hipMemcpyDeviceToHost, c->stream));
    if (movavg_out)
        HIPCHK(c, hipMemcpyAsync(movavg_out, d + o_maf, sizeof(float) * nfft, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_bin_threshold(oth_ctx *c, const float *psd_host, int nrows, int nfft, double srch_bins, float thr_leveler,
                      unsigned char *mask_out, float *noise_out) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !psd_host || !mask_out || nrows < 1 || nfft < 1) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (const char *why = srch_bins_error(srch_bins, nfft)) return fail(c, OTH_ERR_INVALID, why);
    if (use_device(c)) return OTH_ERR_HIP;
    const size_t nb = (size_t)nrows * nfft;
    const size_t o_mask = sizeof(float) * nb, o_noise = up16(o_mask + nb);
    int rc = c->scratch.ensure(c, o_noise + sizeof(float) * nrows);
    if (rc) return rc;
    unsigned char *d = c->scratch.get();
    HIPCHK(c, hipMemcpyAsync(d, psd_host, sizeof(float) * nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_bin_threshold((const float *)d, nrows, nfft, srch_bins, thr_leveler, d + o_mask,
                                   (float *)(d + o_noise), c->stream));
    HIPCHK(c, hipMemcpyAsync(mask_out, d + o_mask, nb, hipMemcpyDeviceToHost, c->stream));
    if (noise_out)
        HIPCHK(c, hipMemcpyAsync(noise_out, d + o_noise, sizeof(float) * nrows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

// Decision stage of the batched scanner on PSD rows that are already in HBM (BASELINE config 5): one launch
// sequence, context-owned scratch, no copy of the rows.  Host results: mask (nullable), noise[nrows],
// power[nrows][nch] (nullable when nch == 0).
int oth_scan_decide_dev(oth_ctx *c, const float *psd_rows_dev, int nrows, int nfft, double srch_bins, float thr_leveler,
                        int nch, const int *lo, const int *hi, unsigned char *mask_out, float *noise_out,
                        float *power_out) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !psd_rows_dev || nrows < 1 || nfft < 1 || nch < 0 || (nch && (!lo || !hi || !power_out)))
        return fail(c, OTH_ERR_INVALID, "bad argument");
    if (const char *why = srch_bins_error(srch_bins, nfft)) return fail(c, OTH_ERR_INVALID, why);
    for (int i = 0; i < nch; ++i)
        if (lo[i] < 0 || hi[i] > nfft) return fail(c, OTH_ERR_INVALID, "channel slice outside [0, nfft]");
    if (use_device(c)) return OTH_ERR_HIP;
    const size_t nb = (size_t)nrows * nfft;
    const size_t o_ma = 0, o_mask = up16(o_ma + sizeof(double) * nb), o_noise = up16(o_mask + nb),
                 o_pw = up16(o_noise + sizeof(float) * nrows), o_tm = up16(o_pw + sizeof(float) * nrows * (nch + 1)),
                 bytes = up16(o_tm + sizeof(float) * nrows * scan_decide_tiles(nfft));
    int rc = c->scratch.ensure(c, bytes);
    if (rc) return rc;
    unsigned char *d = c->scratch.get();
    const int *dlo = nullptr, *dhi = nullptr;
    if ((rc = channel_bounds_dev(c, nch, lo, hi, &dlo, &dhi))) return rc;
    HIPCHK(c, launch_scan_decide(psd_rows_dev, nrows, nfft, srch_bins, thr_leveler, nch, dlo,
                                 dhi, (double *)(d + o_ma), (float *)(d + o_tm), mask_out ? d + o_mask : nullptr,
                                 (float *)(d + o_noise), nch ? (float *)(d + o_pw) : nullptr, c->stream));
    if (mask_out) HIPCHK(c, hipMemcpyAsync(mask_out, d + o_mask, nb, hipMemcpyDeviceToHost, c->stream));
    if (noise_out)
        HIPCHK(c, hipMemcpyAsync(noise_out, d + o_noise, sizeof(float) * nrows, hipMemcpyDeviceToHost, c->stream));
    if (nch)
        HIPCHK(c, hipMemcpyAsync(power_out, d + o_pw, sizeof(float) * nrows * nch, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_scan_decide_dev_out(oth_ctx *c, const float *psd_rows_dev, int nrows, int nfft, double srch_bins, float thr_leveler,
                            int nch, const int *lo, const int *hi, unsigned char *mask_dev, float *noise_dev,
                            float *power_dev) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !psd_rows_dev || !noise_dev || nrows < 1 || nfft < 1 || nch < 0 || (nch && (!lo || !hi || !power_dev)))
        return fail(c, OTH_ERR_INVALID, "bad argument");
    if (const char *why = srch_bins_error(srch_bins, nfft)) return fail(c, OTH_ERR_INVALID, why);
    for (int i = 0; i < nch; ++i)
        if (lo[i] < 0 || hi[i] > nfft) return fail(c, OTH_ERR_INVALID, "channel slice outside [0, nfft]");
    if (use_device(c)) return OTH_ERR_HIP;
    const size_t nb = (size_t)nrows * nfft;
    const size_t o_tm = up16(sizeof(double) * nb), bytes = up16(o_tm + sizeof(float) * nrows * scan_decide_tiles(nfft));
    int rc = c->scratch.ensure(c, bytes);
    if (rc) return rc;
    unsigned char *d = c->scratch.get();
    const int *dlo = nullptr, *dhi = nullptr;      // cached on the device: no host copy on the steady-state path
    if ((rc = channel_bounds_dev(c, nch, lo, hi, &dlo, &dhi))) return rc;
    HIPCHK(c, launch_scan_decide(psd_rows_dev, nrows, nfft, srch_bins, thr_leveler, nch, dlo, dhi, (double *)d,
                                 (float *)(d + o_tm), mask_dev,
                                 noise_dev, nch ? power_dev : nullptr, c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

// xcorr / fac at the lengths the one-workgroup kernel does not take: np.fft calls composed from any_fft_nat()
static int xcorr_any(oth_ctx *c, const void *a, size_t na, const void *b, size_t nb, int L, float *out, int mode) {
    AnyTables t;
    int rc = any_tables_init(c, L, &t);
    if (rc) return rc;
    const size_t nsc = any_fft_nat_scratch(t.sh), nout = (size_t)(L - L / 2);
    rc = c->scratch.ensure(c, sizeof(float2) * (2 * (size_t)L + nsc) + sizeof(float) * nout);
    if (!rc) {
        float2 *A = (float2 *)c->scratch.get(), *Bv = A + L, *sc = Bv + L;
        float *o = (float *)(sc + nsc);
        auto run = [&]() -> int {
            int r;
            HIPCHK(c, hipMemsetAsync(A, 0, sizeof(float2) * 2 * (size_t)L, c->stream));
            HIPCHK(c, hipMemcpyAsync(A, a, sizeof(float2) * na, hipMemcpyHostToDevice, c->stream));
            if ((r = any_fft_nat(c, t, A, sc))) return r;                                                  // e = fft(a, L)
            if (mode == 0) {
                HIPCHK(c, hipMemcpyAsync(Bv, b, sizeof(float2) * nb, hipMemcpyHostToDevice, c->stream));
                if ((r = any_fft_nat(c, t, Bv, sc))) return r;                                             // f = fft(b, L)
                HIPCHK(c, launch_any_ew(4, A, A, Bv, nullptr, L, L, 0, 0, c->stream));                    // conj(f conj(e)) = conj(f) e
                if ((r = any_fft_nat(c, t, A, sc))) return r;                                              // = L conj(ifft(f conj(e)))
                HIPCHK(c, launch_any_abs(o, A, (int)nout, 1.0f / (float)L, c->stream));                   // |fftshift(h)[L/2:]| = |h[:L - L/2]|
            } else {
                HIPCHK(c, launch_any_ew(5, A, A, nullptr, nullptr, L, L, 0, 0, c->stream));               // |fft(d, L)|
                if ((r = any_fft_nat(c, t, A, sc))) return r;
                HIPCHK(c, launch_any_abs(o, A, (int)nout, 1.0f, c->stream));
            }
            HIPCHK(c, hipMemcpyAsync(out, o, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return OTH_OK;
        };
        rc = run();
    }
    if (rc) hipStreamSynchronize(c->stream);      // the tables are released on return
    return rc;
}

static int xcorr_impl(oth_ctx *c, const void *a, size_t na, const void *b, size_t nb, int L, float *out, int mode) {
    if (!c || !a || !out || (mode == 0 && !b)) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (L < 1) return fail(c, OTH_ERR_INVALID, "L must be positive");
    if (na > (size_t)L) na = (size_t)L;      // np.fft.fft(a, L) keeps the first L samples of a longer input
    if (nb > (size_t)L) nb = (size_t)L;
    if (use_device(c)) return OTH_ERR_HIP;
    if (!generic_supported(L)) return xcorr_any(c, a, na, b, nb, L, out, mode);
    const float2 *tw = nullptr;
    int rc = get_twiddles(c, L, &tw);
    if (rc) return rc;
    if ((rc = c->scratch.ensure(c, sizeof(float2) * 3 * (size_t)L))) return rc;
    float2 *d = (float2 *)c->scratch.get();
    HIPCHK(c, hipMemsetAsync(d, 0, sizeof(float2) * 3 * L, c->stream));
    HIPCHK(c, hipMemcpyAsync(d, a, sizeof(float2) * na, hipMemcpyHostToDevice, c->stream));
    if (mode == 0) HIPCHK(c, hipMemcpyAsync(d + L, b, sizeof(float2) * nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_xcorr(L, d, d + L, tw, (float *)(d + 2 * L), mode, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, d + 2 * L, sizeof(float) * (L - L / 2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
}

int oth_xcorr(oth_ctx *c, const void *a, size_t na, const void *b, size_t nb, int L, float *out) {
    OTH_TRY
    CtxGuard guard_(c);
    return xcorr_impl(c, a, na, b, nb, L, out, 0);
    OTH_CATCH(c)
}

int oth_fac(oth_ctx *c, const void *data, size_t n, int L, float *out) {
    OTH_TRY
    CtxGuard guard_(c);
    return xcorr_impl(c, data, n, nullptr, 0, L, out, 1);
    OTH_CATCH(c)
}
}  // extern "C"
