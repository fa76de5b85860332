// C ABI, host side: the polyphase channelizer (oth_channelizer_*) - the prototype's table, the checks, the streaming state
// (the pending tail in one of two device buffers, the absolute frame count behind the circular shift), the one launch of
// chanpfb.hip per push and the host-output form around it.
#include "abi_stat.h"

namespace {
// frames the next push of n samples yields with q pending: frame m covers the samples m D ... m D + L - 1 of tail ++ input
size_t chan_frames(const oth_channelizer *h, size_t n) {
    const size_t total = h->pending + n;
    return total >= h->taps ? (total - h->taps) / (size_t)h->decim + 1 : 0;
}

// Every refusal of the two push entry points, before anything is allocated, staged or launched.
int chan_check(oth_channelizer *h, const void *x, size_t nsamples, const void *out, size_t out_stride, uint64_t *nframes_out, size_t *nframes) {
    oth_ctx *c = h->ctx;
    if ((!x && nsamples) || !nframes_out) return fail(c, OTH_ERR_INVALID, "bad argument");
    *nframes_out = 0;
    *nframes = chan_frames(h, nsamples);
    if (*nframes && !out) return fail(c, OTH_ERR_INVALID, "the output is NULL");
    if (out_stride < *nframes) return fail(c, OTH_ERR_INVALID, "out_stride < frames of this push");
    return OTH_OK;
}

// after chan_check: device in, device out, asynchronous.  The launch reads the frames from d_tail[cur] and x; behind it
// the samples a later frame still needs are saved by stream-ordered copies.
int chan_run(oth_channelizer *h, const float2 *x, size_t n, size_t nframes, float2 *out, size_t out_stride) {
    oth_ctx *c = h->ctx;
    if (!n) return OTH_OK;
    const size_t q = h->pending, D = (size_t)h->decim;
    float2 *old = h->d_tail[h->cur].get();
    if (!nframes) {      // no frame yet: the new samples go behind the pending ones (q + n < L)
        HIPCHK(c, hipMemcpyAsync(old + q, x, n * sizeof(float2), hipMemcpyDeviceToDevice, c->stream));
        h->pending = q + n;
        return OTH_OK;
    }
    const int M = h->nchan;
    const long long ntiles = ((long long)nframes + kChanTile - 1) / kChanTile;
    const int bpc = std::max(1, chan_pfb_blocks_per_cu(M));
    long long W = std::min(ntiles, (long long)c->cu_count * bpc);
    if (h->tune_wg > 0) W = std::min(W, (long long)h->tune_wg);
    ChanPfbArgs a{};
    a.tail = old;
    a.x = x;
    a.h = h->d_h.get();
    a.tw = h->d_tw;
    a.out = out;
    a.out_stride = out_stride;
    a.nframes = (long long)nframes;
    a.pending = (long long)q;
    a.decim = h->decim;
    a.ntaps = h->ntaps;
    a.rot0 = (int)(h->frames_total % (uint64_t)(M / h->decim));
    a.wg_count = (int)W;
    TIMED_LAUNCH(c, launch_chan_pfb(M, a, c->stream));
    h->last_recipe = "kernel=chanpfb nchan=" + std::to_string(M) + " decim=" + std::to_string(h->decim) + " ntaps=" + std::to_string(h->ntaps) +
                     " tile=" + std::to_string(kChanTile) + " W=" + std::to_string(W) + " frames=" + std::to_string(nframes) +
                     " tiles=" + std::to_string(ntiles) + " pending=" + std::to_string(q) + " bpc=" + std::to_string(bpc);
    // the new tail: samples consumed ... q + n of tail ++ x, into the other buffer (at most L - 1 of them)
    const size_t consumed = nframes * D;
    float2 *dst = h->d_tail[h->cur ^ 1].get();
    size_t at = 0;
    if (consumed < q) {
        at = q - consumed;
        HIPCHK(c, hipMemcpyAsync(dst, old + consumed, at * sizeof(float2), hipMemcpyDeviceToDevice, c->stream));
    }
    const size_t from = consumed > q ? consumed - q : 0;
    if (n > from) HIPCHK(c, hipMemcpyAsync(dst + at, x + from, (n - from) * sizeof(float2), hipMemcpyDeviceToDevice, c->stream));
    h->cur ^= 1;
    h->pending = q + n - consumed;
    h->frames_total += nframes;
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_channelizer_create(oth_ctx *c, int nchan, int decim, int ntaps, const float *h, oth_channelizer **out) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !out) return fail(c, OTH_ERR_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (nchan < kChanMin || nchan > kChanMax || (nchan & (nchan - 1)))
        return fail(c, OTH_ERR_UNSUPPORTED, "the channelizer takes a channel count that is a power of two from 64 to 4096, not " + std::to_string(nchan));
    if (decim != nchan && decim != nchan / 2 && decim != nchan / 4) return fail(c, OTH_ERR_INVALID, "decim must be nchan, nchan / 2 or nchan / 4");
    if (ntaps < kChanTapsMin || ntaps > kChanTapsMax)
        return fail(c, OTH_ERR_INVALID, "ntaps must lie in " + std::to_string(kChanTapsMin) + " ... " + std::to_string(kChanTapsMax));
    if (!h) return fail(c, OTH_ERR_INVALID, "h is NULL");
    const size_t L = (size_t)ntaps * (size_t)nchan;
    double s2 = 0.0;
    for (size_t i = 0; i < L; ++i) {
        if (!std::isfinite(h[i])) return fail(c, OTH_ERR_INVALID, "every tap of the prototype must be finite");
        s2 += (double)h[i] * (double)h[i];
    }
    if (!(s2 > 0.0)) return fail(c, OTH_ERR_INVALID, "the prototype is all zero");
    if (use_device(c)) return OTH_ERR_HIP;
    std::unique_ptr<oth_channelizer> ch(new (std::nothrow) oth_channelizer());
    if (!ch) return fail(c, OTH_ERR_NOMEM, "host allocation failed");
    ch->ctx = c;
    ch->nchan = nchan;
    ch->decim = decim;
    ch->ntaps = ntaps;
    ch->taps = L;
    if (const char *e = getenv("OTH_CHAN_WG")) ch->tune_wg = atoi(e);
    if (int rc = get_twiddles(c, nchan, &ch->d_tw)) return rc;
    hipError_t e = ch->d_h.upload(c, h, sizeof(float) * L);
    if (e == hipSuccess) e = ch->d_tail[0].alloc(sizeof(float2) * L);
    if (e == hipSuccess) e = ch->d_tail[1].alloc(sizeof(float2) * L);
    const hipError_t es = hipStreamSynchronize(c->stream);      // also after a failure: the caller's h is the caller's again
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string("channelizer setup: ") + hipGetErrorString(e));
    *out = ch.release();
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_channelizer_destroy(oth_channelizer *h) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return OTH_OK;
    oth_ctx *c = h->ctx;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    delete h;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_channelizer_reset(oth_channelizer *h) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "channelizer is NULL");
    oth_ctx *c = h->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    h->pending = 0;
    h->frames_total = 0;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_channelizer_frames(oth_channelizer *h, size_t nsamples, uint64_t *nframes_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "channelizer is NULL");
    if (!nframes_out) return fail(h->ctx, OTH_ERR_INVALID, "bad argument");
    *nframes_out = (uint64_t)chan_frames(h, nsamples);
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_channelizer_pending(oth_channelizer *h, size_t *nsamples_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "channelizer is NULL");
    if (!nsamples_out) return fail(h->ctx, OTH_ERR_INVALID, "bad argument");
    *nsamples_out = h->pending;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_channelizer_push_dev(oth_channelizer *h, const void *iq_dev, size_t nsamples, void *out_dev, size_t out_stride, uint64_t *nframes_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "channelizer is NULL");
    oth_ctx *c = h->ctx;
    size_t nframes = 0;
    if (int rc = chan_check(h, iq_dev, nsamples, out_dev, out_stride, nframes_out, &nframes)) return rc;
    if (use_device(c)) return OTH_ERR_HIP;
    if (int rc = chan_run(h, (const float2 *)iq_dev, nsamples, nframes, (float2 *)out_dev, out_stride)) return rc;
    *nframes_out = (uint64_t)nframes;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_channelizer_push(oth_channelizer *h, const void *iq, size_t nsamples, int src_is_device, void *out_host, size_t out_stride,
                         uint64_t *nframes_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "channelizer is NULL");
    oth_ctx *c = h->ctx;
    size_t nframes = 0;
    if (int rc = chan_check(h, iq, nsamples, out_host, out_stride, nframes_out, &nframes)) return rc;
    if (!nsamples) return OTH_OK;
    if (use_device(c)) return OTH_ERR_HIP;
    const float2 *src = (const float2 *)iq;
    if (!src_is_device) {
        if (int rc = h->d_stage.ensure(c, nsamples * sizeof(float2))) return rc;
        HIPCHK(c, hipMemcpyAsync(h->d_stage.get(), iq, nsamples * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        src = h->d_stage.get();
    }
    const size_t M = (size_t)h->nchan;
    if (nframes)
        if (int rc = h->d_out.ensure(c, sizeof(float2) * M * nframes)) return rc;
    if (int rc = chan_run(h, src, nsamples, nframes, h->d_out.get(), nframes)) return rc;
    if (nframes) {      // the rows into the caller's layout: nothing but the columns 0 ... nframes - 1 of each row is written
        const size_t row = sizeof(float2) * nframes;
        if (out_stride == nframes) HIPCHK(c, hipMemcpyAsync(out_host, h->d_out.get(), row * M, hipMemcpyDeviceToHost, c->stream));
        else HIPCHK(c, hipMemcpy2DAsync(out_host, sizeof(float2) * out_stride, h->d_out.get(), row, row, M, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the caller's buffer and out_host are the caller's again
    *nframes_out = (uint64_t)nframes;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

// recipe of the handle's last push that launched ("" before the first)
int oth__debug_channelizer_recipe(oth_channelizer *h, char *buf, size_t buflen) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h || !buf || !buflen) return fail(h ? h->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    snprintf(buf, buflen, "%s", h->last_recipe.c_str());
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}
}  // extern "C"
