// C ABI, host side: the streaming periodogram chain (oth_chain_*) - the fused and the coverage launches, the
// synchronous pushes and the asynchronous work() form with its ticket ring.
#include "abi_state.h"

extern "C" {
/* ---- periodogram chain ------------------------------------------------------ */

int oth_chain_create(oth_ctx *c, int nfft, const float *window, int fftshift, int epilogue, int keep_one_in_n,
                     oth_chain **out) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !out) return fail(c, OTH_ERR_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (nfft < 1) return fail(c, OTH_ERR_INVALID, "nfft must be positive");
    const bool any_route = !generic_supported(nfft);      // not a power of two in [64, 16384]: fft_any.hip
    if (epilogue < OTH_EPI_MAG || epilogue > OTH_EPI_MAG2_OVER_N2) return fail(c, OTH_ERR_INVALID, "unknown epilogue");
    if (keep_one_in_n < 1) return fail(c, OTH_ERR_INVALID, "keep_one_in_n must be >= 1");
    if (use_device(c)) return OTH_ERR_HIP;
    std::unique_ptr<oth_chain> h(new (std::nothrow) oth_chain());
    if (!h) return fail(c, OTH_ERR_NOMEM, "host allocation failed");
    h->ctx = c;
    h->nfft = nfft;
    h->fftshift = fftshift != 0;
    h->epilogue = epilogue;
    h->keep_n = h->count = keep_one_in_n;
    int rc = any_route ? any_tables_init(c, nfft, &h->any) : get_twiddles(c, nfft, &h->d_tw);
    if (rc) return rc;
    std::vector<float> w(nfft);
    h->rect = true;
    for (int i = 0; i < nfft; ++i) {
        w[i] = window ? window[i] : 1.0f;
        if (w[i] != 1.0f) h->rect = false;
    }
    hipError_t e = h->d_win.upload(c, w.data(), sizeof(float) * nfft);
    if (e == hipSuccess) e = h->d_iir.alloc(sizeof(float) * nfft);
    if (e == hipSuccess) e = h->d_peak.alloc(sizeof(float) * nfft);
    if (e == hipSuccess) e = h->d_peak_init.alloc(sizeof(int));
    if (e == hipSuccess) e = h->h_tail.alloc(sizeof(float2) * nfft);
    if (e == hipSuccess) e = h->tail_ev.create();
    if (e == hipSuccess) e = hipMemsetAsync(h->d_iir.get(), 0, sizeof(float) * nfft, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_peak.get(), 0, sizeof(float) * nfft, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_peak_init.get(), 0, sizeof(int), c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);      // also after a failure: w dies here
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string("chain setup: ") + hipGetErrorString(e));
    *out = h.release();
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_chain_destroy(oth_chain *h) {
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

int oth_chain_set_keep_one_in_n(oth_chain *h, int n) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
    if (n < 1) return fail(h->ctx, OTH_ERR_INVALID, "keep_one_in_n must be >= 1");
    h->keep_n = h->count = n;   // keep_one_in_n::set_n restarts the count in front of the vector that is still incomplete;
                                // a partial one whose samples were skipped as dropped is kept if the new count says so (its
                                // samples wait in h_tail for the next push that enqueues work)
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_set_iir_log(oth_chain *h, float alpha, float k_db) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
    h->do_iir = alpha > 0.f;
    h->alpha = alpha;
    h->kdb = k_db;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_set_peak_hold(oth_chain *h, int enable) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
    h->do_peak = enable != 0;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_set_kernel(oth_chain *h, int which) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
    if (which < OTH_KERNEL_AUTO || which > OTH_KERNEL_TUNED) return fail(h->ctx, OTH_ERR_INVALID, "unknown kernel id");
    h->kernel = which;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_reset(oth_chain *h) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
    oth_ctx *c = h->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    HIPCHK(c, hipMemsetAsync(h->d_iir.get(), 0, sizeof(float) * h->nfft, c->stream));
    HIPCHK(c, hipMemsetAsync(h->d_peak.get(), 0, sizeof(float) * h->nfft, c->stream));
    HIPCHK(c, hipMemsetAsync(h->d_peak_init.get(), 0, sizeof(int), c->stream));
    h->peak_flag_set = false;
    h->leftover = 0;
    h->leftover_stale = false;
    h->tail_from = 0;
    h->count = h->keep_n;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

// The fused path (segfft.hip): FFT + epilogue + IIR / peak accumulation in one launch over all kept vectors, a
// small tail kernel for the state and the rows the caller wants.  Covers nfft 1024 / 2048 / 4096 with at most one
// of {IIR + log, peak hold} and up to kTailRows rows handed back.
constexpr long long kTailRows = 256;

static bool chain_fused_ok(const oth_chain *h, long long give) {
    const bool big = h->nfft == 8192 || h->nfft == 16384;      // welch16k.hip's chain build
    if (h->kernel == OTH_KERNEL_GENERIC || !(seg_supported(h->nfft) || big)) return false;
    if (h->do_iir && h->do_peak) return false;
    if (h->do_iir && !(h->alpha > 0.f && h->alpha <= 1.f)) return false;
    return give <= kTailRows;
}

static int chain_launch_fused(oth_chain *h, const float2 *x, long long first_vec, long long nrows, float *rows_last,
                              long long give) {
    oth_ctx *c = h->ctx;
    const int N = h->nfft;
    SegArgs a{};
    a.x = x;
    a.stream_stride = 0;
    a.nstreams = 1;
    a.win = h->d_win.get();
    a.tw = h->d_tw;
    a.step = (long long)h->keep_n * N;
    a.first = first_vec * N;
    a.nseg = nrows;
    a.detrend = 0;
    a.chain = 1;
    a.epilogue = h->epilogue;
    a.scale = h->epilogue == OTH_EPI_MAG2_OVER_N2 ? (float)(1.0 / ((double)N * (double)N)) : 1.0f;
    a.fftshift = h->fftshift;
    a.store_from = nrows - give;
    int rc;
    if (h->do_iir) {
        a.acc_mode = 1;
        a.acc_end = a.store_from;
        a.l2 = h->alpha >= 1.f ? -INFINITY : log2f(1.0f - h->alpha);
        if (give) {
            if ((rc = h->d_rows.ensure(c, sizeof(float) * (size_t)give * N))) return rc;
            a.rows = h->d_rows.get();      // raw |X|^2 rows; the tail kernel turns them into dB rows
        }
    } else if (h->do_peak) {
        a.acc_mode = 2;
        a.acc_end = nrows;
        a.rows = rows_last;
    } else {
        // no state: rows nobody asked for are not computed at all (latest wins)
        if (!give) return OTH_OK;
        a.acc_mode = 3;
        a.acc_end = 0;
        a.first += a.store_from * a.step;
        a.nseg = give;
        a.store_from = 0;
        a.rows = rows_last;
    }
    const bool big = N >= 8192;      // one workgroup per segment: 2 (8192) / 1 (16384) per CU
    const int tpc = big ? (N == 8192 ? 2 : 1) : seg_teams_per_cu(N, 2, false);
    interleaved_chunks(a, (long long)c->cu_count * tpc);
    const long long W = a.wg_per_stream;
    int groups = 0;
    if (a.acc_mode != 3) {
        if ((rc = h->d_partial.ensure(c, sizeof(float) * (size_t)W * N))) return rc;
        a.partial = h->d_partial.get();
        groups = chain_tail_groups((int)W, N);
        if (groups && (rc = h->d_tail.ensure(c, sizeof(float) * (size_t)groups * N))) return rc;
    }
    // 16384 points: the one-exchange pipelined loop (welch16k1x.hip, round 4); OTH_CHAIN16K=old keeps the 4 x 4096 build
    // (A/B).  At 8192 points the chain stays on the 2 x 4096 build: the 8-wave one-exchange loop with the chain's epilogue
    // spills 20 registers and measured 48.8-49.3 % against 53.4-54.1 % (windowed), 52.5 against 53.0 % (rectangular) on
    // the same box (round 5, tools/archive/ab_8k.sh; OTH_CHAIN16K=x1 selects it for the A/B)
    static const char *chain16k_mode = getenv("OTH_CHAIN16K");
    const bool x1 = (N == 16384 && !(chain16k_mode && !strcmp(chain16k_mode, "old"))) ||
                    (N == 8192 && chain16k_mode && !strcmp(chain16k_mode, "x1"));
    {
        Timed tm(c);      // the whole push: transform kernel + cross-team reduction + state / rows
        HIPCHK(c, big ? (x1 ? launch_chain16k1x(N, a, h->rect, c->stream) : launch_chain16k(N, a, h->rect, c->stream))
                      : launch_seg(N, a, 2, false, c->stream));
        h->ops += 1;
        if (a.acc_mode != 3) h->ops += (groups ? 2 : 1) + ((a.acc_mode == 1 && give > 8) ? 1 : 0);      // [reduce +] state [+ rows]
        if (a.acc_mode != 3)
            HIPCHK(c, launch_chain_tail(h->d_partial.get(), groups ? h->d_tail.get() : nullptr, (int)W, N,
                                        big ? (x1 ? x1_layout(N) : w16k_layout(N)) : ROW_NATURAL, h->fftshift, a.acc_mode, a.acc_end,
                                        h->alpha, h->kdb, h->d_iir.get(), h->d_peak.get(), h->d_rows.get(), h->do_iir ? give : 0, rows_last,
                                        c->stream));
    }
    if (a.acc_mode == 2 && !h->peak_flag_set) {      // the coverage path (rows_epilogue_kernel) reads the flag
        HIPCHK(c, launch_set_flag(h->d_peak_init.get(), 1, c->stream));
        h->ops += 1;
        h->peak_flag_set = true;
    }
    return OTH_OK;
}

// `nrows` kept vectors of x, vector index first_vec + r * keep_n (r = 0 .. nrows-1), through FFT + epilogue in
// time order (IIR / peak state advance); the LAST `give` post-epilogue rows land in rows_last (device).
static int chain_launch(oth_chain *h, const float2 *x, long long first_vec, long long nrows, float *rows_last,
                        long long give) {
    oth_ctx *c = h->ctx;
    const int N = h->nfft;
    if (!rows_last) give = 0;
    if (chain_fused_ok(h, give)) return chain_launch_fused(h, x, first_vec, nrows, rows_last, give);
    if (!h->do_iir && !h->do_peak) {      // no state: rows nobody asked for are not computed at all (latest wins)
        if (!give) return OTH_OK;
        first_vec += (nrows - give) * h->keep_n;
        nrows = give;
    }
    int rc = h->d_rows.ensure(c, sizeof(float) * (size_t)nrows * N);
    if (rc) return rc;
    PgramArgs a;
    a.x = x;
    a.win = h->d_win.get();
    a.tw = h->d_tw;
    a.rows = h->d_rows.get();
    a.first_vec = first_vec;
    a.nrows = nrows;
    a.keep_n = h->keep_n;
    a.fftshift = h->fftshift;
    a.epilogue = h->epilogue;
    a.scale = h->epilogue == OTH_EPI_MAG2_OVER_N2 ? (float)(1.0 / ((double)N * (double)N)) : 1.0f;
    if (h->any.sh.kind != ANY_NONE) {      // lengths outside the power-of-two kernels (fft_any.hip)
        Timed tm(c);
        if ((rc = any_run(c, h->any, x, nullptr, first_vec * N, (long long)h->keep_n * N, N, h->d_win.get(), false, nrows, nullptr, 0,
                          h->d_rows.get(), a.epilogue, a.scale, a.fftshift)))
            return rc;
    } else {
        Timed tm(c);
        HIPCHK(c, launch_pgram(N, a, c->stream));
    }
    h->ops += h->any.sh.kind == ANY_NONE ? 1 : 3;      // (the any-length routes: one to three launches per chunk)
    if (h->do_iir || h->do_peak) {
        HIPCHK(c, launch_rows_epilogue(h->d_rows.get(), nrows, N, h->alpha, h->kdb, h->d_iir.get(), h->d_peak.get(), h->d_peak_init.get(),
                                       h->do_iir, h->do_peak, c->stream));
        h->ops += h->do_peak ? 2 : 1;
    }
    if (h->do_peak && nrows > 0) h->peak_flag_set = true;
    if (rows_last && give > 0) {      // (rows_last may be pinned host memory - the asynchronous work() form: hipMemcpyDefault)
        HIPCHK(c, hipMemcpyAsync(rows_last, h->d_rows.get() + (size_t)(nrows - give) * N, sizeof(float) * (size_t)give * N,
                                 hipMemcpyDefault, c->stream));
        h->ops += 1;
    }
    return OTH_OK;
}

// Feed nsamples device-resident samples: completes the vector left over from the previous call, runs the full
// vectors straight from `src`, keeps the incomplete tail.  Asynchronous on the context's stream.  rows_dev (may
// be NULL) receives the last min(rows, capacity) rows of this call in time order.
static int chain_feed(oth_chain *h, const float2 *src, size_t nsamples, float *rows_dev, size_t capacity,
                      uint64_t *nrows_out) {
    oth_ctx *c = h->ctx;
    const int N = h->nfft;
    if (h->leftover_stale) return fail(c, OTH_ERR_STATE, "chain: host-only samples of the partial vector were not uploaded");
    int rc = h->d_buf.ensure(c, sizeof(float2) * (size_t)N);
    if (rc) return rc;
    bool head = false;           // a vector completed in d_buf
    if (h->leftover) {
        const size_t take = nsamples < (size_t)N - h->leftover ? nsamples : (size_t)N - h->leftover;
        HIPCHK(c, hipMemcpyAsync(h->d_buf.get() + h->leftover, src, take * sizeof(float2), hipMemcpyDeviceToDevice,
                                 c->stream));
        h->ops += 1;
        h->leftover += take;
        src += take;
        nsamples -= take;
        if (h->leftover == (size_t)N) {
            head = true;
            h->leftover = 0;
        }
    }
    const long long nvec = (long long)(nsamples / N);
    // keep_one_in_n: `count` vectors to go until the next kept one (GNU Radio keeps the LAST of every n)
    long long k_head = 0;
    if (head) {
        if (--h->count == 0) {
            k_head = 1;
            h->count = h->keep_n;
        }
    }
    long long k_body = 0, first = h->count - 1;
    if (nvec > first) k_body = 1 + (nvec - 1 - first) / h->keep_n;
    if (k_body == 0) {
        h->count -= (int)nvec;
    } else {
        const long long last = first + (k_body - 1) * h->keep_n;
        h->count = h->keep_n - (int)(nvec - 1 - last);
    }
    const long long give_body = k_body < (long long)capacity ? k_body : (long long)capacity;
    const long long give_head = k_head < (long long)capacity - give_body ? k_head : (long long)capacity - give_body;
    if (k_head && (rc = chain_launch(h, h->d_buf.get(), 0, 1, rows_dev, rows_dev ? give_head : 0))) return rc;
    if (k_body && (rc = chain_launch(h, src, first, k_body, rows_dev ? rows_dev + (size_t)give_head * N : nullptr,
                                     rows_dev ? give_body : 0)))
        return rc;
    const size_t used = (size_t)nvec * N, keep = nsamples - used;
    if (keep) {      // d_buf is free again: a completed head vector has been consumed by the launch above (stream order)
        HIPCHK(c, hipMemcpyAsync(h->d_buf.get(), src + used, keep * sizeof(float2), hipMemcpyDeviceToDevice, c->stream));
        h->ops += 1;
        h->leftover = keep;
    }
    if (nrows_out) *nrows_out = (uint64_t)(k_head + k_body);
    return OTH_OK;
}

// push / push_dev after asynchronous pushes that skipped part of the current vector: its host-only samples go up first,
// straight from the pinned h_tail; an event behind the copy lets a later dropped push wait for it before rewriting h_tail
// (push_dev stays asynchronous).
static int chain_upload_tail(oth_chain *h) {
    if (!h->leftover_stale) return OTH_OK;
    oth_ctx *c = h->ctx;
    int rc = h->d_buf.ensure(c, sizeof(float2) * (size_t)h->nfft);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(h->d_buf.get() + h->tail_from, h->h_tail.get() + h->tail_from,
                             (h->leftover - h->tail_from) * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(h->tail_ev.get(), c->stream));
    h->tail_ev_live = true;
    h->ops += 1;
    h->leftover_stale = false;
    return OTH_OK;
}

// h_tail may be rewritten once the device has read the last upload from it; false on an error (the push then takes the
// path that enqueues work, which reports it)
static bool chain_tail_writable(oth_chain *h) {
    if (!h->tail_ev_live) return true;
    if (hipEventSynchronize(h->tail_ev.get()) != hipSuccess) return false;
    h->tail_ev_live = false;
    return true;
}

int oth_chain_push_dev(oth_chain *h, const void *iq_dev, size_t nsamples, float *rows_out_dev, size_t rows_capacity,
                       uint64_t *nrows_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
    oth_ctx *c = h->ctx;
    if (nrows_out) *nrows_out = 0;
    if (!iq_dev && nsamples) return fail(c, OTH_ERR_INVALID, "iq is NULL");
    if (!nsamples) return OTH_OK;
    if (use_device(c)) return OTH_ERR_HIP;
    h->ops = 0;
    int rc = chain_upload_tail(h);
    if (rc) return rc;
    return chain_feed(h, (const float2 *)iq_dev, nsamples, rows_out_dev, rows_out_dev ? rows_capacity : 0, nrows_out);
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_push(oth_chain *h, const void *iq, size_t nsamples, int src_is_device, float *rows_out,
                   size_t rows_capacity, uint64_t *nrows_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
    oth_ctx *c = h->ctx;
    if (nrows_out) *nrows_out = 0;
    if (!iq && nsamples) return fail(c, OTH_ERR_INVALID, "iq is NULL");
    if (!nsamples) return OTH_OK;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = h->nfft;
    const float2 *src = (const float2 *)iq;
    int rc;
    h->ops = 0;
    if ((rc = chain_upload_tail(h))) return rc;
    if (!src_is_device) {
        if ((rc = h->d_stage.ensure(c, nsamples * sizeof(float2)))) return rc;
        HIPCHK(c, hipMemcpyAsync(h->d_stage.get(), iq, nsamples * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        src = h->d_stage.get();
    }
    // rows this call can produce at most: one completed leftover vector + the full vectors of the new samples
    size_t cap = rows_out ? rows_capacity : 0;
    const size_t most = nsamples / N + 2;
    if (cap > most) cap = most;
    if (cap && (rc = h->d_out.ensure(c, sizeof(float) * cap * N))) return rc;
    uint64_t nrows = 0;
    if ((rc = chain_feed(h, src, nsamples, cap ? h->d_out.get() : nullptr, cap, &nrows))) return rc;
    const size_t give = nrows < cap ? (size_t)nrows : cap;
    if (give) HIPCHK(c, hipMemcpyAsync(rows_out, h->d_out.get(), sizeof(float) * give * N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the caller's buffer and rows_out are the caller's again
    if (nrows_out) *nrows_out = nrows;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

// A push of which nothing will ever be looked at: no vector it completes is a kept one (keep_one_in_n) and the partial vector it
// leaves behind is not one either.  Then nothing needs to reach the device - only the stream position moves on.  This is the
// common case of a sensor with a low sens_per_sec: spectrum_sensor_v2.py:86-87 keeps one vector in int(Sf / N / sens_per_sec)
// (97 of 98 at 1 MS/s, 1024 points, 10 PSDs per second), and GNU Radio's work() chunks hold 4-32 of them.
// The samples such a push adds to a partial vector are kept on the host (h_tail, a plain memcpy): if the vector turns into a
// kept one later (set_keep_one_in_n), the push that continues it uploads them.
// -> true and the state advanced, or false and nothing touched.
static bool chain_push_dropped(oth_chain *h, const float2 *src, size_t nsamples) {
    const size_t N = (size_t)h->nfft;
    size_t L = h->leftover, rest = nsamples;
    long long count = h->count;
    if (L) {
        const size_t take = rest < N - L ? rest : N - L;
        if (count == 1) return false;      // the vector in progress is a kept one: its samples are needed
        if (L + take < N) {                // it stays partial: keep the new samples on the host
            if (!chain_tail_writable(h)) return false;
            if (!h->leftover_stale) h->tail_from = L;
            memcpy(h->h_tail.get() + L, src, take * sizeof(float2));
            h->leftover = L + take;
            h->leftover_stale = true;
            return true;
        }
        --count;                           // it completes and is dropped
        src += take;
        rest -= take;
    }
    const long long nvec = (long long)(rest / N);
    if (nvec > count - 1) return false;      // a vector of the body is kept
    count -= nvec;
    const size_t keep = rest - (size_t)nvec * N;
    if (keep && count == 1) return false;      // the vector that begins here will be kept
    if (keep && !chain_tail_writable(h)) return false;
    if (keep) memcpy(h->h_tail.get(), src + (size_t)nvec * N, keep * sizeof(float2));
    h->leftover = keep;
    h->leftover_stale = keep != 0;
    h->tail_from = 0;
    h->count = (int)count;
    return true;
}

// sync_block.work() form: copy the scheduler's buffer into a pinned slot, enqueue H2D + kernels, record an event and return.
// The latest row is written by the last kernel straight into the slot's pinned host row (round 6: one stream operation less
// than a D2H copy behind it); the watcher collects it with oth_chain_poll / oth_chain_wait.
int oth_chain_push_async(oth_chain *h, const void *iq_host, size_t nsamples, uint64_t *ticket_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
    oth_ctx *c = h->ctx;
    if (!ticket_out) return fail(c, OTH_ERR_INVALID, "ticket_out is NULL");
    *ticket_out = 0;
    if (!iq_host && nsamples) return fail(c, OTH_ERR_INVALID, "iq is NULL");
    const int N = h->nfft;
    const uint64_t ticket = h->next_ticket;
    const int slot = (int)(ticket % oth_chain::kRing);
    h->ops = 0;
    if (nsamples && chain_push_dropped(h, (const float2 *)iq_host, nsamples)) {      // nothing to compute: no copy, no launch,
        h->noop[slot] = true;                                                          // no event
        h->ticket_of[slot] = ticket;
        h->nrows_of[slot] = 0;
        h->next_ticket = ticket + 1;
        *ticket_out = ticket;
        return OTH_OK;
    }
    if (use_device(c)) return OTH_ERR_HIP;
    if (!h->ev[slot]) {
        HIPCHK(c, h->ev[slot].create());
        HIPCHK(c, h->h_row[slot].alloc(sizeof(float) * N));
    } else {
        // h_in[slot] / h_row[slot] belong to the slot's last real push - kRing tickets ago, or more when dropped tickets
        // (noop) came in between - until its event completes; waits only when the GPU is still that far behind
        HIPCHK(c, hipEventSynchronize(h->ev[slot].get()));
    }
    h->noop[slot] = false;
    // host-only samples of the partial vector (skipped by dropped pushes) go up in front of the new ones
    const size_t tail = nsamples && h->leftover_stale ? h->leftover - h->tail_from : 0;
    const size_t bytes = nsamples * sizeof(float2), tail_bytes = tail * sizeof(float2);
    const bool pinned_src = bytes > kPinnedStageMax && host_ptr_is_pinned(iq_host);
    const bool direct = bytes > kPinnedStageMax && !pinned_src;      // the runtime stages pageable memory itself
    const bool wait_copy = pinned_src && bytes > kPinnedRingMax;
    const size_t in_bytes = (direct || wait_copy ? 0 : bytes) + tail_bytes;
    int rc;
    if ((rc = h->h_in[slot].grow(c, in_bytes))) return rc;
    uint64_t nrows = 0;
    if (nsamples) {
        if ((rc = h->d_stage.ensure(c, tail_bytes + bytes))) return rc;
        char *pin = (char *)h->h_in[slot].get();
        if (tail) memcpy(pin, h->h_tail.get() + h->tail_from, tail_bytes);
        if (wait_copy) {
            if ((rc = copy_in_and_wait(c, h->d_stage.get() + tail, iq_host, bytes))) return rc;
        } else if (direct) {      // the runtime's staged copy returns once the caller's buffer has been read
            HIPCHK(c, hipMemcpyAsync(h->d_stage.get() + tail, iq_host, bytes, hipMemcpyHostToDevice, c->stream));
        } else {
            memcpy(pin + tail_bytes, iq_host, bytes);      // the scheduler's buffer dies when work() returns
        }
        if (in_bytes) HIPCHK(c, hipMemcpyAsync(h->d_stage.get(), pin, in_bytes, hipMemcpyHostToDevice, c->stream));
        h->ops += (direct || wait_copy) && tail ? 2 : 1;
        const size_t leftover0 = h->leftover;
        const int count0 = h->count;
        if (tail) {      // d_buf keeps the vector's first tail_from samples; the rest comes from d_stage
            h->leftover = h->tail_from;
            h->leftover_stale = false;
        }
        // the latest row goes from the closing kernel straight into the slot's pinned row (device-visible host memory)
        if ((rc = chain_feed(h, h->d_stage.get(), tail + nsamples, h->h_row[slot].get(), 1, &nrows))) {
            h->leftover = leftover0;      // the stream position stays where it was: h_tail still holds the samples
            h->leftover_stale = tail != 0;
            h->count = count0;
            return rc;
        }
    }
    HIPCHK(c, hipEventRecord(h->ev[slot].get(), c->stream));
    h->ticket_of[slot] = ticket;
    h->nrows_of[slot] = nrows;
    h->next_ticket = ticket + 1;
    *ticket_out = ticket;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

// -> the ring slot of a ticket, or OTH_ERR_STATE once the ring no longer holds it
static int chain_slot(oth_chain *h, uint64_t ticket, int *slot) {
    *slot = (int)(ticket % oth_chain::kRing);
    if (!ticket || h->ticket_of[*slot] != ticket)
        return fail(h->ctx, OTH_ERR_STATE, "ticket unknown or overwritten (the ring keeps the last 4 pushes: latest wins)");
    return OTH_OK;
}

static int chain_collect(oth_chain *h, uint64_t ticket, float *row_out, uint64_t *nrows_out, int *ready, bool wait) {
    oth_ctx *c = h->ctx;
    int slot;
    if (int rc = chain_slot(h, ticket, &slot)) return rc;
    if (h->noop[slot]) {      // the push enqueued nothing (all its vectors dropped): done when it returned
        if (ready) *ready = 1;
        if (nrows_out) *nrows_out = 0;
        return OTH_OK;
    }
    hipError_t e = wait ? hipEventSynchronize(h->ev[slot].get()) : hipEventQuery(h->ev[slot].get());
    if (e == hipErrorNotReady) {
        if (ready) *ready = 0;
        return OTH_OK;
    }
    if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string("event: ") + hipGetErrorString(e));
    if (ready) *ready = 1;
    if (nrows_out) *nrows_out = h->nrows_of[slot];
    if (row_out && h->nrows_of[slot]) memcpy(row_out, h->h_row[slot].get(), sizeof(float) * h->nfft);
    return OTH_OK;
}

int oth_chain_poll(oth_chain *h, uint64_t ticket, float *row_out, uint64_t *nrows_out, int *ready) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h || !ready) return fail(h ? h->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    *ready = 0;
    return chain_collect(h, ticket, row_out, nrows_out, ready, false);
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_wait(oth_chain *h, uint64_t ticket, float *row_out, uint64_t *nrows_out) {
    OTH_TRY
    // the wait itself runs WITHOUT the context lock: work() on the scheduler thread must be able to enqueue meanwhile
    hipEvent_t ev = nullptr;
    {
        CtxGuard guard_(h ? h->ctx : nullptr);
        if (!h) return fail(nullptr, OTH_ERR_INVALID, "chain is NULL");
        int slot;
        if (int rc = chain_slot(h, ticket, &slot)) return rc;
        if (h->noop[slot]) {
            if (nrows_out) *nrows_out = 0;
            return OTH_OK;
        }
        ev = h->ev[slot].get();
    }
    hipError_t e = hipEventSynchronize(ev);
    if (e != hipSuccess) return fail(h->ctx, OTH_ERR_HIP, std::string("event: ") + hipGetErrorString(e));
    CtxGuard guard_(h->ctx);
    int ready = 0;
    return chain_collect(h, ticket, row_out, nrows_out, &ready, false);
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_ticket_rows(oth_chain *h, uint64_t ticket, uint64_t *nrows_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h || !nrows_out) return fail(h ? h->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    int slot;
    if (int rc = chain_slot(h, ticket, &slot)) return rc;
    *nrows_out = h->nrows_of[slot];
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_last_push_ops(oth_chain *h, uint64_t *ops_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h || !ops_out) return fail(h ? h->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    *ops_out = h->ops;
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_get_peak(oth_chain *h, float *peak_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h || !peak_out) return fail(h ? h->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    oth_ctx *c = h->ctx;
    HIPCHK(c, hipMemcpyAsync(peak_out, h->d_peak.get(), sizeof(float) * h->nfft, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}

int oth_chain_get_iir(oth_chain *h, float *lin_out) {
    OTH_TRY
    CtxGuard guard_(h ? h->ctx : nullptr);
    if (!h || !lin_out) return fail(h ? h->ctx : nullptr, OTH_ERR_INVALID, "bad argument");
    oth_ctx *c = h->ctx;
    HIPCHK(c, hipMemcpyAsync(lin_out, h->d_iir.get(), sizeof(float) * h->nfft, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH((h ? h->ctx : nullptr))
}
}  // extern "C"
