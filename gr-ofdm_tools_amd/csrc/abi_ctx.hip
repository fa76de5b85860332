// C ABI (include/ofdm_tools_hip.h), host side: the shared helpers of abi_state.h, the last-error text, and the context
// entry points - create / destroy / sync / timing, device memory, synthetic IQ, the read probe, oth_iq_power.
#include "abi_state.h"

static thread_local std::string g_err = "no error";

namespace oth {
bool host_ptr_is_pinned(const void *p) {
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();      // unregistered pageable memory: an error on older runtimes, not sticky
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

int fail(oth_ctx *c, int code, const std::string &msg) {
    if (c)
        c->err = msg;
    else
        g_err = msg;
    return code;
}

int fail_nothrow(oth_ctx *c, int code, const char *what) noexcept {
    try {
        if (c)
            c->err = what;
        else
            g_err = what;
    } catch (...) {
    }
    return code;
}

hipStream_t ctx_stream(const oth_ctx *c) { return c->stream; }

int use_device(oth_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    return OTH_OK;
}

int copy_in_and_wait(oth_ctx *c, void *dst, const void *src, size_t bytes) {
    Event ev;
    HIPCHK(c, ev.create());
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipEventRecord(ev.get(), c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev.get());
    if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string("host copy: ") + hipGetErrorString(e));
    return OTH_OK;
}

int get_twiddles(oth_ctx *c, int nfft, const float2 **out) {
    auto it = c->twiddles.find(nfft);
    if (it != c->twiddles.end()) {
        *out = it->second.get();
        return OTH_OK;
    }
    std::vector<float2> h(nfft);
    for (int k = 0; k < nfft; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)nfft;
        h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    DevBuf<float2> d;
    HIPCHK(c, d.upload(c, h.data(), sizeof(float2) * nfft));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = d.get();
    c->twiddles[nfft] = std::move(d);
    return OTH_OK;
}

// The three-shear form of the same twiddles (twiddle16.hip.h, rot3): entry kSymTwOrigin + e holds tan(theta / 2) and sin(theta),
// theta = 2 pi e / 4096, for |e| <= kSymTwOrigin - inside (-0.54 pi, 0.54 pi), where the tangent stays below 1.14.
std::vector<float2> symtw_table() {
    std::vector<float2> h(2 * kSymTwOrigin + 1);
    for (int e = -kSymTwOrigin; e <= kSymTwOrigin; ++e) {
        const double a = 2.0 * M_PI * (double)e / 4096.0;
        h[kSymTwOrigin + e] = make_float2((float)std::tan(0.5 * a), (float)std::sin(a));
    }
    return h;
}
}  // namespace oth

extern "C" {
int oth_abi_version(void) { return OTH_ABI_VERSION; }

const char *oth_strerror(int code) {
    switch (code) {
        case OTH_OK: return "ok";
        case OTH_ERR_INVALID: return "invalid argument";
        case OTH_ERR_HIP: return "HIP runtime error / no usable GPU";
        case OTH_ERR_UNSUPPORTED: return "unsupported size or mode";
        case OTH_ERR_NOMEM: return "out of memory (device or host)";
        case OTH_ERR_STATE: return "invalid call order";
        case OTH_ERR_INTERNAL: return "internal error (C++ exception caught at the ABI)";
        default: return "unknown error";
    }
}

int oth_device_count(int *count) {
    OTH_TRY
    if (!count) return fail(nullptr, OTH_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(nullptr, OTH_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return OTH_OK;
    OTH_CATCH(nullptr)
}

static int ctx_create(int device_id, void *stream, bool adopt, oth_ctx **out) {
    if (!out) return fail(nullptr, OTH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, OTH_ERR_HIP, "no HIP device available (libofdmtools_hip has no CPU fallback)");
    if (device_id < 0 || device_id >= n) return fail(nullptr, OTH_ERR_INVALID, "device_id out of range");
    std::unique_ptr<oth_ctx> c(new (std::nothrow) oth_ctx());
    if (!c) return fail(nullptr, OTH_ERR_NOMEM, "host allocation failed");
    c->device = device_id;
    if ((e = hipSetDevice(device_id)) != hipSuccess)
        return fail(nullptr, OTH_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
        c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        c->name = std::string(prop.name) + " (" + prop.gcnArchName + ")";
    }
    if (adopt) {
        c->stream = reinterpret_cast<hipStream_t>(stream);
        c->own_stream = false;
    } else {
        if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
            return fail(nullptr, OTH_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
        c->own_stream = true;
    }
    if (c->sink.alloc(256) != hipSuccess || c->acc4.alloc(4 * sizeof(double)) != hipSuccess ||
        c->queue.alloc(65 * sizeof(unsigned)) != hipSuccess ||
        hipMemsetAsync(c->queue.get(), 0, 65 * sizeof(unsigned), c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(nullptr, OTH_ERR_NOMEM, "hipMalloc failed for context scratch");
    c->queue_clean = true;
    c->done_count = c->queue.get() + 64;     // zero now; every signalling finalize launch leaves it at zero again
    *out = c.release();
    return OTH_OK;
}

int oth_ctx_create(int device_id, oth_ctx **out) {
    OTH_TRY
    return ctx_create(device_id, nullptr, false, out);
    OTH_CATCH(nullptr)
}
int oth_ctx_create_on_stream(int device_id, void *hip_stream, oth_ctx **out) {
    OTH_TRY
    return ctx_create(device_id, hip_stream, true, out);
    OTH_CATCH(nullptr)
}

int oth_ctx_destroy(oth_ctx *c) {
    OTH_TRY
    if (!c) return OTH_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    delete c;
    return OTH_OK;
    OTH_CATCH(nullptr)
}

int oth__debug_live_resources(int *device_buffers, int *pinned_buffers, int *events) {
    OTH_TRY
    if (device_buffers) *device_buffers = g_live_device.load();
    if (pinned_buffers) *pinned_buffers = g_live_pinned.load();
    if (events) *events = g_live_events.load();
    return OTH_OK;
    OTH_CATCH(nullptr)
}

const char *oth_last_error(oth_ctx *c) { return c ? c->err.c_str() : g_err.c_str(); }

int oth_ctx_sync(oth_ctx *c) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c) return fail(nullptr, OTH_ERR_INVALID, "ctx is NULL");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_ctx_device_name(oth_ctx *c, char *buf, size_t buflen) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !buf || !buflen) return fail(c, OTH_ERR_INVALID, "bad argument");
    std::snprintf(buf, buflen, "%s", c->name.c_str());
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_ctx_set_timing(oth_ctx *c, int enable) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c) return fail(nullptr, OTH_ERR_INVALID, "ctx is NULL");
    c->timing = enable != 0;
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_ctx_get_timing(oth_ctx *c, double *total_ms, uint64_t *launches, int reset) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c) return fail(nullptr, OTH_ERR_INVALID, "ctx is NULL");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &ev : c->events) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev.first.get(), ev.second.get()));
        c->total_ms += ms;
        c->free_events.push_back(std::move(ev));
    }
    c->events.clear();
    if (total_ms) *total_ms = c->total_ms;
    if (launches) *launches = c->launches;
    if (reset) {
        c->total_ms = 0.0;
        c->launches = 0;
    }
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_dev_alloc(oth_ctx *c, size_t bytes, void **dptr) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !dptr) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (use_device(c)) return OTH_ERR_HIP;
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(c, OTH_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_dev_free(oth_ctx *c, void *dptr) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c) return fail(nullptr, OTH_ERR_INVALID, "ctx is NULL");
    if (!dptr) return OTH_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(dptr));
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_memcpy_h2d(oth_ctx *c, void *dst, const void *src, size_t bytes) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !dst || !src) return fail(c, OTH_ERR_INVALID, "bad argument");
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_memcpy_d2h(oth_ctx *c, void *dst, const void *src, size_t bytes) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !dst || !src) return fail(c, OTH_ERR_INVALID, "bad argument");
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_synth_iq(oth_ctx *c, void *iq_dev, size_t nsamples, uint64_t seed, int ntones, const float *tone_amp,
                 const float *tone_freq, float dc_re, float dc_im) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !iq_dev || ntones < 0 || ntones > 8 || (ntones && (!tone_amp || !tone_freq)))
        return fail(c, OTH_ERR_INVALID, "bad argument (at most 8 tones)");
    if (use_device(c)) return OTH_ERR_HIP;
    HIPCHK(c, launch_synth((float2 *)iq_dev, nsamples, seed, ntones, tone_amp, tone_freq, dc_re, dc_im, c->stream));
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_stream_read_probe(oth_ctx *c, const void *dptr, size_t bytes, int repeats, double *ms_per_pass) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !dptr || bytes < 16 || repeats == 0 || !ms_per_pass) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (use_device(c)) return OTH_ERR_HIP;
    Event a, b;
    HIPCHK(c, a.create(hipEventDefault));
    HIPCHK(c, b.create(hipEventDefault));
    // repeats < 0: the 8-bytes-per-lane variant (the access width of the FFT kernels' sample loads), |repeats| passes
    const bool narrow = repeats < 0;
    if (narrow) repeats = -repeats;
    auto probe = [&]() { return narrow ? launch_read_probe8(dptr, bytes, c->sink.get(), c->stream) : launch_read_probe(dptr, bytes, c->sink.get(), c->stream); };
    HIPCHK(c, probe());   // warm-up
    HIPCHK(c, hipEventRecord(a.get(), c->stream));
    for (int i = 0; i < repeats; ++i) HIPCHK(c, probe());
    HIPCHK(c, hipEventRecord(b.get(), c->stream));
    HIPCHK(c, hipEventSynchronize(b.get()));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, a.get(), b.get()));
    *ms_per_pass = (double)ms / repeats;
    return OTH_OK;
    OTH_CATCH(c)
}

int oth_iq_power(oth_ctx *c, const void *iq_dev, size_t nsamples, double *mean_re, double *mean_im, double *var) {
    OTH_TRY
    CtxGuard guard_(c);
    if (!c || !iq_dev || !nsamples) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (use_device(c)) return OTH_ERR_HIP;
    HIPCHK(c, hipMemsetAsync(c->acc4.get(), 0, 4 * sizeof(double), c->stream));
    HIPCHK(c, launch_iq_power((const float2 *)iq_dev, nsamples, c->acc4.get(), c->stream));
    double h[4];
    HIPCHK(c, hipMemcpyAsync(h, c->acc4.get(), sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double mr = h[0] / nsamples, mi = h[1] / nsamples;
    if (mean_re) *mean_re = mr;
    if (mean_im) *mean_im = mi;
    if (var) *var = h[2] / nsamples - (mr * mr + mi * mi);
    return OTH_OK;
    OTH_CATCH(c)
}
}  // extern "C"
