// Owning holders of the GPU resources of the C ABI's host side (abi_state.h): device memory, pinned host memory and
// events.  A context, plan, chain or table set keeps each resource in one of them, so a new buffer is one field - its
// release is the holder's destructor, on every path (destroy, a refused construction, an exception caught by the
// barrier).  The holders never synchronise when they release: oth_*_destroy drains the stream before it deletes the
// object, ensure() before it replaces a buffer that queued work may still read.
#pragma once
#include "../../include/ofdm_tools_hip.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <string>
#include <utility>

struct oth_ctx;

namespace oth {
int fail(oth_ctx *c, int code, const std::string &msg);
hipStream_t ctx_stream(const oth_ctx *c);      // c->stream (oth_ctx is defined behind the holders it is made of)

#define HIPCHK(c, expr)                                                                                 \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail((c), OTH_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

// what the holders of this process hold right now (oth__debug_live_resources)
inline std::atomic<int> g_live_device{0}, g_live_pinned{0}, g_live_events{0};

// A refused allocation is reported by its return value; the runtime's last-error slot is cleared, or the next launch
// (whose launcher reads that slot) would report it again.
inline hipError_t refused(hipError_t e) {
    (void)hipGetLastError();
    return e;
}

// Device memory: the pointer and its capacity in bytes.
template <typename T> class DevBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept {      // a swap: `o` releases what this held
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }      // for the kernel argument structs
    explicit operator bool() const { return p_ != nullptr; }

    void reset() {
        if (p_ && hipFree(p_) == hipSuccess) --g_live_device;
        p_ = nullptr;
        cap_ = 0;
    }

    // a fresh buffer of exactly `bytes` (the tables of fixed size)
    hipError_t alloc(size_t bytes) {
        reset();
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return refused(e);
        p_ = static_cast<T *>(p);
        cap_ = bytes;
        ++g_live_device;
        return hipSuccess;
    }

    // alloc + asynchronous copy of a host table on the context's stream: the caller synchronises before the table dies
    hipError_t upload(oth_ctx *c, const void *host, size_t bytes) {
        const hipError_t e = alloc(bytes);
        return e != hipSuccess ? e : hipMemcpyAsync(p_, host, bytes, hipMemcpyHostToDevice, ctx_stream(c));
    }

    // at least need_bytes, contents undefined: a short buffer is replaced once the stream has drained (a queued launch
    // never reads a freed buffer)
    int ensure(oth_ctx *c, size_t need_bytes) {
        if (cap_ >= need_bytes && p_) return OTH_OK;
        if (p_) {
            HIPCHK(c, hipStreamSynchronize(ctx_stream(c)));
            reset();
        }
        const hipError_t e = alloc(need_bytes);
        if (e != hipSuccess) return fail(c, OTH_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        return OTH_OK;
    }

    // grow (by a quarter more than asked) while keeping the first keep_bytes
    int ensure_keep(oth_ctx *c, size_t need_bytes, size_t keep_bytes) {
        if (cap_ >= need_bytes && p_) return OTH_OK;
        DevBuf grown;
        const hipError_t e = grown.alloc(need_bytes + need_bytes / 4);
        if (e != hipSuccess) return fail(c, OTH_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        if (p_) {
            if (keep_bytes) HIPCHK(c, hipMemcpyAsync(grown.p_, p_, keep_bytes, hipMemcpyDeviceToDevice, ctx_stream(c)));
            HIPCHK(c, hipStreamSynchronize(ctx_stream(c)));
        }
        *this = std::move(grown);
        return OTH_OK;
    }
};

// Pinned (device-visible) host memory.
template <typename T> class PinnedBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;

public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept { *this = std::move(o); }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~PinnedBuf() { reset(); }

    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

    void reset() {
        if (p_ && hipHostFree(p_) == hipSuccess) --g_live_pinned;
        p_ = nullptr;
        cap_ = 0;
    }

    hipError_t alloc(size_t bytes) {
        reset();
        void *p = nullptr;
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return refused(e);
        p_ = static_cast<T *>(p);
        cap_ = bytes;
        ++g_live_pinned;
        return hipSuccess;
    }

    // at least `bytes` (the staging rings): a short buffer is replaced by one half as large again (+ 4 KiB), so that a
    // caller whose chunks grow slowly does not reallocate on every call.  The caller has waited for the slot's last reader.
    int grow(oth_ctx *c, size_t bytes) {
        if (cap_ >= bytes) return OTH_OK;
        const hipError_t e = alloc(bytes + bytes / 2 + 4096);
        if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        return OTH_OK;
    }
};

// An event, created on first use.
class Event {
    hipEvent_t ev_ = nullptr;

public:
    Event() = default;
    Event(Event &&o) noexcept { *this = std::move(o); }
    Event &operator=(Event &&o) noexcept {
        std::swap(ev_, o.ev_);
        return *this;
    }
    ~Event() { reset(); }

    hipEvent_t get() const { return ev_; }
    explicit operator bool() const { return ev_ != nullptr; }

    void reset() {
        if (ev_ && hipEventDestroy(ev_) == hipSuccess) --g_live_events;
        ev_ = nullptr;
    }

    // no-op when the event exists
    hipError_t create(unsigned flags = hipEventDisableTiming) {
        if (ev_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&ev_, flags);
        if (e != hipSuccess) ev_ = nullptr;
        else ++g_live_events;
        return e;
    }
};
}  // namespace oth
