// Private header of the host files of the C ABI (abi_*.hip): the context, plan and chain state, the helpers every entry
// point uses, and the functions one host file calls in another.  The library exports the oth_* entry points only
// (abi_exports.map); everything declared here stays inside it.
#pragma once
#include "../../include/ofdm_tools_hip.h"
#include "oth_internal.h"
#include "abi_barrier.h"
#include "abi_mem.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

using namespace oth;

struct oth_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int cu_count = 256;
    std::string err;
    std::string name;
    bool timing = false;
    std::vector<std::pair<Event, Event>> events;      // timing pairs recorded since the last oth_ctx_get_timing
    std::vector<std::pair<Event, Event>> free_events;
    double total_ms = 0.0;
    uint64_t launches = 0;
    std::map<int, DevBuf<float2>> twiddles;      // W_n^k per length (get_twiddles): plans, chains and tables borrow them
    DevBuf<float> sink;
    DevBuf<double> acc4;
    DevBuf<unsigned> queue;            // 64 chunk tickets for the dynamic segment schedule
    unsigned *done_count = nullptr;    // arrival counter of a finalize launch that signals a polling host (FinalizeArgs):
                                       // word 64 of `queue`
    std::recursive_mutex mu;           // every entry point that takes this context (or a plan / chain of it) holds it
    bool queue_clean = false;          // all zero on the stream's timeline (finalize_kernel re-zeroes what a launch used)
    int queue_used = 0;                // counters the last averaging launch drew from
    DevBuf<unsigned char> scratch;     // device scratch of the small ops (channel power, decision stage, xcorr): grown on
                                       // demand, never freed per call
    // channel slice bounds of the decision stage (oth_scan_decide_dev*): a scanner passes the same lo / hi on every
    // call, so they live on the device and are uploaded again only when their contents change - through a pinned
    // staging buffer, so that the upload is a real asynchronous copy (from pageable memory hipMemcpyAsync may hold the
    // host until the stream has drained, which would make the "asynchronous" entry points wait for the PSD kernels)
    std::vector<int> bounds_host;      // lo[nch] then hi[nch], as last uploaded
    DevBuf<int> d_bounds;
    PinnedBuf<int> h_bounds;
    Event bounds_ev;                   // behind the last upload: the pinned words may be rewritten after it
    ~oth_ctx() {
        if (own_stream) hipStreamDestroy(stream);
    }
};

// Device tables and scratch of the any-length route (fft_any.hip) of one plan / chain
struct AnyTables {
    AnyShape sh{};                     // kind ANY_NONE: not in use
    const float2 *tw = nullptr;        // W_L^k, L entries (borrowed: the context's twiddle cache owns it)
    DevBuf<float2> chirp;              // Bluestein c[n] = exp(-i pi n^2 / nfft), nfft entries
    DevBuf<float2> midtab;             // Bluestein FFT_M(conj c) / M, M entries by natural index
    DevBuf<float2> ws;                 // workspace [channel][segment of the chunk][L]
    DevBuf<float4> mean;               // [channel][segment of the chunk] hi / lo means
};

struct oth_plan {
    oth_ctx *ctx = nullptr;
    int nfft = 0, nperseg = 0, noverlap = 0, step = 0, detrend = 0, scaling = 0, fftshift = 0, trim = 0;
    int db = 0, kernel = OTH_KERNEL_AUTO, sched = OTH_SCHED_DYNAMIC;
    double fs = 1.0, scale = 1.0;      // scale applies to the MEAN over segments
    DevBuf<float> d_win;
    const float2 *d_tw = nullptr;      // borrowed: the context's twiddle cache owns it
    DevBuf<float4> d_fd;               // window spectrum for the frequency-domain detrend (welch4096ws), or empty
    DevBuf<float4> d_fd1x;             // the same for welch16k1x_half_kernel (16384 points, spectrum confined to |k| < 16)
    DevBuf<float2> d_pilot;            // per-stream pilots of the frequency-domain detrend (WelchArgs.pilot)
    bool fast_detrend = false;         // OTH_DETREND_CONSTANT_FAST: the builds without the pilot (WelchArgs.pilot)
    bool rect_window = false;          // every window value is 1 (window == NULL or boxcar): builds without the multiply
    bool compl_window = false;         // w[n] + w[n + nfft / 2] = 1 to one float32 ulp (window_is_complementary, abi_welch.hip)
                                       // and, in a detrending plan, a spectrum inside [-136, 120) (d_fd_sym)
    DevBuf<float2> d_symtw;            // compl_window: WelchArgs.symtw
    DevBuf<float2> d_fd_sym;           // compl_window, detrending: WelchArgs.fd_sym
    DevBuf<float> d_partial;
    DevBuf<float> d_reduce;            // stage-1 output of the two-stage partial-sum reduction
    DevBuf<float> d_out;               // [4][nfft] + pxy extra
    // Host-output ring of oth_welch_exec / _exec_async (round 5).  The finalize launch writes the PSD straight into a
    // pinned, device-visible row (no copy-engine hop) and then a completion word next to it (FinalizeArgs.host_seq);
    // the host polls that word instead of sleeping in hipStreamSynchronize.  A slot is reused kOutRing launches later.
    static constexpr int kOutRing = 4;
    PinnedBuf<float> h_out;            // [kOutRing][nfft]
    PinnedBuf<unsigned> h_seq;         // [kOutRing]: low 32 bits of the ticket whose row is complete
    uint64_t out_ticket[kOutRing] = {0, 0, 0, 0};
    uint64_t out_nseg[kOutRing] = {0, 0, 0, 0};
    uint64_t next_out_ticket = 1;
    bool pilot_launch = false;         // A/B + parity: the pilot from pilot_mean_kernel also where the kernel could form it
    std::string last_recipe;           // recipe_text() of the last averaging launch (oth__debug_last_recipe)
    DevBuf<float2> d_stage;            // host-input staging (x then y)
    // streaming state
    DevBuf<float> d_sum;               // raw sum |X|^2, natural order
    DevBuf<float> d_wpm;               // 65536-point plans on welch32k.hip: w[n] + w[n + 32768], then w[n] - w[n + 32768] (n < 32768)
    uint64_t nseg_total = 0;
    size_t carry = 0;                  // samples kept at the front of d_stream
    DevBuf<float2> d_stream;
    // launch tuning (A/B tools and the parity suite): the OTH_W4096_* environment variables are read ONCE, when
    // the plan is created; oth_plan_set_tuning() changes them afterwards.  0 / -1 / empty = library default.
    std::string tune_variant;
    int tune_sched = -1, tune_chunk = 0, tune_tail = 0;
    // pinned staging ring of the streaming form (oth_welch_accumulate): the caller's buffer is copied here, the
    // H2D copy and the kernels are enqueued, and the call returns without waiting for the GPU
    PinnedBuf<char> h_ring[4];
    Event h_ring_ev[4];                // behind the H2D copy out of the slot
    unsigned h_ring_next = 0;
    AnyTables any;                     // any.sh.kind != ANY_NONE: the plan's length runs through fft_any.hip
    // Blocking oth_welch_exec calls on one plan run one at a time (enqueue + collect under this mutex; the CONTEXT lock is
    // free while they wait): with the 4-slot output ring a fifth concurrent caller's launch would otherwise rewrite the
    // first caller's row before it was copied out (advisor, round 5).
    std::mutex exec_mu;
    int hostwait = 0;                  // 0 poll the completion word (default), 1 hipStreamSynchronize (oth_plan_set_hostwait)
    // average = OTH_AVERAGE_MEDIAN (oth_plan_set_average): the rows producer writes one raw |X|^2 row per segment into
    // d_rows ([stream][segment][nfft], grown on demand: ensure() drains the stream before it frees, so a queued ticket
    // never reads a freed buffer), median.hip selects into d_med, finalize_kernel scales by scale / bias
    int average = OTH_AVERAGE_MEAN;
    DevBuf<float> d_rows;
    DevBuf<float> d_med;               // [nstreams][nfft] medians, natural bin order
    DevBuf<unsigned> d_msel;           // radix-select scratch (median_scratch_words)
    AnyTables rows_any;                // the any-length tables of a power-of-two plan's rows (p->any serves the others)
    long long bias_nseg = 0;           // _median_bias(bias_nseg) = bias, cached
    double bias = 1.0;
    // multitaper plans (oth_mtm_plan, abi_mtm.hip): ntapers > 0; run_average hands every launch to mtm_run, d_win stays null
    int ntapers = 0;
    DevBuf<float> d_tapers;            // [ntapers][nfft], zero-extended behind nperseg
    DevBuf<float> d_coef;              // [ntapers] c_k: normalised weight (over the taper's energy with OTH_SCALE_DENSITY)
    bool mtm_csd = false;              // oth_mtm_csd_plan only: the oth_csd_* calls run mtmcsd.hip instead of being refused
    DevBuf<float2> d_mtm_ws;           // mtmcsd.hip's per-workgroup spectrum rows (MtmCsdArgs.ws; 16384 points only)
    // the harmonic F-test (oth_mtm_ftest*, mtmftest.hip): every multitaper plan carries the tapers' sums
    DevBuf<float> d_mtm_u;             // [ntapers] U_k = sum_n v_k[n] (summed in double)
    double mtm_s = 0.0;                // sum_k U_k^2 of the uploaded values
    DevBuf<float> d_ftest_ws;          // mtmftest.hip's per-workgroup sy / p rows (MtmFtestArgs.ws; 16384 points only)
    // adaptive weighting (oth_mtm_set_ratios, oth_mtm_adaptive*: abi_adapt.hip / mtmadapt.hip)
    std::vector<float> mtm_inv_g;      // [ntapers] 1 / sum_n v_k[n]^2 (summed in double; 0 for an all-zero taper)
    DevBuf<float> d_mtm_lam;           // [3][ntapers] lambda_k, max(1 - lambda_k, 0) - formed in double - and mtm_inv_g; empty
                                       // until oth_mtm_set_ratios
    DevBuf<float> d_adapt_ws;          // mtmadapt.hip's per-workgroup eigenspectra rows (MtmAdaptArgs.ws; from 1024 points on)
    // the jackknife (oth_mtm_jackknife*, oth_mtm_csd_jackknife*: abi_jack.hip / mtmjack.hip)
    bool mtm_uniform = true;           // every weight a_k is the same: the (segment, taper) items are exchangeable
    DevBuf<float> d_jack_tot;          // totals of the first pass: [nstreams][nfft], or [4][nfft] + the natural-order Cxy row
    // spectral kurtosis (oth_welch_sk*, abi_sk.hip / welchsk.hip): Welch plans only
    double sk_g = 1.0;                 // 1 / sum w^2 (1 for an all-zero window): the periodograms' scale inside the kernel
    // cyclic spectrum and coherence (oth_welch_set_cycles, oth_welch_cyclic*: abi_cyc.hip / welchcyc.hip): Welch plans only
    std::vector<float> win_host;       // the window as uploaded (nperseg values): the complex tapers are formed from it in double
    int ncycles = 0;                   // 0 until oth_welch_set_cycles
    DevBuf<float2> d_cyc_tap;          // [ncycles][nfft] w[n] e^{-j 2 pi alpha_a n}
    DevBuf<double> d_cyc_alpha;        // [ncycles]
    DevBuf<float2> d_cyc_ws;           // welchcyc.hip's per-workgroup spectrum rows (WelchCycArgs.ws; 16384 points only)
    int tune_cyc_group = 0;            // OTH_CYC_GROUP, read when the plan is created: 1, 2 or 4 forces that build of welchcyc.hip
                                       // (A/B tools and the parity suite); 0 = the library's choice
    // cyclic autocorrelation (oth_welch_set_lags, oth_welch_caf*: abi_lag.hip / welchlag.hip): Welch plans only
    int nlags = 0;                     // 0 until oth_welch_set_lags
    int lag_max = 0;                   // the largest lag of the set: the segments are counted on nsamples - lag_max
    DevBuf<int> d_lags;                // [nlags] tau_l in samples
    DevBuf<double> d_lag_means;        // welchlag.hip's per-workgroup sums of the products' means (WelchLagArgs.means)
    int tune_lag_group = 0;            // OTH_LAG_GROUP, read when the plan is created: 1 or 2 forces that build of welchlag.hip
                                       // (A/B tools and the parity suite); 0 = the library's choice
    // polyphase filter-bank PSD (oth_welch_set_prototype, oth_welch_pfb*: abi_pfb.hip / welchpfb.hip): Welch plans only
    int pfb_taps = 0;                  // taps per branch P; 0 until oth_welch_set_prototype
    DevBuf<float> d_pfb_h;             // [pfb_taps][nfft] the prototype h
    DevBuf<float> d_pfb_fold;          // [nfft] hfold[n] = sum_p h[n + p nfft], formed in double
    double pfb_sum = 0.0, pfb_sum2 = 0.0;      // sum h and sum h^2, in double
    double pfb_scale = 1.0;            // the plan's scaling with h in the window's place; applies to the MEAN over frames
    // spectral matrix of C channels (oth_welch_matrix*: abi_mat.hip / welchmat.hip): Welch plans only
    DevBuf<float2> d_mat_ws;           // welchmat.hip's per-workgroup spectrum rows (WelchMatArgs.ws; the builds that keep them in memory)
    DevBuf<double> d_mat_totals;       // [nchan][nchan][nfft]: the summed rows between its two finalize launches
    // direction spectra (oth_welch_set_steering, oth_welch_matrix_doa*: abi_doa.hip / matdoa.hip): Welch plans only
    int doa_ndir = 0, doa_nchan = 0;   // 0 until oth_welch_set_steering
    DevBuf<double> d_doa_steer;        // [2][doa_ndir][doa_nchan]: the delays tau in samples, then frac(fc tau) reduced on the host
    DevBuf<double> d_doa_basis;        // mateig.hip's basis build: [mat_eig_basis_entries(cc)][nfft] eigenvalues and vectors
};

struct oth_chain {
    oth_ctx *ctx = nullptr;
    int nfft = 0, fftshift = 0, epilogue = 0, keep_n = 1, count = 1;
    DevBuf<float> d_win;
    const float2 *d_tw = nullptr;      // borrowed: the context's twiddle cache owns it
    DevBuf<float2> d_buf;              // leftover + new samples
    size_t leftover = 0;               // samples at the front of d_buf
    DevBuf<float> d_rows;
    int do_iir = 0, do_peak = 0;
    float alpha = 0.f, kdb = 0.f;
    DevBuf<float> d_iir, d_peak;
    DevBuf<int> d_peak_init;
    DevBuf<float2> d_stage;            // host input lands here (H2D), then feeds the kernels
    DevBuf<float> d_partial;           // per-team accumulator rows of the fused kernel
    DevBuf<float> d_tail;              // group rows of the two-launch cross-team reduction
    bool peak_flag_set = false;        // d_peak_init is 1 on the stream's timeline
    bool rect = false;                 // the window is all ones (fft_vcc's `()`): the 8192 / 16384 chain skips the multiply
    int kernel = OTH_KERNEL_AUTO;      // OTH_KERNEL_GENERIC forces the coverage kernels (parity tests)
    DevBuf<float> d_out;               // rows handed back by the host-output forms
    // asynchronous work() form (oth_chain_push_async): pinned input ring + pinned latest-row ring.  A slot is
    // reused kRing tickets later; before it is written again the push waits for the event of the slot's last push that
    // enqueued work - however many dropped tickets lie in between - which costs nothing once the GPU has caught up.
    static constexpr int kRing = 4;
    PinnedBuf<char> h_in[kRing];
    PinnedBuf<float> h_row[kRing];
    Event ev[kRing];                   // recorded behind the D2H of the slot's row
    uint64_t ticket_of[kRing] = {0, 0, 0, 0};
    uint64_t nrows_of[kRing] = {0, 0, 0, 0};
    uint64_t next_ticket = 1;
    AnyTables any;                     // any.sh.kind != ANY_NONE: the chain's length runs through fft_any.hip
    // round 6: what a work()-sized push costs
    uint64_t ops = 0;                  // stream operations (asynchronous copies + kernel launches) the last push enqueued
    bool noop[kRing] = {false, false, false, false};      // the slot's ticket enqueued nothing (every vector dropped): ready at
                                                          // once; ev[slot] still belongs to the slot's last real push
    // A partial vector whose samples came (in part) from pushes chain_push_dropped skipped: d_buf holds its first
    // tail_from samples, h_tail its samples [tail_from, leftover) - copied on the host, no stream operation.  The next
    // push that enqueues work uploads them first; set_keep_one_in_n may make the vector a kept one meanwhile.
    bool leftover_stale = false;
    size_t tail_from = 0;
    PinnedBuf<float2> h_tail;          // nfft samples
    Event tail_ev;                     // recorded behind push / push_dev's upload from h_tail
    bool tail_ev_live = false;         // ... which a dropped push waits for before it rewrites h_tail
};

// Polyphase channelizer (oth_channelizer_*, abi_chan.hip / chanpfb.hip): one wideband stream in, nchan baseband rows out
struct oth_channelizer {
    oth_ctx *ctx = nullptr;
    int nchan = 0, decim = 0, ntaps = 0;
    size_t taps = 0;                   // L = ntaps nchan: the samples a frame covers
    DevBuf<float> d_h;                 // [ntaps][nchan] the prototype
    const float2 *d_tw = nullptr;      // borrowed: the context's twiddle cache owns it
    // streaming state: the samples a later frame still needs (fewer than L) sit in d_tail[cur]; a push that yields frames
    // saves its tail into the other buffer behind its launch (a push shorter than L would otherwise copy onto its own source)
    DevBuf<float2> d_tail[2];          // L samples each
    int cur = 0;
    size_t pending = 0;                // samples in d_tail[cur]
    uint64_t frames_total = 0;         // frames since creation or the last reset: the circular shift's absolute frame index
    DevBuf<float2> d_stage;            // host input lands here (H2D), then feeds the kernel
    DevBuf<float2> d_out;              // [nchan][frames] of the host-output form
    int tune_wg = 0;                   // OTH_CHAN_WG, read when the handle is created: at most that many workgroups per launch
                                       // (A/B tools and the parity suite); 0 = the library's choice
    std::string last_recipe;           // of the last push that launched (oth__debug_channelizer_recipe)
};

namespace oth {
// host chunks up to this size go through the pinned staging rings (work()-sized buffers: the copy is trivial and the
// call returns at once); larger ones use the runtime's staged copy from pageable memory directly
constexpr size_t kPinnedStageMax = 1u << 20;
// a PINNED / registered source above this size is not copied into the ring (that would pin as much again): its DMA is
// enqueued directly and the call waits for that one copy - the only case in which a push waits for the stream
constexpr size_t kPinnedRingMax = 64u << 20;

// A host buffer the runtime can DMA from directly (hipHostMalloc / hipHostRegister'd, e.g. a torch pinned tensor or a
// registered scheduler buffer): hipMemcpyAsync from it returns before the bytes are read, so the "input valid only
// during the call" contract of work() needs a copy that has finished when the call returns.  Pageable memory is
// staged by the runtime before hipMemcpyAsync returns.
bool host_ptr_is_pinned(const void *p);

// Serialises the entry points per context: GNU Radio runs each block's work() on its own thread and the
// blocks of one process share the default context (scratch buffers, ticket counters, timing events).
struct CtxGuard {
    oth_ctx *c;
    explicit CtxGuard(oth_ctx *ctx) : c(ctx) {
        if (c) c->mu.lock();
    }
    ~CtxGuard() {
        if (c) c->mu.unlock();
    }
    CtxGuard(const CtxGuard &) = delete;
    CtxGuard &operator=(const CtxGuard &) = delete;
};

// The exception barrier of the C ABI (include/ofdm_tools_hip.h: "nothing throws or aborts").  Every extern "C" body
// sits between OTH_TRY and OTH_CATCH(context): a std::bad_alloc (std::vector / std::string growth), a
// std::system_error (the context's recursive mutex) or anything else a C++ runtime call may raise becomes an error
// code + last-error text instead of std::terminate() inside the host's ctypes call.  The handlers themselves must not
// throw: the text is stored through fail_nothrow().
int fail_nothrow(oth_ctx *c, int code, const char *what) noexcept;

// OTH_TRY / OTH_CATCH(context): csrc/abi_barrier.h (shared with the host-only probe the CPU suite builds)

int use_device(oth_ctx *c);

// H2D copy of a caller's host buffer that must be consumed before the call returns, without a ring slot
int copy_in_and_wait(oth_ctx *c, void *dst, const void *src, size_t bytes);

int get_twiddles(oth_ctx *c, int nfft, const float2 **out);
std::vector<float2> symtw_table();      // WelchArgs.symtw (host)

struct Timed {
    oth_ctx *c;
    Event a, b;
    explicit Timed(oth_ctx *ctx) : c(ctx) {
        if (!c->timing) return;
        if (c->events.size() >= 8192) {   // fold what we have
            hipStreamSynchronize(c->stream);
            for (auto &ev : c->events) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, ev.first.get(), ev.second.get()) == hipSuccess) c->total_ms += ms;
                c->free_events.push_back(std::move(ev));
            }
            c->events.clear();
        }
        if (!c->free_events.empty()) {
            a = std::move(c->free_events.back().first);
            b = std::move(c->free_events.back().second);
            c->free_events.pop_back();
        } else if (a.create(hipEventDefault) != hipSuccess || b.create(hipEventDefault) != hipSuccess) {
            a.reset();
            return;
        }
        hipEventRecord(a.get(), c->stream);
    }
    ~Timed() {
        if (!a) return;
        hipEventRecord(b.get(), c->stream);
        c->events.emplace_back(std::move(a), std::move(b));
        c->launches++;
    }
};

// The interleaved schedule of a rows / chain launch of segfft.hip or welch16k.hip over a.nseg segments, for at most
// teams_max resident teams: segments per chunk 8 once every team gets two chunks (+2-4 % over 4), fewer for short
// launches so that more teams take part; chunk c goes to team c mod wg_per_stream.
inline void interleaved_chunks(SegArgs &a, long long teams_max) {
    a.chunk = a.nseg >= 16 * teams_max ? 8 : (a.nseg >= 4 * teams_max ? 4 : 2);
    const long long nchunks = (a.nseg + a.chunk - 1) / a.chunk;
    a.wg_per_stream = (int)std::max(1LL, std::min(teams_max, nchunks));
    a.sched = 1;
    a.tail_chunk = a.chunk;
    a.nbig = a.nseg / a.chunk;
}

// ---- abi_route.hip: which kernel build runs a launch ---------------------------------------------------------------------
// Build variants of the welch4096 kernel; OTH_W4096_VARIANT=<tag> selects one (experiments only).
struct W4096Variant {
    const char *tag;
    hipError_t (*launch)(const WelchArgs &, hipStream_t);
    int (*blocks_per_cu)();
    int chunk;      // default segments per chunk of the dynamic schedule (same-box A/B, tools/archive/ab_variants.py)
    bool fd;        // detrends in the frequency domain: needs WelchArgs.fd (a window with a confined spectrum)
    bool inline_pilot = false;      // forms the pilot of the constant detrend in its own prologue (WelchArgs.pilot_inline)
};
bool w4096_variant_known(const char *tag);      // a tag of abi_route.hip's table of builds (oth_plan_set_tuning)

enum RecipeKernel {
    RK_GENERIC = 0,      // welch_generic_kernel (coverage Stockham kernel; also the two-channel coverage path)
    RK_W4096,            // welch4096[ws]_kernel: the build in `variant`
    RK_CSD4096,          // csd4096_kernel (one role)
    RK_CSD4096WS,        // csd4096ws_kernel (role-split pairs)
    RK_W16K,             // welch16k_kernel<., F> (4 x 4096 / 2 x 4096)
    RK_W16K1X,           // welch16k1x_pipe_kernel / welch16k1x_kernel (one exchange, no overlap)
    RK_W16K1X_HALF,      // welch16k1x_half_kernel (one exchange, 50 % overlap)
    RK_SEG,              // seg_kernel<R, ...>
    RK_SEGWS,            // segws_kernel<R, DET>
    RK_SEGPAD,           // seg_kernel<R, ..., NA> zero-padded
    RK_ANY,              // any_fft_kernel launches (fft_any.hip): lengths the kernels above do not take
};
extern const char *const kAnyKindName[];      // AnyKind -> name

// what resolve_recipe() needs to know of a plan (oth_plan holds the same fields; the debug entry builds one by hand)
struct PlanShape {
    int nfft = 0, nperseg = 0, step = 0;
    bool detrend = false, fast_detrend = false;
    bool fd_ok = false;          // a window-spectrum table exists for this size (oth_plan::d_fd)
    bool fd1x_ok = false;        // ... and the one for welch16k1x_half (spectrum confined to |k| < 16)
    bool rect_window = false;
    int kernel = OTH_KERNEL_AUTO, sched = OTH_SCHED_DYNAMIC;
    bool pilot_launch = false;
    std::string tune_variant;
    int tune_sched = -1, tune_chunk = 0, tune_tail = 0;
    AnyShape any{};              // kind != ANY_NONE: the any-length route
};

// resident workgroups (teams) per CU of a tuned build: the runtime asks the occupancy calculator (needs a device), the
// debug entry uses abi_route.hip's table_bpc - what the calculator returns on MI355X for the shipped builds
// (tests/test_hip_parity.py::test_recipe_occupancy_table_matches_the_runtime compares the two on the GPU)
struct OccupancyKey {
    RecipeKernel kern;
    const char *variant;      // RK_W4096
    int nfft, nperseg, seg_kind;
    bool seg_wps4;
    bool half_ws;             // RK_W16K1X_HALF at 8192 points: the role-split build (one 1024-thread workgroup per CU)
};
int runtime_bpc(const OccupancyKey &k);

struct LaunchRecipe {
    RecipeKernel kern = RK_GENERIC;
    const W4096Variant *variant = nullptr;      // RK_W4096
    bool csd = false;
    int form = 0;                // constant detrend: 0 none, 1 before the window (time domain), 2 after the transform (needs the table)
    int pilot = 0;               // 0 none (no detrend, or OTH_DETREND_CONSTANT_FAST), 1 pilot_mean_kernel in front, 2 in the kernel's prologue
    bool use_fd1x = false;       // the table handed to the kernel is d_fd1x
    int seg_kind = 0, seg_det = 0;
    bool seg_wps4 = false;
    bool x1_window = false, x1_plain = false;      // RK_W16K1X: windowed build / the un-pipelined loop
    bool half_ws = false;                          // RK_W16K1X_HALF, 8192 points: welch8kws_kernel
    int bpc = 0;                 // resident workgroups (teams) per CU (0: generic grid rule)
    int W = 1, nch = 1;
    RowLayout layout = ROW_NATURAL;
    int sched = 0, chunk = 1, tail_chunk = 1;
    long long nbig = 0;
    bool tickets = false;        // draws chunk tickets from the context's queue
    int any_kind = 0;            // RK_ANY: AnyKind
    bool any_r16 = false;        // ... on fft_tl.hip's register radix-16 kernels (32768 / 65536 points)
    bool any_onewg = false;      // ... 32768 points, one channel, full segments: welch32k.hip (the segment never leaves the CU)
};

// -> OTH_OK, or OTH_ERR_UNSUPPORTED with *why set (OTH_KERNEL_TUNED on a plan no tuned kernel covers)
int resolve_recipe(const PlanShape &p, bool csd, long long nseg, int nstreams, int cu_count, int (*bpc_of)(const OccupancyKey &),
                   LaunchRecipe *out, const char **why);
std::string recipe_text(const LaunchRecipe &r, int nfft);
PlanShape shape_of(const oth_plan *p);

// ---- abi_any.hip: the any-length host driver (fft_any.hip, fft_tl.hip, welch32k.hip) --------------------------------------
int any_tables_init(oth_ctx *c, int nfft, AnyTables *t);
int any_partial_rows(const AnyShape &sh, long long nseg, int cu_count);
int any_run(oth_ctx *c, AnyTables &t, const float2 *x, const float2 *y, long long first, long long seg_step, int nperseg,
            const float *win, bool detrend, long long nseg, float *partial, int W, float *rows, int epilogue, float scale,
            int fftshift, bool coverage_only = false);
// points of scratch any_fft_nat() needs behind the data
inline size_t any_fft_nat_scratch(const AnyShape &sh) { return 2 * (size_t)sh.L; }
int any_fft_nat(oth_ctx *c, const AnyTables &t, float2 *data, float2 *scratch);
void host_fft_pow2(std::vector<double> &re, std::vector<double> &im);

// ---- the finalize launch of a plan ---------------------------------------------------------------------------------------------
// the plan's output stage, and the one of the raw forms (partial, accumulate, the time-sharded sums): natural order, no dB
inline OutStage out_stage(const oth_plan *p) { return OutStage{p->fftshift, p->trim, p->db, p->nfft - 2 * p->trim}; }
inline OutStage raw_stage(const oth_plan *p) { return OutStage{0, 0, 0, p->nfft}; }

// finalize_kernel's view of W partial rows of nch channels per stream in `layout`, as the plan's averaging launch leaves them
// in d_partial (reduced through d_reduce), leaving through `stage`.  The caller adds the outputs, scale and accumulate.
inline FinalizeArgs finalize_args(const oth_plan *p, int W, RowLayout layout, int nch, const OutStage &stage) {
    FinalizeArgs f{};
    f.partial = p->d_partial.get();
    f.scratch = p->d_reduce.get();
    f.W = W;
    f.nfft = p->nfft;
    f.nch = nch;
    f.layout = layout;
    f.l1 = p->any.sh.L1, f.l2 = p->any.sh.L2;
    f.out = stage;
    return f;
}

// ---- abi_welch.hip -----------------------------------------------------------------------------------------------------------
// What oth_welch_plan and oth_mtm_plan share: the checks of the arguments both take, then a fresh plan on the context's
// device with the common fields set (the detrend code normalised, OTH_HOSTWAIT read).  The caller adds its tables.
int plan_begin(oth_ctx *c, int nfft, int nperseg, int noverlap, int detrend, int scaling, double fs, int fftshift, int trim_bins,
               std::unique_ptr<oth_plan> *out);

// ---- abi_mtm.hip: multitaper plans ------------------------------------------------------------------------------------------
// the averaging launch of a multitaper plan (run_average branches here before resolve_recipe): W partial rows per stream
// in natural order (ROW_NATURAL) into p->d_partial
//   y != nullptr (plans of oth_mtm_csd_plan only): the two-channel launch, four rows per workgroup
int mtm_run(oth_plan *p, const float2 *x, const float2 *y, long long nseg, int nstreams, size_t stride, int *W_out);
// the launch description the taper-loop kernels share, from the plan's tables and sizes (partial: p->d_partial as it is now)
MtmArgs mtm_args(const oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, int W);
// OTH_ERR_UNSUPPORTED with the reason: `what` is not available on a multitaper plan
int refuse_mtm(oth_plan *p, const char *what, const char *why);
// the oth_csd_* entry points: OTH_OK on a plan that holds two channels (every plan but oth_mtm_plan's), else refuse_mtm
int mtm_csd_gate(oth_plan *p, const char *what);
}  // namespace oth
