// What the host files of the per-bin statistics (abi_ftest, abi_sk, abi_jack, abi_adapt, abi_cyc, abi_lag, abi_mat, abi_eig, abi_doa, abi_gcc, abi_pfb; mtm_run for the work split
// and the recipe) share: the size rule, the plan and stream-shape refusals, the kernel arguments a Welch statistic takes from
// its plan, the work split over resident workgroups, the recipe text, the timed launch, the host and device forms around a
// device run, and the replacement of a plan's tables.
#pragma once
#include "abi_state.h"

namespace oth {
// the transform lengths the taper-loop kernels are built for (OTH_MTM_FOR_EACH_N)
inline bool stat_size(int nfft) { return nfft >= 64 && nfft <= 16384 && (nfft & (nfft - 1)) == 0; }

// What kind of plan a statistic of Welch segments (`what`: "the cyclic spectrum") takes, in the header's order: no
// multitaper plan - its segments' `segments` ("transforms") are Welch's -, no median - `rows` ("its rows are means") over
// segments -, a size the kernels are built for.
inline int welch_stat_plan(oth_plan *p, const std::string &what, const char *segments = "transforms", const char *rows = "its rows are means") {
    oth_ctx *c = p->ctx;
    if (p->ntapers) return refuse_mtm(p, what.c_str(), ("its segments' " + std::string(segments) + " are Welch's (oth_welch_plan)").c_str());
    if (p->average == OTH_AVERAGE_MEDIAN)
        return fail(c, OTH_ERR_UNSUPPORTED, what + " is not available with OTH_AVERAGE_MEDIAN: " + rows +
                                                " over segments (oth_plan_set_average(OTH_AVERAGE_MEAN) first)");
    if (!stat_size(p->nfft))
        return fail(c, OTH_ERR_UNSUPPORTED, what + " takes a transform length that is a power of two from 64 to 16384, not " + std::to_string(p->nfft));
    return OTH_OK;
}

// The refusals of a statistic's stream shape in their common order - "bad argument" (args_ok: the caller's pointers), the
// stride, the input's length (a segment reaches `reach` samples past its nperseg - the caf's largest lag, the filter bank's
// ntaps - 1 transform lengths -, and too_short is
// the refusal's text where that is not 0), the stream limit (too_many: its text; nullptr where the caller has tested it in
// front) - and the segment count.  A family's check calls it where that keeps the family's precedence.
inline int stream_shape(oth_plan *p, bool args_ok, size_t nsamples, int nstreams, size_t stride, const char *too_many, long long *nseg,
                        size_t reach = 0, const char *too_short = "input shorter than nperseg") {
    oth_ctx *c = p->ctx;
    if (!args_ok || nstreams < 1) return fail(c, OTH_ERR_INVALID, "bad argument");
    if (nstreams > 1 && stride < nsamples) return fail(c, OTH_ERR_INVALID, "stream_stride < nsamples");
    if (nsamples < reach + (size_t)p->nperseg) return fail(c, OTH_ERR_INVALID, too_short);
    if (too_many && nstreams > 65535) return fail(c, OTH_ERR_UNSUPPORTED, too_many);
    *nseg = (long long)((nsamples - reach - (size_t)p->noverlap) / (size_t)p->step);
    return OTH_OK;
}
constexpr const char *kMtmTooMany = "multitaper plans take at most 65535 streams per launch";

// The fields the kernel arguments of the Welch statistics share (Args: WelchSkArgs, WelchCycArgs, WelchLagArgs, WelchPfbArgs), from the plan
// and the launch's shape, as mtm_args does for the taper loop; the rest of Args stays zero for the caller.  WelchMatArgs
// names three of them after its channels (chan_stride, wg_count, nchan) and fills its own; WelchPfbArgs.win is the prototype,
// which its caller puts in the window's place.
template <typename Args> Args welch_stat_args(const oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, int W) {
    Args a{};
    a.x = x;
    a.win = p->d_win.get();
    a.tw = p->d_tw;
    a.partial = p->d_partial.get();
    a.nseg = nseg;
    a.stream_stride = stride;
    a.nperseg = p->nperseg;
    a.step = p->step;
    a.detrend = p->detrend != OTH_DETREND_NONE;
    a.wg_per_stream = W;
    a.nstreams = nstreams;
    return a;
}

// Workgroups per stream of a launch whose streams' work items (segments, or (segment, taper) pairs) go to workgroups in
// contiguous runs: what the device holds at once (bpc per CU over launch_streams streams and groups), min_per_stream at
// least, an item each at most.
inline int segment_workgroups(const oth_ctx *c, long long items, long long min_per_stream, long long launch_streams, int bpc) {
    const long long resident = (long long)c->cu_count * bpc;
    return (int)std::min(items, std::max(min_per_stream, resident / launch_streams));
}

// last_recipe of a taper-loop launch: `front` (" ntapers=7 iters=4") follows nfft, `back` (" ncyc=3 group=2") the work split
inline std::string stat_recipe(const char *kernel, const oth_plan *p, const std::string &front, int W, long long nseg, int nstreams,
                               const std::string &back, int bpc) {
    return std::string("kernel=") + kernel + " nfft=" + std::to_string(p->nfft) + front + " W=" + std::to_string(W) +
           " nseg=" + std::to_string(nseg) + " nstreams=" + std::to_string(nstreams) + back + " bpc=" + std::to_string(bpc);
}

// one launch between the context's timing events
#define TIMED_LAUNCH(c, call) \
    do {                      \
        Timed tm_(c);         \
        HIPCHK(c, call);      \
    } while (0)

// A row of a host form: where the caller wants it (nullptr: not at all) and its length in floats.
struct HostRow {
    float *host;
    size_t floats;
};

// The host form of a statistic after its check: stages x (and y behind it) unless they are device memory, lays the R rows
// out in p->d_out one behind the other - never below 5 nfft floats, which the plan's other calls count on - and calls
// run(dx, dy, dev) with the rows' device addresses, nullptr for a row the caller left out; then one copy per wanted row,
// the wait, and nseg_out.
template <size_t R, typename Run>
int host_form(oth_plan *p, const void *x, const void *y, size_t nsamples, int src_is_device, const HostRow (&rows)[R], long long nseg,
              uint64_t *nseg_out, Run run) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const float2 *dx = (const float2 *)x, *dy = (const float2 *)y;
    if (!src_is_device) {
        const size_t bytes = nsamples * sizeof(float2);
        if (int rc = p->d_stage.ensure(c, (y ? 2 : 1) * bytes)) return rc;
        dx = p->d_stage.get();
        HIPCHK(c, hipMemcpyAsync(p->d_stage.get(), x, bytes, hipMemcpyHostToDevice, c->stream));
        if (y) {
            dy = dx + nsamples;
            HIPCHK(c, hipMemcpyAsync(p->d_stage.get() + nsamples, y, bytes, hipMemcpyHostToDevice, c->stream));
        }
    }
    size_t total = 0;
    for (const HostRow &r : rows) total += r.floats;
    if (int rc = p->d_out.ensure(c, sizeof(float) * std::max(total, 5 * (size_t)p->nfft))) return rc;
    float *dev[R], *at = p->d_out.get();
    for (size_t r = 0; r < R; ++r) {
        dev[r] = rows[r].host ? at : nullptr;
        at += rows[r].floats;
    }
    if (int rc = run(dx, dy, dev)) return rc;
    for (size_t r = 0; r < R; ++r)
        if (dev[r]) HIPCHK(c, hipMemcpyAsync(rows[r].host, dev[r], sizeof(float) * rows[r].floats, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nseg_out) *nseg_out = (uint64_t)nseg;
    return OTH_OK;
}

// The _dev form of a statistic between its OTH_TRY and OTH_CATCH: the plan, check(&nseg) - every refusal -, run(nseg), nseg_out.
template <typename Check, typename Run> int dev_form(oth_plan *p, uint64_t *nseg_out, Check check, Run run) {
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = check(&nseg)) return rc;
    if (int rc = run(nseg)) return rc;
    if (nseg_out) *nseg_out = (uint64_t)nseg;
    return OTH_OK;
}

// abi_mat.hip: the matrix family's averaging launch after its check, shared by oth_welch_matrix*, oth_welch_matrix_eig*
// (abi_eig.hip), oth_welch_matrix_doa* (abi_doa.hip) and oth_welch_matrix_gcc* (abi_gcc.hip) - workspaces, launch_welch_mat, the finalize arguments with their rows left NULL, the recipe text
int welch_mat_sums(oth_plan *p, const float2 *x, long long nseg, int nchan, size_t stride, MatFinalizeArgs &f, std::string &recipe);

// Fresh device tables take the place of a plan's earlier ones only when they are complete: launches queued on the old ones
// drain first, `upload` fills fresh holders, and the stream is awaited also after a failure - the host tables die with the
// caller.  On OTH_OK the caller moves the holders into the plan.
template <typename Upload> int upload_tables(oth_ctx *c, const char *who, Upload upload) {
    if (use_device(c)) return OTH_ERR_HIP;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipError_t e = upload();
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, OTH_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return OTH_OK;
}
}  // namespace oth
