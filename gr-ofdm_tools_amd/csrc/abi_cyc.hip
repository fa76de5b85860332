// C ABI, host side: cyclic spectrum and cyclic coherence of a Welch plan (oth_welch_set_cycles, oth_welch_cyclic / _dev) -
// the cycle set's tables, the checks, the (W, nstreams, groups) launch of welchcyc.hip and its finalize launch into the
// scf, coh and PSD rows.
#include "abi_stat.h"

namespace {
// What kind of plan takes cycle frequencies: shared by set_cycles and the exec entry points, in the header's order.
int cyc_plan_check(oth_plan *p) { return welch_stat_plan(p, "the cyclic spectrum"); }

// Every refusal of the two exec entry points, before anything is allocated, staged or launched.
int cyc_check(oth_plan *p, const void *x, size_t nsamples, int nstreams, size_t stride, const float *coh_out, long long *nseg_out) {
    oth_ctx *c = p->ctx;
    if (int rc = cyc_plan_check(p)) return rc;
    if (!p->ncycles) return fail(c, OTH_ERR_UNSUPPORTED, "the cyclic spectrum needs its cycle frequencies: call oth_welch_set_cycles on this plan");
    return stream_shape(p, x && coh_out, nsamples, nstreams, stride, "the cyclic spectrum takes at most 65535 streams per launch", nseg_out);
}

// Cycle frequencies per workgroup: welchcyc.hip's three builds (GA = 1, 2, 4).  A grouped build transforms X once per segment
// for up to GA cycle frequencies - 1 + GA transforms instead of 2 GA - and pays in registers: at 4096 points GA = 4 leaves one
// workgroup per CU against two, from 8192 points on its sums live in memory (GA = 2: from 16384).  Measured
// (profiles/welch_cyclic_ab.txt; ms of GA = 2 / GA = 4 over GA = 1, 64 short streams / one long capture):
//   one cycle frequency   nothing to share: GA = 1 (GA = 4 at 4096 points x1.28 / x1.35).
//   up to 4096 points     GA = 2: at 4096 points x0.74 ... 0.88 for every A >= 2 against x0.82 ... 1.10; at 256 points the
//                         three lie within 10 % of each other but for A = 16.  64, 128, 512 ... 2048 points go with these - the
//                         sums are registers in every build there - by analogy, not by a measurement.
//   8192 points           GA = 2 (x0.84 / 0.80 at A = 2, x0.79 / 0.74 at 4, x0.76 / 0.73 at 16: level with GA = 4 or ahead),
//                         but three cycle frequencies as one group of GA = 4 (x0.67 / 0.80 against x0.79 / 0.93 for 2 + 1).
//   16384 points          GA = 4 from three on (x0.63 ... 0.76 against x0.75 ... 0.88); two: GA = 2, the same launch.
int cyc_group(const oth_plan *p, int ncyc) {
    if (p->tune_cyc_group == 1 || p->tune_cyc_group == 2 || p->tune_cyc_group == kCycGroup) return p->tune_cyc_group;
    if (ncyc <= 2) return ncyc;
    if (p->nfft <= 4096) return 2;
    if (p->nfft == 8192) return ncyc == 3 ? kCycGroup : 2;
    return kCycGroup;
}

// after cyc_check: device in, device out
int cyc_run(oth_plan *p, const float2 *x, long long nseg, int nstreams, size_t stride, float *scf_out, float *coh_out, float *psd_out) {
    oth_ctx *c = p->ctx;
    if (use_device(c)) return OTH_ERR_HIP;
    const int N = p->nfft, A = p->ncycles;
    const int ga = cyc_group(p, A), G = (A + ga - 1) / ga, R = 1 + 3 * ga;
    // whole segments go to W workgroups per stream and group in contiguous runs: what the device holds at once, a segment at least
    const int bpc = std::max(1, welch_cyc_blocks_per_cu(N, ga));
    const int W = segment_workgroups(c, nseg, 1, (long long)nstreams * G, bpc);
    const size_t slots = (size_t)nstreams * G * W;
    if (int rc = p->d_partial.ensure(c, sizeof(float) * slots * R * N)) return rc;
    if (const size_t pts = welch_cyc_ws_points(N))
        if (int rc = p->d_cyc_ws.ensure(c, sizeof(float2) * slots * pts)) return rc;
    WelchCycArgs a = welch_stat_args<WelchCycArgs>(p, x, nseg, nstreams, stride, W);
    a.ctap = p->d_cyc_tap.get();
    a.alpha = p->d_cyc_alpha.get();
    a.ws = p->d_cyc_ws.get();
    a.ncyc = A;
    CycFinalizeArgs f{};
    f.partial = p->d_partial.get();
    f.scf_out = scf_out;
    f.coh_out = coh_out;
    f.psd_out = psd_out;
    f.scf_scale = p->scale / (double)nseg;
    f.W = W;
    f.G = G;
    f.ga = ga;
    f.ncyc = A;
    f.nfft = N;
    f.out = out_stage(p);
    TIMED_LAUNCH(c, launch_welch_cyc(N, ga, G, a, c->stream));
    TIMED_LAUNCH(c, launch_cyc_finalize(f, nstreams, c->stream));
    p->last_recipe = stat_recipe("welchcyc", p, "", W, nseg, nstreams, " ncyc=" + std::to_string(A) + " group=" + std::to_string(ga), bpc);
    return OTH_OK;
}
}  // namespace

extern "C" {
int oth_welch_set_cycles(oth_plan *p, int ncycles, const double *alphas) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    oth_ctx *c = p->ctx;
    if (int rc = cyc_plan_check(p)) return rc;
    if (ncycles < 1 || ncycles > kCycMax) return fail(c, OTH_ERR_INVALID, "ncycles must lie in 1 ... " + std::to_string(kCycMax));
    if (!alphas) return fail(c, OTH_ERR_INVALID, "alphas is NULL");
    for (int a = 0; a < ncycles; ++a)
        if (!std::isfinite(alphas[a]) || std::fabs(alphas[a]) > 0.5)
            return fail(c, OTH_ERR_INVALID, "every cycle frequency must be finite with |alpha| <= 0.5 cycles per sample");
    // w[n] e^{-j 2 pi alpha n} in double, rounded once; alpha n < 2^13 turns, so its fraction is good to 2^-40
    const int N = p->nfft, L = p->nperseg;
    std::vector<float2> tab((size_t)ncycles * N, make_float2(0.f, 0.f));
    const double two_pi = 6.283185307179586476925286766559;
    for (int a = 0; a < ncycles; ++a) {
        for (int n = 0; n < L; ++n) {
            const double turns = alphas[a] * (double)n, ang = two_pi * (turns - std::rint(turns)), w = (double)p->win_host[n];
            tab[(size_t)a * N + n] = make_float2((float)(w * std::cos(ang)), (float)(-w * std::sin(ang)));
        }
    }
    DevBuf<float2> taps;
    DevBuf<double> alpha;
    if (int rc = upload_tables(c, "oth_welch_set_cycles", [&] {
            const hipError_t e = taps.upload(c, tab.data(), sizeof(float2) * tab.size());
            return e != hipSuccess ? e : alpha.upload(c, alphas, sizeof(double) * ncycles);
        }))
        return rc;
    p->d_cyc_tap = std::move(taps);
    p->d_cyc_alpha = std::move(alpha);
    p->ncycles = ncycles;
    return OTH_OK;
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_cyclic_dev(oth_plan *p, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, float *scf_out_dev,
                         float *coh_out_dev, float *psd_out_dev, uint64_t *nseg_out) {
    OTH_TRY
    return dev_form(p, nseg_out, [&](long long *nseg) { return cyc_check(p, iq_dev, nsamples, nstreams, stream_stride, coh_out_dev, nseg); },
                    [&](long long nseg) {
                        return cyc_run(p, (const float2 *)iq_dev, nseg, nstreams, stream_stride, scf_out_dev, coh_out_dev, psd_out_dev);
                    });
    OTH_CATCH((p ? p->ctx : nullptr))
}

int oth_welch_cyclic(oth_plan *p, const void *iq, size_t nsamples, int src_is_device, float *scf_out, float *coh_out, float *psd_out,
                     uint64_t *nseg_out) {
    OTH_TRY
    CtxGuard guard_(p ? p->ctx : nullptr);
    if (!p) return fail(nullptr, OTH_ERR_INVALID, "plan is NULL");
    long long nseg = 0;
    if (int rc = cyc_check(p, iq, nsamples, 1, nsamples, coh_out, &nseg)) return rc;
    const size_t nout = (size_t)(p->nfft - 2 * p->trim), rows_a = (size_t)p->ncycles * nout;
    const HostRow rows[] = {{coh_out, rows_a}, {scf_out, 2 * rows_a}, {psd_out, nout}};      // [A][nout] coh, [A][nout] scf pairs, the PSD row
    return host_form(p, iq, nullptr, nsamples, src_is_device, rows, nseg, nseg_out,
                     [&](const float2 *dx, const float2 *, float *const *dev) { return cyc_run(p, dx, nseg, 1, nsamples, dev[1], dev[0], dev[2]); });
    OTH_CATCH((p ? p->ctx : nullptr))
}
}  // extern "C"
