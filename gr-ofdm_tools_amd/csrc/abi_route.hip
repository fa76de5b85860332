// C ABI, host side.
#include "abi_state.h"

// ---- routing as data (round 5) ---------------------------------------------------------------------------------------
// Which kernel build runs a launch, with which detrend form, pilot, schedule, chunk sizes, grid and partial-row layout,
// is decided by resolve_recipe() from the plan's shape and the launch's segment count - pure host logic, no HIP call, so
// tests/test_abi_cpu.py::test_launch_recipes_table can enumerate it without a GPU through oth__debug_recipe().
// run_average() (abi_welch.hip) only allocates, fills the argument structs and dispatches on the recipe.

namespace {
// fewest segments per stream for which a detrending plan picks the frequency-domain detrend builds (run_average)
constexpr long long kFdMinSegments = 8;

const W4096Variant kVariants[] = {
    {"dpp", launch_welch_tuned4096_dpp, tuned4096_blocks_per_cu_dpp, 8, false},          // any step
    {"pipe", launch_welch_tuned4096_pipe, tuned4096_blocks_per_cu_pipe, 16, false},      // step 2048 (50 % overlap)
    {"ws", launch_welch_tuned4096_ws, tuned4096_blocks_per_cu_ws, 20, true, true},       // step 2048, confined window spectrum
};
// the three shipped builds are looked up by tag, never by position: the table is edited between rounds
const W4096Variant *variant_by_tag(const char *tag) {
    for (const auto &v : kVariants)
        if (!strcmp(v.tag, tag)) return &v;
    return &kVariants[0];
}
const W4096Variant *w4096_variant(int step, bool fd_ok, const std::string &want) {
    const W4096Variant *const dpp = variant_by_tag("dpp"), *const pipe = variant_by_tag("pipe"), *const ws = variant_by_tag("ws");
    const W4096Variant *pick = (step == 2048) ? (fd_ok ? ws : pipe) : dpp;
    if (!want.empty())
        for (const auto &v : kVariants)
            if (want == v.tag || (want == "wsgen" && !strcmp(v.tag, "ws"))) pick = &v;      // "wsgen": ws, general-window producer
    // the wave-specialised build detrends in the frequency domain: only with a confined window spectrum
    if (pick->fd && !fd_ok) pick = pipe;
    // the pipelined builds keep the overlapped half in registers: only for step = nperseg / 2
    if (pick != dpp && step != 2048) pick = dpp;
    return pick;
}

const char *const kRecipeKernelName[] = {"welch_generic", "welch4096", "csd4096", "csd4096ws", "welch16k", "welch16k1x",
                                         "welch16k1x_half", "seg", "segws", "seg_padded", "anyfft"};

int table_bpc(const OccupancyKey &k) {
    switch (k.kern) {
        case RK_W4096: return !strcmp(k.variant, "ws") ? 2 : 4;      // 78 KiB of LDS / 35 KiB and 128 VGPRs
        case RK_CSD4096: return 3;
        case RK_CSD4096WS: return 1;
        case RK_SEGWS: return k.nfft == 1024 ? 8 : 4;
        case RK_SEG: {      // teams per CU: waves per SIMD (3; "seg4": 4) x 4 SIMDs x teams per wave / waves per team
            const int tpw = k.nfft == 256 ? 4 : (k.nfft == 512 ? 2 : 1), wpt = k.nfft <= 1024 ? 1 : k.nfft / 1024;
            return 4 * (k.seg_wps4 ? 4 : 3) * tpw / wpt;
        }
        case RK_SEGPAD:      // 2048: NA = 4 at four waves per SIMD; NA = 8 at three, where the half-load pilot build takes 130 VGPRs
            return k.nfft == 1024 ? 16 : (k.nperseg * 4 == k.nfft ? 8 : (k.seg_kind == 0 ? 6 : 8));
        case RK_W16K: case RK_W16K1X: case RK_W16K1X_HALF: return k.nfft == 8192 && !k.half_ws ? 2 : 1;
        default: return 0;
    }
}

int generic_wg_for(int cu_count, int nfft, long long nseg, int nstreams) {
    const size_t lds = generic_lds_bytes(nfft);
    long long occ = (long long)(160 * 1024 / lds);
    const long long tocc = 2048 / generic_threads_for(nfft);
    if (occ > tocc) occ = tocc;
    if (occ < 1) occ = 1;
    if (occ > 4) occ = 4;
    long long w = ((long long)cu_count * occ + nstreams - 1) / nstreams;
    if (w > nseg) w = nseg;
    if (w < 1) w = 1;
    return (int)w;
}
}  // namespace

namespace oth {
const char *const kAnyKindName[] = {"none", "direct", "twolevel", "bluestein", "bluestein2"};

bool w4096_variant_known(const char *tag) {
    for (const auto &v : kVariants)
        if (!strcmp(tag, v.tag)) return true;
    return false;
}

int runtime_bpc(const OccupancyKey &k) {
    switch (k.kern) {
        case RK_W4096: return variant_by_tag(k.variant)->blocks_per_cu();
        case RK_CSD4096: return csd4096_blocks_per_cu();
        case RK_CSD4096WS: return csd4096ws_blocks_per_cu();
        case RK_SEG: return seg_teams_per_cu(k.nfft, k.seg_kind, k.seg_wps4);
        case RK_SEGWS: return segws_teams_per_cu(k.nfft);
        case RK_SEGPAD: return seg_padded_teams_per_cu(k.nfft, k.nperseg, k.seg_kind);
        case RK_W16K: case RK_W16K1X: case RK_W16K1X_HALF: return k.nfft == 8192 && !k.half_ws ? 2 : 1;      // 70 / 139 (145) KiB of LDS
        default: return 0;
    }
}

// -> OTH_OK, or OTH_ERR_UNSUPPORTED with *why set (OTH_KERNEL_TUNED on a plan no tuned kernel covers)
int resolve_recipe(const PlanShape &p, bool csd, long long nseg, int nstreams, int cu_count, int (*bpc_of)(const OccupancyKey &),
                   LaunchRecipe *out, const char **why) {
    LaunchRecipe r;
    r.csd = csd;
    r.nch = csd ? 4 : 1;
    if (p.any.kind != ANY_NONE) {
        // lengths outside the power-of-two kernels: detrend in the time domain from each segment's own mean (no pilot),
        // contiguous strided rows of segments, partial rows in natural order (two-level: [k1][k2], ROW_TWOLEVEL)
        if (p.kernel == OTH_KERNEL_TUNED) {
            if (why) *why = "tuned kernel does not cover this plan";
            return OTH_ERR_UNSUPPORTED;
        }
        r.kern = RK_ANY;
        r.any_kind = p.any.kind;
        r.any_onewg = p.any.kind == ANY_TWOLEVEL && (p.any.L == 32768 || p.any.L == 65536) && p.nperseg == p.any.L && !csd &&
                      p.tune_variant != "anycov" && p.tune_variant != "r16";                             // welch32k.hip
        r.any_r16 = !r.any_onewg && p.any.kind == ANY_TWOLEVEL && tl_supported(p.any.L) && p.tune_variant != "anycov";      // fft_tl.hip
        r.form = p.detrend ? 1 : 0;
        r.W = r.any_onewg ? welch32k_rows(nseg, cu_count, p.any.L == 65536) : any_partial_rows(p.any, nseg, cu_count);
        r.layout = r.any_onewg ? w32k_layout(p.any.L) : (p.any.kind == ANY_TWOLEVEL ? ROW_TWOLEVEL : ROW_NATURAL);
        *out = r;
        return OTH_OK;
    }
    const std::string &tv = p.tune_variant;
    const bool want_tuned = p.kernel != OTH_KERNEL_GENERIC;
    const bool half_step = p.step * 2 == p.nperseg;
    // ---- detrend form.  After the transform (FFT((x - m) w) = FFT(x w) - m FFT(w), the role-split / half-keeping
    // builds) only with a window-spectrum table and at least kFdMinSegments segments per stream: below that the
    // time-domain builds run in both detrend modes (the pilot is one value per launch; an offset that moves within a
    // one- or two-segment launch has nothing to average its rounding down - advisor, round 4 - and such launches do not
    // need the fast builds' throughput).  A variant forced through oth_plan_set_tuning is honoured; "td" forces the
    // time-domain builds at any length.
    const bool fd_forced = !tv.empty() && tv != "td" && tv != "plaunch";
    const bool fd = p.fd_ok && tv != "td" && (fd_forced || nseg >= kFdMinSegments);
    const bool fd1x = fd && p.fd1x_ok;
    // ---- kernel family
    const bool pow2_nperseg = p.nperseg >= 256 && (p.nperseg & (p.nperseg - 1)) == 0;
    const bool seg_size = p.nfft == 256 || p.nfft == 512 || p.nfft == 1024 || p.nfft == 2048;
    const bool big_size = p.nfft == 8192 || p.nfft == 16384;
    if (csd) {
        if (want_tuned && p.nfft == 4096 && p.nperseg == 4096) {
            // role-split pairs: 50 % overlap, frequency-domain detrend, 32-bit segment indices; "csd1" forces the one-role kernel
            const bool ws = p.step == 2048 && (!p.detrend || fd) && nseg < (1LL << 30) && tv != "csd1";
            r.kern = ws ? RK_CSD4096WS : RK_CSD4096;
        }
    } else if (want_tuned && p.nfft == 4096 && pow2_nperseg) {      // nperseg = 256 ... 4096, zero-padded to 4096
        r.kern = RK_W4096;
        const bool fd_ok = (!p.detrend || fd) && nseg < (1LL << 30);      // ws: 32-bit segment indices
        r.variant = w4096_variant(p.nperseg == 4096 ? p.step : 0, fd_ok, tv);
    } else if (want_tuned && big_size && (p.nperseg == p.nfft || p.nperseg * 4 == p.nfft)) {      // (nfft / 4: the sweeper's zero padding)
        r.kern = RK_W16K;
        if (p.nperseg == p.nfft && tv != "16k4") {
            // one cross-wave exchange per segment (16384: 16 waves, one workgroup per CU; 8192, round 5: 8 waves, two
            // radix-8 butterflies in pass 2, two workgroups per CU): vectors that do not overlap without a detrend (the
            // scanner of BASELINE config 5; at 8192 points the pipelined rectangular build only), and 50 % overlap with
            // the kept half in registers (a constant detrend needs the |k| < 16 table)
            if (p.step >= p.nfft && !p.detrend && (p.nfft == 16384 || (p.rect_window && tv != "16kplain"))) r.kern = RK_W16K1X;
            else if (p.step * 2 == p.nfft && (!p.detrend || fd1x)) {
                r.kern = RK_W16K1X_HALF;
                // the role-split build at 8192 points walks contiguous runs only (what this shape takes by default)
                const bool contiguous = (p.tune_sched < 0 && p.sched == OTH_SCHED_DYNAMIC) ||
                                        (p.tune_sched >= 0 ? p.tune_sched : p.sched) == OTH_SCHED_CONTIGUOUS;
                r.half_ws = p.nfft == 8192 && contiguous && nseg < (1LL << 31) && tv != "8k1role";      // ("8k1role": the A/B)
            }
        }
    } else if (want_tuned && seg_size && seg_padded_supported(p.nfft, p.nperseg)) {
        r.kern = RK_SEGPAD;      // nperseg = nfft / 4 (the sweeper's call, spectrum_sweeper.py:263) or nfft / 2 at 1024 / 2048
    } else if (want_tuned && seg_size && p.nperseg == p.nfft) {
        r.kern = RK_SEG;
    }
    if (p.kernel == OTH_KERNEL_TUNED && r.kern == RK_GENERIC) {
        if (why) *why = "tuned kernel does not cover this plan";
        return OTH_ERR_UNSUPPORTED;
    }
    if (r.kern == RK_SEG || r.kern == RK_SEGPAD) {
        r.seg_kind = half_step ? 0 : 1;
        r.seg_wps4 = tv == "seg4";
        // role-split build: 50 % overlap; detrend in the time domain at 1024 (one producer wave), after the transform at
        // 2048 (needs the table); "seg3" / "seg4" force the one-role builds
        r.seg_det = !p.detrend ? 0 : (p.nfft == 1024 ? 1 : 2);
        if (r.kern == RK_SEG && p.nfft >= 1024 && r.seg_kind == 0 && tv != "seg3" && !r.seg_wps4 && (r.seg_det != 2 || fd))
            r.kern = RK_SEGWS;
    }
    // ---- detrend form and pilot of the kernel chosen
    if (p.detrend) {
        const bool after = r.kern == RK_CSD4096WS || r.kern == RK_W16K1X_HALF || (r.kern == RK_W4096 && r.variant->fd) ||
                           (r.kern == RK_SEGWS && r.seg_det == 2) || (r.kern == RK_W16K && fd && half_step && p.nperseg == p.nfft);
        r.form = after ? 2 : 1;
        r.use_fd1x = r.kern == RK_W16K1X_HALF;
        if (!p.fast_detrend) {
            const bool can_inline = ((r.kern == RK_W4096 && r.variant->inline_pilot) || r.kern == RK_CSD4096WS ||
                                     r.kern == RK_W16K1X_HALF) &&
                                    !p.pilot_launch && tv != "plaunch";
            r.pilot = can_inline ? 2 : 1;
        }
    }
    if (r.kern == RK_W16K1X) {
        r.x1_window = !p.rect_window;
        r.x1_plain = tv == "16kplain";
    }
    // ---- grid: exactly the resident workgroups (one wave of workgroups, no tail round); generic: by LDS footprint
    if (r.kern == RK_GENERIC) {
        r.W = generic_wg_for(cu_count, p.nfft, nseg, nstreams);
    } else {
        const OccupancyKey key{r.kern, r.kern == RK_W4096 ? r.variant->tag : "", p.nfft, p.nperseg, r.seg_kind, r.seg_wps4, r.half_ws};
        r.bpc = bpc_of(key);
        if (r.bpc < 1) r.bpc = 1;
        const long long w = ((long long)cu_count * r.bpc + nstreams - 1) / nstreams;
        r.W = (int)(w > nseg ? nseg : (w < 1 ? 1 : w));
    }
    r.layout = (r.kern == RK_W4096 || r.kern == RK_CSD4096 || r.kern == RK_CSD4096WS) ? ROW_W4096
               : (r.kern == RK_W16K1X || r.kern == RK_W16K1X_HALF) ? x1_layout(p.nfft)
               : (r.kern == RK_W16K ? w16k_layout(p.nfft) : ROW_NATURAL);
    // ---- schedule and chunks (tuned kernels only; the coverage kernel walks contiguous runs)
    if (r.kern != RK_GENERIC) {
        const bool auto_sched = p.tune_sched < 0 && p.sched == OTH_SCHED_DYNAMIC;      // "the library's choice"
        const long long per_team = nseg / (r.W > 0 ? r.W : 1);
        const bool is_seg = r.kern == RK_SEG || r.kern == RK_SEGPAD || r.kern == RK_SEGWS;
        const bool big = r.kern == RK_W16K || r.kern == RK_W16K1X || r.kern == RK_W16K1X_HALF;
        r.sched = p.tune_sched >= 0 ? p.tune_sched : p.sched;
        int static_chunk = 0;
        if (auto_sched) {
            // one 1024-thread workgroup per CU and equal work per segment: contiguous runs beat the ticket queue (+3 %)
            if (r.kern == RK_CSD4096WS) r.sched = OTH_SCHED_CONTIGUOUS;
            // the role-split 1024 kernel: eight two-wave workgroups per CU even out by themselves (+4 % over the tickets)
            if (r.kern == RK_SEGWS && p.nfft == 1024 && nstreams == 1) r.sched = OTH_SCHED_CONTIGUOUS;
            if (r.kern == RK_SEG || r.kern == RK_SEGPAD) {
                // 256 / 512 points (and the zero-padded builds: nfft / 8 new samples per segment) at 50 % overlap: a ticket
                // per sixteen 2-4 KiB segments costs more than it evens out (17-35 % of the roofline at every launch size).
                // Static instead: interleaved chunks of 32 / 16 segments while every team gets two of them (256 points,
                // 2^27 samples: 66 % against 43 %), one contiguous run per team below that.
                if (r.seg_kind == 0 && (p.nfft <= 512 || r.kern == RK_SEGPAD)) {
                    static_chunk = per_team >= 64 ? 32 : (per_team >= 32 ? 16 : 0);
                    r.sched = static_chunk ? OTH_SCHED_INTERLEAVED : OTH_SCHED_CONTIGUOUS;
                }
                // whole-segment loads (steps other than nfft / 2): the next chunk's first segment is prefetched across the
                // chunk boundary only under the interleaved schedule - 8-segment chunks: 1024 points, no overlap, 70 % of
                // the roofline against 49 % with tickets
                if (r.seg_kind == 1) {
                    static_chunk = per_team >= 16 ? 8 : 0;
                    r.sched = static_chunk ? OTH_SCHED_INTERLEAVED : OTH_SCHED_CONTIGUOUS;
                }
            }
            // short launches (fewer than 32 segments per resident workgroup): one contiguous run each - the tickets' guided
            // tail has nothing to even out and costs 5-20 % (2048 points, 2^22 samples: 17.3 % against 14.0 %)
            if ((r.kern == RK_W4096 || r.kern == RK_SEGWS) && per_team < 32) r.sched = OTH_SCHED_CONTIGUOUS;
            // the one-exchange 16384-point scanner kernel: one workgroup per CU, equal work per segment, no chunk head to
            // re-read - contiguous runs (0.417-0.418 against 0.421-0.424 ms with tickets, same box) unless a workgroup gets
            // so few segments that an uneven split shows
            if (r.kern == RK_W16K1X && per_team >= 8) r.sched = OTH_SCHED_CONTIGUOUS;
            // 16384 points at 50 % overlap: contiguous runs (no chunk head is read twice): 30.8 % against 29.3 % with tickets
            if (big && p.nfft == 16384 && half_step && p.nperseg == p.nfft) r.sched = OTH_SCHED_CONTIGUOUS;
            // the one-exchange 50 %-overlap build prefetches across its run, and a chunk head costs it a synchronous load
            if (r.kern == RK_W16K1X_HALF) r.sched = OTH_SCHED_CONTIGUOUS;
            // 8192 (round 4): contiguous runs take the same time as tickets over chunks of 16 and read no chunk head twice
            if (big && p.nfft == 8192 && half_step && p.nperseg == p.nfft && per_team >= 16) r.sched = OTH_SCHED_CONTIGUOUS;
        }
        if (r.sched < 0 || r.sched > 2) r.sched = 0;
        // segments per chunk
        int chunk;
        if (p.tune_chunk > 0) chunk = p.tune_chunk;
        else if (big) {
            const bool halves = half_step && (p.nperseg == p.nfft || p.nperseg * 4 == p.nfft);      // a kept half: longer chunks
            chunk = halves ? 16 : 2;
        } else if (r.kern == RK_W4096) chunk = r.variant->chunk;
        else if (is_seg) chunk = static_chunk ? static_chunk
                                              : (((p.nfft == 1024 && r.kern != RK_SEGWS) || (p.nfft == 2048 && r.kern == RK_SEGWS)) ? 32 : 16);
        else chunk = 8;      // the one-role two-channel kernel
        if (chunk < 1) chunk = 1;
        // welch16k1x: the ticket for the NEXT chunk is published with a chunk's first segment and read at its last
        if (r.kern == RK_W16K1X && chunk < 2) chunk = 2;
        r.chunk = chunk;
        r.tail_chunk = chunk;
        r.nbig = nseg / chunk;
        if (r.sched == OTH_SCHED_DYNAMIC) {
            if (nstreams > 64) {
                r.sched = OTH_SCHED_INTERLEAVED;      // the context holds 64 ticket words
            } else {
                r.tickets = true;
                // guided tail: the last half round of work goes out in quarter-size chunks
                r.tail_chunk = p.tune_tail > 0 ? p.tune_tail : (chunk >= 4 ? chunk / 4 : 1);
                if (r.tail_chunk < 1) r.tail_chunk = 1;
                if (r.kern == RK_W16K1X && r.tail_chunk < 2) r.tail_chunk = 2;
                const long long tail_segs = (long long)r.W * chunk / 2;
                r.nbig = nseg > tail_segs ? (nseg - tail_segs) / chunk : 0;
            }
        }
    }
    *out = r;
    return OTH_OK;
}

// the recipe as text (oth__debug_recipe, bench.py's kernel labels)
std::string recipe_text(const LaunchRecipe &r, int nfft) {
    static const char *const kForm[] = {"none", "time", "freq"}, *const kPilot[] = {"none", "launch", "inline"},
                             *const kSched[] = {"contiguous", "interleaved", "dynamic"};
    char buf[384];
    std::string k = kRecipeKernelName[r.kern];
    if (r.kern == RK_W4096) k += std::string(":") + r.variant->tag;
    if (r.kern == RK_SEG) k += std::string(r.seg_kind ? ":full" : ":half") + (r.seg_wps4 ? ":wps4" : "");
    if (r.kern == RK_SEGPAD) k += r.seg_kind ? ":full" : ":half";
    if (r.kern == RK_W16K1X) k += std::string(r.x1_plain || r.x1_window ? ":plain" : ":pipe") + (r.x1_window ? ":window" : "");
    if (r.kern == RK_W16K1X_HALF && r.half_ws) k += ":ws";
    if (r.kern == RK_ANY) k += r.any_onewg ? std::string(":onewg") : std::string(":") + kAnyKindName[r.any_kind] + (r.any_r16 ? ":r16" : "");
    // rows=1: every kernel leaves one partial row per workgroup; the field stays because the text is compared byte for byte
    snprintf(buf, sizeof buf, "kernel=%s nfft=%d form=%s pilot=%s sched=%s chunk=%d tail=%d nbig=%lld bpc=%d W=%d rows=1 nch=%d layout=%d",
             k.c_str(), nfft, kForm[r.form], kPilot[r.pilot], kSched[r.sched], r.chunk, r.tail_chunk, r.nbig, r.bpc, r.W,
             r.nch, (int)r.layout);
    return buf;
}

PlanShape shape_of(const oth_plan *p) {
    PlanShape s;
    s.nfft = p->nfft;
    s.nperseg = p->nperseg;
    s.step = p->step;
    s.detrend = p->detrend != OTH_DETREND_NONE;
    s.fast_detrend = p->fast_detrend;
    s.fd_ok = p->d_fd.get() != nullptr;
    s.fd1x_ok = p->d_fd1x.get() != nullptr;
    s.rect_window = p->rect_window;
    s.kernel = p->kernel;
    s.sched = p->sched;
    s.pilot_launch = p->pilot_launch;
    s.tune_variant = p->tune_variant;
    s.tune_sched = p->tune_sched;
    s.tune_chunk = p->tune_chunk;
    s.tune_tail = p->tune_tail;
    s.any = p->any.sh;
    return s;
}
}  // namespace oth

extern "C" {
// The launch recipe of a plan shape as text, WITHOUT a device (pure host logic; runtime_occupancy = 0 takes the resident
// workgroups per CU from the built-in MI355X table, 1 asks the occupancy calculator and needs a GPU).
//   window_class: 0 all ones, 1 spectrum confined (periodic cosine-sum windows: both detrend tables exist), 2 wide
//   (e.g. a symmetric Hamming: no table), 3 confined to 256 F bins but not to |k| < 16 (16384 points only)
//   detrend_mode: OTH_DETREND_*;  kernel_pref: OTH_KERNEL_*;  sched_pref: OTH_SCHED_*;  variant: as oth_plan_set_tuning
//   oth__debug_recipe_tuned: the same with the overrides of oth_plan_set_tuning (sched -1, chunk 0, tail_chunk 0: none)
int oth__debug_recipe_tuned(int nfft, int nperseg, int noverlap, int window_class, int detrend_mode, int two_channel, int kernel_pref,
                            const char *variant, int sched_pref, long long nseg, int nstreams, int cu_count, int runtime_occupancy,
                            int tune_sched, int tune_chunk, int tune_tail, char *buf, size_t buflen) {
    OTH_TRY
    if (!buf || !buflen || nperseg < 1 || nperseg > nfft || noverlap < 0 || noverlap >= nperseg || nseg < 1 || nstreams < 1)
        return fail(nullptr, OTH_ERR_INVALID, "bad argument");
    PlanShape sh;
    sh.nfft = nfft;
    sh.nperseg = nperseg;
    sh.step = nperseg - noverlap;
    sh.detrend = detrend_mode != OTH_DETREND_NONE;
    sh.fast_detrend = detrend_mode == OTH_DETREND_CONSTANT_FAST;
    // the tables oth_welch_plan builds: 4096 / 2048 / 8192 / 16384 points, nperseg = nfft, a confined window spectrum
    const bool table_size = (nfft == 4096 || nfft == 2048 || nfft == 8192 || nfft == 16384) && nperseg == nfft;
    sh.fd_ok = sh.detrend && table_size && (window_class == 0 || window_class == 1 || window_class == 3);
    sh.fd1x_ok = sh.detrend && (nfft == 16384 || nfft == 8192) && nperseg == nfft && (window_class == 0 || window_class == 1);
    sh.rect_window = window_class == 0;
    sh.kernel = kernel_pref;
    sh.sched = sched_pref;
    sh.tune_variant = variant ? variant : "";
    sh.tune_sched = tune_sched;
    sh.tune_chunk = tune_chunk;
    sh.tune_tail = tune_tail;
    if (!generic_supported(nfft) && any_describe(nfft, &sh.any))
        return fail(nullptr, OTH_ERR_UNSUPPORTED, "transform length outside [1, 1048576] (Bluestein: n <= 524288)");
    LaunchRecipe r;
    const char *why = "";
    if (int rc = resolve_recipe(sh, two_channel != 0, nseg, nstreams, cu_count > 0 ? cu_count : 256,
                                runtime_occupancy ? runtime_bpc : table_bpc, &r, &why))
        return fail(nullptr, rc, why);
    snprintf(buf, buflen, "%s", recipe_text(r, nfft).c_str());
    return OTH_OK;
    OTH_CATCH(nullptr)
}

int oth__debug_recipe(int nfft, int nperseg, int noverlap, int window_class, int detrend_mode, int two_channel, int kernel_pref,
                      const char *variant, int sched_pref, long long nseg, int nstreams, int cu_count, int runtime_occupancy,
                      char *buf, size_t buflen) {
    OTH_TRY
    return oth__debug_recipe_tuned(nfft, nperseg, noverlap, window_class, detrend_mode, two_channel, kernel_pref, variant, sched_pref,
                                   nseg, nstreams, cu_count, runtime_occupancy, -1, 0, 0, buf, buflen);
    OTH_CATCH(nullptr)
}
}  // extern "C"
