// welch4096ws: wave-specialised form of the headline kernel (nperseg = nfft = 4096, 50 % overlap).
//
// Same arithmetic as welch4096.hip (radix-16 x 16 x 16, same LDS image), but a 512-thread workgroup is
// split into a PRODUCER half (threads 0..255: loads, window, pass 1, exchange-1 writes) and a CONSUMER
// half (threads 256..511: pass 2, exchange 2, pass 3, |X|^2 accumulation) that work one segment apart on
// two LDS images.  Why: in the one-role kernel every thread carries the constants of all three passes
// (window, both twiddle sets, accumulators, the kept half and the prefetch) and has to rebuild both
// twiddle sets every segment to stay at 128 VGPRs.  Split by role, the producer holds window + data
// pipeline and rebuilds only its twiddles, the consumer holds its 15 twiddles and the accumulators in
// registers: 9 % fewer VALU instructions per segment, one workgroup barrier per segment instead of two,
// and the loads of the producer overlap the butterflies of the consumer by construction.
//
// The constant detrend runs in the frequency domain: FFT((x - m) w) = FFT(x w) - m FFT(w).  For every
// window whose spectrum is confined to bins [0,256) U [3840,4096) (host check at plan time; exact for the
// periodic cosine-sum windows scipy.signal.welch builds) those are the k2 = 0 and k2 = 15 outputs of
// pass 3, so each consumer thread fixes two of its sixteen bins with its own pair of FFT(w) values
// (WelchArgs.fd).  The producer therefore never needs the mean: it publishes per-wave sums of the raw
// samples next to the image, and windows samples as soon as they arrive.
//
// Per step `it` (one LDS-only barrier):  producer: segment it -> image[it & 1];  consumer: right behind the
// barrier pass 2 of image[it & 1] (its LDS reads in one batch with the item word), then, once the item word
// says it is a segment, exchange 2, pass 3 and the accumulation.  The consumer is the critical path (443
// VALU instructions per step against the producer's 336): its butterflies run at a higher wave priority.
// The samples are read once (a chunk's first half twice, by two workgroups far apart in time): non-temporal
// loads (load_once) keep them from displacing the twiddle / window tables and the partial sums in L2 (-1.4 % kernel
// time); the first half of a chunk's head, which a second workgroup reads again, stays a plain load.
// The producer keeps six pass-1 twiddle powers (W^1,2,3,4,8,12: nine products per segment instead of thirteen) and
// pays for their eight registers by reading the second half of its window values from an 8 KiB LDS table per step
// (same-box A/B, five interleaved runs each: 0.5855 against 0.5906 ms = -0.9 %, profiles/r03_ab_headline_pow6.txt)
// Complementary windows (welch4096ws_compl_kernel; WelchArgs.compl_win, checked at plan time: w[n] + w[n + 2048] = 1 to one
// float32 ulp - SciPy's periodic Hann, the reference's call): r w[n + 2048] = fma(-r, w[n], r), so window rows 8..15 are not
// needed, rows 0..7 take their place in the LDS table and no window value stays in a register.  The kept half stays
// UNWINDOWED: its product with w[n] contracts into the two additions of the first butterfly layer (windowed ahead, the
// pair cost sixteen instructions more than the general form), so the window costs what it did and the eight freed
// registers plus what the form leaves over held thirteen pass-1 twiddle powers (two products per segment; fourteen and
// fifteen spilled in the PILOT flavour; now eight (tan, sin) pairs, below).  Producer hot loop 311 -> 281 VALU per segment
// (same-box A/B against the parent library with the change below, alternating runs of bench.py: kernel 0.5993-0.6013
// against 0.6132-0.6147 ms = -2.3 %, step 0.613-0.616 against 0.627-0.630 ms, profiles/ab_headline_compl.txt)
// The consumer waits ONCE for its table loads, in front of its loop: fifteen s_waitcnt vmcnt(n) per segment, one in front
// of each pass-2 twiddle product, are gone from the critical path (measured together with the above, not on its own)
// The consumer's EXECUTED path per segment went from 426 to 406 VALU instructions (the budget test read 407 on the former: it
// leaves out a loop-header block that every segment ran through): one instance of pass 2 on the data path instead of two
// whose outputs were copied into each other's registers (16 v_mov), the item word compared in scalar registers (2 v_cmp ->
// 1 v_readfirstlane), no dummy operand on the first counted wait of a read batch (2 v_mov); and the item word and the
// per-wave sums are read by dft16_from_lds itself, where the compiler's own reads in front of it drew an s_waitcnt
// lgkmcnt(1) into the first butterfly layer behind every barrier.  Producer 281 -> 277 (two opaque copies of stored
// twiddle powers instead of six).  Same-box A/B against the parent library, six alternating runs of bench.py each: step
// 0.5766-0.5804 against 0.5835-0.5862 ms, kernel 0.5636-0.5658 against 0.5710-0.5722 ms = -1.2 %; SQ_INSTS_VALU 3.737e8 ->
// 3.616e8, SQ_WAIT_INST_LDS -6.8 % per launch; outputs bit for bit the parent's (profiles/ab_headline_consumer_path.txt)
// Signed digits and three-shear twiddles (the complementary-window build; DESIGN 4.1, model: tests/test_symtw_model_cpu.py).
// With n = 256 a + 16 b + c measured from sample 136 - n' = 256 a + tau, tau = 16 (b - 8) + (c - 8) = t - 136 - and the output
// digits of passes 1 and 2 read as kappa = sym16(k0), lambda = sym16(k1) in [-8, 8), k = kappa + 16 lambda + 256 mu, the
// pass-1 twiddle is W4096^(kappa tau) and the pass-2 twiddle W256^(lambda (c - 8)): |theta| <= 0.54 pi.  The butterflies keep
// the plain digits b, c; that leaves (-1)^lambda on all sixteen inputs of a pass-3 transform, (-1)^mu on its output and the
// origin's unit phase on X[k], none of which survives |X|^2.  No thread holds other samples, no load or LDS address moves;
// register mu of consumer thread (k0, k1) holds another bin, and the final store puts it where finalize layout 1 wants it.
// Inside that range a rotation is three shears - three v_fma_f32 against cmul's four instructions, no scale left behind
// (rot3, twiddle16.hip.h) - from eight stored (tan(theta / 2), sin(theta)) pairs per role (WelchArgs.symtw), the conjugate by
// operand negation: sixteen twiddle registers in the producer (26 before: thirteen powers, two products per segment) and in
// the consumer (30).  The registers mu = 0 are the bins [-136, 120): the plan checks that the window's spectrum stays inside
// them, and each consumer thread detrends that one register (WelchArgs.fd_sym carries the phase and the sign).
// Producer 277 -> 252, consumer 406 -> 385 VALU per segment, 124 / 105 / 108 VGPRs, no scratch; the general build's code is
// unchanged instruction for instruction.  Same-box A/B against the parent library, six alternating runs of bench.py each:
// step 0.5778-0.5808 against 0.5915-0.5954 ms, kernel 0.5647-0.5676 against 0.5776-0.5807 ms = -2.2 %; SQ_INSTS_VALU
// 3.616e8 -> 3.375e8 per launch, SQ_WAIT_INST_LDS +58 % (a rotation is a chain of three dependent operations in front of its
// exchange write); one-segment rows 0.86 against 0.80 ulp of the row's peak amplitude (profiles/ab_headline_symtw.txt)
// Exchange-2 stores inside pass 2's last butterfly layer (the complementary-window build's consumer): the +58 % above was
// where the rotations left the stores - all sixteen behind the last FMA, in front of pass 3's first counted wait, the four
// consumer waves at once.  dft16_layer2_scatter_sym (fft4096.hip.h) issues butterfly g, then the rotations and single
// ds_write_b64 of group g - 1; pass2() writes exchange 2 itself, before the item word is looked at.  385 VALU per segment
// still, 119 / 107 / 105 VGPRs; same-box A/B against the parent library, six alternating runs of bench.py each: step
// 0.5637-0.5651 against 0.5749-0.5763 ms, kernel 0.5492-0.5500 against 0.5604-0.5616 ms = -2.1 % (a second, busy box: -0.7 % in
// the mean, no separation); SQ_WAIT_INST_LDS 1.566e8 -> 0.913e8, SQ_INSTS_VALU unchanged, outputs bit for bit the parent's
// (profiles/ab_headline_exchange_overlap.txt, profiles/exchange_overlap_device_diff.txt)
// tried: the eight loads of a step spread over 2 / 3 places instead of one burst, no gain (NOTES 8,
// profiles/r05_ab_headline_spread_loads.txt)
// tried: the same pipeline for the producer's exchange-1 stores (the first layer, then dft16_layer2_scatter_sym<RS>), its
// section at wave priority 2, at 0, and at 0 up to the last store group: +0.9 %, +0.4 %, +0.9 % against the parent, and with
// the consumer's together -0.8 % instead of -2.1 % (profiles/ab_headline_exchange_overlap.txt, NOTES 4.1)
// not tried: the two components of the segment sum reduced in one interleaved DPP sequence (ten s_nop per segment in the
// producer, which is not the critical path)

#include <type_traits>
#include "fft4096.hip.h"
#include "launch.h"

namespace oth {
namespace {

constexpr int TWS = 512;
constexpr int WS_RED = 32;                 // float2: per image the four producer waves' segment sums (8 slots each)
constexpr int WS_CTRL = 16;                // ints: item kind per image [0..1], next-chunk ticket [4]
constexpr size_t WS_WIN_BYTES = 256 * 2 * sizeof(float4);      // window values 8..15 of every producer thread
constexpr size_t WS_LDS_BYTES = (2 * LDS_X + WS_RED) * sizeof(float2) + WS_CTRL * sizeof(int) + WS_WIN_BYTES;

// wave priorities: producer latency sections / butterflies / twiddles + exchange-1 writes, consumer latency sections /
// butterflies
constexpr int WS_PAL = 2, WS_PAC = 0, WS_PAS = WS_PAL, WS_PBL = 2;
constexpr int WS_PBC = 1;                  // the consumer is the critical path: its butterflies go ahead of the producer's (-4.5 %)

enum { ITEM_STOP = 0, ITEM_DATA = 1, ITEM_BUBBLE = 2 };

// COMPL: the complementary-window producer (w[n] + w[n + 2048] = 1, see the file header); everything else is shared
template <bool DETREND, bool PILOT, bool COMPL>
__device__ __forceinline__ void welch4096ws_body(const WelchArgs &p) {
    static_assert(DETREND || !PILOT, "the pilot belongs to the detrend");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *img = reinterpret_cast<float2 *>(smem);             // two images of LDS_X float2
    float2 *red = img + 2 * LDS_X;                              // [2][8]
    int *ctrl = reinterpret_cast<int *>(red + WS_RED);          // item kind [0..1], next ticket [4]; re-read after every
                                                                // lds_barrier() (it is a compiler memory barrier)

    const int tid = threadIdx.x;
    const bool producer = tid < 256;
    const int t = tid & 255;
    const int hi = t >> 4, lo = t & 15;
    const int wave = t >> 6;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    const int sched = p.sched;
    const long long nchunks = sched ? chunk_count(p) : 1;

    // LDS addresses inside an image (float2): exchange-1 write/read, exchange-2 write/read
    const int w1 = hi * 17 + lo, r1 = hi * RS + lo, w2 = hi * RS + lo, r2 = hi * RS + lo * 17;

    if (producer) {
        // ------------------------------------------------------------------ producer
        float win[COMPL ? 1 : 8];      // (COMPL: no window value stays in a register)
        float4 *wl = reinterpret_cast<float4 *>(ctrl + WS_CTRL) + t;      // [2][256] float4: win[8..11], win[12..15] (COMPL: 0..3, 4..7)
        constexpr int WROW = COMPL ? 0 : 8;
        if constexpr (!COMPL) {
#pragma unroll
            for (int a = 0; a < 8; ++a) win[a] = p.win[256 * a + t];
        }
        wl[0] = make_float4(p.win[256 * WROW + t], p.win[256 * (WROW + 1) + t], p.win[256 * (WROW + 2) + t], p.win[256 * (WROW + 3) + t]);
        wl[256] = make_float4(p.win[256 * (WROW + 4) + t], p.win[256 * (WROW + 5) + t], p.win[256 * (WROW + 6) + t],
                              p.win[256 * (WROW + 7) + t]);
        Pow6 b6;                       // general build: W^1, 2, 3, 4, 8, 12 of this thread
        float2 ts1[COMPL ? 8 : 1];     // COMPL: (tan, sin) pairs of |kappa| (t - 136), |kappa| = 1..8 (file header)
        if constexpr (COMPL) {
#pragma unroll
            for (int m = 1; m <= 8; ++m) ts1[m - 1] = p.symtw[kSymTwOrigin + m * (t - kSymShift)];
        } else {
            b6 = Pow6{p.tw[t], p.tw[2 * t], p.tw[3 * t], p.tw[4 * t], p.tw[8 * t], p.tw[(12 * t) & 4095]};
        }
        float2 kw[8], nxt[8];
        float2 prev_new = make_float2(0.f, 0.f);     // this wave's sum of the previous segment's new half
        // PILOT (every detrending plan but OTH_DETREND_CONSTANT_FAST): WelchArgs.pilot comes off every sample as it arrives, so the transform and
        // the sums see x - pilot (two scalar registers, two subtractions per sample: +1 % on the launch)
        // pilot_inline (round 5): formed in the launch from eight 2 KiB probes (below, behind the first sample loads)
        // instead of by a launch in front of this one
        float2 pv = make_float2(0.f, 0.f);
        if (PILOT && !p.pilot_inline) pv = load_pilot(p.pilot, stream);
        int it = 0;
        unsigned ticket = 0;
        using std::false_type;
        using std::true_type;
        using mid = std::integral_constant<int, 0>;     // prefetch the half after next of this chunk
        using head = std::integral_constant<int, 1>;    // last segment of the chunk: prefetch the next chunk's first segment
        using none = std::integral_constant<int, 2>;    // nothing to prefetch

        // segment indices are wave-uniform ints pinned to scalar registers (the launcher checks nseg < 2^30), so
        // the loads use scalar base + per-thread offset and cost no vector address arithmetic
        auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
        auto load_chunk_head = [&](int first_seg) {
            const float2 *xs = xb + (size_t)uni(first_seg) * 2048;      // scalar base, unsigned 32-bit lane offset
#pragma unroll
            for (int j = 0; j < 4; ++j) {      // one scalar base per pair of rows: offsets t and t + 256 (immediate)
                const float2 *xj = xs + 512 * j;
                kw[2 * j] = *(xj + (unsigned)t);      // raw: the chunk's first item windows them in place
                kw[2 * j + 1] = *(xj + ((unsigned)t + 256u));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 *xj = xs + 2048 + 512 * j;
                nxt[2 * j] = load_once(xj + (unsigned)t);
                nxt[2 * j + 1] = load_once(xj + ((unsigned)t + 256u));
            }
        };
        auto step_end = [&](int item) {
            if (t == 0) ctrl[it & 1] = item;
            lds_barrier();
            ++it;
        };
        // One segment: image (it & 1).  Every flavour leaves the same state behind - kw = windowed first half of the
        // following segment, nxt = its second half in flight - so the hot (false, mid) flavour is straight-line code
        // with one group of eight loads per step.
        auto item = [&](auto first_, auto mode_, int s, int nsb, bool publish) {
            constexpr bool FIRST = decltype(first_)::value;
            constexpr int MODE = decltype(mode_)::value;
            const int q = it & 1;
            float2 *lx = img + q * LDS_X;
            // COMPL: the flavours keep their own code - hoisted above the branch between two of them, their common head
            // loses the contraction of the window products into the butterflies and spills 4-26 registers
            if constexpr (COMPL) asm volatile("; item %0 %1" ::"n"((int)FIRST), "n"(MODE));
            __builtin_amdgcn_s_setprio(WS_PAL);
            float2 v[16];
            float2 sumf = make_float2(0.f, 0.f), sum = make_float2(0.f, 0.f);
            const float4 wa = wl[0], wb = wl[256];      // own slots: no barrier needed
            const float wh[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};      // window values 8..15 (COMPL: 0..7), this step only
            if (FIRST) {
#pragma unroll
                for (int a = 0; a < 8; ++a) {      // kw still holds the raw first half of the chunk's first segment
                    if (PILOT) kw[a] = csub(kw[a], pv);
                    sumf = cadd(sumf, kw[a]);
                    if constexpr (!COMPL) kw[a] = make_float2(kw[a].x * win[a], kw[a].y * win[a]);
                }
            }
#pragma unroll
            for (int a = 0; a < 8; ++a) {      // the new half is windowed for both of its roles as it arrives
                const float2 r = PILOT ? csub(nxt[a], pv) : nxt[a];
                if constexpr (COMPL) {
                    // kw is the kept half UNWINDOWED: its product with w[n] is contracted into the first butterfly layer's
                    // two additions (as the general build's r w[n + 2048] is), so keeping it costs nothing;
                    // r w[n + 2048] = r (1 - w[n]) = fma(-r, w[n], r): one rounding, no second window value
                    v[a] = make_float2(kw[a].x * wh[a], kw[a].y * wh[a]);
                    v[8 + a] = make_float2(fmaf(-r.x, wh[a], r.x), fmaf(-r.y, wh[a], r.y));
                    if (MODE == 0) kw[a] = r;
                } else {
                    v[a] = kw[a];
                    v[8 + a] = make_float2(r.x * wh[a], r.y * wh[a]);
                    if (MODE == 0) kw[a] = make_float2(r.x * win[a], r.y * win[a]);      // (else kw is reloaded below)
                }
                sum = (COMPL && a == 0) ? r : cadd(sum, r);      // (COMPL: no 0 + r in front of the chain)
            }
            // dynamic schedule: the ticket of the chunk after this one is drawn with the chunk's first segment and
            // published (a wait for the atomic's return) before this step's loads go out, one step later if possible
            if (sched == 2 && t == 0) {
                if (FIRST) ticket = atomicAdd(p.queue + stream, 1u);
                if (publish) ctrl[4] = (int)ticket;
            }
            const float2 *xn = xb + (size_t)uni(s + 2) * 2048;      // (MODE 0 only)
            // one burst of eight loads (kept as a lambda: written in line the same loads are scheduled differently)
            auto load_next = [&]() {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float2 *xj = xn + 512 * j;
                    nxt[2 * j] = load_once(xj + (unsigned)t);
                    nxt[2 * j + 1] = load_once(xj + ((unsigned)t + 256u));
                }
            };
            if (MODE == 0) {
                load_next();
            } else if (MODE == 1) {
                load_chunk_head(nsb);
            }
            if (DETREND) {      // per-wave sums of both halves of this segment, side by side for the consumer
                sum.x = wave_total_lane63(sum.x);      // (these live in lane 63 of each wave only)
                sum.y = wave_total_lane63(sum.y);
                float2 other = prev_new;
                if (FIRST) other = make_float2(wave_total_lane63(sumf.x), wave_total_lane63(sumf.y));
                if ((t & 63) == 63) red[q * 8 + wave] = cadd(sum, other);
                prev_new = sum;
            }
            __builtin_amdgcn_s_setprio(WS_PAC);
            dft16(v);
            __builtin_amdgcn_s_setprio(WS_PAS);
            if constexpr (COMPL) scatter_sym16<RS>(v, lx + w1, ts1);
            else scatter_pow16_six<RS>(v, lx + w1, b6);
            step_end(ITEM_DATA);
        };

        int cur = 0, sb = 0, se = 0;
        auto range = [&](int c, int &b, int &e) {
            long long lb, le;
            chunk_range(p, c, lb, le);
            b = uni((int)lb);
            e = uni((int)le);
        };
        auto open_chunk = [&](int c) -> bool {
            cur = c;
            if (sched) {
                if (cur >= nchunks) return false;
                range(cur, sb, se);
                return true;
            }
            sb = uni((int)((p.nseg * wg) / W));
            se = uni((int)((p.nseg * (wg + 1)) / W));
            return sb < se;
        };
        bool have = open_chunk(sched ? wg : 0);
        if (have) load_chunk_head(sb);
        if (PILOT && p.pilot_inline) {
            // the probe loads go out behind the chunk head's (one memory round trip for both); per-wave totals into
            // image 1, which no step writes before the barrier of step 0; one extra workgroup barrier (the consumers
            // take it in front of their loop)
            // Contiguous runs (short launches - fewer than 32 segments per workgroup - and OTH_SCHED_CONTIGUOUS): the eight
            // probes are spread over THIS workgroup's run, so the pilot follows an offset that moves through the launch
            // (round 6: a drift of 1200 sigma over 2047 segments read 1.05e-4 with one pilot per launch; every segment is
            // one workgroup's, so the pilots need not agree between workgroups).  Chunked schedules keep the launch-wide
            // probes: a workgroup's chunks lie anywhere in the stream.
            const bool own = sched == 0 && have;
            const PilotProbes probes = inline_pilot_load(own ? xb + (size_t)sb * 2048 : xb, own ? (long long)(se - sb) : p.nseg, 2048, t);
            inline_pilot_store(probes, t, img + LDS_X);
            lds_barrier();
            pv = inline_pilot_value(img + LDS_X);
        }
        while (have) {
            const int n = se - sb;
            int ncur = 0;
            if (n >= 2) {
                item(true_type{}, mid{}, sb, 0, n == 2);
                int s = sb + 1;
                if (s < se - 1) item(false_type{}, mid{}, s++, 0, true);
                for (; s + 1 < se - 1; s += 2) {      // two per trip: kw's registers swap roles instead of being copied
                    item(false_type{}, mid{}, s, 0, false);
                    item(false_type{}, mid{}, s + 1, 0, false);
                }
                if (s < se - 1) item(false_type{}, mid{}, s, 0, false);
                // last segment: the next chunk's ticket was published at least one barrier ago
                ncur = (sched == 1) ? cur + W : W + uni(ctrl[4]);
                int nsb = 0, nse = 0;
                const bool have_next = sched && ncur < nchunks;
                if (have_next) {
                    range(ncur, nsb, nse);
                    item(false_type{}, head{}, se - 1, nsb, false);
                    cur = ncur;
                    sb = nsb;
                    se = nse;
                    continue;
                }
                item(false_type{}, none{}, se - 1, 0, false);
                break;
            }
            // one-segment chunk: no prefetch across the chunk boundary; the ticket needs a barrier to become visible
            item(true_type{}, none{}, sb, 0, true);
            if (sched == 0) break;
            if (sched == 2) {
                step_end(ITEM_BUBBLE);      // the only idle step there is, always behind a segment: the consumer's loop relies on it
                ncur = W + uni(ctrl[4]);
            } else {
                ncur = cur + W;
            }
            have = open_chunk(ncur);
            if (have) load_chunk_head(sb);
        }
        step_end(ITEM_STOP);
    } else {
        // ------------------------------------------------------------------ consumer
        float2 tw2[COMPL ? 1 : 16];      // general build: W256^(k1 c), c = lo
        float2 ts2[COMPL ? 8 : 1];       // COMPL: (tan, sin) pairs of W256^(|lambda| (c - 8)), |lambda| = 1..8
        float4 fw = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (COMPL) {
#pragma unroll
            for (int m = 1; m <= 8; ++m) ts2[m - 1] = p.symtw[kSymTwOrigin + 16 * m * (lo - 8)];
            if (DETREND) {      // the re-phased FFT(w) at this thread's mu = 0 bin, the only one the window reaches
                const float2 f = p.fd_sym[t];
                fw.x = f.x, fw.y = f.y;
            }
        } else {
#pragma unroll
            for (int k = 1; k < 16; ++k) tw2[k] = p.tw[16 * lo * k];
            if (DETREND) fw = p.fd[t];      // FFT(w) at this thread's k2 = 0 and k2 = 15 bins
        }
        float acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.f;
        float2 v[16];
        float2 mean = make_float2(0.f, 0.f);
        // The table loads above are this role's only vector-memory operations.  One wait here, with the values made opaque:
        // the compiler otherwise carries their wait-count state into the loop and re-emits an s_waitcnt vmcnt(n) in front
        // of every pass-2 twiddle product of every step (fifteen issue turns of the critical path per segment).
        if constexpr (COMPL) {
            asm volatile("s_waitcnt vmcnt(0)"
                         : "+v"(ts2[0].x), "+v"(ts2[0].y), "+v"(ts2[1].x), "+v"(ts2[1].y), "+v"(ts2[2].x), "+v"(ts2[2].y), "+v"(ts2[3].x),
                           "+v"(ts2[3].y), "+v"(ts2[4].x), "+v"(ts2[4].y), "+v"(ts2[5].x), "+v"(ts2[5].y), "+v"(ts2[6].x), "+v"(ts2[6].y));
            asm volatile("" : "+v"(ts2[7].x), "+v"(ts2[7].y), "+v"(fw.x), "+v"(fw.y));
        } else {
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(tw2[1].x), "+v"(tw2[1].y), "+v"(tw2[2].x), "+v"(tw2[2].y), "+v"(tw2[3].x), "+v"(tw2[3].y), "+v"(tw2[4].x),
                       "+v"(tw2[4].y), "+v"(tw2[5].x), "+v"(tw2[5].y), "+v"(tw2[6].x), "+v"(tw2[6].y), "+v"(tw2[7].x), "+v"(tw2[7].y));
        asm volatile("" : "+v"(tw2[8].x), "+v"(tw2[8].y), "+v"(tw2[9].x), "+v"(tw2[9].y), "+v"(tw2[10].x), "+v"(tw2[10].y),
                          "+v"(tw2[11].x), "+v"(tw2[11].y), "+v"(tw2[12].x), "+v"(tw2[12].y), "+v"(tw2[13].x), "+v"(tw2[13].y));
        asm volatile("" : "+v"(tw2[14].x), "+v"(tw2[14].y), "+v"(tw2[15].x), "+v"(tw2[15].y), "+v"(fw.x), "+v"(fw.y), "+v"(fw.z),
                          "+v"(fw.w));
        }
        int it = 0;
        // What the producer left in image q: the item kind and, in the same batch of LDS reads (harmless when it is not a
        // segment), the per-wave sums and pass 2's sixteen exchange-1 reads as full-rate ds_read_b64 on counted waits.
        // Pass 2 therefore runs before the item word is looked at - on junk in an idle step and in the last.  All nineteen
        // reads are the helper's: with the item word and the sums read by the compiler in front of it, the first add of
        // the sums was scheduled into the first butterfly layer behind an s_waitcnt lgkmcnt(1), which waits for eighteen
        // of the nineteen and made the counted waits void right behind every step's barrier.
        auto pass2 = [&](int q) -> int {
            LdsCtl<true, DETREND> c;
            c.word_at = ctrl + q, c.sums_at = red + q * 8;
            if constexpr (COMPL) {
                // exchange 2 goes out with pass 2's last butterfly layer (dft16_layer2_scatter_sym), before the item word is
                // looked at.  In place: each thread rewrites exactly the sixteen elements it read above, and those reads
                // were complete at the last counted wait of the first layer.  In an idle step and in the last it rewrites
                // junk with junk: image q is this role's until the next barrier, which waits for the stores.
                int qs = q;      // (w2 == r1: the store address is formed on its own from an opaque image index, one
                asm volatile("" : "+s"(qs));      // v_add as in the parent - the budget tests pin the count with ==)
                float2 *ox = img + qs * LDS_X + w2;
                dft16_from_lds<17>(v, img + q * LDS_X + r1, [] { __builtin_amdgcn_s_setprio(WS_PBC); }, LdsNoMid(), &c,
                                   [&](float2 (&u)[16]) { dft16_layer2_scatter_sym<17>(u, ox, ts2); });
            } else {
            dft16_from_lds<17>(v, img + q * LDS_X + r1, [] { __builtin_amdgcn_s_setprio(WS_PBC); }, LdsNoMid(), &c);
            }
            if (DETREND) {
                const float2 h0 = make_float2(c.s[0].x, c.s[0].y), h1 = make_float2(c.s[0].z, c.s[0].w);
                const float2 h2 = make_float2(c.s[1].x, c.s[1].y), h3 = make_float2(c.s[1].z, c.s[1].w);
                const float2 tot = cadd(cadd(h0, h1), cadd(h2, h3));
                mean = make_float2(tot.x * (1.0f / 4096.0f), tot.y * (1.0f / 4096.0f));
            }
            return __builtin_amdgcn_readfirstlane(c.word);      // (an asm output counts as divergent)
        };
        // barrier of step `it`, then pass 2 of image it & 1
        auto next_item = [&]() -> int {
            __builtin_amdgcn_s_setprio(WS_PBL);
            lds_barrier();
            const int kind = pass2(it & 1);
            ++it;
            return kind;
        };
        // the same step without pass 2: the barrier and the item word only
        auto idle_step = [&]() -> int {
            __builtin_amdgcn_s_setprio(WS_PBL);
            lds_barrier();
            const int kind = ctrl[it & 1];
            ++it;
            return kind;
        };
        if (PILOT && p.pilot_inline) lds_barrier();      // the producers' pilot barrier
        // ONE instance of pass 2 feeds the body on the data path, the call at the body's end: with a second one in an idle
        // loop at the loop's head - while (item == ITEM_BUBBLE) item = next_item(); - the two instances' outputs sat in
        // different registers and every segment paid sixteen v_mov in the loop header.  Idle steps take their barrier and
        // read the item word, nothing else; the segment behind them gets its pass 2 on the way out, on the rare edge.
        // The loop's only exit is its own condition and the body is unconditional inside it: every further exit or
        // conditional around the body makes the compiler's control-flow structurizer merge two versions of the sixteen
        // accumulators per step (with the idle loop and the body in one conditional they were copied twice per step).
        // INVARIANT the loop relies on: step 0 is a segment or the stop, never an idle step - the producer publishes
        // ITEM_BUBBLE in one place only, behind a one-segment chunk under sched == 2, so a segment always comes first.
        // Entered with ITEM_BUBBLE this loop would accumulate pass 2 of junk (the loop it replaces tolerated that);
        // whoever gives the producer another idle step has to send the first item through the idle exit below as well.
        int item = next_item();           // nothing to consume in front of step 0
        while (item != ITEM_STOP) {       // (the producer left after the barrier of the step that published it)
            float2 *lx = img + ((it & 1) ^ 1) * LDS_X;      // v holds pass 2 of image (it - 1) & 1
            __builtin_amdgcn_s_setprio(WS_PBL);
            // in place: each thread rewrites exactly the sixteen elements it read (COMPL: pass2() has written them)
            if constexpr (!COMPL) {
                lx[w2] = v[r16(0)];
#pragma unroll
                for (int k1 = 1; k1 < 16; ++k1) lx[w2 + k1 * 17] = cmul(v[r16(k1)], tw2[k1]);
            }
            wave_lds_sync();              // exchange 2 stays inside the wave: program order is enough (COMPL: this is the
                                          // point between pass2()'s last store and the first read below)
            // exchange-2 reads as ordered ds_read_b64, the first butterfly layer on counted waits (-1.7 % kernel
            // time against the sixteen plain reads, which hipcc pairs into ds_read2_b64 behind one lgkmcnt(0);
            // the same treatment of the exchange-1 reads, which needs the butterfly before the item word is
            // looked at, gave 1.3 % back - whether with or without the stray wait described at pass2 is not recorded)
            dft16_from_lds<1>(v, lx + r2, [] { __builtin_amdgcn_s_setprio(WS_PBC); });
            if (DETREND) {                // X[k] -= mean * FFT(w)[k] where FFT(w) is not negligible
                v[r16(0)] = make_float2(v[r16(0)].x - (mean.x * fw.x - mean.y * fw.y),
                                        v[r16(0)].y - (mean.x * fw.y + mean.y * fw.x));
                if constexpr (!COMPL)      // (COMPL: the window's spectrum lies in [-136, 120), all of it in register 0)
                    v[r16(15)] = make_float2(v[r16(15)].x - (mean.x * fw.z - mean.y * fw.w),
                                             v[r16(15)].y - (mean.x * fw.w + mean.y * fw.z));
            }
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const float2 X = v[r16(k2)];
                acc[k2] = fmaf(X.x, X.x, fmaf(X.y, X.y, acc[k2]));
            }
            // the accumulation ends HERE: left free, the compiler sinks half of pass 3 and the sums of squares below the
            // rare branch behind the next pass 2 - their only reader is the next trip - and spills 36-51 registers
            asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]),
                              "+v"(acc[7]));
            asm volatile("" : "+v"(acc[8]), "+v"(acc[9]), "+v"(acc[10]), "+v"(acc[11]), "+v"(acc[12]), "+v"(acc[13]),
                              "+v"(acc[14]), "+v"(acc[15]));
            item = next_item();
            if (__builtin_expect(item == ITEM_BUBBLE, 0)) {
                do item = idle_step(); while (item == ITEM_BUBBLE);
                if (item == ITEM_DATA) pass2((it & 1) ^ 1);      // its barrier was the idle step's
            }
        }
        // bin k0 + 16 k1 + 256 k2 of this workgroup sits at t + 256 k2 (finalize_kernel layout 1)
        float *dst = p.partial + ((size_t)stream * W + wg) * 4096;
        if constexpr (COMPL) {
            // register mu of thread (k0, k1) = (hi, lo) holds bin kappa + 16 lambda + 256 mu with kappa = sym16(k0),
            // lambda = sym16(k1): in plain digits k0, k1 - [k0 >= 8] (mod 16) and mu less the borrows
            const int g = hi >> 3;
            const int down = (lo >> 3) + (lo == 0 ? g : 0);      // (never both)
            const int at = 16 * hi + ((lo - g) & 15);
#pragma unroll
            for (int mu = 0; mu < 16; ++mu) dst[((256 * mu - 256 * down) & 4095) + at] = acc[mu];
        } else {
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) dst[256 * k2 + t] = acc[k2];
        }
    }
}

template <bool DETREND, bool PILOT = false>
__global__ __launch_bounds__(TWS, 4) void welch4096ws_kernel(WelchArgs p) {
    welch4096ws_body<DETREND, PILOT, false>(p);
}
template <bool DETREND, bool PILOT = false>
__global__ __launch_bounds__(TWS, 4) void welch4096ws_compl_kernel(WelchArgs p) {
    welch4096ws_body<DETREND, PILOT, true>(p);
}

}  // namespace

int tuned4096_blocks_per_cu_ws() { return resident_blocks<welch4096ws_kernel<true, false>>(TWS, WS_LDS_BYTES); }

// 70 KiB of dynamic LDS: the opt-in is launch_lds's, once per build and device
hipError_t launch_welch_tuned4096_ws(const WelchArgs &a, hipStream_t s) {
    const dim3 grid(a.wg_per_stream, a.nstreams);
    const bool pilot = a.detrend && (a.pilot || a.pilot_inline);
    if (!a.compl_win) {
        if (pilot) return launch_lds<welch4096ws_kernel<true, true>>(grid, dim3(TWS), WS_LDS_BYTES, s, a);
        if (a.detrend) return launch_lds<welch4096ws_kernel<true, false>>(grid, dim3(TWS), WS_LDS_BYTES, s, a);
        return launch_lds<welch4096ws_kernel<false, false>>(grid, dim3(TWS), WS_LDS_BYTES, s, a);
    }
    // w[n] + w[n + 2048] = 1 (plan-time check, abi_welch.hip window_is_complementary)
    if (pilot) return launch_lds<welch4096ws_compl_kernel<true, true>>(grid, dim3(TWS), WS_LDS_BYTES, s, a);
    if (a.detrend) return launch_lds<welch4096ws_compl_kernel<true, false>>(grid, dim3(TWS), WS_LDS_BYTES, s, a);
    return launch_lds<welch4096ws_compl_kernel<false, false>>(grid, dim3(TWS), WS_LDS_BYTES, s, a);
}

}  // namespace oth
