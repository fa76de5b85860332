// csd4096ws: two-channel Welch cross spectrum for nperseg = nfft = 4096, 50 % overlap (BASELINE config 3) as TWO
// wave-specialised pairs in one 1024-thread workgroup per CU.
//
// Semantics of scipy.signal.csd / coherence with the Welch parameters of ofdm_cr_tools.py:322,342 (SURVEY.md 8a
// row a13: the producer of coherence_detector's first input, coherence_detector.py:45):
//     Pxx += |X|^2    Pyy += |Y|^2    Pxy += conj(X) Y
//
// Threads   0..255  Px  producer of stream x: loads, window, pass 1, exchange-1 writes        (as welch4096ws.hip)
//         256..511  Py  producer of stream y
//         512..1023 C   eight consumer waves; in each, lanes 0..31 consume x and lanes 32..63 consume y FOR THE SAME
//                       BINS (consumer index t = 32 wave + lane % 32 on the lane half's own pair of LDS images):
//                       pass 2, exchange 2, pass 3; then the lane halves trade spectra and each accumulates all four
//                       sums of eight of the sixteen bins.
// Each stream's pair of images works exactly as in the headline kernel (one LDS-only barrier per step, the consumers
// one segment behind the producers).  What is new is the exchange of spectra: X[k] and Y[k] of one bin sit in
// lanes l and l + 32 of one wave.  For bins k2 = j and j + 8 one v_permlane32_swap_b32 per component (gfx950: swaps
// the upper lane half of one register with the lower half of another - VALU, no LDS) leaves X[j], Y[j] in lane l and
// X[j + 8], Y[j + 8] in lane l + 32: sixteen swaps per step.  (Round 2 handed each lane its partner's sixteen bins
// through 32 ds_bpermute_b32 and chose Re / Im per lane half with 32 v_cndmask.)  Every thread carries 32
// accumulators (the one-role csd4096 kernel: 64, which held it at three waves per SIMD with no room to keep the
// overlapped halves or to prefetch): both streams are read once, the halves stay in registers, the next halves are
// prefetched, four waves per SIMD.  The fifteen pass-2 twiddles are multiplied out of two seeds per step (52 VALU).
// tried: the fifteen kept in registers (no room beside 32 accumulators at 128 VGPRs), and read from a 2 KiB LDS table
// between the butterfly layers of pass 2 (0.3126 against 0.3111 ms, 0.3495 against 0.3486 ms: no gain, NOTES 4.1c).
// tried: welch4096ws.hip's complementary-window producers (WelchArgs.compl_win; here eight of the sixteen window registers
// would go, for stored pass-1 twiddle powers: 650 -> 620 VALU per two segments with six stored).  Does not fit: beside the
// consumers' 32 accumulators the allocation already stands at 127 VGPRs, and with four, six, eight or ten stored powers
// both flavours came out at 128 VGPRs with 24-96 B of scratch (one reload per segment in the PILOT hot loop, 4-28
// accesses in the one-segment-chunk path), with and without the fence that keeps item()'s flavours apart there.  This
// kernel ignores compl_win.  (Its consumers load two seeds, not fifteen twiddles: one s_waitcnt vmcnt in their loop, left as it is.)
// The consumers' loop has the shape of welch4096ws.hip's (one instance of pass 2 on the data path, idle steps without one,
// every control read of a batch issued by dft16_from_lds itself): the path a segment pair executes went from 559 to 527
// VALU instructions (32 of 36 register copies in the loop header; scatter_pow16's four stay), and two compiler waits
// left the read batches - an lgkmcnt(0) for the item word in front of the exchange-1 reads, an lgkmcnt(1) behind the
// first counted wait of exchange 2.  121 / 127 VGPRs as before, no scratch.
//
// The two pairs run the same chunk schedule (Px draws the tickets, Py reads them), so x_s and y_s are always in
// the same step.  Frequency-domain detrend as in welch4096ws.hip (needs WelchArgs.fd).
#include <mutex>
#include <type_traits>
#include "fft4096.hip.h"
#include "launch.h"

namespace oth {
namespace {

constexpr int TCS = 1024;
constexpr int CS_RED = 32;                 // float2 per pair: per image the four producer waves' segment sums
constexpr int CS_CTRL = 16;                // ints per pair: item kind per image [0..1], next-chunk ticket [4] (pair 0)
constexpr size_t CS_PAIR_BYTES = (2 * LDS_X + CS_RED) * sizeof(float2) + CS_CTRL * sizeof(int);
constexpr size_t CS_FW_BYTES = 256 * sizeof(float4);      // window-spectrum entries of the detrend, one per t
constexpr size_t CS_LDS_BYTES = 2 * CS_PAIR_BYTES + CS_FW_BYTES;
static_assert((2 * CS_PAIR_BYTES) % 16 == 0, "the detrend table is read as float4");

enum { CS_STOP = 0, CS_DATA = 1, CS_BUBBLE = 2 };

// wave priorities: producer latency sections / butterflies, consumer latency sections / butterflies / swap + accumulate
// (profiles/r05_ab_c3_priorities.txt: every other assignment was slower, by 0.1-4 %)
constexpr int CS_PAL = 2, CS_PAC = 0, CS_PBL = 2, CS_PBC = 1, CS_PBA = 2;

template <bool DETREND, bool PILOT = false>
__global__ __launch_bounds__(TCS, 4) void csd4096ws_kernel(WelchArgs p) {
    static_assert(DETREND || !PILOT, "the pilot belongs to the detrend");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const bool producer = tid < 512;
    const int cidx = tid - 512;                                   // consumers: x in lanes 0..31, y in lanes 32..63
    int *ctrl0 = reinterpret_cast<int *>(reinterpret_cast<float2 *>(smem) + 2 * LDS_X + CS_RED);   // pair 0's: the ticket

    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y;
    const int sched = p.sched;
    const long long nchunks = sched ? chunk_count(p) : 1;

    if (producer) {
        // ------------------------------------------------------------------ producer (welch4096ws.hip)
        // One stream per team: the team index is wave-uniform and is taken INSIDE this branch, so that the stream's base
        // address and the team's LDS addresses are scalars (round 5: formed in front of the branch as a select between
        // the producers' uniform value and the consumers' per-lane one they were vector registers - every sample load
        // carried a 64-bit VGPR address and a v_lshl_add_u64, 450 of them in the file, and the PILOT build spilled).
        // (the thread index likewise: as a select with the consumers' index its range was unknown, and a lane offset that is
        // not provably below 2^32 bytes rules out the scalar-base + 32-bit-offset form of global_load)
        const int pair = __builtin_amdgcn_readfirstlane(tid >> 8);
        const int t = tid & 255, hi = t >> 4, lo = t & 15, wave = t >> 6;
        const int w1 = hi * 17 + lo;
        float2 *img = reinterpret_cast<float2 *>(smem + pair * CS_PAIR_BYTES);      // two images of LDS_X float2
        float2 *red = img + 2 * LDS_X;
        int *ctrl = reinterpret_cast<int *>(red + CS_RED);
        const float2 *xb = (pair ? p.y : p.x) + (size_t)stream * p.stream_stride;
        float win[16];
#pragma unroll
        for (int a = 0; a < 16; ++a) win[a] = p.win[256 * a + t];
        const float2 b1 = p.tw[t], b4 = p.tw[4 * t];
        float2 kw[8], nxt[8];
        float2 prev_new = make_float2(0.f, 0.f);
        // PILOT (every detrending plan but OTH_DETREND_CONSTANT_FAST): WelchArgs.pilot of this team's channel comes off every sample as it arrives
        float2 pv = make_float2(0.f, 0.f);      // pilot_inline: formed below, behind the first sample loads (welch4096ws.hip)
        if (PILOT && !p.pilot_inline) pv = load_pilot(p.pilot, pair * p.nstreams + stream);
        int it = 0;
        unsigned ticket = 0;
        using std::false_type;
        using std::true_type;
        using mid = std::integral_constant<int, 0>;
        using head = std::integral_constant<int, 1>;
        using none = std::integral_constant<int, 2>;
        auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
        auto load_chunk_head = [&](int first_seg) {
            const float2 *xs = xb + (size_t)uni(first_seg) * 2048;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 *xj = xs + 512 * j;
                kw[2 * j] = xj[(unsigned)t];
                kw[2 * j + 1] = xj[(unsigned)t + 256u];
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
        auto item = [&](auto first_, auto mode_, int s, int nsb, bool publish) {
            constexpr bool FIRST = decltype(first_)::value;
            constexpr int MODE = decltype(mode_)::value;
            const int q = it & 1;
            float2 *lx = img + q * LDS_X;
            __builtin_amdgcn_s_setprio(CS_PAL);
            float2 v[16];
            float2 sumf = make_float2(0.f, 0.f), sum = make_float2(0.f, 0.f);
            if (FIRST) {
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    if (PILOT) kw[a] = csub(kw[a], pv);
                    sumf = cadd(sumf, kw[a]);
                    kw[a] = make_float2(kw[a].x * win[a], kw[a].y * win[a]);
                }
            }
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const float2 r = PILOT ? csub(nxt[a], pv) : nxt[a];
                v[a] = kw[a];
                v[8 + a] = make_float2(r.x * win[8 + a], r.y * win[8 + a]);
                if (MODE == 0) kw[a] = make_float2(r.x * win[a], r.y * win[a]);
                sum = cadd(sum, r);
            }
            if (sched == 2 && t == 0 && pair == 0) {      // one ticket stream for both pairs
                if (FIRST) ticket = atomicAdd(p.queue + stream, 1u);
                if (publish) ctrl0[4] = (int)ticket;
            }
            if (MODE == 0) {
                const float2 *xn = xb + (size_t)uni(s + 2) * 2048;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float2 *xj = xn + 512 * j;
                    nxt[2 * j] = load_once(xj + (unsigned)t);
                    nxt[2 * j + 1] = load_once(xj + ((unsigned)t + 256u));
                }
            } else if (MODE == 1) {
                load_chunk_head(nsb);
            }
            if (DETREND) {
                sum.x = wave_total_lane63(sum.x);
                sum.y = wave_total_lane63(sum.y);
                float2 other = prev_new;
                if (FIRST) other = make_float2(wave_total_lane63(sumf.x), wave_total_lane63(sumf.y));
                if ((t & 63) == 63) red[q * 8 + wave] = cadd(sum, other);
                prev_new = sum;
            }
            __builtin_amdgcn_s_setprio(CS_PAC);
            dft16(v);
            __builtin_amdgcn_s_setprio(CS_PAL);
            scatter_pow16<RS>(v, lx + w1, b1, b4);
            step_end(CS_DATA);
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
        if (PILOT && p.pilot_inline) {      // this team's stream; per-wave totals into its image 1 (welch4096ws.hip)
            const PilotProbes probes = inline_pilot_load(xb, p.nseg, 2048, t);
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
                for (; s + 1 < se - 1; s += 2) {
                    item(false_type{}, mid{}, s, 0, false);
                    item(false_type{}, mid{}, s + 1, 0, false);
                }
                if (s < se - 1) item(false_type{}, mid{}, s, 0, false);
                ncur = (sched == 1) ? cur + W : W + uni(ctrl0[4]);
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
            item(true_type{}, none{}, sb, 0, true);
            if (sched == 0) break;
            if (sched == 2) {
                step_end(CS_BUBBLE);      // the only idle step, always behind a segment: the consumers' loop relies on it
                ncur = W + uni(ctrl0[4]);
            } else {
                ncur = cur + W;
            }
            have = open_chunk(ncur);
            if (have) load_chunk_head(sb);
        }
        step_end(CS_STOP);
    } else {
        // ------------------------------------------------------------------ consumer
        const int pair = (cidx >> 5) & 1;      // per lane half: x in lanes 0..31, y in lanes 32..63
        const int t = ((cidx >> 6) << 5) | (cidx & 31), hi = t >> 4, lo = t & 15;
        const int r1 = hi * RS + lo, w2 = hi * RS + lo, r2 = hi * RS + lo * 17;
        float2 *img = reinterpret_cast<float2 *>(smem + pair * CS_PAIR_BYTES);
        float2 *red = img + 2 * LDS_X;
        // W256^c, W256^(4c): the fifteen pass-2 twiddles are multiplied out per item (32 accumulators leave no room
        // for the thirty registers the headline kernel's consumer spends on them)
        const float2 c1 = p.tw[16 * lo], c4 = p.tw[64 * lo];
        // The detrend's window-spectrum entries and the segment mean are fetched from LDS where they are used: held in
        // registers across the step they pushed the allocation past 128 VGPRs, and the one spilled register came
        // back through scratch memory behind an s_waitcnt vmcnt(0) in every step (42 % of the consumers' time).
        float4 *fwl = reinterpret_cast<float4 *>(smem + 2 * CS_PAIR_BYTES);
        if (DETREND && pair == 0) fwl[t] = p.fd[t];      // lanes l and l + 32 (same t) are in one wave: ordered
        float axx[8], ayy[8], are[8], aim[8];      // lanes 0..31: bins k2 = j, lanes 32..63: bins k2 = j + 8
#pragma unroll
        for (int k = 0; k < 8; ++k) axx[k] = ayy[k] = are[k] = aim[k] = 0.f;
        float2 v[16];
        int it = 0;

        // What the producer left in image q: pass 2, with the item word read by the helper in the same batch (read by the
        // compiler in front of it, its readfirstlane drew an s_waitcnt lgkmcnt(0) in FRONT of the sixteen reads: one
        // exposed LDS round trip behind every step's barrier before the batch even went out)
        auto pass2 = [&](int q) -> int {
            LdsCtl<true, false> c;
            c.word_at = ctrl0 + q;
            dft16_from_lds<17>(v, img + q * LDS_X + r1, [] { __builtin_amdgcn_s_setprio(CS_PBC); }, LdsNoMid(), &c);
            return __builtin_amdgcn_readfirstlane(c.word);      // both streams run the same schedule
        };
        // barrier A of step `it`, then pass 2 of image it & 1
        auto next_item = [&]() -> int {
            __builtin_amdgcn_s_setprio(CS_PBL);
            lds_barrier();
            const int kind = pass2(it & 1);
            ++it;
            return kind;
        };
        // the same step without pass 2: the barrier and the item word only
        auto idle_step = [&]() -> int {
            __builtin_amdgcn_s_setprio(CS_PBL);
            lds_barrier();
            const int kind = __builtin_amdgcn_readfirstlane(ctrl0[it & 1]);
            ++it;
            return kind;
        };
        if (PILOT && p.pilot_inline) lds_barrier();      // the producers' pilot barrier
        // The loop as in welch4096ws.hip's consumer: one instance of pass 2 on the data path (the call at the body's end),
        // idle steps that take the barrier and read the item word only, the loop's condition its only exit, and the
        // accumulators pinned at the end of the body.  With next_item() also in an idle loop at the head the two
        // instances' outputs sat in different registers: 36 v_mov per segment in the loop header.
        // INVARIANT (as there): step 0 is a segment or the stop - the producers publish CS_BUBBLE only behind a
        // one-segment chunk under sched == 2; entered with CS_BUBBLE the loop would accumulate pass 2 of junk
        int item = next_item();
        while (item != CS_STOP) {
            const int q = (it & 1) ^ 1;   // the image whose pass 2 sits in v
            float2 *lx = img + q * LDS_X;
            __builtin_amdgcn_s_setprio(CS_PBL);
            scatter_pow16<17>(v, lx + w2, c1, c4);
            wave_lds_sync();
            // image q's sums stay valid until the barrier of the next step: the helper reads them in front of the
            // exchange-2 batch; the window-spectrum entries are fetched between the butterfly layers (mid(): behind the
            // counted waits, with the second layer to hide behind)
            float4 fw = make_float4(0.f, 0.f, 0.f, 0.f);
            LdsCtl<false, DETREND> c;
            c.sums_at = red + q * 8;
            dft16_from_lds<1>(v, lx + r2, [] { __builtin_amdgcn_s_setprio(CS_PBC); }, [&] { if (DETREND) fw = fwl[t]; }, &c);
            if (DETREND) {
                const float2 h0 = make_float2(c.s[0].x, c.s[0].y), h1 = make_float2(c.s[0].z, c.s[0].w);
                const float2 h2 = make_float2(c.s[1].x, c.s[1].y), h3 = make_float2(c.s[1].z, c.s[1].w);
                const float2 tot = cadd(cadd(h0, h1), cadd(h2, h3));
                const float2 mean = make_float2(tot.x * (1.0f / 4096.0f), tot.y * (1.0f / 4096.0f));
                v[r16(0)] = make_float2(v[r16(0)].x - (mean.x * fw.x - mean.y * fw.y),
                                        v[r16(0)].y - (mean.x * fw.y + mean.y * fw.x));
                v[r16(15)] = make_float2(v[r16(15)].x - (mean.x * fw.z - mean.y * fw.w),
                                         v[r16(15)].y - (mean.x * fw.w + mean.y * fw.z));
            }
            __builtin_amdgcn_s_setprio(CS_PBA);
            // v_permlane32_swap_b32 a, b swaps a's lanes 32..63 with b's lanes 0..31.  With a = bin j and b = bin j + 8
            // (x-stream values in lanes 0..31, y-stream values in lanes 32..63 of both): a' = X[j] | X[j + 8],
            // b' = Y[j] | Y[j + 8] - lane l holds bin j of both streams, lane l + 32 bin j + 8.
            //   Pxx += |X|^2,  Pyy += |Y|^2,  Pxy += conj(X) Y = (Xr Yr + Xi Yi) + i (Xr Yi - Xi Yr)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float2 a = v[r16(j)], b = v[r16(j + 8)];
                const auto sr = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
                const auto si = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
                const float2 X = make_float2(__uint_as_float(sr[0]), __uint_as_float(si[0]));
                const float2 Y = make_float2(__uint_as_float(sr[1]), __uint_as_float(si[1]));
                axx[j] = fmaf(X.x, X.x, fmaf(X.y, X.y, axx[j]));
                ayy[j] = fmaf(Y.x, Y.x, fmaf(Y.y, Y.y, ayy[j]));
                are[j] = fmaf(X.x, Y.x, fmaf(X.y, Y.y, are[j]));
                aim[j] += cross_im(X, Y);
            }
            // the accumulation ends here (left free it is sunk below the rare branch behind the next pass 2)
            asm volatile("" : "+v"(axx[0]), "+v"(axx[1]), "+v"(axx[2]), "+v"(axx[3]), "+v"(axx[4]), "+v"(axx[5]), "+v"(axx[6]), "+v"(axx[7]));
            asm volatile("" : "+v"(ayy[0]), "+v"(ayy[1]), "+v"(ayy[2]), "+v"(ayy[3]), "+v"(ayy[4]), "+v"(ayy[5]), "+v"(ayy[6]), "+v"(ayy[7]));
            asm volatile("" : "+v"(are[0]), "+v"(are[1]), "+v"(are[2]), "+v"(are[3]), "+v"(are[4]), "+v"(are[5]), "+v"(are[6]), "+v"(are[7]));
            asm volatile("" : "+v"(aim[0]), "+v"(aim[1]), "+v"(aim[2]), "+v"(aim[3]), "+v"(aim[4]), "+v"(aim[5]), "+v"(aim[6]), "+v"(aim[7]));
            item = next_item();
            if (__builtin_expect(item == CS_BUBBLE, 0)) {
                do item = idle_step(); while (item == CS_BUBBLE);
                if (item == CS_DATA) pass2((it & 1) ^ 1);      // its barrier was the idle step's
            }
        }
        // channels xx, yy, re, im; bin k0 + 16 k1 + 256 k2 at t + 256 k2 (finalize_kernel layout 1)
        float *dst = p.partial + ((size_t)stream * W + wg) * 4 * 4096;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int o = 256 * (pair ? j + 8 : j) + t;
            dst[o] = axx[j];
            dst[4096 + o] = ayy[j];
            dst[8192 + o] = are[j];
            dst[12288 + o] = aim[j];
        }
    }
}

}  // namespace

int csd4096ws_blocks_per_cu() { return resident_blocks<csd4096ws_kernel<true, false>>(TCS, CS_LDS_BYTES); }

hipError_t launch_csd_tuned4096ws(const WelchArgs &a_in, hipStream_t s) {
    WelchArgs a = a_in;
    const dim3 grid(a.wg_per_stream, a.nstreams);
    // A plan WITHOUT detrend runs the detrending build on an all-zero window-spectrum table (round 6): X - mean * 0 is X
    // bit for bit, the per-wave sums cost the step ~1 %, and the build without them - csd4096ws_kernel<false, false> - was
    // the one two-channel build that spilled (five registers around the producer's chunk boundary; verdict r5).
    static float4 *zero_fd[64] = {};
    if (!a.detrend) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
        {
            static std::mutex once;      // contexts of several threads may come here at the same time
            std::lock_guard<std::mutex> g(once);
            if (!zero_fd[dev]) {
                float4 *z = nullptr;
                hipError_t e = hipMalloc(&z, 256 * sizeof(float4));
                // hipMemset of device memory may return before the fill has run, and a non-blocking stream is not ordered
                // behind it: the first launch then read whatever the block held before (a freed window-spectrum table of
                // an earlier plan took the DC line out of a plan WITHOUT detrend).  Once per device: wait for it.
                if (e == hipSuccess) e = hipMemset(z, 0, 256 * sizeof(float4));
                if (e == hipSuccess) e = hipDeviceSynchronize();
                if (e != hipSuccess) return e;
                zero_fd[dev] = z;
            }
        }
        a.fd = zero_fd[dev];
        a.detrend = 1;
        a.pilot = nullptr;
        a.pilot_inline = 0;
    }
    // 140 KiB of dynamic LDS: the opt-in is launch_lds's, once per build and device
    if (a.pilot || a.pilot_inline) return launch_lds<csd4096ws_kernel<true, true>>(grid, dim3(TCS), CS_LDS_BYTES, s, a);
    return launch_lds<csd4096ws_kernel<true, false>>(grid, dim3(TCS), CS_LDS_BYTES, s, a);
}

}  // namespace oth
