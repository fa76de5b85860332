// Internal declarations shared by the HIP translation units of libofdmtools_hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "row_layout.h"

namespace oth {

// Launch description of the segment-averaging (Welch / CSD) kernels.
constexpr int kPilotProbes = 8;      // segment means per stream behind WelchArgs.pilot / SegArgs.pilot

struct WelchArgs {
    const float2 *x;        // device IQ, stream 0
    const float2 *y;        // second channel (CSD) or nullptr
    const float *win;       // device window, nperseg floats
    const float2 *tw;       // device twiddle table W_nfft^k, nfft entries
    float *partial;         // [nstreams][wg_per_stream][nch][nfft] partial sums
    long long nseg;         // segments per stream
    size_t stream_stride;   // samples between streams
    int nperseg;
    int step;               // nperseg - noverlap
    int detrend;
    int wg_per_stream;
    int nstreams;
    // welch4096 segment schedule: 0 contiguous, 1 interleaved chunks, 2 dynamic chunk queue
    int sched;
    int chunk;              // segments per chunk (sched 1, 2)
    int tail_chunk;         // segments per chunk after the first nbig chunks
    long long nbig;         // number of full-size chunks
    unsigned *queue;        // [nstreams] tickets, zeroed before the launch (sched 2)
    // welch4096ws frequency-domain detrend: per consumer thread t = 16 k0 + k1 the window spectrum at bins
    // k0 + 16 k1 and k0 + 16 k1 + 3840 (re, im, re, im); nullptr when the window's spectrum is not confined
    const float4 *fd;
    // Pilot of the constant detrend (round 4; every plan but OTH_DETREND_CONSTANT_FAST): per stream (x streams, then y
    // streams) kPilotProbes segment means spread over the launch (launch_pilot_mean); load_pilot() averages them into one
    // complex value NEAR the stream's mean.  The PILOT build of every detrending kernel subtracts it from each sample
    // as it is loaded, so the sums, the window products and (in the builds that detrend after the transform) the
    // transform itself see x - pilot: no DC line whose float32 rounding would stay behind, and the segment mean that is
    // removed afterwards is a small residual known to its own rounding.  The result is mathematically unchanged (a
    // constant detrend removes any constant); numerically bins 0, +-1 go from the float32 mean's 1e-4 ... 5e-3 (SciPy
    // on complex64 included) to 1e-6.  nullptr: the builds without.
    const float2 *pilot;
    // 1 (round 5; the role-split 4096-point kernels, one- and two-channel): the PILOT build forms its pilot itself in
    // the launch's prologue - every producer team adds eight probes of 256 consecutive samples spread over its stream
    // (inline_pilot() in fft4096.hip.h) - instead of reading WelchArgs.pilot: no pilot_mean_kernel launch in front of the
    // transform (5.9 us + a dependent-launch gap per step).  The pilot only has to be NEAR the mean; every workgroup reads
    // the same samples in the same order, so all hold the same bits.
    int pilot_inline;
    // 1 (welch4096ws only): the plan's window satisfies w[n] + w[n + nfft / 2] = 1 to one float32 ulp (SciPy's periodic
    // Hann; checked in double at plan time), so the producer forms r w[n + nfft / 2] as fma(-r, w[n], r) and holds no
    // window value in a register.  0: the general build, any window.
    int compl_win;
    // compl_win only.  symtw: the plan's (tan(theta / 2), sin(theta)) pairs, theta = 2 pi e / 4096, entry kSymTwOrigin + e for
    // |e| <= kSymTwOrigin (symtw_table(), abi_ctx.hip) - the three-shear twiddles of the build's signed-digit passes.
    // fd_sym (detrending plans): per consumer thread t = 16 k0 + k1 the window spectrum at the bin of its register 0,
    // k = sym16(k0) + 16 sym16(k1) in [-136, 120), times the phase and sign the build leaves on that register
    // (window_spectrum_table_sym(), abi_welch.hip); the plan has checked that the window's spectrum is negligible elsewhere.
    const float2 *symtw;
    const float2 *fd_sym;
};
constexpr int kSymShift = 136;          // welch4096ws, compl_win: time origin of the transform (n' = n - 136 = 256 a + 16 (b - 8) + (c - 8))
constexpr int kSymTwOrigin = 1100;      // exponents read: |kappa (t - 136)| <= 8 * 136 = 1088, |16 lambda (c - 8)| <= 1024

// Launch description of segfft.hip: segment transforms of 1024 / 2048 / 4096 points by teams of nfft / 16
// threads, Welch average or periodogram chain (see the file header).
struct SegArgs {
    const float2 *x;        // device IQ, stream 0
    size_t stream_stride;   // samples between streams
    int nstreams;
    const float *win;       // nfft floats
    const float2 *tw;       // W_nfft^k, nfft entries
    const float4 *fd;       // role-split build, frequency-domain detrend: [nfft / 16 threads][16 / R] window-spectrum pairs
    const float2 *pilot;    // per stream, as WelchArgs.pilot (nullptr: none)
    long long first;        // sample index of segment 0 (chain: first kept vector)
    long long step;         // samples between segment starts (chain: keep_n * nfft)
    long long nseg;         // segments per stream
    int detrend;
    int chain;              // 0: Welch average (sum |X|^2 of every segment); 1: periodogram chain
    float *partial;         // [nstreams][wg_per_stream][nfft] accumulator rows, natural bin order (or nullptr)
    // chain only
    int acc_mode;           // 1 weighted sum (IIR), 2 max (peak hold), 3 none
    long long acc_end;      // segments s < acc_end take part in the accumulation
    float l2;               // log2(1 - alpha): weight of segment s is 2^(l2 (acc_end - 1 - s))
    float *rows;            // [nstreams][nseg - store_from][nfft]: epilogue values of segments s >= store_from
    long long store_from;
    int epilogue;           // OTH_EPI_*
    float scale;            // applied to |X|^2 (MAG2_OVER_N2)
    int fftshift;
    // schedule (as WelchArgs)
    int wg_per_stream;
    int sched;
    int chunk;
    int tail_chunk;
    long long nbig;
    unsigned *queue;
};

struct PgramArgs {
    const float2 *x;
    const float *win;       // nfft floats
    const float2 *tw;
    float *rows;            // [nrows][nfft]
    long long first_vec;    // index of the first kept vector in x
    long long nrows;
    int keep_n;
    int fftshift;
    int epilogue;
    float scale;            // applied to |X|^2 (OVER_N2)
};

constexpr int kReduceGroups = 16;   // row groups of the two-stage partial-sum reduction
// Many SHORT partial rows (256 ... 1024 points: 2048 ... 12288 teams' rows of 1 ... 4 KiB): the one-launch reduction has
// nfft / 16 = 16 ... 64 workgroups to read 8-12 MiB with (63 / 33 / 13 us at 256 / 512 / 1024 points, late round 5).
// There the rows go through `finalize_row_groups(nfft, W)` groups first - enough for 256 workgroups - and the one-launch
// kernel then takes the group rows.  0: not this shape.
inline int finalize_row_groups(int nfft, int W, int nch) {
    if (nch != 1 || nfft > 1024 || (nfft % 256) != 0 || W < 1024) return 0;
    return 65536 / nfft;      // (nfft / 256) x groups = 256 workgroups: 256 / 128 / 64 groups
}

// ---- the output stage of a finalize launch (out_stage.hip.h; abi_state.h fills it from the plan) ---------------------------
struct OutStage {
    int fftshift, trim;
    int db;                 // the PSD rows only (psd_value)
    int nout;               // nfft - 2 trim
};

struct FinalizeArgs {
    const float *partial;   // [nstreams][W][nch][nfft]
    float *scratch;         // [nstreams][kReduceGroups][nch][nfft] or nullptr (single-stage)
    float *out0;            // psd / pxx      [nstreams][nout]
    float *out1;            // pyy  (CSD)
    float *out2;            // pxy  interleaved (CSD)
    float *out3;            // cxy  (CSD)
    double scale;
    int W;
    int nfft;
    int nch;                // 1 or 4
    RowLayout layout;       // bin order of the partial rows (row_layout.h)
    int l1, l2;             // ROW_TWOLEVEL only
    OutStage out;
    int accumulate;         // one channel (store_psd): 0 out0 = scaled output; 1 out0 += raw sums (streaming form);
                            // 2 out0 = raw sums as they are (oth_welch_partial_dev, first pass of the jackknife)
    unsigned *queue_reset;  // chunk-ticket counters of the averaging kernel, zeroed here for the next launch (or null)
    int queue_n;
    // Completion word for a host that polls instead of sleeping in hipStreamSynchronize (oth_welch_exec / _poll / _wait,
    // round 5): the outputs go straight to pinned host memory; every block makes its stores visible at system scope and
    // arrives on done_count (device; the last block re-arms it to 0), and the last one to arrive then stores seq_value
    // into *host_seq (pinned).  nullptr: none of this runs.
    unsigned *done_count;
    unsigned *host_seq;
    unsigned seq_value;
};

// Every launcher returns hipSuccess / error of the launch only (asynchronous).
hipError_t launch_welch_generic(int nfft, const WelchArgs &a, hipStream_t s);
// welch4096.hip is built once per variant tag (Makefile: dpp, pipe); nfft 4096, nperseg 4096, y == nullptr
#define OTH_DECL_W4096(tag)                                                     \
    hipError_t launch_welch_tuned4096_##tag(const WelchArgs &a, hipStream_t s); \
    int tuned4096_blocks_per_cu_##tag();
OTH_DECL_W4096(dpp)
OTH_DECL_W4096(pipe)
// welch4096ws.hip: wave-specialised producer/consumer form; step 2048, detrend needs WelchArgs.fd
OTH_DECL_W4096(ws)
// csd4096.hip: two-channel cross spectrum, nfft = nperseg = 4096
hipError_t launch_csd_tuned4096(const WelchArgs &a, hipStream_t s);
int csd4096_blocks_per_cu();
// csd4096ws.hip: the same as two wave-specialised pairs in one 1024-thread workgroup; step 2048, WelchArgs.fd for detrend
hipError_t launch_csd_tuned4096ws(const WelchArgs &a, hipStream_t s);
int csd4096ws_blocks_per_cu();
// welch16k.hip: nfft = nperseg = 16384 (one 1024-thread workgroup per CU) or 8192 (two 512-thread workgroups)
hipError_t launch_welch_tuned16k(int nfft, const WelchArgs &a, hipStream_t s);
// welch16k1x.hip: nfft = nperseg = 16384, no detrend, whole-segment loads (the scanner's non-overlapping vectors): one
// cross-wave exchange, two workgroup barriers per segment; partial rows in x1_layout(nfft)
hipError_t launch_welch_tuned16k1x(int nfft, const WelchArgs &a, bool window, bool plain, hipStream_t s);
// the same transform at step = 8192 (50 % overlap, the kept half in registers); WelchArgs.fd = window_spectrum_table_16k1x
hipError_t launch_welch_tuned16k1x_half(int nfft, const WelchArgs &a, hipStream_t s);
hipError_t launch_welch_tuned8kws(const WelchArgs &a, hipStream_t s);      // 8192 points, 50 % overlap, role-split (contiguous runs only)
// the fused periodogram chain at 8192 / 16384 points (one workgroup per segment; workgroups per CU: 2 / 1)
hipError_t launch_chain16k(int nfft, const SegArgs &a, bool rect, hipStream_t s);
// the same chain at 16384 points on the one-exchange pipelined loop (welch16k1x.hip); partial rows in ROW_X1_16K; needs
// chunks of at least two segments
hipError_t launch_chain16k1x(int nfft, const SegArgs &a, bool rect, hipStream_t s);
hipError_t launch_pgram(int nfft, const PgramArgs &a, hipStream_t s);
// segfft.hip
bool seg_supported(int nfft);
// kind: 0 Welch with step = nfft / 2 (the overlapped half stays in registers), 1 Welch with any step, 2 chain
int seg_teams_per_cu(int nfft, int kind, bool wps4);
hipError_t launch_seg(int nfft, const SegArgs &a, int kind, bool wps4, hipStream_t s);
// zero-padded segments (nperseg = nfft / 4 or nfft / 2 at nfft = 1024 / 2048: the sweeper's call at those sizes)
bool seg_padded_supported(int nfft, int nperseg);
int seg_padded_teams_per_cu(int nfft, int nperseg, int kind);
hipError_t launch_seg_padded(int nfft, int nperseg, const SegArgs &a, int kind, hipStream_t s);
int segws_teams_per_cu(int nfft);
hipError_t launch_segws(int nfft, const SegArgs &a, int det, hipStream_t s);
// partial rows of a chain launch + the stored raw rows -> IIR / peak state and the rows handed back; `scratch` holds
// chain_tail_groups(W, nfft) rows of nfft floats (0 rows: not needed)
int chain_tail_groups(int W, int nfft);
// layout: bin order of the partial rows (row_layout.h)
hipError_t launch_chain_tail(const float *partial, float *scratch, int W, int nfft, RowLayout layout, int fftshift, int acc_mode, long long nbase,
                             float alpha, float kdb, float *iir_state, float *peak_state, const float *raw_rows,
                             long long nraw, float *rows_out, hipStream_t s);
hipError_t launch_set_flag(int *flag, int v, hipStream_t s);
hipError_t launch_finalize(const FinalizeArgs &a, int nstreams, hipStream_t s);
hipError_t launch_scale(const float *sum, float *out, int nfft, double scale, const OutStage &stage, hipStream_t s);
hipError_t launch_csd_scale(const float *sums, int nfft, double scale, const OutStage &stage, float *pxx, float *pyy, float *pxy,
                            float *cxy, hipStream_t s);
hipError_t launch_rows_epilogue(float *rows, long long nrows, int nfft, float alpha, float kdb, float *iir_state,
                                float *peak_state, int *peak_init, int do_iir, int do_peak, hipStream_t s);
hipError_t launch_group_mean(const float *rows, long long ngroups, int nfft, int group, float *out, hipStream_t s);
hipError_t launch_channel_power(const float *psd, int nrows, int nfft, double srch_bins, int nch, const int *lo,
                                const int *hi, double *movavg, float *power, float *movavg_f, hipStream_t s);
// tile_min: nrows x scan_decide_tiles(nfft) floats of scratch (the per-tile minima of the moving average)
int scan_decide_tiles(int nfft);
hipError_t launch_scan_decide(const float *psd, int nrows, int nfft, double srch_bins, float thr, int nch, const int *lo,
                              const int *hi, double *movavg, float *tile_min, unsigned char *mask, float *noise, float *power,
                              hipStream_t s);
hipError_t launch_bin_threshold(const float *psd, int nrows, int nfft, double srch_bins, float thr,
                                unsigned char *mask, float *noise, hipStream_t s);
hipError_t launch_xcorr(int L, const float2 *a, const float2 *b, const float2 *tw, float *out, int mode,
                        hipStream_t s);
hipError_t launch_synth(float2 *iq, size_t n, uint64_t seed, int ntones, const float *amp, const float *freq,
                        float dc_re, float dc_im, hipStream_t s);
hipError_t launch_read_probe(const void *p, size_t bytes, float *sink, hipStream_t s);
hipError_t launch_read_probe8(const void *p, size_t bytes, float *sink, hipStream_t s);
hipError_t launch_iq_power(const float2 *iq, size_t n, double *acc4, hipStream_t s);
// out[(channel * nstreams + stream) * kPilotProbes + k] = mean of the n samples of segment (nseg - 1) k / (kPilotProbes - 1)
// of stream `stream` of x (channel 0) and, when y != nullptr, of y (channel 1)
hipError_t launch_pilot_mean(const float2 *x, const float2 *y, size_t stream_stride, int n, long long step, long long nseg,
                             int nstreams, float2 *out, hipStream_t s);

bool generic_supported(int nfft);
size_t generic_lds_bytes(int nfft);
int generic_threads_for(int nfft);

// ---- fft_any.hip: transforms of any length (round 6) -------------------------------------------------------------------
constexpr int kAnyMaxPasses = 12;            // 2 * 3^8 = 13122 takes nine passes
constexpr int kAnyMaxTile = 16384;           // points of one LDS tile (128 KiB)
constexpr int kAnyMaxFft = 1 << 20;          // longest transform (and longest Bluestein M): L1 = 4096 rows of L2 = 256
enum AnyKind { ANY_NONE = 0, ANY_DIRECT, ANY_TWOLEVEL, ANY_BLUESTEIN, ANY_BLUESTEIN2 };

struct AnyShape {        // pure host description of a length (any_describe): needs no device
    int nfft;            // the transform the caller asked for
    int kind;            // AnyKind
    int L;               // length of the transforms that run (nfft, or Bluestein's M)
    int L1, L2, C;       // two-level split L = L1 L2 (L2 = row length) and columns per K1 / K3 tile
};
int any_describe(int nfft, AnyShape *out);      // 0, or -1 when the length is outside [1, kAnyMaxFft] (Bluestein: M too long)
bool any_smooth(int n);
int any_threads_for(int points);

struct AnyPass {
    int R;               // radix: 16, 8, 4, 2, 3, 5, 7
    int NS;              // length of the sub-transforms this pass combines
    int nbf;             // butterflies per column = n / R
    int inner;           // twiddle index step in units of W_n: n / (NS R)
    float inv_ns;
};
struct AnyFftDesc {
    int n, logC, npass;
    int tws;             // table order / n: W_n^j = tw[j tws]
    int tw_lds;          // 1: the kernel stages the n twiddles W_n^j in LDS behind the tile
    const float2 *tw;    // W_order^k
    AnyPass pass[kAnyMaxPasses];
};
void any_make_desc(int n, int C, const float2 *tw, int order, AnyFftDesc *d);

struct AnyArgs {
    AnyFftDesc f;
    // element (i, c) of tile t (blockIdx.x) of segment s sits at  i * es + t * tile_stride + c * cs  of the segment:
    // column tiles (cs = 1: C adjacent columns, es = the row length) or row tiles (es = 1, cs = the row length)
    int es, tile_stride, cs;
    float inv_n;               // 1 / f.n (row tiles)
    long long nseg;            // segments of this launch (rows blockIdx.y, blockIdx.y + gridDim.y, ...)
    // load 1 (stage): samples x[first + s seg_step + n], n < nperseg, (x - mean) * win [* chirp], zero padded
    int load_op;
    const float2 *x, *y;
    long long first, seg_step;
    int nperseg;
    const float *win;
    const float4 *mean;        // [channel][segment] (hi.re, hi.im, lo.re, lo.im) or nullptr
    size_t mean_ch_stride;
    const float2 *chirp;       // Bluestein c[n] or nullptr
    // load 0 / store 0: the workspace, [channel][segment][L]
    float2 *ws;
    size_t ws_seg_stride, ws_ch_stride;
    // mid 1: v = conj(v * midtab[nat]) and the transform again
    int mid_op;
    const float2 *midtab;
    // natural index of element (i, c) of tile t: i nat_i + t nat_t + c nat_c; position in a partial row likewise (pp_*)
    int nat_i, nat_t, nat_c, pp_i, pp_t, pp_c;
    // store 0: optional four-step twiddle twbig[i (t tw_t + c tw_c)]
    const float2 *twbig;
    int tw_t, tw_c;
    // store 1 / 2: partial[gridDim.y rows][channels][nbins]
    float *partial;
    int nbins;                 // bins kept (Bluestein: the first nfft of M)
    int first_chunk;           // overwrite (1) or add to (0) the partial rows
    int conj_out;              // the transform leaves conj(X) (Bluestein): matters for the cross term only
    // store 3: rows[s][nbins]
    float *rows;
    int epilogue, fftshift;
    float scale;
};
hipError_t launch_any_fft(const AnyArgs &a, int tiles, int gy, int gz, int store, hipStream_t s);
hipError_t launch_any_mean(const float2 *x, const float2 *y, long long first, long long seg_step, int nperseg, long long nseg,
                           float4 *out, size_t ch_stride, hipStream_t s);
hipError_t launch_any_ew(int op, float2 *dst, const float2 *src, const float2 *src2, const float2 *tab, int n, int nsrc, int L1,
                         int L2, hipStream_t s);
hipError_t launch_any_abs(float *out, const float2 *src, int n, float scale, hipStream_t s);

// ---- fft_tl.hip: the four-step route at 32768 / 65536 points on register radix-16 butterflies ---------------------------
struct TlArgs {
    const float2 *x;           // samples; segment s starts at x[first + s seg_step]
    const float2 *y;           // second channel (two-channel sums) or nullptr
    size_t aux_ch_stride;      // entries between the channels' means / sub-block sums
    size_t ws_ch_stride;       // points between the channels' workspaces
    long long first, seg_step;
    int nperseg;               // samples per segment (zero padded to L)
    const float *win;          // L window values, zero behind nperseg (oth_welch_plan's zero-extended table)
    const float4 *mean;        // per segment (hi.re, hi.im, lo.re, lo.im) or nullptr
    const double2 *bsum;       // or: sums of sub-blocks of kTlSub samples from x[first] on; segment s takes nsub of them
    int nsub, sub_step;        // from index s * sub_step
    float2 *ws;                // workspace [segment][k1][n2]
    size_t ws_seg_stride;
    long long nseg;
    const float2 *tw;          // W_L^k
    float *partial;            // [W][channels 1 | 4][L] sums in ROW_TWOLEVEL
    int first_chunk;
};
constexpr int kTlSub = 4096;
bool tl_supported(int L);
// welch32k.hip: 32768-point segments inside one workgroup
struct W32kArgs {
    const float2 *x;           // samples; segment s starts at x[first + s step]
    long long first, step;
    long long nseg;
    const float *win;          // 32768 window values
    const float2 *tw;          // W_32768^k, k < 32768
    float *partial;            // [W][32768] sums in ROW_W32K (front: [W][65536] in ROW_W64K)
    int detrend;
    int front;                 // 1: 65536-point segments, a pair of workgroups each (win: 65536 values, tw: W_65536^k)
    const float *wpm;          // front + detrend: w[n] + w[n + 32768] (n < 32768), then w[n] - w[n + 32768]
};
int welch32k_rows(long long nseg, int cus, bool front = false);
hipError_t launch_welch32k(const W32kArgs &a, int W, hipStream_t s);
hipError_t launch_tl_blocksum(const float2 *x, long long first, long long nblocks, double2 *out, hipStream_t s);
hipError_t launch_tl_mean(const float2 *x, long long first, long long seg_step, int nperseg, long long nseg, float4 *out, hipStream_t s);
hipError_t launch_tl_k1(int L, const TlArgs &a, hipStream_t s);
hipError_t launch_tl_k2(int L, const TlArgs &a, int W, hipStream_t s);

// ---- median over segments (scipy.signal.welch average='median') ------------------------------------------------------
// segfft.hip: one raw |X|^2 row per segment, [stream][segment][nfft] in natural bin order, nperseg = nfft 256 ... 4096;
// a.detrend: each segment's own mean comes off (time domain, before the transform).  SegArgs as the chain's (chain = 1).
int seg_rows_teams_per_cu(int nfft);
hipError_t launch_seg_rows(int nfft, const SegArgs &a, hipStream_t s);

// median.hip: exact order statistics of nseg rows per bin by a radix select over the float bit patterns (8-bit digits
// from the top, four passes; integer counts only, so the result does not depend on the schedule).
struct MedianArgs {
    const unsigned *rows;   // [nstreams][nseg][nfft] bit patterns of non-negative floats (|X|^2)
    long long nseg;
    long long seg_per_wg;   // segments of one histogram workgroup (grid.y chunks per tile)
    int nfft;
    int nstreams;
    unsigned *counts;       // [nstreams][nfft][256] digit counts of the pass, all zero between passes
    unsigned *state;        // [nstreams][nfft][2]: key prefix fixed so far, rank left inside it
    unsigned *above;        // [nstreams][nfft]: smallest key above the final 24-bit bucket (last pass)
    unsigned *nanflag;      // [nstreams][nfft]: 1 when a segment value of the bin is NaN
    float *med;             // [nstreams][nfft] the median (mean of the two middle values for even nseg)
};
constexpr int kMedianTile = 64;                 // bins per histogram workgroup
size_t median_scratch_words(int nfft, int nstreams);      // counts + state + above + nanflag
void median_bind_scratch(MedianArgs &a, unsigned *scratch);
long long median_seg_per_wg(long long nseg, int nfft, int nstreams, int cu_count);
hipError_t launch_median_select(const MedianArgs &a, hipStream_t s);

// ---- mtm.hip: multitaper PSD, sum_k c_k |FFT((x - mean) v_k)|^2 per segment, nfft a power of two 64 ... 16384 ----------
struct MtmArgs {
    const float2 *x;        // device IQ, stream 0
    const float *tapers;    // [ntapers][nfft], each taper zero-extended behind nperseg
    const float *coef;      // [ntapers] c_k
    const float2 *tw;       // W_nfft^k, nfft entries
    float *partial;         // [nstreams][wg_per_stream][nfft] partial sums, natural bin order
    long long nseg;         // segments per stream
    size_t stream_stride;   // samples between streams
    int nperseg;
    int step;
    int detrend;            // != 0: each segment's own mean comes off (pilot + residual)
    int ntapers;
    int wg_per_stream;      // workgroups of a stream: each walks a contiguous run of the nseg x ntapers (segment, taper) items
    int nstreams;
};
// resident workgroups per CU of the build (occupancy calculator: needs a device; 0 when it fails)
int mtm_blocks_per_cu(int nfft);
hipError_t launch_mtm(int nfft, const MtmArgs &a, hipStream_t s);

// ---- mtmcsd.hip: the same taper loop on two channels - sum_k c_k of |X_k|^2, |Y_k|^2, Re and Im conj(X_k) Y_k ----------
struct MtmCsdArgs {
    MtmArgs m;              // x, the tables and the work split as mtm.hip's; partial: [nstreams][wg_per_stream][4][nfft]
    const float2 *y;        // second channel, laid out as x
    float2 *ws;             // [nstreams][wg_per_stream][mtmcsd_ws_points(nfft)]: where X's spectrum waits for Y's (16384 points)
};
size_t mtmcsd_ws_points(int nfft);      // 0: the build keeps both spectra in LDS
int mtmcsd_blocks_per_cu(int nfft);
hipError_t launch_mtmcsd(int nfft, const MtmCsdArgs &a, hipStream_t s);

// ---- mtmftest.hip: Thomson's harmonic F-test on the same taper loop; the work item is a whole segment ------------------
struct MtmFtestArgs {
    MtmArgs m;              // x, the tables and the sizes as mtm.hip's (coef unused); wg_per_stream: each workgroup walks a
                            // contiguous run of the nseg segments; partial: [nstreams][wg_per_stream][2][nfft] sum num, sum den
    const float *u;         // [ntapers] U_k = sum_n v_k[n]
    float inv_s;            // 1 / sum_k U_k^2
    float *ws;              // [nstreams][wg_per_stream][mtm_ftest_ws_floats(nfft)]: a segment's sy / p between its tapers (16384 points)
};
struct FtestFinalizeArgs {
    const float *partial;   // [nstreams][W][2][nfft], natural bin order
    float *f_out;           // [nstreams][nout]
    float *line_out;        // or nullptr
    float *resid_out;       // or nullptr
    double km1;             // K - 1
    double line_scale;      // 1 / (S nseg)
    double resid_scale;     // scale / ((K - 1) nseg)
    int W, nfft;
    OutStage out;
};
size_t mtm_ftest_ws_floats(int nfft);      // 0: the build keeps sy / p in registers
int mtm_ftest_blocks_per_cu(int nfft);
hipError_t launch_mtm_ftest(int nfft, const MtmFtestArgs &a, hipStream_t s);
hipError_t launch_ftest_finalize(const FtestFinalizeArgs &a, int nstreams, hipStream_t s);

// ---- mtmjack.hip: the jackknife over the (segment, taper) items, second pass (the first is the plan's own averaging) ------
struct MtmJackArgs {
    MtmArgs m;              // as mtm.hip's; partial: [nstreams][wg_per_stream][2][nfft] sum l, sum l^2
    const float *totals;    // [nstreams][nfft] S = sum_i p_i of the first pass, natural bin order
};
struct MtmCsdJackArgs {
    MtmCsdArgs c;           // as mtmcsd.hip's; partial: [nstreams][wg_per_stream][6][nfft] sum lx, lx^2, ly, ly^2, d, d^2
    const float *totals;    // [nstreams][4][nfft] Sxx, Syy, Sxy (re, im interleaved) of the first pass, natural bin order
};
struct JackFinalizeArgs {
    const float *partial;   // [nstreams][W][2 npairs][nfft], natural bin order
    float *sd_out[3];       // [nstreams][nout] root of the jackknife variance of pair 0 ... npairs - 1, or nullptr
    const float *cxy_nat;   // [nstreams][nfft] Cxy of the first pass in natural order (two channels), for cxy_out
    float *cxy_out;         // or nullptr
    double m;               // the item count M
    double mm1_over_m;      // (M - 1) / M
    int npairs;             // 1 (lnsd) or 3 (lnsd x, lnsd y, zsd)
    int W, nfft;
    OutStage out;
};
size_t mtmcsd_jack_ws_points(int nfft);      // 0: the build keeps both spectra in LDS
int mtm_jack_blocks_per_cu(int nfft);
int mtmcsd_jack_blocks_per_cu(int nfft);
hipError_t launch_mtm_jack(int nfft, const MtmJackArgs &a, hipStream_t s);
hipError_t launch_mtmcsd_jack(int nfft, const MtmCsdJackArgs &a, hipStream_t s);
hipError_t launch_jack_finalize(const JackFinalizeArgs &a, int nstreams, hipStream_t s);

// ---- mtmadapt.hip: Thomson's adaptive weighting on the same taper loop; the work item is a whole segment -----------------
struct MtmAdaptArgs {
    MtmArgs m;              // as mtmftest.hip's (coef unused); partial: [nstreams][wg_per_stream][2][nfft] sum S_s, sum nu_s
    const float *lam;       // [3][ntapers] lambda_k, 1 - lambda_k, 1 / g_k (oth_mtm_set_ratios)
    float *ws;              // [nstreams][wg_per_stream][mtm_adapt_ws_floats(nfft, ntapers)]: a segment's eigenspectra (from 1024 points on)
    int iters;              // updates of S, 1 ... 64
};
struct AdaptFinalizeArgs {
    const float *partial;   // [nstreams][W][2][nfft], natural bin order
    float *psd_out;         // [nstreams][nout]
    float *dof_out;         // or nullptr
    double psd_scale;       // scale / nseg
    double inv_nseg;
    int W, nfft;
    OutStage out;
};
size_t mtm_adapt_lds_bytes(int nfft, int ntapers);      // dynamic LDS of the launch: up to 512 points it holds the eigenspectra
size_t mtm_adapt_ws_floats(int nfft, int ntapers);      // 0: the build keeps the eigenspectra in LDS
int mtm_adapt_blocks_per_cu(int nfft, int ntapers);
hipError_t launch_mtm_adapt(int nfft, const MtmAdaptArgs &a, hipStream_t s);
hipError_t launch_adapt_finalize(const AdaptFinalizeArgs &a, int nstreams, hipStream_t s);

// ---- welchsk.hip: spectral kurtosis of a Welch plan - per bin sum_m P_m and sum_m P_m^2, P_m = g |FFT((x_m - mean) w)|^2 ---
struct WelchSkArgs {
    const float2 *x;        // device IQ, stream 0
    const float *win;       // the plan's window, nfft floats (zero-extended behind nperseg)
    const float2 *tw;       // W_nfft^k, nfft entries
    float *partial;         // [nstreams][wg_per_stream][2][nfft] S1, S2 of each workgroup's run, natural bin order
    long long nseg;         // segments per stream
    size_t stream_stride;   // samples between streams
    int nperseg;
    int step;
    int detrend;            // != 0: each segment's own mean comes off (pilot + residual)
    int wg_per_stream;      // workgroups of a stream: each walks a contiguous run of the nseg segments
    int nstreams;
    float g;                // 1 / sum w^2
};
struct SkFinalizeArgs {
    const float *partial;   // [nstreams][W][2][nfft], natural bin order
    float *sk_out;          // [nstreams][nout]
    float *psd_out;         // or nullptr
    double m;               // the segment count M
    double mp1_over_mm1;    // (M + 1) / (M - 1)
    double psd_scale;       // scale / (g M), g as the kernel's float
    int W, nfft;
    OutStage out;
};
int welch_sk_blocks_per_cu(int nfft);
hipError_t launch_welch_sk(int nfft, const WelchSkArgs &a, hipStream_t s);
hipError_t launch_sk_finalize(const SkFinalizeArgs &a, int nstreams, hipStream_t s);

// ---- welchcyc.hip: cyclic spectrum and coherence of a Welch plan - sum_s |X|^2 and, per cycle frequency, sum_s |U|^2 and
// sum_s U conj(X), U the same segment under the complex taper w[n] e^{-j 2 pi alpha n} and the segment's phase ---------------
constexpr int kCycMax = 64;      // cycle frequencies of a plan at most
constexpr int kCycGroup = 4;     // cycle frequencies per workgroup of the widest build (the others take one and two)
struct WelchCycArgs {
    const float2 *x;        // device IQ, stream 0
    const float *win;       // the plan's window, nfft floats (zero-extended behind nperseg)
    const float2 *ctap;     // [ncyc][nfft] w[n] e^{-j 2 pi alpha_a n}, formed in double (zero-extended behind nperseg)
    const double *alpha;    // [ncyc] cycles per sample
    const float2 *tw;       // W_nfft^k, nfft entries
    float *partial;         // [nstreams][groups][wg_per_stream][1 + 3 GA][nfft]: |X|^2 (group 0 only), then per cycle
                            // frequency of the group |U|^2, Re and Im sum U conj(X); natural bin order
    float2 *ws;             // [nstreams][groups][wg_per_stream][welch_cyc_ws_points(nfft)]: X's spectrum (16384 points)
    long long nseg;         // segments per stream
    size_t stream_stride;   // samples between streams
    int nperseg;
    int step;
    int detrend;            // != 0: each segment's own mean comes off (pilot + residual)
    int wg_per_stream;      // workgroups of a stream and group: each walks a contiguous run of the nseg segments
    int nstreams;
    int ncyc;
};
struct CycFinalizeArgs {
    const float *partial;   // as WelchCycArgs.partial
    float *scf_out;         // [nstreams][ncyc][nout] re, im interleaved, or nullptr
    float *coh_out;         // [nstreams][ncyc][nout]
    float *psd_out;         // [nstreams][nout], or nullptr
    double scf_scale;       // scale / M
    int W, G, ga, ncyc, nfft;
    OutStage out;
};
size_t welch_cyc_ws_points(int nfft);      // 0: the build keeps both spectra in LDS
int welch_cyc_blocks_per_cu(int nfft, int ga);      // ga: 1, 2 or kCycGroup
hipError_t launch_welch_cyc(int nfft, int ga, int groups, const WelchCycArgs &a, hipStream_t s);
hipError_t launch_cyc_finalize(const CycFinalizeArgs &a, int nstreams, hipStream_t s);

// ---- welchlag.hip: cyclic autocorrelation of a Welch plan - per lag sum_s |FFT((z_s - m) w)|^2 of the lag product
// z_s[n] = x[s step + n + tau] conj(x[s step + n]), and sum_s of the products' segment means -------------------------------
constexpr int kLagMax = 64;      // lags of a plan at most
constexpr int kLagTauMax = 65535;
constexpr int kLagGroup = 2;     // lags per workgroup of the grouped build (the other takes one)
struct WelchLagArgs {
    const float2 *x;        // device IQ, stream 0
    const float *win;       // the plan's window, nfft floats (zero-extended behind nperseg)
    const float2 *tw;       // W_nfft^k, nfft entries
    const int *lags;        // [nlags] tau_l in samples
    float *partial;         // [nstreams][groups][wg_per_stream][GL][nfft]: per lag of the group sum |Z|^2; natural bin order
    double *means;          // [nstreams][groups][wg_per_stream][GL] re, im: per lag of the group the run's sum of mbar
    long long nseg;         // segments per stream, counted on nsamples - max tau: no lagged read leaves the stream
    size_t stream_stride;   // samples between streams
    int nperseg;
    int step;
    int detrend;            // != 0: each product segment's own mean comes off (pilot + residual)
    int wg_per_stream;      // workgroups of a stream and group: each walks a contiguous run of the nseg segments
    int nstreams;
    int nlags;
};
struct LagFinalizeArgs {
    const float *partial;   // as WelchLagArgs.partial
    const double *means;    // as WelchLagArgs.means
    float *caf_out;         // [nstreams][nlags][nout]
    float *r_out;           // [nstreams][nlags] re, im interleaved, or nullptr
    double scale;           // scale / M
    double inv_m;           // 1 / M
    int W, G, gl, nlags, nfft;
    OutStage out;
};
int welch_lag_blocks_per_cu(int nfft, int gl);      // gl: 1 or kLagGroup
hipError_t launch_welch_lag(int nfft, int gl, int groups, const WelchLagArgs &a, hipStream_t s);
hipError_t launch_lag_finalize(const LagFinalizeArgs &a, int nstreams, hipStream_t s);

// ---- welchpfb.hip: polyphase filter-bank (WOLA) PSD of a Welch plan - sum_s |FFT(y_s)|^2 of the folded frame
// y_s[n] = sum_p h[n + p nfft] (x[s step + n + p nfft] - m_s); the finalize launch is launch_lag_finalize on one row -----------
constexpr int kPfbTapsMin = 2, kPfbTapsMax = 16;      // taps per branch P
struct WelchPfbArgs {
    const float2 *x;        // device IQ, stream 0
    const float *win;       // the prototype h, [ntaps][nfft] floats (the plan's window takes no part)
    const float *hfold;     // [nfft] sum_p h[n + p nfft], formed in double
    const float2 *tw;       // W_nfft^k, nfft entries
    float *partial;         // [nstreams][wg_per_stream][nfft] sum |X|^2 of each workgroup's run, natural bin order
    long long nseg;         // frames per stream, counted on nsamples - (ntaps - 1) nfft: no read of a frame leaves the stream
    size_t stream_stride;   // samples between streams
    int nperseg;            // = nfft
    int step;
    int detrend;            // != 0: each frame's own mean over its ntaps nfft samples comes off (pilot + residual)
    int wg_per_stream;      // workgroups of a stream: each walks a contiguous run of the nseg frames
    int nstreams;
    int ntaps;              // P
};
int welch_pfb_blocks_per_cu(int nfft);
hipError_t launch_welch_pfb(int nfft, const WelchPfbArgs &a, hipStream_t s);

// ---- chanpfb.hip: polyphase channelizer (oth_channelizer) - the fold of welchpfb.hip without detrend, the circular shift
// by (m decim) mod nchan, the transform, and the frames' bins out channel-major: out[k][m] = FFT(v_m)[k] -------------------------
constexpr int kChanTapsMin = 1, kChanTapsMax = 16;      // taps per branch P
constexpr int kChanMin = 64, kChanMax = 4096;           // channels M, a power of two
constexpr int kChanTile = 8;                            // F: frames of a tile, 8 F bytes of a channel row leave at once
struct ChanPfbArgs {
    const float2 *tail;     // the `pending` samples in front of x that earlier pushes left (frame m starts at sample m decim of tail ++ x)
    const float2 *x;        // the new samples
    const float *h;         // the prototype, [ntaps][nchan] floats
    const float2 *tw;       // W_nchan^k, nchan entries
    float2 *out;            // [nchan][out_stride]: frame m of this push in column m
    size_t out_stride;      // complex samples between channel rows, >= nframes
    long long nframes;      // frames of this push: (nframes - 1) decim + ntaps nchan <= pending + the new samples
    long long pending;      // samples in tail, < ntaps nchan
    int decim;              // hop D: nchan, nchan / 2 or nchan / 4
    int ntaps;              // P
    int rot0;               // (frames before this push) mod (nchan / decim): frame m is shifted by ((rot0 + m) mod (nchan / decim)) decim
    int wg_count;           // workgroups: each walks a contiguous run of whole tiles of kChanTile frames
};
int chan_pfb_blocks_per_cu(int nchan);
hipError_t launch_chan_pfb(int nchan, const ChanPfbArgs &a, hipStream_t s);

// ---- cpsync.hip: cyclic-prefix symbol timing and carrier offset (oth_cp_sync) - the lag products z[n] = x[n + Tu] conj(x[n])
// and the energies e[n] folded over the symbols by residue n mod Ts, the circular cp-window, the maximum of Lambda ---------------
constexpr int kCpsHypMax = 16;                          // hypotheses (Tu, cp) of a call at most
constexpr int kCpsTuMin = 8, kCpsTuMax = 16384;         // Tu; 1 <= cp <= Tu, so Ts = Tu + cp <= 32768
constexpr int kCpsSymBlock = 64;                        // symbols a float32 sum runs over before it is added in double
constexpr int kCpsBlock = 64;                           // residues of a block of the window's block sums
constexpr int kCpsGroupRows = 32, kCpsGroupMax = 32;    // the totals launch: about kCpsGroupRows runs to a group, kCpsGroupMax groups at most
struct CpsArgs {
    const float2 *x;        // device IQ, stream 0
    double *rows;           // per hypothesis h from part_off[h]: [nstreams][w[h]][3][Ts_h] F re, F im, G of each run of symbols;
                            // from grp_off[h]: [nstreams][ng[h]][3][Ts_h] the rows of each group of runs added up;
                            // from tot_off[h]: [nstreams] x ([3][Ts_h] totals, [3][nb_h] their block sums)
    float2 *gamma;          // [nstreams][nhyp][row_stride], or nullptr
    float *phi;             // [nstreams][nhyp][row_stride], or nullptr
    float *est;             // [nstreams][nhyp][4] theta, eps, rho_hat, Lambda[theta]
    size_t stream_stride;   // samples between streams
    size_t row_stride;      // entries between the rows of gamma and phi, >= every Ts_h
    double rho;
    int nstreams, nhyp;
    int tiles_max;          // residue tiles of the fold launch: the largest ceil(Ts_h / (4 threads))
    int w_max;              // the largest w[h]
    int nb_max;             // the largest nb_h = ceil(Ts_h / kCpsBlock)
    int ng_max;             // the largest ng[h]
    int tu[kCpsHypMax], cp[kCpsHypMax];
    int w[kCpsHypMax];      // runs of symbols per stream: each workgroup walks a contiguous run of the nsym[h] symbols
    int ng[kCpsHypMax];     // groups of contiguous runs the totals launch adds up on their own, 1 ... kCpsGroupMax
    long long nsym[kCpsHypMax];      // S_h: (S_h - 1) Ts_h + Ts_h - 1 + Tu_h < nsamples, the bound of every load
    size_t part_off[kCpsHypMax], grp_off[kCpsHypMax], tot_off[kCpsHypMax];      // in doubles from `rows`
};
int cps_fold_threads(int ts_max);                 // 64, 128 or 256 by the launch's largest Ts
int cps_fold_blocks_per_cu(int threads);
hipError_t launch_cps_fold(int threads, const CpsArgs &a, hipStream_t s);
hipError_t launch_cps_finalize(const CpsArgs &a, hipStream_t s);      // two launches: the groups' rows, then the totals, the window and est

// ---- welchmat.hip: spectral matrix of C coherent channels on a Welch plan - sum_s conj(X_s,a) X_s,b for a <= b, then
// S = scale T / M and the generalized coherence 1 - det G, G_ab = T_ab / sqrt(T_aa T_bb) ---------------------------------------
constexpr int kMatChanMax = 8;      // channels at most; the kernels are built for a capacity of 2, 4 and 8
struct WelchMatArgs {
    const float2 *x;        // device IQ, channel 0
    const float *win;       // the plan's window, nfft floats (zero-extended behind nperseg)
    const float2 *tw;       // W_nfft^k, nfft entries
    float *partial;         // [wg_count][nchan][nchan][nfft]: [a][b] is Re T_ab for a <= b and Im T_ba for a > b; natural bin order
    float2 *ws;             // [wg_count][nchan][welch_mat_ws_points]: the channels' spectra where they do not stay in registers
    long long nseg;         // segments per channel
    size_t chan_stride;     // samples between channels
    int nperseg;
    int step;
    int detrend;            // != 0: each segment's own mean comes off per channel (pilot + residual)
    int wg_count;           // workgroups: each walks a contiguous run of the nseg segments
    int nchan;              // 2 ... the build's capacity
};
struct MatFinalizeArgs {
    const float *partial;   // as WelchMatArgs.partial
    double *totals;         // [nchan][nchan][nfft]: the workgroups' rows added up (live bins), mat_det_kernel's input
    float *s_out;           // [nchan (nchan + 1) / 2][nout] re, im interleaved, the upper triangle row by row; or nullptr
    float *gcoh_out;        // [nout], or nullptr
    double s_scale;         // scale / M
    int W, nchan, nfft;
    OutStage out;
};
int welch_mat_capacity(int nchan);                   // the build that takes nchan channels: 2, 4 or kMatChanMax
size_t welch_mat_ws_points(int nfft, int cc);        // 0: the build keeps the spectra in registers
int welch_mat_blocks_per_cu(int nfft, int cc);
hipError_t launch_welch_mat(int nfft, int cc, const WelchMatArgs &a, hipStream_t s);
hipError_t launch_mat_totals(const MatFinalizeArgs &a, hipStream_t s);        // the first of the two: the workgroups' rows into a.totals
hipError_t launch_mat_finalize(const MatFinalizeArgs &a, hipStream_t s);      // two launches: the totals, then S and gcoh

// ---- mateig.hip: eigenvalues and the principal eigenvector of the spectral matrix S or of the coherence matrix G per bin,
// from the totals row of launch_mat_totals, by a cyclic Hermitian Jacobi in double ------------------------------------------------
struct MatEigArgs {
    const double *totals;   // [nchan][nchan][nfft] as MatFinalizeArgs.totals
    float *eig_out;         // [nchan][nout], row k the k-th largest eigenvalue; or nullptr
    float *vec_out;         // [nchan][nout] re, im interleaved: the eigenvector of the largest eigenvalue; or nullptr
    double s_scale;         // scale / M (of S)
    int of;                 // 0: S, 1: G
    int nchan, nfft;
    OutStage out;           // fftshift and trim; the rows are always linear
};
hipError_t launch_mat_eig(int cc, const MatEigArgs &a, hipStream_t s);        // cc: welch_mat_capacity(a.nchan)
// the basis build: the ranked eigenvalues (clamped at 0) and the whole ranked V in double to basis
// [mat_eig_basis_entries(cc)][nfft] - entry i < cc the i-th largest eigenvalue, entry cc + 2 (i cc + c) and the one behind it
// re and im of component c of its vector; a.eig_out and a.vec_out are not read
constexpr int mat_basis_at(int cc, int i, int c) { return cc + 2 * (i * cc + c); }      // re of component c of vector i
size_t mat_eig_basis_entries(int cc);
hipError_t launch_mat_eig_basis(int cc, const MatEigArgs &a, double *basis, hipStream_t s);

// ---- matdoa.hip: Bartlett, Capon and MUSIC direction spectra per bin and direction from the basis of launch_mat_eig_basis
// and a steering table of delays ----------------------------------------------------------------------------------------------
constexpr int kDoaDirsMax = 1024;      // OTH_DOA_DIRS_MAX
struct MatDoaArgs {
    const double *basis;    // [mat_eig_basis_entries(cc)][nfft]
    const double *tau;      // [ndir][nchan] delays in samples
    const double *frac;     // [ndir][nchan] frac(fc tau), reduced on the host
    float *bartlett_out;    // [ndir][nout] each, always linear; or nullptr
    float *capon_out;
    float *music_out;
    double loading;         // delta = loading trace / nchan
    int nsrc;               // MUSIC: the signal subspace's dimension, 1 ... nchan - 1 (read with music_out only)
    int ndir, nchan, nfft;
    OutStage out;           // fftshift and trim
};
hipError_t launch_mat_doa(int cc, const MatDoaArgs &a, hipStream_t s);        // cc: welch_mat_capacity(a.nchan)

// ---- matgcc.hip: generalized cross-correlation (PHAT, SCOT, plain) and the delay of every channel pair a < b, from the totals
// row of launch_mat_totals over all nfft bins (its OutStage without shift and trim) -------------------------------------------
constexpr int kGccUpsampleMax = 8;     // OTH_GCC_UPSAMPLE_MAX
constexpr int kGccPointsMax = 16384;   // NI = upsample nfft at most: one LDS tile
struct MatGccArgs {
    const double *totals;   // [nchan][nchan][nfft] as MatFinalizeArgs.totals, every bin live
    const float2 *tw;       // W_NI^k, NI entries (get_twiddles(NI): the plan's own table only where NI == nfft)
    float *gcc_out;         // [nchan (nchan - 1) / 2][2 maxlag + 1] re, im interleaved, lags -maxlag ... maxlag; or nullptr
    float *peak_out;        // [nchan (nchan - 1) / 2][3] delay in samples, |R| and arg R at the peak; or nullptr
    int weighting;          // 0 plain, 1 PHAT, 2 SCOT
    int band_lo, band_hi;   // signed bins of the nfft-point transform, both inclusive, in [-nfft / 2, nfft / 2 - 1]
    int maxlag;             // 0 ... NI / 2 - 1, in units of 1 / upsample sample
    int nchan, nfft;
};
hipError_t launch_mat_gcc(int ni, const MatGccArgs &a, hipStream_t s);        // ni: upsample a.nfft, a power of two 64 ... 16384

}  // namespace oth
