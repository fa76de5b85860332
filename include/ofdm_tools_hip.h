/*
 * ofdm_tools_hip.h - C ABI of libofdmtools_hip.so, the MI355X (gfx950) back end
 * of the gr-ofdm_tools spectrum-sensing hot path.
 *
 * The reference (gercap/gr-ofdm_tools) has NO native boundary of its own
 * (swig/ofdm_tools_swig.i:1-11 wraps nothing, python/__init__.py:45 leaves the
 * swig import commented out): its PSD arithmetic is delegated to GNU Radio C++
 * blocks and to scipy.signal.welch / numpy.fft from Python.  Each entry point
 * below therefore names the reference call site (file:line, relative to the
 * upstream tree) whose arithmetic it replaces.  The reference-side binding is a
 * ctypes stub; INTEGRATION.md shows it.
 *
 * Conventions
 *   - C linkage, plain C types, no C++/torch types in any signature.
 *   - Every function returns OTH_OK (0) or a negative OTH_ERR_* code; nothing
 *     throws or aborts: each entry point is a try/catch barrier, a C++
 *     exception raised below it (std::bad_alloc, std::system_error, ...) comes
 *     back as OTH_ERR_NOMEM / OTH_ERR_INTERNAL.  oth_last_error() gives the
 *     text for the last failure on that context (for a NULL context: the
 *     calling thread's last context-less failure).
 *   - IQ data is interleaved float32 (re, im) = numpy.complex64 = gr_complex.
 *   - The caller owns every buffer it passes.  The library owns contexts, plans
 *     and their device scratch.  A context wraps one device + one HIP stream.
 *     Entry points that take a context, or a plan / chain made from it, hold
 *     that context's lock for the duration of the call, so the blocks of one
 *     flowgraph (one scheduler thread each) may share a context; calls are then
 *     serialised and their kernels run in call order on its stream.
 *     oth_last_error() reports the context's most recent failure, whichever
 *     thread caused it.  oth_ctx_destroy() must not race with other calls.
 *   - "_dev" entry points take device pointers, are asynchronous on the
 *     context's stream and never synchronise; the others take host pointers
 *     (or a device source when src_is_device != 0), and return with the host
 *     output written.
 *   - No CPU fallback exists: without a usable GPU every compute entry point
 *     returns OTH_ERR_HIP.
 */
#ifndef OFDM_TOOLS_HIP_H
#define OFDM_TOOLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTH_ABI_VERSION 6      /* 3 = 2 + oth_chain_ticket_rows, oth_scan_decide_dev_out; 4 = 3 + OTH_ERR_INTERNAL,
                                  OTH_DETREND_CONSTANT_EXACT, OTH_DETREND_CONSTANT_FAST; 5 = 4 + oth_welch_exec_async /
                                  _poll / _wait; 6 = 5 + transform lengths outside the powers of two 64 ... 16384
                                  (TRANSFORM LENGTHS below), oth_plan_set_hostwait (additions only) */

/* TRANSFORM LENGTHS (ABI 6).  The reference puts no limit on a transform length - fft.fft_vcc(self.fft_len, ...)
 * (psd_logger.py:48, spectrum_sensor_v2.py:90, local_worker.py:62-63), sg.welch(nperseg=nFFT, nfft=nFFT)
 * (ofdm_cr_tools.py:214,322,342), np.fft.fft(., nFFT) (ofdm_cr_tools.py:177,157-160), fast_spectrum_scan's own
 * nFFT = 2^ceil(log2(npts)) (ofdm_cr_tools.py:474-475), the web gateway's free --nfft
 * (sdr_webserver/local_hw_gateway.py:284-285) - and neither do oth_welch_plan, oth_chain_create, oth_xcorr, oth_fac:
 *   powers of two 64 ... 16384             the tuned kernels and the radix-4 coverage kernels (as before)
 *   2-3-5-7-smooth lengths up to 16384     one launch, mixed-radix Stockham in LDS               "anyfft:direct"
 *   powers of two 32768 ... 1048576        four-step L1 x L2 through a workspace in HBM / L2      "anyfft:twolevel"
 *                                          (32768, 65536: register radix-16 kernels,              "anyfft:twolevel:r16")
 *   32768 / 65536, one channel,            the segment inside one workgroup's registers (65536:   "anyfft:onewg"
 *   nperseg = nfft                         a pair of workgroups, even / odd bins)
 *   every other length n <= 524288         Bluestein through 2^ceil(log2(2 n - 1)) points         "anyfft:bluestein[2]"
 * (the quoted names are what oth__debug_last_recipe reports).  Still refused, OTH_ERR_UNSUPPORTED with the reason in
 * oth_last_error(): powers of two above 1048576 and other lengths above 524288; OTH_KERNEL_TUNED on any of the new
 * lengths.  Semantics, tolerances and every other argument are unchanged; a constant detrend at these lengths is taken
 * from each segment's own mean (added in double, removed as a float pair) in every detrend mode. */

#define OTH_OK               0
#define OTH_ERR_INVALID     -1   /* bad argument */
#define OTH_ERR_HIP         -2   /* HIP runtime failure / no device */
#define OTH_ERR_UNSUPPORTED -3   /* size or mode not built */
#define OTH_ERR_NOMEM       -4
#define OTH_ERR_STATE       -5   /* call order (e.g. finalize with no data) */
#define OTH_ERR_INTERNAL    -6   /* a C++ exception was caught at the ABI (text in oth_last_error) */

/* detrend (scipy.signal.welch detrend=...) */
#define OTH_DETREND_NONE     0
#define OTH_DETREND_CONSTANT 1   /* per-segment mean removal, SciPy default - computed on x - pilot: before anything else
                                   every kernel takes a pilot value per stream (the average of eight probe means
                                   spread over the launch: formed in the prologue of the role-split 4096-point kernels,
                                   by one small launch in front of the others) off each sample as it is loaded,
                                   so no float32 arithmetic ever handles the DC line - neither the transform (the fastest
                                   2048 / 4096 / 8192 / 16384-point builds at 50 % overlap remove the mean after it,
                                   FFT(x w) - m FFT(w)) nor the segment mean, which becomes a small residual.
                                   Mathematically the same result; measured against float64: every
                                   bin inside 1e-4 at 1 ... 9 segments and |m| = 35 sigma, every bin at 2e-7 with 2047
                                   segments and a DC line of 3000 sigma (70 dB above the signal), bins 0, +-1 at 1e-6
                                   where SciPy on complex64 input reads 1e-4 ... 5e-3.  That is for a CONSTANT
                                   offset.  The pilot is one value per stream and launch - per workgroup where a
                                   workgroup walks one contiguous run of segments (launches of fewer than 32 segments
                                   per resident workgroup, OTH_SCHED_CONTIGUOUS: the 4096-point role-split kernel spreads
                                   its probes over its own run, round 6) - so an offset that MOVES by D within the reach
                                   of one pilot leaves a line of about D / 2 (a step: of D, in the one or two segments
                                   that hold it) to the float32 transform; the exact time-domain form sees the same
                                   line as real signal.  Measured over eight noise seeds at 2047 segments of 4096 points:
                                   every bin inside 1e-4 for a 3000-sigma opening transient (worst 8.9e-5; SciPy on
                                   complex64: 1.08e-4) and 2e-7 for drifts of up to 1200 sigma on the default plan; the
                                   time-domain builds within 4 ulp of the spectrum's peak amplitude on every bin and
                                   1e-4 on every bin at or above the median (tests/test_hip_parity.py
                                   test_pilot_under_a_transient_and_a_drifting_offset, profiles/r06_moving_offset.txt).
                                   Launches of fewer than 8 segments per stream detrend before the window (their own
                                   mean per segment); with 1-3 segments and an offset moving by 100 sigma every bin
                                   stays within 4 ulp of the row's peak amplitude (what a single float32 transform of a
                                   strong ramp leaves: 1e-4 ... 3e-4 of the weakest bins; SciPy on complex64: up to
                                   7e-4).  Chunked streaming (oth_welch_accumulate) takes a fresh pilot per chunk. */
#define OTH_DETREND_CONSTANT_EXACT 2 /* = OTH_DETREND_CONSTANT (the name under which the offset-proof detrend was first
                                   asked for; accepted, same builds) */
#define OTH_DETREND_CONSTANT_FAST 3 /* the same operation on the raw samples, -1 ... +2 % of the launch (no pilot, no
                                   subtractions).  Launches of fewer than 8 segments per stream detrend before the
                                   window (as above); the fast builds detrend after the transform, which then carries the
                                   rounding of the DC line m sum(w): about 1e-7 sqrt(nfft / nseg) |m| / sigma of the
                                   detrended power in every bin (measured on MI355X at 2047 segments of 4096 points:
                                   1e-6 at |m| = 30 sigma, 4e-5 at 300 sigma, 1.5e-4 at 3000 sigma), and bins 0, +-1
                                   stand where any float32 mean of the raw samples leaves them, SciPy's included
                                   (2 * 2^-23 |m| |W[k]| / |X[k]|) - inside the 1e-4 parity gate up to a DC line
                                   ~50 dB above the signal's total power. */

/* scaling of the averaged |X|^2 */
#define OTH_SCALE_RAW        0   /* mean over segments of |X|^2 */
#define OTH_SCALE_DENSITY    1   /* / (fs * sum(w^2))   scipy scaling='density' */
#define OTH_SCALE_OVER_N2    2   /* / nfft^2            spectrum_sensor_v2.py:93 */
#define OTH_SCALE_SPECTRUM   3   /* / sum(w)^2          scipy scaling='spectrum' */

/* epilogue of the per-vector periodogram chain */
#define OTH_EPI_MAG          0   /* |X|                 blocks.complex_to_mag, psd_logger.py:53 */
#define OTH_EPI_MAG2         1   /* |X|^2               blocks.complex_to_mag_squared, local_worker.py:65 */
#define OTH_EPI_MAG2_OVER_N2 2   /* |X|^2 / nfft^2      spectrum_sensor_v2.py:92-93 */

/* kernel selection (diagnostics / parity tests) */
#define OTH_KERNEL_AUTO      0
#define OTH_KERNEL_GENERIC   1   /* radix-4 Stockham, powers of two 64 ... 16384 (other lengths: always the any-length kernels) */
#define OTH_KERNEL_TUNED     2   /* register/LDS radix-16 kernels (nfft 256 ... 16384) */

/* how the tuned kernels hand segments to workgroups */
#define OTH_SCHED_CONTIGUOUS  0   /* fixed contiguous runs: bit-reproducible sums */
#define OTH_SCHED_INTERLEAVED 1   /* fixed round-robin chunks: bit-reproducible sums */
#define OTH_SCHED_DYNAMIC     2   /* the plan's initial value = the library's choice: chunks drawn from an atomic
                                     ticket for long 2048 / 4096-point launches (load-balanced; the fp32 summation
                                     order - hence the last bits - may vary run to run), a static schedule where that
                                     measures faster (256 / 512 / 1024 points, whole-segment loads, short launches) */

typedef struct oth_ctx oth_ctx;
typedef struct oth_plan oth_plan;
typedef struct oth_chain oth_chain;
typedef struct oth_channelizer oth_channelizer;

/* ---- library / context ------------------------------------------------- */
int         oth_abi_version(void);
const char *oth_strerror(int code);
int         oth_device_count(int *count);

int         oth_ctx_create(int device_id, oth_ctx **out);
/* adopt an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
int         oth_ctx_create_on_stream(int device_id, void *hip_stream, oth_ctx **out);
int         oth_ctx_destroy(oth_ctx *ctx);
const char *oth_last_error(oth_ctx *ctx);
int         oth_ctx_sync(oth_ctx *ctx);
int         oth_ctx_device_name(oth_ctx *ctx, char *buf, size_t buflen);

/* HIP-event timing of the dominant (FFT) kernel on the context's stream.
 * enable != 0 brackets every such launch with events; get() synchronises the
 * stream and returns the sum / count since the last reset. */
int         oth_ctx_set_timing(oth_ctx *ctx, int enable);
int         oth_ctx_get_timing(oth_ctx *ctx, double *total_ms, uint64_t *launches, int reset);

/* ---- device memory helpers (so ctypes-only hosts need no torch) --------- */
int oth_dev_alloc(oth_ctx *ctx, size_t bytes, void **dptr);
int oth_dev_free(oth_ctx *ctx, void *dptr);
int oth_memcpy_h2d(oth_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int oth_memcpy_d2h(oth_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* Synthetic IQ written straight into HBM: unit-power complex
 * AWGN from a counter-based generator + ntones complex exponentials + DC. */
int oth_synth_iq(oth_ctx *ctx, void *iq_dev, size_t nsamples, uint64_t seed, int ntones,
                 const float *tone_amp, const float *tone_freq, float dc_re, float dc_im);

/* Streaming-read probe: a float4 sum over [dptr, dptr+bytes); reports the
 * kernel time so the caller can state the achievable HBM-read peak.  repeats < 0: |repeats| passes of the
 * 8-bytes-per-lane variant (non-temporal float2 loads, the access the FFT kernels use for samples). */
int oth_stream_read_probe(oth_ctx *ctx, const void *dptr, size_t bytes, int repeats, double *ms_per_pass);

/* mean(|x - mean(x)|^2) of a device IQ buffer (Parseval check at full size) */
int oth_iq_power(oth_ctx *ctx, const void *iq_dev, size_t nsamples, double *mean_re, double *mean_im,
                 double *var);

/* ---- Welch PSD ----------------------------------------------------------
 * Replaces scipy.signal.welch as the reference calls it:
 *   ofdm_cr_tools.py:214  (window='flattop', nperseg=nfft)        src_power_welch
 *   ofdm_cr_tools.py:322  (default hann, 50 % overlap)            welch_plot_dB
 *   ofdm_cr_tools.py:342  (same)                                  welch_power_estimate
 *   spectrum_sweeper.py:263 (flattop, nperseg=nfft/4 zero-padded) _src_power
 * followed by the fftshift / excess-bin trim / 10*log10 of
 * spectrum_sweeper.py:265-276.  Two-sided, mean over segments (the default; oth_plan_set_average below selects
 * scipy.signal.welch's average='median').
 *
 * window: nperseg host floats (NULL = rectangular).  trim_bins bins are dropped
 * from each end AFTER the optional fftshift (np.fft.fftshift: bin k to (k + nfft / 2) mod nfft, odd nfft included);
 * output length = nfft - 2*trim_bins.  nfft: any length, see TRANSFORM LENGTHS above.
 */
int oth_welch_plan(oth_ctx *ctx, int nfft, int nperseg, int noverlap, const float *window,
                   int detrend, int scaling, double fs, int fftshift, int trim_bins, oth_plan **out);
int oth_plan_destroy(oth_plan *plan);
int oth_plan_set_output_db(oth_plan *plan, int enable);      /* 10*log10 in the finalize kernel */
int oth_plan_set_kernel(oth_plan *plan, int which);           /* OTH_KERNEL_* */
int oth_plan_set_schedule(oth_plan *plan, int which);         /* OTH_SCHED_* */
int oth_plan_out_len(oth_plan *plan, int *n);
/* How the blocking / waiting host-output calls of this plan (oth_welch_exec, oth_welch_wait) wait for the GPU (ABI 6; a
 * per-plan setting - round 5 read OTH_HOSTWAIT once per process).  POLL (default): the thread polls the completion word
 * the last launch writes into pinned memory - pause instructions for at most 2 ms, yielding the CPU between looks up to
 * 20 ms, then hipStreamSynchronize; the lowest latency (no interrupt wake-up), at the price of a busy core while it
 * waits.  SYNC: hipStreamSynchronize at once - the mode for a flowgraph with many blocking sensors.  The OTH_HOSTWAIT
 * environment variable ("sync") gives the initial value and is read once, in oth_welch_plan(). */
#define OTH_HOSTWAIT_POLL 0
#define OTH_HOSTWAIT_SYNC 1
int oth_plan_set_hostwait(oth_plan *plan, int mode);
/* Launch tuning for A/B tools and the parity suite: which build of the 4096-point kernel ("dpp", "pipe", "ws"; "wsgen": "ws"
 * with the general-window producer also where the window is complementary, w[n] + w[n + nfft / 2] = 1, as periodic Hann) or
 * of the 256 ... 2048-point kernels ("seg3", "seg4": registers held to 3 / 4 waves per SIMD; NULL or "" = the
 * library's choice), or only the detrend form of the size's default kernel ("fd": after the transform even below 8
 * segments per stream of an OTH_DETREND_CONSTANT_FAST plan; "td": before it at any length), the one-role kernel at 8192 points /
 * 50 % overlap instead of the role-split default ("8k1role"), the pilot from its own launch ("plaunch"), a schedule override
 * (-1 = the plan's), segments per chunk and per tail chunk
 * (0 = default).  The OTH_W4096_VARIANT / _SCHED / _CHUNK / _TAIL environment variables give the initial values
 * and are read once, in oth_welch_plan(). */
int oth_plan_set_tuning(oth_plan *plan, const char *variant, int sched, int chunk, int tail_chunk);

/* MEDIAN AVERAGE and PER-SEGMENT ROWS.  Additions inside ABI 6 (OTH_ABI_VERSION stays 6): a caller probes for them by the
 * symbols oth_plan_set_average / oth_welch_segments_dev.
 * oth_plan_set_average(MEDIAN): oth_welch_exec, oth_welch_exec_async / _poll / _wait and oth_welch_exec_dev (one median
 * per stream) return scipy.signal.welch(..., average='median'): per bin the median over segments of |X|^2 (numpy's: the
 * mean of the two middle values for an even count; NaN where a segment value is NaN), divided by SciPy's
 * _median_bias(nseg) = 1 + sum_{i=1}^{(nseg-1)//2} (1/(2i+1) - 1/(2i)), then the plan's scaling, fftshift, trim and dB.
 * The selection is exact (a radix select over the float bit patterns with integer counts, bit-identical under every
 * schedule); nseg_out is unchanged.  The rows take a device workspace of nstreams x nseg x nfft x 4 bytes, grown on demand
 * (OTH_ERR_NOMEM with the size when it cannot be had).  Refused with OTH_ERR_UNSUPPORTED under MEDIAN (a median is not a
 * sum of partials): oth_welch_partial_dev / _scale_dev (and so the time-sharded multi-GPU form), oth_welch_accumulate /
 * _finalize, every oth_csd_* call.  oth_plan_set_average during an unfinished accumulation: OTH_ERR_STATE. */
#define OTH_AVERAGE_MEAN   0   /* default */
#define OTH_AVERAGE_MEDIAN 1
int oth_plan_set_average(oth_plan *plan, int mode);
/* One row per segment, [nseg][out_len] floats at rows_dev, each with the plan's scaling, fftshift, trim and dB:
 * scipy.signal.spectrogram(..., mode='psd', return_onesided=False) with the axes swapped (segmentation, window, zero padding
 * and the per-segment constant detrend as the plan's).  Device in, device out, asynchronous; either average mode.
 * OTH_ERR_INVALID when capacity_rows < nseg. */
int oth_welch_segments_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, float *rows_dev, uint64_t capacity_rows,
                           uint64_t *nseg_out);

/* MULTITAPER (Thomson) PSD.  Additions inside ABI 6 (OTH_ABI_VERSION stays 6): a caller probes for them by the symbols
 * oth_dpss / oth_mtm_plan / oth_mtm_csd_plan.  The estimator for SHORT captures - one work()-sized vector, one row per scanner channel -
 * where Welch can only lower the variance by cutting the capture into shorter segments: K orthogonal Slepian tapers on the
 * same samples give the variance of K averages at a known bandwidth of 2 NW bins.
 *
 * oth_dpss: the kmax Slepian sequences (DPSS) of length n and time-half-bandwidth nw with the largest concentration, as
 * scipy.signal.windows.dpss(n, nw, kmax, return_ratios=True): tapers[k][n] by falling eigenvalue, each of unit L2 norm,
 * SciPy's signs (even orders: positive sum; odd orders: the first entry whose square exceeds max(1e-7, 1 / n) is
 * positive); ratios[k] (may be NULL) the concentration sum_{m,n} v_k[m] A[m - n] v_k[n], A[0] = 2 W, A[d] =
 * sin(2 pi W d) / (pi d), W = nw / n.  Host only, double throughout, no context and no GPU: eigenpairs of the symmetric
 * tridiagonal Slepian matrix by bisection and inverse iteration, O(n) memory (n = 16384, kmax = 7: 0.14 s on one core).  Needs n >= 2,
 * 0 < nw < n / 2, 1 <= kmax <= n; anything else is OTH_ERR_INVALID (text in oth_last_error(NULL)). */
int oth_dpss(int n, double nw, int kmax, double *tapers, double *ratios);
/* oth_mtm_plan: an ordinary oth_plan - the exec forms, oth_plan_set_output_db, _set_hostwait, _out_len and _destroy apply
 * unchanged.  Per stream: segments as oth_welch_plan's; each segment's own mean comes off (every detrend mode other than
 * OTH_DETREND_NONE means this); X_k = FFT_nfft((x_s - m_s) v_k), zero-padded when nperseg < nfft; the segment's estimate
 * is sum_k c_k |X_k|^2 with the weights a_k normalised to sum 1 (weights == NULL: uniform) and
 *   OTH_SCALE_DENSITY  c_k = a_k / sum_n v_k[n]^2, the result over fs
 *   OTH_SCALE_RAW      c_k = a_k
 *   OTH_SCALE_OVER_N2  c_k = a_k, the result over nfft^2;
 * the output is the mean over segments, then the plan's fftshift, trim and dB.  One taper and NULL weights: the Welch plan
 * of that window.  tapers: [ntapers][nperseg] host floats (any real tapers; oth_dpss gives Slepian's).
 * nfft: a power of two from 64 to 16384 (others: OTH_ERR_UNSUPPORTED); 1 <= nperseg <= nfft, any value; 0 <= noverlap <
 * nperseg; 1 <= ntapers <= 64; weights finite, non-negative, with a positive sum.
 * One launch per call whatever ntapers (csrc/mtm.hip: the (segment, taper) pairs of a stream are spread over workgroups in
 * contiguous runs, a segment is loaded once for all of a run's tapers); sums in a fixed order, bit-identical run to run.
 * Works: oth_welch_exec, _exec_async / _poll / _wait, _exec_dev with nstreams (at most 65535), _partial_dev / _scale_dev,
 * _accumulate / _finalize / _reset.  Refused with OTH_ERR_UNSUPPORTED and the reason in oth_last_error(): OTH_SCALE_SPECTRUM
 * (an odd taper sums to zero), oth_plan_set_average(MEDIAN), oth_welch_segments_dev, every oth_csd_* call,
 * oth_plan_set_kernel(TUNED), a non-empty variant in oth_plan_set_tuning.  oth_plan_set_schedule is accepted and has no
 * effect. */
int oth_mtm_plan(oth_ctx *ctx, int nfft, int nperseg, int noverlap, int ntapers, const float *tapers, const float *weights,
                 int detrend, int scaling, double fs, int fftshift, int trim_bins, oth_plan **out);
/* oth_mtm_csd_plan (an addition inside ABI 6; probe by the symbol): a multitaper plan - arguments, checks, error texts and
 * every call listed above as oth_mtm_plan's, the one-channel exec forms on the same kernel - on which the two-channel calls
 * WORK: oth_csd_exec, _exec_dev, _partial_dev, _scale_dev (plans of oth_mtm_plan go on refusing them).  It produces the three
 * inputs of coherence_detector - coherence, MTM-L, MTM-R - from one capture pair, where a Welch coherence is biased high by
 * about 1 / nseg.  Per segment s (segmentation as oth_welch_plan's) each channel's own mean comes off,
 * X_k = FFT_nfft((x_s - m_x) v_k), Y_k = FFT_nfft((y_s - m_y) v_k), and with oth_mtm_plan's c_k
 *   Sxx = sum_s sum_k c_k |X_k|^2,  Syy = sum_s sum_k c_k |Y_k|^2,  Sxy = sum_s sum_k c_k conj(X_k) Y_k;
 * Pxx, Pyy, Pxy = S scale / nseg, Cxy = |Pxy|^2 / (Pxx Pyy), then the plan's fftshift and trim; layouts as oth_csd_exec's.
 * oth_csd_partial_dev leaves the raw float[4 nfft] sums (the c_k applied), oth_csd_scale_dev scales them; partials of ranks
 * add.  One launch per call (csrc/mtmcsd.hip), sums in a fixed order, bit-identical run to run.
 * Degenerate input: the two-channel contract below (the same output stage closes the launch).  K nseg = 1 - one taper on
 * one segment - is a single periodogram pair and gives Cxy = 1 in every bin: the estimate needs K nseg >= 2.
 * Refused with OTH_ERR_UNSUPPORTED as on oth_mtm_plan's plans: OTH_SCALE_SPECTRUM, OTH_AVERAGE_MEDIAN,
 * oth_welch_segments_dev, OTH_KERNEL_TUNED, a non-empty tuning variant, sizes other than powers of two 64 ... 16384; and, as
 * on Welch plans, dB output on any oth_csd_* call. */
int oth_mtm_csd_plan(oth_ctx *ctx, int nfft, int nperseg, int noverlap, int ntapers, const float *tapers,
                     const float *weights, int detrend, int scaling, double fs, int fftshift, int trim_bins, oth_plan **out);
/* oth_mtm_ftest_dev / oth_mtm_ftest (additions inside ABI 6; probe by the symbols): Thomson's harmonic F-test - per bin, "is
 * there a coherent line at this frequency, whatever the background level" - on any plan of oth_mtm_plan or oth_mtm_csd_plan.
 * With U_k = sum_n v_k[n] (formed in double when the plan is created), S = sum_k U_k^2, and per segment s and bin j
 * y_k = FFT_nfft((x_s - m_s) v_k)[j] (segmentation, the per-segment mean removal and zero padding as the plan's exec forms):
 *   mu_s  = sum_k U_k y_k / S                 the complex amplitude of a line at bin j
 *   num_s = S |mu_s|^2,   den_s = sum_k |y_k|^2 - num_s   ( = sum_k |y_k - mu_s U_k|^2 )
 *   F     = (K - 1) sum_s num_s / sum_s den_s            F(2 nseg, 2 nseg (K - 1)) distributed where there is no line
 *   line  = (1 / nseg) sum_s |mu_s|^2                    the power of the sinusoid, input units squared
 *   resid = scale sum_s den_s / ((K - 1) nseg)           the background with the line removed; scale = the plan's 1 / fs,
 *                                                        1 / nfft^2 or 1
 * The plan's weights take no part (the test is unweighted).  The three rows take the plan's fftshift and trim and are always
 * linear: oth_plan_set_output_db does not apply.  Layout [nstreams][out_len] each; line_out and resid_out may be NULL.
 * A bin with sum den <= 0 reads F = 0 when sum num = 0 and +INF otherwise, and resid = 0 there: finite input never gives NaN;
 * all-zero input, and constant input on a detrending plan, give three rows of zeros.
 * One averaging launch per call (csrc/mtmftest.hip: a workgroup takes whole segments, K transforms each), then a small
 * finalize launch; sums in a fixed order, bit-identical run to run.  _dev: device in, device out, asynchronous, nstreams
 * as oth_welch_exec_dev (at most 65535).  oth_mtm_ftest: one stream, host or device source, host outputs, blocking.
 * Refused with OTH_ERR_UNSUPPORTED and the reason in oth_last_error(): a plan without tapers (oth_welch_plan's), ntapers < 2,
 * tapers whose sums are all zero (S = 0).  Input shorter than nperseg: OTH_ERR_INVALID, as oth_welch_exec_dev. */
int oth_mtm_ftest_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                      float *f_out_dev, float *line_out_dev, float *resid_out_dev, uint64_t *nseg_out);
int oth_mtm_ftest(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device, float *f_out, float *line_out,
                  float *resid_out, uint64_t *nseg_out);

/* oth_welch_sk_dev / oth_welch_sk (additions inside ABI 6; probe by the symbols): the spectral kurtosis estimator of Nita &
 * Gary on a plan of oth_welch_plan - per bin, "is what sits here noise-like, steady or intermittent", whatever its level.
 * With M the plan's segment count for the input, g = 1 / sum_n w[n]^2 (formed in double when the plan is created) and per
 * segment m and bin j  P_m = g |FFT_nfft((x_m - mean_m) w)[j]|^2  (segmentation, window, zero padding and the per-segment
 * mean removal - only on a detrending plan - as the plan's exec forms):
 *   S1 = sum_m P_m,   S2 = sum_m P_m^2,   SK = (M + 1) / (M - 1) (M S2 / S1^2 - 1)
 * SK is 1 in expectation for Gaussian noise at any level, goes towards 0 for a steady line and lies well above 1 for a signal
 * present in under half of the segments.  The SK row takes the plan's fftshift and trim and is never in dB.  psd_out (may be
 * NULL): the row oth_welch_exec_dev gives for the same plan and input - S1 scale / (g M), then fftshift, trim and dB.
 * Layout [nstreams][out_len] each.  A bin with S1 = 0 reads SK = 0 (silence, a constant under detrend, the DC bin of a
 * noiseless detrended input): finite input never gives NaN; non-finite input may.
 * One averaging launch per call (csrc/welchsk.hip: a workgroup takes whole segments and carries both sums), then a small
 * finalize launch that adds the workgroups' rows in double in a fixed order: bit-identical run to run.  _dev: device in,
 * device out, asynchronous, nstreams as oth_welch_exec_dev (at most 65535).  oth_welch_sk: one stream, host or device
 * source, host outputs, blocking.
 * Refused, the reason in oth_last_error(), before anything is staged, and the plan goes on working: OTH_ERR_UNSUPPORTED on a
 * multitaper plan, on a plan set to OTH_AVERAGE_MEDIAN, and for a transform length that is not a power of two from 64 to
 * 16384; OTH_ERR_INVALID for fewer than two segments (M - 1 divides), a NULL input or SK pointer, nstreams < 1,
 * stream_stride < nsamples, input shorter than nperseg. */
int oth_welch_sk_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                     float *sk_out_dev, float *psd_out_dev, uint64_t *nseg_out);
int oth_welch_sk(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device, float *sk_out, float *psd_out,
                 uint64_t *nseg_out);

/* oth_mtm_jackknife_dev / oth_mtm_jackknife, oth_mtm_csd_jackknife_dev / oth_mtm_csd_jackknife (additions inside ABI 6; probe
 * by the symbols): Thomson & Chave's jackknife over the M = K nseg (segment, taper) items of a multitaper estimate - per bin,
 * "how far can this PSD / this coherence be trusted", with no assumption on the distribution.  Segmentation, per-segment mean
 * removal, zero padding and tapers as the plan's exec forms; c_k the plan's coefficient (a_k / sum_n v_k[n]^2 under
 * OTH_SCALE_DENSITY, a_k otherwise); CL = 1 - 2^-24.  Per item i = (s, k) and bin:
 *   X_i = FFT_nfft((x_s - m_s) v_k), Y_i likewise;   p_i = c_k |X_i|^2,  q_i = c_k |Y_i|^2,  r_i = c_k conj(X_i) Y_i
 *   Sxx = sum_i p_i,  Syy = sum_i q_i,  Sxy = sum_i r_i      (what oth_welch_partial_dev / oth_csd_partial_dev leave)
 * ln PSD (one channel, and each channel of a pair):
 *   t_i = min(p_i / Sxx, CL),  l_i = log1p(-t_i)             the delete-one ln((Sxx - p_i) / (M - 1)) up to a constant
 *   var = (M - 1) / M (sum l_i^2 - (sum l_i)^2 / M), clamped at 0;   lnsd = sqrt(var)
 * lnsd is in natural-log units, never dB and never scaled; a bin with Sxx <= 0 reads 0.
 * Coherence (two channels), with C = |Sxy|^2 / (Sxx Syy) and z(c) = atanh(min(sqrt(c), CL)):
 *   C_i = |Sxy - r_i|^2 / (Sxx (1 - tx_i) Syy (1 - ty_i)),   d_i = z(C_i) - z(C)
 *   zvar = (M - 1) / M (sum d_i^2 - (sum d_i)^2 / M), clamped at 0;   zsd = sqrt(zvar)
 * A bin with Sxx <= 0 or Syy <= 0 reads zsd = 0.  Finite input never gives NaN in lnsd or zsd (cxy_out is the plan's own Cxy:
 * 0 / 0 = NaN for a silent channel, as oth_csd_exec_dev documents).  A confidence interval is
 * psd exp(-+ q lnsd) resp. tanh(max(0, z -+ q zsd))^2 with q the Student-t quantile at M - 1 degrees of freedom.  The phase
 * jackknife is not provided.
 * Every row takes the plan's fftshift and trim, layout [nstreams][out_len].  psd_out (may be NULL): the row
 * oth_welch_exec_dev gives for the same plan and input, bit for bit (dB applies to it alone).  cxy_out (may be NULL): the
 * Cxy row of oth_csd_exec_dev, bit for bit; lnsdx_out / lnsdy_out may be NULL, zsd_out not.
 * Two passes per call: the plan's own averaging launch and reduction leave the totals in a buffer of the plan, then
 * csrc/mtmjack.hip walks the items again (mtm.hip's work split) with the running sums and a small finalize launch adds the
 * workgroups' rows in double in a fixed order: bit-identical run to run.  _dev: device in, device out, asynchronous; the
 * one-channel form takes nstreams as oth_welch_exec_dev (at most 65535), the two-channel form one stream.  The forms without
 * _dev: one stream, host or device source, host outputs, blocking.
 * The one-channel calls work on plans of oth_mtm_plan and oth_mtm_csd_plan, the two-channel calls on oth_mtm_csd_plan's only.
 * Refused, the reason in oth_last_error(), before anything is staged, and the plan goes on working: OTH_ERR_UNSUPPORTED on a
 * plan without tapers, on a plan whose weights are not all equal (the items must be exchangeable), for more than 65535
 * streams, and for the two-channel calls on a plan of oth_mtm_plan; OTH_ERR_INVALID for M < 2 (one channel) or M < 3 (two:
 * with one item left every delete-one coherence is 1), a NULL input or required output pointer, nstreams < 1,
 * stream_stride < nsamples, input shorter than nperseg. */
int oth_mtm_jackknife_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                          float *lnsd_out_dev, float *psd_out_dev, uint64_t *nseg_out);
int oth_mtm_jackknife(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device, float *lnsd_out, float *psd_out,
                      uint64_t *nseg_out);
int oth_mtm_csd_jackknife_dev(oth_plan *plan, const void *x_dev, const void *y_dev, size_t nsamples, float *cxy_out_dev,
                              float *zsd_out_dev, float *lnsdx_out_dev, float *lnsdy_out_dev, uint64_t *nseg_out);
int oth_mtm_csd_jackknife(oth_plan *plan, const void *x, const void *y, size_t nsamples, int src_is_device, float *cxy_out,
                          float *zsd_out, float *lnsdx_out, float *lnsdy_out, uint64_t *nseg_out);

/* oth_mtm_set_ratios, oth_mtm_adaptive_dev / oth_mtm_adaptive (additions inside ABI 6; probe by the symbols): Thomson's
 * adaptive-weight multitaper PSD and its per-bin equivalent degrees of freedom, on any plan of oth_mtm_plan or
 * oth_mtm_csd_plan with K = ntapers >= 2.  The fixed weights of a plan let the high-order tapers' leakage (1 - lambda_k of
 * their energy lies outside the band) lift an empty band next to a strong one; the adaptive weights take a taper out of a
 * bin as far as its leakage would dominate there.  With the tapers v_k, g_k = sum_n v_k[n]^2 (formed in double when the plan
 * is created) and the concentration ratios lambda_k of oth_mtm_set_ratios, per stream, segment s and bin j - segmentation,
 * per-segment mean removal and zero padding as the plan's exec forms:
 *   P_k     = |FFT_nfft((x_s - m_s) v_k)[j]|^2 / g_k                 the eigenspectra
 *   sigma^2 = (1 / nperseg) sum_n |x_s[n] - m_s|^2                   so that white noise has E P_k = sigma^2
 *   S^0     = (P_0 + P_1) / 2
 *   `iters` times:   b_k = S / (lambda_k S + (1 - lambda_k) sigma^2),   w_k = lambda_k b_k^2,
 *                    S <- sum_k w_k P_k / sum_k w_k
 *   then b_k and w_k once more from the final S, and   nu_s = 2 (sum_k w_k)^2 / sum_k w_k^2
 * A bin where sum_k w_k is not > 0, or a segment with sigma^2 = 0, reads S_s = 0 and nu_s = 0: finite input never gives NaN
 * or Inf; all-zero input, and constant input on a detrending plan, give two rows of zeros.  The outputs, [nstreams][out_len]
 * float32 each:
 *   psd = scale (1 / nseg) sum_s S_s      scale = 1 / fs (OTH_SCALE_DENSITY), 1 (OTH_SCALE_RAW), 1 / nfft^2
 *                                         (OTH_SCALE_OVER_N2) - for unit-norm tapers the plan's own scaling; the row takes
 *                                         the plan's fftshift, trim and dB
 *   dof = (1 / nseg) sum_s nu_s           between 2 and 2 K: what a chi-square threshold or interval on a bin needs; takes
 *                                         fftshift and trim, always linear; dof_out may be NULL
 * The plan's weights take no part.  The iteration count is fixed (1 <= iters <= 64, 4 is a good default) and there is no
 * convergence test: single bins approach the fixed point very slowly while the floor of an empty band settles after three
 * or four updates, and a fixed count makes the estimate a definite function of its input.
 * oth_mtm_set_ratios: K host doubles, each in (0, 1] (oth_dpss's `ratios` for Slepian tapers); lambda_k and
 * max(1 - lambda_k, 0) are formed in double and then rounded to float - 1 - lambda_0 is 3e-10 at NW 4 and cannot be formed
 * from a float lambda.  It replaces any earlier set, waits for the plan's queued work, and has no effect on any other call.
 * One averaging launch per call (csrc/mtmadapt.hip: a workgroup takes whole segments, K transforms each, and keeps the
 * segment's eigenspectra in LDS or in a workspace row of its own), then a small finalize launch that adds the workgroups'
 * rows in double in a fixed order: bit-identical run to run.  _dev: device in, device out, asynchronous, nstreams as
 * oth_welch_exec_dev (at most 65535).  oth_mtm_adaptive: one stream, host or device source, host outputs, blocking.
 * Refused with OTH_ERR_UNSUPPORTED and the reason in oth_last_error(), before anything is staged, and the plan goes on
 * working: a plan without tapers (oth_welch_plan's), ntapers < 2, a plan on which no ratios were set.  OTH_ERR_INVALID: a
 * ratio outside (0, 1], iters outside 1 ... 64, a NULL input or psd pointer, nstreams < 1, stream_stride < nsamples, input
 * shorter than nperseg. */
int oth_mtm_set_ratios(oth_plan *plan, const double *ratios);
int oth_mtm_adaptive_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride, int iters,
                         float *psd_out_dev, float *dof_out_dev, uint64_t *nseg_out);
int oth_mtm_adaptive(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device, int iters, float *psd_out,
                     float *dof_out, uint64_t *nseg_out);

/* oth_welch_set_cycles, oth_welch_cyclic_dev / oth_welch_cyclic (additions inside ABI 6; probe by the symbols): the cyclic
 * spectrum (spectral correlation density) and the cyclic coherence of a plan of oth_welch_plan at a set of A cycle
 * frequencies alpha_a in cycles per sample - cyclostationary feature detection.  A cyclic-prefix OFDM signal is correlated
 * with itself at lag +-Tu with period Ts = Tu + Tcp, so E[X(f + alpha) X*(f)] is non-zero at alpha = k / Ts; stationary noise
 * has none at any alpha != 0, whatever its level or colour - a detector that needs no noise floor.  The estimate is the
 * time-smoothed cyclic cross periodogram.  With the plan's window w, step = nperseg - noverlap and its M segments
 * (segmentation, per-segment mean removal m_s and zero padding as the plan's exec forms), per stream, segment s and bin j:
 *   X_s[j]   = FFT_nfft((x_s[n] - m_s) w[n])[j]
 *   U_s,a[j] = FFT_nfft((x_s[n] - m_s) w[n] e^{-j 2 pi alpha_a (n + s step)})[j]      X at frequency j / nfft + alpha_a, with
 *                                                                                    the capture's first sample as time 0
 *   Sxx = sum_s |X_s|^2,   Suu_a = sum_s |U_s,a|^2,   Sux_a = sum_s U_s,a conj(X_s)
 *   scf_a = scale Sux_a / M                  the plan's scaling, as Pxy of oth_csd_exec: estimates E[X(f_j + alpha) X*(f_j)],
 *                                            the spectral correlation density at centre frequency f_j + alpha / 2
 *   coh_a = |Sux_a|^2 / (Suu_a Sxx)          the cyclic coherence, in [0, 1], independent of level and scaling; 1 / M on
 *                                            average for stationary noise over independent segments
 *   psd   = scale Sxx / M                    the plan's own PSD row (dB applies to it alone)
 * Every row takes the plan's fftshift and trim.  A bin with Suu_a Sxx <= 0 reads scf = 0, coh = 0: finite input never gives
 * NaN or Inf; all-zero input, and constant input on a detrending plan, give rows of zeros.  alpha = 0 gives coh = 1, a zero
 * imaginary part and scf = psd in linear units.  One segment is allowed: the coherence is then 1 everywhere, as
 * oth_csd_exec's.
 * Phase: e^{-j 2 pi alpha_a n}, n < nperseg, is formed on the host in double and rounded once, multiplied into the window as
 * a complex taper; the segment's factor e^{-j 2 pi alpha_a s step} comes from the fractional part of alpha_a s step taken
 * in double - at 2^24 samples a cycle frequency one resolution cell 1 / (M step) off the true one already reads the null
 * level, and a float32 product of the sample index is useless there.  That is why the cycle frequencies are doubles.
 * oth_welch_set_cycles: 1 <= ncycles <= 64 host doubles, each finite with |alpha| <= 0.5.  It replaces any earlier set, waits
 * for the plan's queued work, and has no effect on any other call of the plan.
 * Outputs: scf [nstreams][A][out_len] interleaved re, im; coh [nstreams][A][out_len]; psd [nstreams][out_len]; scf_out and
 * psd_out may be NULL, coh_out not.  One averaging launch per call (csrc/welchcyc.hip: a workgroup takes whole segments for
 * a group of up to 4 consecutive cycle frequencies, transforms X once per segment and every U of the group against it),
 * then a small finalize launch that adds the workgroups' rows in double in a fixed order: bit-identical run to run.
 * _dev: device in, device out, asynchronous, nstreams as oth_welch_exec_dev (at most 65535).  oth_welch_cyclic: one stream,
 * host or device source, host outputs, blocking.
 * Refused, the reason in oth_last_error(), before anything is staged, and the plan goes on working: OTH_ERR_UNSUPPORTED on a
 * multitaper plan, a plan set to OTH_AVERAGE_MEDIAN, a transform length that is not a power of two from 64 to 16384, a plan
 * on which no cycles were set, more than 65535 streams; OTH_ERR_INVALID for ncycles outside 1 ... 64, a non-finite alpha or
 * |alpha| > 0.5, a NULL alphas, input or coh pointer, nstreams < 1, stream_stride < nsamples, input shorter than nperseg.
 * Not provided: the conjugate cyclic spectrum E[X(f + alpha) X(-f)], a search over alpha (the caller supplies the cycle
 * frequencies; oth_welch_caf below finds those of a CP-OFDM signal), multitaper plans, any-length transforms. */
int oth_welch_set_cycles(oth_plan *plan, int ncycles, const double *alphas);
int oth_welch_cyclic_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                         float *scf_out_dev, float *coh_out_dev, float *psd_out_dev, uint64_t *nseg_out);
int oth_welch_cyclic(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device, float *scf_out, float *coh_out,
                     float *psd_out, uint64_t *nseg_out);

/* oth_welch_set_lags, oth_welch_caf_dev / oth_welch_caf (additions inside ABI 6; probe by the symbols): the cyclic
 * autocorrelation function of a plan of oth_welch_plan at a set of L lags tau_l >= 0 in samples, as the plan's Welch PSD of
 * the lag product - the blind counterpart of oth_welch_cyclic, which needs the cycle frequencies beforehand.  For a
 * cyclic-prefix OFDM signal with useful length Tu and symbol period Ts = Tu + Tcp the lag product at tau = Tu has a non-zero
 * mean and periodic components at alpha = k / Ts; at any other lag, and for stationary noise at every lag but 0, it has
 * neither.  A handful of candidate lags therefore finds Tu and Tcp with no prior knowledge - the input of
 * oth_welch_set_cycles.  With the plan's window w, nperseg, step = nperseg - noverlap, nfft, detrend mode and scaling, and
 * T = max_l tau_l: M is the plan's segment count for an input of nsamples - T samples, so that every lagged sample a segment
 * reads lies inside the stream's own nsamples.  Per stream, segment s and lag l, for n < nperseg:
 *   z_s,l[n] = x[s step + n + tau_l] conj(x[s step + n])     float32: re = fma(ar, br, ai bi), im = ai br - ar bi
 *   mbar_s,l = (1 / nperseg) sum_n z_s,l[n]                  always formed (it feeds r)
 *   Z_s,l[q] = FFT_nfft((z_s,l[n] - m) w[n])[q]              m = mbar_s,l on a detrending plan, 0 otherwise; zero-padded when
 *                                                            nperseg < nfft
 *   caf_l[q] = scale (1 / M) sum_s |Z_s,l[q]|^2              the plan's scaling, then its fftshift, trim and dB
 *   r_l      = (1 / M) sum_s mbar_s,l                        complex: the ordinary autocorrelation estimate R(tau_l)
 * Bin q of caf is the cycle frequency alpha = q / nfft cycles per sample; the upper half of a row holds negative alpha, as
 * for a PSD.  The segments are averaged incoherently: the resolution in alpha is one bin of the transform, and a cycle
 * frequency off the grid is not nulled.  The mean comes off as in the multitaper kernels - a pilot (the mean of the first
 * min(64, nperseg) products), then the residual mean as a fixed-order block sum: lag 0 and a DC offset in x both give z a
 * mean far above its fluctuation.
 * Outputs: caf [nstreams][L][out_len] float32; r [nstreams][L] interleaved re, im, never scaled and never in dB; r_out may
 * be NULL, caf_out not.  tau = 0 is allowed: its r is the mean power with an imaginary part of exactly 0, so |r_l| / r_0 is
 * the correlation coefficient of lag l when lag 0 is in the list.  All-zero input gives rows of exact zeros and r = 0; a
 * constant input on a detrending plan gives exact-zero caf rows (-inf under dB).  A sample with a NaN or +-inf part: every
 * caf row of that stream whose lag products include the sample reads NaN in every bin, never inf; other streams of the
 * launch are untouched bit for bit.
 * One averaging launch per call (csrc/welchlag.hip: a workgroup takes whole segments of one stream for one lag, or for
 * two consecutive lags that share one load of the base segment), then a small finalize launch that adds the workgroups' rows, and
 * the mbar sums, in double in a fixed order: bit-identical run to run.
 * oth_welch_set_lags: 1 <= nlags <= 64 host ints, each 0 <= tau <= 65535.  It replaces any earlier set, waits for the plan's
 * queued work, and has no effect on any other call of the plan.
 * _dev: device in, device out, asynchronous, nstreams as oth_welch_exec_dev (at most 65535).  oth_welch_caf: one stream,
 * host or device source, host outputs, blocking.
 * Refused, the reason in oth_last_error(), before anything is staged, and the plan goes on working: OTH_ERR_UNSUPPORTED on a
 * multitaper plan, a plan set to OTH_AVERAGE_MEDIAN, a transform length that is not a power of two from 64 to 16384, a plan
 * on which no lags were set, more than 65535 streams; OTH_ERR_INVALID for nlags outside 1 ... 64, a lag outside 0 ... 65535,
 * a NULL lags, input or caf pointer, nstreams < 1, stream_stride < nsamples, nsamples < T + nperseg.
 * Not provided: the conjugate cyclic autocorrelation x[n + tau] x[n], negative lags (R(-tau; alpha) follows from
 * R(tau; alpha)), coherent averaging across segments, multitaper plans, any-length transforms. */
int oth_welch_set_lags(oth_plan *plan, int nlags, const int *lags);
int oth_welch_caf_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                      float *caf_out_dev, float *r_out_dev, uint64_t *nseg_out);
int oth_welch_caf(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device, float *caf_out, float *r_out,
                  uint64_t *nseg_out);

/* oth_welch_matrix_dev / oth_welch_matrix (additions inside ABI 6; probe by the symbols): the spectral matrix of C coherent
 * channels, 2 <= C <= 8 (the ports of one receiver), on a plan of oth_welch_plan, and the generalized coherence that follows
 * from it - a detector that needs no noise floor and no calibration of the channels' gains.  oth_csd_exec takes one pair;
 * C channels pair by pair cost C (C - 1) / 2 launches and transform every channel C - 1 times.  Here a channel of a segment
 * is transformed once.  With the plan's window w, nperseg, step = nperseg - noverlap, nfft, detrend mode and scaling; channel
 * a is nsamples long and begins a chan_stride samples behind channel 0; M is the plan's segment count for nsamples, common to
 * all channels.  Per segment s, channel a and bin j:
 *   X_s,a[j] = FFT_nfft((x_a,s[n] - m_s,a) w[n])[j]     m_s,a: the segment's mean on a detrending plan, else 0
 *   T_ab[j]  = sum_s conj(X_s,a[j]) X_s,b[j]             a <= b; T_aa is real.  float32: |X|^2 = fma(Xr, Xr, Xi Xi),
 *                                                        Re = fma(Ar, Br, Ai Bi), Im = Ar Bi - Ai Br (two rounded products)
 *   S_ab     = scale T_ab / M                            scipy.signal.csd(x_a, x_b) with the plan's parameters;
 *                                                        S_aa = scipy.signal.welch(x_a)
 *   G_ab     = T_ab / sqrt(T_aa T_bb)                    the coherence matrix, in double
 *   gcoh[j]  = 1 - det G[j]                              in [0, 1] (Hadamard's inequality); the Hadamard ratio
 *                                                        det S / prod_a S_aa taken from 1, the GLRT statistic for a common
 *                                                        signal in uncalibrated receivers.  For C = 2 it is
 *                                                        |S_01|^2 / (S_00 S_11), the coherence of oth_csd_exec.
 * gcoh does not change under a complex gain per channel.  On independent noise over M independent segments (no overlap) its
 * expectation is 1 - prod_{k=1}^{C-1} (M - k) / M, whatever the channels' levels.
 * Outputs: s_out [C (C + 1) / 2][out_len] interleaved re, im - the upper triangle row by row, (0,0), (0,1), ..., (0,C-1),
 * (1,1), ...; S_ba = conj(S_ab); the imaginary part of a diagonal row is exactly 0.  The matrix is always linear: on a plan
 * set to dB (oth_plan_set_output_db) it is the linear twin's bit for bit, as scf is in oth_welch_cyclic.  gcoh_out
 * [out_len].  Both take the plan's fftshift and trim.  Either pointer may be NULL, not both.
 * Degenerate input (the cyclic family's rules, not SciPy's 0 / 0): a bin in which a channel holds no power (T_aa <= 0:
 * silence, a constant under detrend) reads 0 in every S_ab that involves the channel and gcoh = 0; finite input never gives
 * NaN or inf.  A sample with a NaN or +-inf part in channel a makes every S_ab that involves a NaN in every bin, never inf,
 * and gcoh NaN in every bin; every other entry of the matrix stays bit for bit what it is without the bad sample.  M = 1 is
 * allowed, as in oth_csd_exec: the matrix has rank one and gcoh = 1.  With M < C the matrix is singular and gcoh reads 1 up
 * to rounding in every bin - nothing is refused, the caller sees M in nseg_out.  Two identical channels give bit-identical
 * rows S_aa, S_bb and Re S_ab, Im S_ab = 0 exactly and gcoh = 1 up to rounding; exchanging two channels exchanges their rows
 * and conjugates S_ab exactly.  gcoh is clamped to [0, 1], as coh is.
 * One averaging launch per call (csrc/welchmat.hip: a workgroup takes whole segments and transforms the C channels of each
 * one behind the other; built for a channel capacity of 2, 4 and 8), then two small finalize launches: the workgroups' rows
 * added in double in a fixed order, then per bin S, G and det G by LDL^H in double.  Bit-identical run to run.
 * _dev: device in, device out, asynchronous.  oth_welch_matrix: iq is [nchan][nsamples] contiguous, host or device source,
 * host outputs, blocking.
 * Refused, the reason in oth_last_error(), before anything is staged, and the plan goes on working: OTH_ERR_UNSUPPORTED on a
 * multitaper plan, a plan set to OTH_AVERAGE_MEDIAN, a transform length that is not a power of two from 64 to 16384;
 * OTH_ERR_INVALID for nchan outside 2 ... 8, a NULL input, both outputs NULL, chan_stride < nsamples, input shorter than
 * nperseg.
 * Not provided: partial sums for time-sharded multi-GPU runs, multitaper plans, any-length transforms, more than 8 channels.
 * (Eigenvalues: oth_welch_matrix_eig below.) */
int oth_welch_matrix_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nchan, size_t chan_stride,
                         float *s_out_dev, float *gcoh_out_dev, uint64_t *nseg_out);
int oth_welch_matrix(oth_plan *plan, const void *iq, size_t nsamples, int nchan, int src_is_device,
                     float *s_out, float *gcoh_out, uint64_t *nseg_out);      /* iq: [nchan][nsamples], blocking */

/* oth_welch_matrix_eig_dev / oth_welch_matrix_eig (additions inside ABI 6; probe by the symbols): per bin, the eigenvalues
 * and the principal eigenvector of the spectral matrix S of oth_welch_matrix (of = OTH_EIG_OF_S) or of its coherence matrix G
 * (of = OTH_EIG_OF_G: unit diagonal, unchanged by a complex gain per channel).  The blind multi-antenna detectors are
 * functions of these eigenvalues - the largest over the smallest (MME), the arithmetic over the geometric mean (sphericity),
 * the MDL / AIC source count -, and the eigenvector of the largest one is the array response of the strongest emitter in the
 * bin.  Same plan, segmentation, window, detrend, scaling, M, fftshift and trim as oth_welch_matrix, and the same sums T;
 * always linear: a plan set to dB gives its linear twin's rows bit for bit.
 * Outputs: eig_out [C][out_len] float32, row k the k-th largest eigenvalue of the bin (the rows descend); a value below 0
 * from rounding reads 0.  vec_out [C][out_len] interleaved re, im: row a is component a of the eigenvector of the largest
 * eigenvalue, of unit 2-norm, rotated so that component 0 is real and >= 0 with its imaginary part stored as exactly 0 (a
 * vector whose component 0 is exactly 0 is left as computed); among equal largest eigenvalues it belongs to the lowest
 * Jacobi column index.  Either pointer may be NULL, not both; the eigenvalue rows are the same bits with and without vec_out.
 * Degenerate input (the matrix family's rules): finite input never gives NaN or inf.  A channel whose T_aa is not finite (a
 * NaN or +-inf sample) makes every eig and vec entry NaN in every bin, never inf.  OTH_EIG_OF_S, a channel with T_aa <= 0 in
 * a bin (silence, a constant under detrend): its row and column of S are 0, as s_out reads, the decomposition is of that
 * matrix and one eigenvalue reads exactly 0; all channels silent: every eigenvalue is 0 and vec = e_0.  OTH_EIG_OF_G, any
 * silent channel: G is taken as the identity, which is what gcoh = 0 says - every eigenvalue reads 1 and vec = e_0.  M = 1
 * and M < C are not refused: the matrix is singular and the trailing eigenvalues read 0 up to rounding.
 * Three launches per call: the averaging launch and the totals launch of oth_welch_matrix, then one thread per bin
 * (csrc/mateig.hip): the matrix in double from the totals, a cyclic Hermitian Jacobi (row-cyclic, Rutishauser's rotation, a
 * rotation with |a_pq| exactly 0 skipped, sweeps until the off-diagonal norm squared is at most 2^-104 of the diagonal's, a
 * fixed cap on sweeps), the diagonal sorted, clamped at 0 and cast to float.  The result is a function of the double totals
 * only.  Bit-identical run to run.
 * _dev: device in, device out, asynchronous.  oth_welch_matrix_eig: iq is [nchan][nsamples] contiguous, host or device
 * source, host outputs, blocking.
 * Refused, the reason in oth_last_error(), before anything is allocated, staged or launched, and the plan goes on working, in
 * this order: OTH_ERR_UNSUPPORTED on a multitaper plan, a plan set to OTH_AVERAGE_MEDIAN, a transform length that is not a
 * power of two from 64 to 16384; OTH_ERR_INVALID for nchan outside 2 ... 8, of not OTH_EIG_OF_S or OTH_EIG_OF_G, a NULL input,
 * both outputs NULL, chan_stride < nsamples, input shorter than nperseg.
 * Not provided: all C eigenvectors, multitaper plans, any-length transforms, more than 8 channels, partial sums for
 * time-sharded runs.  (Bartlett, Capon and MUSIC spectra: oth_welch_matrix_doa below.) */
#define OTH_EIG_OF_S 0   /* the spectral matrix S = scale T / M        */
#define OTH_EIG_OF_G 1   /* the coherence matrix G_ab = T_ab / sqrt(T_aa T_bb): unit diagonal, gain-invariant */
int oth_welch_matrix_eig_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nchan, size_t chan_stride,
                             int of, float *eig_out_dev, float *vec_out_dev, uint64_t *nseg_out);
int oth_welch_matrix_eig(oth_plan *plan, const void *iq, size_t nsamples, int nchan, int src_is_device,
                         int of, float *eig_out, float *vec_out, uint64_t *nseg_out);   /* iq: [nchan][nsamples], blocking */

/* oth_welch_set_steering, oth_welch_matrix_doa_dev / oth_welch_matrix_doa (additions inside ABI 6; probe by the symbols):
 * where is the emitter?  Per bin and per direction of a steering table, the Bartlett (conventional beamformer), Capon (MVDR)
 * and MUSIC spectra of the matrix oth_welch_matrix_eig decomposes - S (of = OTH_EIG_OF_S) or G (of = OTH_EIG_OF_G, on which a
 * gain per channel drops out) -, with the same plan, segmentation, window, detrend, scaling, M, fftshift and trim, the same
 * sums T and the same `empty` / `bad` rules.
 * oth_welch_set_steering: delays[ndir][nchan] host doubles in samples, fractional or negative as they come; fc the carrier
 * in cycles per sample.  1 <= ndir <= OTH_DOA_DIRS_MAX, 2 <= nchan <= 8.  Channel c carries s(t - tau_c), so at bin k its
 * transform obeys X_c = X_s exp(-j 2 pi (fc + f_k) tau_dc), f_k the signed bin frequency k / nfft for k < nfft / 2 and
 * (k - nfft) / nfft from there on (it does not depend on the plan's fs).  With S_ab = E[conj(X_a) X_b] the vector of every
 * quadratic form below is w_c(d, k) = exp(+j 2 pi (fc + f_k) tau_dc).  The library keeps tau and frac(fc tau) in double - the
 * carrier's whole cycles come off on the host, exactly - and the kernel forms frac(fc tau) + f_k tau in double per bin and
 * takes sincospi of twice that: no recurrence over bins.  A second call replaces the first table, after the plan's queued
 * launches have drained; ndir = 0 clears it.  Refused: a plan that is refused below, ndir or nchan out of range, delays
 * NULL, fc or a delay (or their product) not finite.
 * With A the matrix, l_1 >= ... >= l_C its eigenvalues clamped at 0 and ranked as oth_welch_matrix_eig ranks them, v_i its
 * eigenvectors, y_i = v_i^H w, p_i = |y_i|^2 and delta = loading trace(A) / C:
 *   bartlett = sum_i l_i p_i / C^2                   = w^H A w / C^2
 *   capon    = 1 / sum_i p_i / (l_i + delta)         = 1 / w^H (A + delta I)^-1 w;  exactly 0 in a bin where l_C + delta <= 0
 *   music    = C / sum_{i > nsrc} p_i                +inf where the sum is exactly 0
 * Outputs: float32 [ndir][out_len] each, row d the table's direction d, always linear (a plan set to dB gives its linear
 * twin's rows bit for bit), with the plan's fftshift and trim.  Any pointer may be NULL, not all three; a row is the same
 * bits alone or with the others, and a direction's row does not depend on the other directions of the table.  nsrc, the
 * dimension of the signal subspace, is read only with music_out.  A bin with a non-finite channel reads NaN in every row.
 * Among equal eigenvalues the subspaces are taken as computed (the lower Jacobi index first).
 * Four launches per call: the averaging launch and the totals launch of oth_welch_matrix, the basis build of csrc/mateig.hip
 * (the Jacobi of oth_welch_matrix_eig; the ranked eigenvalues and all C vectors stay on the device in double), then
 * csrc/matdoa.hip over bins x directions: one projection onto the eigenbasis serves the three spectra.  Bit-identical run
 * to run.
 * _dev: device in, device out, asynchronous.  oth_welch_matrix_doa: iq is [nchan][nsamples] contiguous, host or device
 * source, host outputs, blocking.
 * Refused, the reason in oth_last_error(), before anything is allocated, staged or launched, and the plan goes on working, in
 * this order: OTH_ERR_UNSUPPORTED on a multitaper plan, a plan set to OTH_AVERAGE_MEDIAN, a transform length that is not a
 * power of two from 64 to 16384; OTH_ERR_INVALID for nchan outside 2 ... 8, of not OTH_EIG_OF_S or OTH_EIG_OF_G, a NULL input,
 * all three outputs NULL; OTH_ERR_UNSUPPORTED without a steering table; OTH_ERR_INVALID for nchan other than the table's,
 * nsrc outside 1 ... nchan - 1 when music_out is given, loading not finite or below 0, chan_stride < nsamples, input shorter
 * than nperseg.
 * Not provided: a wideband combination over bins on the device, tabulated (calibrated) array manifolds, more than 8 channels,
 * multitaper plans. */
#define OTH_DOA_DIRS_MAX 1024
int oth_welch_set_steering(oth_plan *plan, int ndir, int nchan, const double *delays, double fc);
int oth_welch_matrix_doa_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nchan, size_t chan_stride, int of, int nsrc,
                             double loading, float *bartlett_out_dev, float *capon_out_dev, float *music_out_dev, uint64_t *nseg_out);
int oth_welch_matrix_doa(oth_plan *plan, const void *iq, size_t nsamples, int nchan, int src_is_device, int of, int nsrc,
                         double loading, float *bartlett_out, float *capon_out, float *music_out, uint64_t *nseg_out);

/* oth_welch_matrix_gcc_dev / oth_welch_matrix_gcc (additions inside ABI 6; probe by the symbols): what are the delays between
 * the channels?  The generalized cross-correlation of Knapp and Carter for every pair a < b of the C channels, and the delay
 * at its peak - the figure a steering table of oth_welch_set_steering has to be calibrated with (cable and front-end delays),
 * and the TDOA of separated receivers.  Same plan, segmentation, window, detrend and M as oth_welch_matrix, and the same sums
 * T; the plan's fftshift, trim, dB switch and scaling take no part: the outputs are rows over lags, and every weighting
 * cancels the scale.
 * Band: band_lo <= band_hi, signed bins of the natural transform (bin k at frequency k / nfft cycles per sample), both
 * inclusive, each in -nfft / 2 ... nfft / 2 - 1.  Upsampling: upsample = U is 1, 2, 4 or 8 with NI = U nfft <= 16384; signed
 * bin k goes to index k mod NI of an NI-point inverse transform (band-limited interpolation), so lags count 1 / U sample.
 * Per pair, with Z and the weights in double and the weighted phasors handed to a float32 transform:
 *   u_k = T_ab[k] / |T_ab[k]|       0 where |T_ab[k]| = 0, or where T_aa[k] <= 0, or where T_bb[k] <= 0
 *   w_k = 1 (OTH_GCC_PHAT), |T_ab| / sqrt(T_aa T_bb) (OTH_GCC_SCOT), |T_ab| (OTH_GCC_PLAIN)
 *   Z   = the number of in-band bins with u_k != 0 (PHAT, SCOT);  sqrt(sum_k T_aa[k] sum_k T_bb[k]) over the band (PLAIN)
 *   R_ab[l] = (1 / Z) sum_{k in band} w_k u_k e^(+j 2 pi k l / NI),    l = -maxlag ... maxlag,   0 <= maxlag <= NI / 2 - 1
 * |R| <= 1 under all three; PLAIN is the correlation coefficient of the band, and the SCOT peak is the mean coherence
 * magnitude along the delay.  Channel c carries s(t - tau_c), the convention of oth_welch_set_steering: |R_ab| peaks at
 * l / U = tau_b - tau_a.
 * Outputs, P = C (C - 1) / 2 pairs in the order (0,1), (0,2), ..., (C-2,C-1); either pointer may be NULL, not both, and each is
 * the same bytes with and without the other:
 *   gcc_out  [P][2 maxlag + 1] interleaved re, im, float32: R_ab at the lags -maxlag ... maxlag
 *   peak_out [P][3] float32, with i the lag of the largest |R| of the window (the lowest lag among equals): the delay in
 *            samples (i + d) / U, d = 0.5 (y- - y+) / (y- - 2 y0 + y+) on |R| at i - 1, i, i + 1, and d = 0 where i is a
 *            window edge or the denominator is not negative; |R[i]|; arg R[i] in radians (at a carrier fc cycles per sample:
 *            -2 pi fc (tau_b - tau_a) modulo 2 pi).
 * The parabola on |R| at U = 1 is biased towards the nearest whole lag; upsample is what removes the bias.
 * Degenerate input (the matrix family's rules): finite input never gives NaN or inf.  Z = 0 (a silent channel, or a constant
 * under detrend, across the band) gives an all-zero row and a peak of (0, 0, 0).  A channel with a non-finite sum inside the
 * band (a NaN or +-inf sample) makes every output of every pair that involves it NaN, never inf; every other pair stays bit
 * for bit what it is without the bad sample.  M = 1 is allowed.  Bit-identical run to run.
 * Three launches per call: the averaging launch and the totals launch of oth_welch_matrix (over every bin, whatever the plan
 * trims), then one workgroup per pair (csrc/matgcc.hip): w_k u_k / Z in double into an NI-point tile of LDS, the inverse
 * transform, the window and a fixed-order argmax.
 * _dev: device in, device out, asynchronous.  oth_welch_matrix_gcc: iq is [nchan][nsamples] contiguous, host or device
 * source, host outputs, blocking.
 * Refused, the reason in oth_last_error(), before anything is allocated, staged or launched, and the plan goes on working, in
 * this order: OTH_ERR_UNSUPPORTED on a multitaper plan, a plan set to OTH_AVERAGE_MEDIAN, a transform length that is not a
 * power of two from 64 to 16384; OTH_ERR_INVALID for nchan outside 2 ... 8, a NULL input, chan_stride < nsamples, input shorter
 * than nperseg, a weighting that is not one of the three, a band outside the range or band_lo > band_hi, upsample not 1, 2, 4
 * or 8; OTH_ERR_UNSUPPORTED for upsample nfft > 16384; OTH_ERR_INVALID for maxlag outside 0 ... NI / 2 - 1, both outputs NULL.
 * Not provided: the ML / Hannan-Thomson weighting, coherence-gated weights, more than 8 channels, multitaper plans, partial
 * sums for time-sharded runs. */
#define OTH_GCC_PLAIN 0   /* w = |T_ab|: the band's correlation coefficient             */
#define OTH_GCC_PHAT  1   /* w = 1: the phase transform                                 */
#define OTH_GCC_SCOT  2   /* w = |T_ab| / sqrt(T_aa T_bb): the smoothed coherence transform */
#define OTH_GCC_UPSAMPLE_MAX 8
int oth_welch_matrix_gcc_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nchan, size_t chan_stride,
                             int weighting, int band_lo, int band_hi, int upsample, int maxlag,
                             float *gcc_out_dev, float *peak_out_dev, uint64_t *nseg_out);
int oth_welch_matrix_gcc(oth_plan *plan, const void *iq, size_t nsamples, int nchan, int src_is_device,
                         int weighting, int band_lo, int band_hi, int upsample, int maxlag,
                         float *gcc_out, float *peak_out, uint64_t *nseg_out);   /* iq: [nchan][nsamples], blocking */

/* oth_welch_set_prototype, oth_welch_pfb_dev / oth_welch_pfb (additions inside ABI 6; probe by the symbols): the PSD of a
 * polyphase filter bank (weighted overlap-add, WOLA) on a plan of oth_welch_plan with nperseg == nfft = N.  Every other PSD
 * of the library uses a window no longer than the transform, and such a bin has a skirt: a strong neighbour leaks into an
 * empty channel and sets the floor of a detector that sums bins over it.  Here a real prototype h of P N taps (P taps per
 * branch, 2 <= P <= 16; ofdm_tools.windows.pfb_prototype gives a Kaiser-windowed sinc) is folded onto one transform length
 * in front of the FFT: a bin has a flat top and a stop band that starts one bin away.  The hop is the plan's
 * step = N - noverlap: noverlap = 0 is the critically sampled bank, N / 2 the 2x oversampled one, any value the plan accepts
 * is allowed.  Per stream, frame s covers the P N samples from s step:
 *   M       = (nsamples - P N) / step + 1                              integer division; nsamples >= P N
 *   m_s     = (1 / (P N)) sum_{i < P N} x[s step + i]                  on a detrending plan, 0 otherwise
 *   y_s[n]  = sum_{p < P} h[n + p N] (x[s step + n + p N] - m_s)       n < N
 *   X_s     = FFT_N(y_s)
 *   pfb[k]  = scale (1 / M) sum_s |X_s[k]|^2                           then the plan's fftshift, trim and dB
 *   scale   = 1 / (fs sum h^2) (OTH_SCALE_DENSITY), 1 / (sum h)^2 (OTH_SCALE_SPECTRUM), 1 / N^2 (OTH_SCALE_OVER_N2), 1 otherwise
 * The sums of h are formed in double when the prototype is set.  The plan's own window takes no part.  In real arithmetic the
 * row equals every P-th bin of scipy.signal.welch(x, fs, window=h, nperseg=P N, noverlap=P N - step, nfft=P N,
 * detrend='constant' | False, return_onesided=False, scaling=...) - a plan of P N points with h as its window runs P times
 * the transforms at P times the length, and only while P N is a supported length; the fold runs one N-point transform per
 * frame.  The mean comes off as in the multitaper kernels: a pilot (the mean of the frame's first 64 samples) comes off
 * every sample as it is loaded, the residual mean of the frame then comes off by linearity,
 * y[n] -= m hfold[n] with hfold[n] = sum_p h[n + p N] (formed in double), so a frame is read once.
 * Output: pfb [nstreams][out_len] float32.  All-zero input gives a row of exact zeros; a constant input on a detrending plan
 * gives exact zeros (-inf under dB).  A sample with a NaN or +-inf part inside a stream's frames: that stream's row reads NaN
 * in every bin, linear or dB, never inf; other streams of the launch are untouched bit for bit.
 * One averaging launch per call (csrc/welchpfb.hip: a workgroup takes whole frames of one stream in a contiguous run), then
 * a small finalize launch that adds the workgroups' rows in double in a fixed order: bit-identical run to run.
 * oth_welch_set_prototype: ntaps = P, h = ntaps * nfft host floats.  It replaces any earlier prototype, waits for the plan's
 * queued work, and has no effect on any other call of the plan.
 * _dev: device in, device out, asynchronous, nstreams as oth_welch_exec_dev (at most 65535).  oth_welch_pfb: one stream,
 * host or device source, host output, blocking.
 * Refused, the reason in oth_last_error(), before anything is staged, and the plan goes on working.  OTH_ERR_UNSUPPORTED:
 *   a multitaper plan          "the filter-bank PSD is not available on a multitaper plan: its segments' transforms are
 *                              Welch's (oth_welch_plan)"
 *   OTH_AVERAGE_MEDIAN         "the filter-bank PSD is not available with OTH_AVERAGE_MEDIAN: its rows are means over segments
 *                              (oth_plan_set_average(OTH_AVERAGE_MEAN) first)"
 *   the transform length       "the filter-bank PSD takes a transform length that is a power of two from 64 to 16384, not <nfft>"
 *   nperseg != nfft            "the filter-bank PSD folds whole transform lengths: it takes a plan with nperseg == nfft, not
 *                              <nperseg> and <nfft>"
 *   no prototype set           "the filter-bank PSD needs its prototype: call oth_welch_set_prototype on this plan"
 *   more than 65535 streams    "the filter-bank PSD takes at most 65535 streams per launch"
 * OTH_ERR_INVALID:
 *   ntaps outside 2 ... 16     "ntaps must lie in 2 ... 16"
 *   a NULL h                   "h is NULL"
 *   a non-finite tap           "every tap of the prototype must be finite"
 *   sum h^2 == 0               "the prototype is all zero"
 *   sum h == 0, SPECTRUM       "OTH_SCALE_SPECTRUM needs a prototype with a non-zero sum"
 *   a NULL input or output, nstreams < 1     "bad argument"
 *   stream_stride < nsamples   "stream_stride < nsamples"
 *   nsamples < P N             "input shorter than ntaps * nfft (<P> * <nfft> samples)"
 * in this order: the plan's kind (both setter and run), then the setter's arguments, or the missing prototype and the run's
 * arguments with the stream limit last.
 * Not provided: complex prototypes, a sliding window that carries P - 1 blocks across frames (consecutive
 * frames re-read their shared samples from L2), time-sharded partial sums, multitaper plans, the median average,
 * any-length transforms, a ticketed asynchronous form.  The bank's time-domain outputs, in the circular-shift form that keeps
 * the phase continuous between hops, are oth_channelizer_* below. */
int oth_welch_set_prototype(oth_plan *plan, int ntaps, const float *h);
int oth_welch_pfb_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                      float *pfb_out_dev, uint64_t *nseg_out);
int oth_welch_pfb(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device, float *pfb_out, uint64_t *nseg_out);

/* Degenerate inputs of the one-channel average - oth_welch_exec, _exec_async, _exec_dev, _scale_dev and _finalize, plans
 * of oth_welch_plan and oth_mtm_plan, every kernel route and detrend mode (tests/test_degenerate_gpu.py): the rule is the
 * two-channel path's, and SciPy's result is the specification.  A sample with a NaN or +-inf part makes every bin of that
 * stream's output NaN, linear or dB, never inf (an inf sample leaves NaN in all bins of SciPy's transform, inf in some of
 * this one's: the output stage writes NaN for every scaled sum that float32 does not hold), so a bin whose float32 sum of
 * |X|^2 overflowed reads NaN too, never inf, while the other bins of the row stay right.  The other streams of the launch
 * are untouched, bit for bit under the static schedules, and so is the next call on the plan: nothing of a poisoned launch
 * stays in a workspace, and oth_welch_reset clears the streaming form.  oth_welch_partial_dev hands back the raw sums as
 * they are, non-finite or not: the rule applies where sums are scaled.  oth_welch_segments_dev: exactly the rows of the
 * segments that hold the sample are non-finite (NaN) in every bin.  Silence gives exact zeros, -inf under
 * oth_plan_set_output_db (numpy's 10 log10(0)); a constant gives exact zeros under OTH_DETREND_CONSTANT and at most
 * (4 ulp)^2 of the undetrended line under OTH_DETREND_CONSTANT_FAST.  A gain that is a power of two scales the output by
 * its square bit for bit while no value leaves float32's normal range. */
/* one-shot: nsamples complex64 -> psd_out[nfft - 2*trim] (host).  Blocking: returns when the PSD is in psd_out.  The
 * last launch writes the row and a completion word into pinned host memory and the call polls that word (no interrupt
 * wake-up; after 20 ms it falls back to a stream synchronisation, which also reports a failed launch;
 * oth_plan_set_hostwait).  Any number of threads may call it on one plan: they run one after the other. */
int oth_welch_exec(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device,
                   float *psd_out, uint64_t *nseg_out);
/* The same step without blocking (ABI 5) - what a gr.sync_block's work() or message handler needs for a Welch scan
 * (reference: python/spectrum_sensor.py:71-75,105-117 -> ofdm_cr_tools.py:471-537; the chain has oth_chain_push_async):
 * _exec_async enqueues copy + kernels and returns a ticket (> 0) at once - the caller's host buffer may be reused when
 * it returns (buffers up to 1 MiB go through a pinned ring and never wait; a larger pageable buffer is staged by the HIP
 * runtime, which may hold the call until earlier work on the stream has finished); _poll looks once (*ready = 0: still running; 1: psd_out / nseg_out are filled); _wait polls until the
 * row is there.  Neither holds the context while it waits.  The plan keeps the last 4 launches: an older ticket
 * reports OTH_ERR_STATE, and _exec_async itself waits only when the GPU is 4 launches behind.  psd_out may be NULL
 * (completion only). */
int oth_welch_exec_async(oth_plan *plan, const void *iq, size_t nsamples, int src_is_device, uint64_t *ticket_out);
int oth_welch_poll(oth_plan *plan, uint64_t ticket, float *psd_out, uint64_t *nseg_out, int *ready);
int oth_welch_wait(oth_plan *plan, uint64_t ticket, float *psd_out, uint64_t *nseg_out);
/* nstreams independent streams laid out every stream_stride samples; device in,
 * device out [nstreams][out_len]; asynchronous. */
int oth_welch_exec_dev(oth_plan *plan, const void *iq_dev, size_t nsamples, int nstreams,
                       size_t stream_stride, float *psd_out_dev, uint64_t *nseg_out);
/* raw sum over segments of |X|^2 (natural bin order, no scale) for time-sharded
 * multi-GPU Welch: partial sums from ranks add, then oth_welch_scale_dev(). */
int oth_welch_partial_dev(oth_plan *plan, const void *iq_dev, size_t nsamples,
                          float *sum_out_dev, uint64_t *nseg_out);
int oth_welch_scale_dev(oth_plan *plan, const float *sum_dev, uint64_t nseg_total, float *psd_out_dev);

/* streaming form used by the sync_block work() host (python/spectrum_sensor.py:71-75
 * contract): chunks of any length; the overlap tail is carried between calls.  accumulate() copies the
 * caller's buffer into a pinned staging slot, enqueues the H2D copy and the kernels, and returns without
 * waiting for the GPU (it waits only if the GPU is still four calls behind); finalize() synchronises. */
int oth_welch_accumulate(oth_plan *plan, const void *iq_host, size_t nsamples);
int oth_welch_finalize(oth_plan *plan, float *psd_out, uint64_t *nseg_out);   /* then resets */
int oth_welch_reset(oth_plan *plan);

/* ---- two-channel cross spectrum / coherence -------
 * Semantics of scipy.signal.csd / coherence with the plan's Welch parameters;
 * produces the first input of coherence_detector (coherence_detector.py:45).
 * Outputs (host, natural FFT order unless the plan has fftshift): pxx, pyy,
 * cxy are float[nfft]; pxy is interleaved re,im float[2*nfft].  Any may be NULL.
 *
 * Degenerate inputs: SciPy's result is the specification, on every route (tests/test_csd_gpu.py).  A silent channel
 * gives Pyy = Pxy = 0 exactly and Cxy = 0 / 0 = NaN in every bin.  A NaN or inf sample in one channel makes that channel's
 * power, Pxy and Cxy NaN in every bin and leaves the other channel's power untouched (the output stage writes NaN for
 * every sum that is not finite - an inf sample leaves NaN in all bins of SciPy's transform, inf in some of this one's -
 * so sums that overflow float32 read NaN too, never inf).  A channel against itself gives
 * Im Pxy = 0 exactly (Im(conj(X) Y) is formed from two rounded products, antisymmetric bit for bit) and Cxy = 1.
 * Gains that are powers of two leave Cxy unchanged.
 *
 * dB output is not defined for a complex cross spectrum: on a plan with oth_plan_set_output_db(1) EVERY oth_csd_* call -
 * _exec, _exec_dev, and the raw sums and scale stage _partial_dev / _scale_dev with them - returns OTH_ERR_UNSUPPORTED
 * before anything is launched; the plan and the context stay usable.  OTH_KERNEL_TUNED covers the two-channel path at
 * nfft = nperseg = 4096 only and is refused (OTH_ERR_UNSUPPORTED) elsewhere; the plan works again under OTH_KERNEL_AUTO. */
int oth_csd_exec(oth_plan *plan, const void *x, const void *y, size_t nsamples, int src_is_device,
                 float *pxx, float *pyy, float *pxy, float *cxy, uint64_t *nseg_out);

/* Device forms of the same (asynchronous on the context's stream; any output pointer may be NULL). */
int oth_csd_exec_dev(oth_plan *plan, const void *x_dev, const void *y_dev, size_t nsamples, float *pxx_dev,
                     float *pyy_dev, float *pxy_dev, float *cxy_dev, uint64_t *nseg_out);
/* Raw sums over segments for time-sharded multi-GPU coherence: sums_out_dev is
 * float[4 * nfft] = sum |X|^2 [nfft], sum |Y|^2 [nfft], sum conj(X) Y [nfft] interleaved re,im; natural bin order,
 * no scale / shift / trim.  Partial sums of ranks add; oth_csd_scale_dev() then applies the plan's scaling for
 * nseg_total segments, its fftshift / trim, and forms Cxy = |Pxy|^2 / (Pxx Pyy). */
int oth_csd_partial_dev(oth_plan *plan, const void *x_dev, const void *y_dev, size_t nsamples, float *sums_out_dev,
                        uint64_t *nseg_out);
int oth_csd_scale_dev(oth_plan *plan, const float *sums_dev, uint64_t nseg_total, float *pxx_dev, float *pyy_dev,
                      float *pxy_dev, float *cxy_dev);

/* ---- per-vector periodogram chain ----------------------------------------
 * Replaces the GNU Radio chain
 *   stream_to_vector -> keep_one_in_n -> fft_vcc(N, True, window, shift) ->
 *   complex_to_mag[_squared] [-> multiply_const(1/N^2)]
 *   [-> single_pole_iir_filter_ff -> nlog10_ff]
 * of spectrum_sensor_v2.py:85-93, psd_logger.py:43-53, local_worker.py:58-69,
 * multichannel_scanner.py:78-86.  The chain keeps GNU Radio's stream state
 * between calls: leftover samples of a partial vector, the keep_one_in_n
 * counter, the IIR memory and the peak-hold vector.  nfft: any length (TRANSFORM LENGTHS above).
 * oth_chain_set_keep_one_in_n is GNU Radio 3.7's keep_one_in_n::set_n (d_n = d_count = n): the count restarts in
 * front of the vector that is still incomplete.  That vector is kept if the new count says so even when
 * oth_chain_push_async skipped its first samples as dropped: such samples wait in host memory (a plain copy, no
 * stream operation) and go to the device with the next push that enqueues work.
 *
 * Degenerate inputs (tests/test_degenerate_gpu.py): a NaN or +-inf sample makes the row of its vector non-finite in every
 * bin - NaN or inf: which of the two is not pinned, GNU Radio's own blocks differ there - and leaves every other raw row
 * untouched bit for bit.  From that vector on every bin of the IIR memory, of the dB rows and of the peak-hold vector is
 * non-finite and stays so across pushes until oth_chain_reset: the peak is the reference's np.maximum, which keeps a NaN
 * (a NaN ranks above +inf above every finite value), not IEEE maxNum, which drops it.  A bad sample inside a vector that
 * keep_one_in_n drops changes nothing.  After oth_chain_reset the chain gives what a new one gives, bit for bit.
 */
int oth_chain_create(oth_ctx *ctx, int nfft, const float *window, int fftshift, int epilogue,
                     int keep_one_in_n, oth_chain **out);
int oth_chain_destroy(oth_chain *chain);
int oth_chain_set_keep_one_in_n(oth_chain *chain, int n);     /* local_worker.py:85-87 set_rate */
/* single_pole_iir_filter_ff(alpha) + nlog10_ff(10, N, k_db); alpha<=0 disables */
int oth_chain_set_iir_log(oth_chain *chain, float alpha, float k_db);
int oth_chain_set_peak_hold(oth_chain *chain, int enable);    /* psd_logger.py:85 */
int oth_chain_set_kernel(oth_chain *chain, int which);         /* OTH_KERNEL_GENERIC: coverage kernels (parity tests) */
int oth_chain_reset(oth_chain *chain);
/* feed nsamples (host, or device when src_is_device); rows_out (host, may be
 * NULL) receives up to rows_capacity post-epilogue rows (dB rows when the IIR/log
 * stage is on); nrows_out = rows produced by this call. */
int oth_chain_push(oth_chain *chain, const void *iq, size_t nsamples, int src_is_device,
                   float *rows_out, size_t rows_capacity, uint64_t *nrows_out);
/* device in, device out ([rows_capacity][nfft], may be NULL), asynchronous, never synchronises */
int oth_chain_push_dev(oth_chain *chain, const void *iq_dev, size_t nsamples, float *rows_out_dev,
                       size_t rows_capacity, uint64_t *nrows_out);
/* The sync_block.work() form (python/spectrum_sensor.py:71-75: must not block; input valid only during the
 * call; consumers behind message_sink(dont_block) + msg_queue(2) see the latest vector,
 * spectrum_sensor_v2.py:71-72,97,404-414): the samples are copied into a pinned ring slot, the H2D copy + the kernels
 * are enqueued - the closing kernel writes the LATEST row straight into the slot's pinned host row - an event is
 * recorded and the call returns a ticket.  A push none of whose vectors survives keep_one_in_n enqueues nothing at all.  poll() is
 * non-blocking (ready = 0 while the GPU is still working); wait() blocks without holding the context.  The ring
 * keeps the last four tickets: an older one returns OTH_ERR_STATE (it lost against newer vectors). */
/* (Pushes above 1 MiB of PAGEABLE host memory skip the pinned slot and use the runtime's staged copy, which returns once
 * the caller's buffer has been read but may hold the host until the stream reaches the copy; GNU Radio's work() chunks
 * are far smaller.) */
int oth_chain_push_async(oth_chain *chain, const void *iq_host, size_t nsamples, uint64_t *ticket_out);
int oth_chain_poll(oth_chain *chain, uint64_t ticket, float *row_out, uint64_t *nrows_out, int *ready);
int oth_chain_wait(oth_chain *chain, uint64_t ticket, float *row_out, uint64_t *nrows_out);
/* rows the push behind `ticket` produces (known when it is enqueued; never waits): lets a consumer that counts
 * vectors - the waterfall's keep_one_in_n(sens_per_sec), spectrum_sensor_v2.py:102 - count the ones it drops too */
int oth_chain_ticket_rows(oth_chain *chain, uint64_t ticket, uint64_t *nrows_out);
/* Stream operations (asynchronous copies + kernel launches; event records not counted) the LAST push of this chain
 * enqueued (ABI 6) - what a work()-sized push costs the scheduler thread: 0 for a push all of whose vectors keep_one_in_n
 * drops (nothing is copied or launched; the ticket is ready at once), 2 for a chain without state (H2D + one kernel that
 * writes the latest row into pinned host memory), 3 with the IIR / peak-hold state (tests/test_blocks_gpu.py). */
int oth_chain_last_push_ops(oth_chain *chain, uint64_t *ops_out);
int oth_chain_get_peak(oth_chain *chain, float *peak_out);    /* float[nfft] */
int oth_chain_get_iir(oth_chain *chain, float *lin_out);      /* float[nfft], linear IIR state */
/* mean of each `group` consecutive rows (BASELINE config 1 "8-seg avg") */
int oth_rows_group_mean(oth_ctx *ctx, const float *rows_host, size_t nrows, int nfft, int group,
                        float *out_host);

/* ---- polyphase channelizer (additions inside ABI 6; probe by the symbols) ------------------------------------------------
 * oth_channelizer_*: one wideband stream in, nchan baseband IQ rows out, on the device - the rows are the `nstreams` streams
 * every `stream_stride` samples that the _dev statistics take (oth_welch_exec_dev, _sk_dev, _cyclic_dev, _caf_dev, _pfb_dev,
 * the multitaper _dev forms).  A handle of its own, as oth_chain: M = nchan channels, hop D = decim (a new output sample of
 * every channel per D input samples), a real prototype h of L = ntaps * nchan taps (ntaps = P taps per branch;
 * ofdm_tools.windows.pfb_prototype gives a Kaiser-windowed sinc).  With t counting the input samples since creation or the
 * last reset, frame m = 0, 1, ... covers the samples m D ... m D + L - 1 and
 *   y_k[m] = sum_{n < L} h[n] x[m D + n] e^{-j 2 pi k (m D + n) / M}       k = 0 ... M - 1, natural order (k >= M / 2: the
 *                                                                          negative frequencies)
 * - channel k / M cycles per sample mixed to DC by the phase of the absolute sample index, filtered by h, every D-th output
 * kept: each row is a proper baseband stream at rate fs / D, and a tone delta bins off a channel's centre advances
 * delta D / M cycles per output.  Computed as the fold of the filter-bank PSD, a circular shift and one transform per frame,
 *   u_m[r] = sum_{p < P} h[r + p M] x[m D + r + p M]  (r < M),   v_m[(r + m D) mod M] = u_m[r],   y_.[m] = FFT_M(v_m)
 * with m D mod M taken from the absolute frame index in integer arithmetic: it survives any number of pushes.  ntaps = 1 is
 * the short-time Fourier transform under h in the phase-continuous convention.  No detrend, no scale, no fftshift.
 * oth_channelizer_create: h = ntaps * nchan host floats; the prototype goes to the device once.
 * oth_channelizer_reset: the sample count back to 0, the pending tail emptied; waits for the context's queued work.
 * oth_channelizer_frames: host arithmetic - the frames the NEXT push of nsamples will yield: with q samples pending,
 *   q + nsamples >= L ? (q + nsamples - L) / D + 1 : 0.      oth_channelizer_pending: q, always at most L - 1.
 * oth_channelizer_push_dev: device in, device out, asynchronous on the context's stream.  out_dev is [nchan][out_stride]
 * complex64: channel k starts at out_dev + k * out_stride and this push's frames go to its columns 0 ... nframes - 1;
 * nothing else of the buffer is written.  out_dev may be NULL when the push yields no frame.  The input may be reused once
 * the stream has passed the call: the samples a later frame still needs (fewer than L) are kept in a device tail of the
 * handle.  One launch per push (csrc/chanpfb.hip) and at most two small device copies for the tail.
 * oth_channelizer_push: blocking, host or device source, host output in the same layout.
 * Any split of a stream into pushes gives the same bytes as one push: a result depends on the absolute frame index alone.
 * All-zero input gives exact zeros; a NaN or +-inf sample makes exactly the frames that cover it non-finite, in every
 * channel, and leaves every other frame as it is bit for bit; a gain that is a power of two scales the output bit for bit.
 * Refused, the reason in oth_last_error(), before anything is allocated, staged or launched; the handle goes on working.
 * At creation, in this order:
 *   OTH_ERR_UNSUPPORTED  nchan no power of two 64 ... 4096   "the channelizer takes a channel count that is a power of two
 *                                                            from 64 to 4096, not <nchan>"
 *   OTH_ERR_INVALID      decim                               "decim must be nchan, nchan / 2 or nchan / 4"
 *                        ntaps outside 1 ... 16              "ntaps must lie in 1 ... 16"
 *                        a NULL h                            "h is NULL"
 *                        a non-finite tap                    "every tap of the prototype must be finite"
 *                        sum h^2 == 0                        "the prototype is all zero"
 * On a push, OTH_ERR_INVALID, in this order:
 *   a NULL input with nsamples > 0, a NULL nframes_out       "bad argument"
 *   frames to deliver and a NULL output                      "the output is NULL"
 *   out_stride below the push's frame count                  "out_stride < frames of this push"
 * nsamples == 0 is no error: 0 frames.
 * Not provided: complex prototypes, hops other than nchan, nchan / 2 and nchan / 4, fewer than 64 or more than 4096
 * channels, a channel subset, a synthesis bank, a ticketed asynchronous form, a sliding register window across frames
 * (consecutive frames re-read their shared samples from L2, as in csrc/welchpfb.hip). */
int oth_channelizer_create(oth_ctx *ctx, int nchan, int decim, int ntaps, const float *h, oth_channelizer **out);
int oth_channelizer_destroy(oth_channelizer *ch);
int oth_channelizer_reset(oth_channelizer *ch);
int oth_channelizer_frames(oth_channelizer *ch, size_t nsamples, uint64_t *nframes_out);
int oth_channelizer_pending(oth_channelizer *ch, size_t *nsamples_out);
int oth_channelizer_push_dev(oth_channelizer *ch, const void *iq_dev, size_t nsamples, void *out_dev, size_t out_stride,
                             uint64_t *nframes_out);
int oth_channelizer_push(oth_channelizer *ch, const void *iq, size_t nsamples, int src_is_device, void *out_host,
                         size_t out_stride, uint64_t *nframes_out);

/* ---- cyclic-prefix symbol timing and carrier offset (additions inside ABI 6; probe by the symbols) -------------------------
 * oth_cp_sync_dev / oth_cp_sync: where a symbol of a CP-OFDM signal starts and how far its carrier is off, by the
 * cyclic-prefix correlator (van de Beek, Sandell, Boerjesson 1997) folded over all symbols of a capture - the step behind
 * oth_welch_caf (which finds Tu and cp) and oth_welch_cyclic (which confirms the signal).  They hang off the context, not a
 * plan: no transform, window or scaling is involved.  Per stream x of nsamples complex64 samples and per hypothesis
 * h = (Tu, cp), with 8 <= Tu <= 16384, 1 <= cp <= Tu and Ts = Tu + cp <= 32768:
 *   S        = floor((nsamples - Tu) / Ts)                     symbols folded; S >= 1 or the call is refused
 *   z[n]     = x[n + Tu] conj(x[n])                            the lag product of oth_welch_caf: re = fma(ar, br, ai bi), im = ai br - ar bi
 *   e[n]     = (|x[n]|^2 + |x[n + Tu]|^2) / 2
 *   F[r]     = sum_{s < S} z[r + s Ts]        G[r] = sum_{s < S} e[r + s Ts]           r < Ts
 *   Gamma[t] = sum_{j < cp} F[(t + j) mod Ts] Phi[t] = sum_{j < cp} G[(t + j) mod Ts]  t < Ts   (circular window)
 *   Lambda[t]= |Gamma[t]| - rho Phi[t]                         rho a caller's float, 0 <= rho <= 1
 *   theta    = the lowest t that maximises Lambda
 *   eps      = arg(Gamma[theta]) / (2 pi)                      carrier offset in subcarrier spacings, |eps| <= 1/2; in cycles per sample: eps / Tu
 *   rho_hat  = |Gamma[theta]| / Phi[theta]   (0 where Phi == 0)    -> SNR = rho_hat / (1 - rho_hat)
 * The last sample read is S Ts - 1 + Tu <= nsamples - 1: nothing behind a stream's own nsamples is touched.  theta counts
 * from sample 0 of the stream to the first sample of a cyclic prefix, modulo Ts.
 * Outputs: gamma [nstreams][nhyp][row_stride] complex64 and phi [nstreams][nhyp][row_stride] float32, of which the columns
 * Ts_h ... row_stride - 1 are not written; est [nstreams][nhyp][4] float32 = theta, eps, rho_hat, Lambda[theta] (theta is
 * exact as a float: Ts <= 32768); nsym_out host uint64[nhyp] = S per hypothesis, by host arithmetic.  gamma and phi may be
 * NULL, est may not.
 * oth_cp_sync_dev: device in, device out, asynchronous on the context's stream; nstreams streams every stream_stride samples
 * as oth_welch_exec_dev (at most 65535) - the rows of oth_channelizer_push_dev as they are.  oth_cp_sync: one stream from a
 * host or device source, host outputs, blocking.  Three launches (csrc/cpsync.hip): the fold into one row of F re, F im, G per
 * run of symbols (float32 over blocks of at most 64 symbols, the blocks in double), the rows' totals, and the window with
 * the maximum - all sums behind the first in double, Gamma and Phi rounded to float32 once, Lambda formed from the unrounded
 * sums.  No atomics: the same call on the same device gives the same bytes.  The runs of symbols (W per hypothesis: what the
 * device holds at once over streams x hypotheses, at most S; the environment variable OTH_CPS_WG, read per call, caps it)
 * decide the order of the sums, so a hypothesis gives the same bytes alone and next to others whenever its W is the same
 * (always when S is below the device's share, or under OTH_CPS_WG).  The rows live in scratch the context owns; it grows when
 * needed and a call that finds it large enough allocates nothing.
 * All-zero input: Gamma, Phi and Lambda are exact zeros and est is (0, 0, 0, 0).  A sample with a NaN or +-inf part poisons
 * the residues it enters (n mod Ts and (n - Tu) mod Ts): every Gamma / Phi entry whose window covers a poisoned residue reads
 * NaN (never inf), every other entry of the row keeps the clean run's bits, est of a row with a non-finite entry is four
 * NaNs, and the other streams and hypotheses of the call are untouched bit for bit.
 * Refused, the reason in oth_last_error(), before anything is allocated, staged or launched; the context goes on working.
 * In this order:
 *   OTH_ERR_INVALID      a NULL input, tu, cp, est or nsym_out; nstreams < 1     "bad argument"
 *                        nhyp outside 1 ... 16                                    "nhyp must lie in 1 ... 16"
 *                        Tu outside 8 ... 16384                                   "Tu must lie in 8 ... 16384, not <Tu>"
 *                        cp outside 1 ... Tu                                      "cp must lie in 1 ... Tu, not <cp>"
 *                        rho outside [0, 1] or not finite                         "rho must be a finite value in 0 ... 1"
 *                        stream_stride < nsamples                                 "stream_stride < nsamples"
 *   OTH_ERR_UNSUPPORTED  more than 65535 streams                                  "cp_sync takes at most 65535 streams per launch"
 *   OTH_ERR_INVALID      row_stride below the largest Ts                          "row_stride below the largest Tu + cp (<Ts>)"
 *                        a hypothesis with S == 0                                 "input shorter than one symbol and its lag
 *                                                                                 (2 Tu + cp = <n> samples)"
 * Not provided: a streaming form that carries F / G across calls, fractional-sample timing, the integer part of the carrier
 * offset, pilot- or preamble-based synchronisation, Ts above 32768. */
int oth_cp_sync_dev(oth_ctx *ctx, const void *iq_dev, size_t nsamples, int nstreams, size_t stream_stride,
                    int nhyp, const int *tu, const int *cp, float rho, size_t row_stride,
                    float *gamma_out_dev, float *phi_out_dev, float *est_out_dev, uint64_t *nsym_out);
int oth_cp_sync(oth_ctx *ctx, const void *iq, size_t nsamples, int src_is_device,
                int nhyp, const int *tu, const int *cp, float rho, size_t row_stride,
                float *gamma_out, float *phi_out, float *est_out, uint64_t *nsym_out);

/* ---- channel power -------------------------------------------------------
 * src_power (ofdm_cr_tools.py:232-249): |convolve(psd, ones(int(sb))/sb, 'same')|
 * then per-channel slice sums.  lo/hi are the slice bounds the host computed with
 * the reference's int() arithmetic; power_out[nch]; also returns min power. */
int oth_channel_power(oth_ctx *ctx, const float *psd_host, int nfft, double srch_bins, int nch,
                      const int *lo, const int *hi, float *power_out, float *movavg_out /*nullable*/);

/* Per-bin energy detection for the batched scanner (BASELINE config 5; the per-bin analogue of the
 * channel threshold of spectrum_sensor_v2.py:465-477): noise = min_k movingaverage(psd)[k],
 * mask[k] = psd[k] > thr_leveler * noise.  nrows PSD rows of nfft bins each (host); mask_out is
 * uint8[nrows][nfft], noise_out float[nrows] (nullable).
 * The moving average here, in oth_channel_power and in oth_scan_decide_dev[_out] is np.convolve's: an output is inf / NaN
 * exactly where its window holds an inf / NaN bin.  The minimum is numpy's: one NaN output makes the row's noise floor NaN
 * and its mask all zero.  1 <= int(srch_bins) <= nfft, else OTH_ERR_INVALID: with a longer window the reference's
 * movingaverage returns int(srch_bins) values in another centring, which no nfft-long result is. */
int oth_bin_threshold(oth_ctx *ctx, const float *psd_host, int nrows, int nfft, double srch_bins,
                      float thr_leveler, unsigned char *mask_out, float *noise_out);

/* Decision stage of the batched scanner on PSD rows that are already in HBM (oth_welch_exec_dev with nstreams
 * rows): moving average once per row, channel slice sums (src_power, ofdm_cr_tools.py:232-249), noise floor and
 * per-bin mask (as oth_bin_threshold) in one launch sequence on context-owned scratch - no copy of the rows, no
 * allocation per call.  Host outputs: mask_out uint8[nrows][nfft] (nullable), noise_out float[nrows] (nullable),
 * power_out float[nrows][nch] (required when nch > 0).  Slices are Python's psd[lo:hi] with 0 <= lo, hi <= nfft (lo >= hi:
 * empty, sum 0).  Non-finite bins, NaN and the noise floor, int(srch_bins) <= nfft: as oth_bin_threshold. */
int oth_scan_decide_dev(oth_ctx *ctx, const float *psd_rows_dev, int nrows, int nfft, double srch_bins,
                        float thr_leveler, int nch, const int *lo, const int *hi, unsigned char *mask_out,
                        float *noise_out, float *power_out);
/* the same stage with DEVICE outputs (asynchronous on the context's stream, no host copy of anything but the
 * channel slice bounds): mask_dev [nrows][nfft] bytes (nullable), noise_dev [nrows], power_dev [nrows][nch]
 * (nullable when nch == 0).  The sharded scanner (multichannel_scanner over ranks) feeds these
 * straight into its all-gather. */
int oth_scan_decide_dev_out(oth_ctx *ctx, const float *psd_rows_dev, int nrows, int nfft, double srch_bins,
                            float thr_leveler, int nch, const int *lo, const int *hi, unsigned char *mask_dev,
                            float *noise_dev, float *power_dev);

/* ---- xcorr (ofdm_cr_tools.py:155-161) ------------------------------------
 * |fftshift(ifft(fft(b,L) * conj(fft(a,L))))[L/2:]| for any L (TRANSFORM LENGTHS above; `L/2` is the reference's
 * Python-2 integer division: L - L/2 outputs); a, b host complex64 of na, nb samples, zero-padded to L or, like
 * np.fft.fft(a, L), cut to their first L; out float[L - L/2]. */
int oth_xcorr(oth_ctx *ctx, const void *a, size_t na, const void *b, size_t nb, int L, float *out);
/* fac (ofdm_cr_tools.py:163-166): |fftshift(fft(|fft(data,L)|, L))[L/2:]| */
int oth_fac(oth_ctx *ctx, const void *data, size_t n, int L, float *out);

/* ---- diagnostics (ABI 5) ------------------------------------------------------------------------------------------
 * Which kernel build, detrend form, pilot, schedule, chunk sizes, grid and partial-row layout a launch takes is decided by
 * pure host logic (csrc/abi_route.hip resolve_recipe) and can be read back as text:
 *   "kernel=welch4096:ws nfft=4096 form=freq pilot=inline sched=dynamic chunk=20 tail=5 nbig=6297 bpc=2 W=512 rows=1 nch=1 layout=1"
 * oth__debug_recipe needs NO device: window_class 0 = all ones, 1 = confined spectrum (periodic cosine-sum windows),
 * 2 = wide (no detrend table), 3 = confined to 256 nfft / 4096 bins only; runtime_occupancy 0 = resident workgroups per CU
 * from the built-in MI355X table, 1 = from the occupancy calculator (needs a GPU).  oth__debug_last_recipe: the recipe of
 * the plan's last averaging launch; every call that launches one writes it (the statistics, the median average and
 * oth_welch_segments_dev name their own kernels), so it never names an earlier call.
 * oth__debug_live_resources needs no context and no device: how many device buffers, pinned host buffers and events the
 * library's contexts, plans and chains hold in this process right now (memory from oth_dev_alloc is the caller's and is
 * not counted).  Any pointer may be NULL.  After every context has been destroyed all three are zero.
 * oth__debug_channelizer_recipe: the launch of the handle's last push that yielded frames,
 *   "kernel=chanpfb nchan=64 decim=32 ntaps=8 tile=8 W=5 frames=37 tiles=5 pending=0 bpc=16"
 * (tile: frames of a tile, W: workgroups, each walking tiles / W whole tiles). */
int oth__debug_recipe(int nfft, int nperseg, int noverlap, int window_class, int detrend_mode, int two_channel, int kernel_pref,
                      const char *variant, int sched_pref, long long nseg, int nstreams, int cu_count, int runtime_occupancy,
                      char *buf, size_t buflen);
/* oth__debug_recipe with the overrides of oth_plan_set_tuning: sched (-1: none), chunk and tail_chunk (0: none) */
int oth__debug_recipe_tuned(int nfft, int nperseg, int noverlap, int window_class, int detrend_mode, int two_channel, int kernel_pref,
                            const char *variant, int sched_pref, long long nseg, int nstreams, int cu_count, int runtime_occupancy,
                            int tune_sched, int tune_chunk, int tune_tail, char *buf, size_t buflen);
int oth__debug_last_recipe(oth_plan *plan, char *buf, size_t buflen);
int oth__debug_channelizer_recipe(oth_channelizer *ch, char *buf, size_t buflen);
int oth__debug_live_resources(int *device_buffers, int *pinned_buffers, int *events);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_TOOLS_HIP_H */
