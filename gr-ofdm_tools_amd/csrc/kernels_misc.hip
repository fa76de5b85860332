// Small kernels around the FFT kernels: cross-workgroup reduction + scaling +
// fftshift/trim/dB (spectrum_sweeper.py:265-276), the time-recursive row
// epilogues (single_pole_iir_filter_ff + nlog10_ff of local_worker.py:66-69,
// peak hold of psd_logger.py:85), channel power (ofdm_cr_tools.py:168-170,
// 232-249), the synthetic IQ generator and the measurement probes.
#include <cstdint>

#include "fft_lds.hip.h"
#include "out_stage.hip.h"

namespace oth {

// Output stage of the two-channel path, shared by the finalize kernels and csd_scale_kernel.  An inf sample leaves NaN in
// every bin of SciPy's result (its transform multiplies the inf by twiddle zeros); here the register butterflies of the
// 4096-point kernels leave inf where all terms of a bin agree in sign (56 bins of 4096 measured) and NaN elsewhere, the LDS
// kernels NaN everywhere.  SciPy's result is the specification (include/ofdm_tools_hip.h): a power that is not finite, and
// a cross term with a part that is not finite, leave as NaN on every route.  Cxy = |Sxy|^2 / (Sxx Syy) on the raw sums
// (0 / 0 = NaN for a silent channel, inf / inf = NaN).
__device__ __forceinline__ void csd_store(double sxx, double syy, double sre, double sim, double scale, size_t o, float *pxx,
                                          float *pyy, float *pxy, float *cxy) {
    const double nan = __builtin_nan("");
    const bool cross_ok = isfinite(sre) && isfinite(sim);
    if (pxx) pxx[o] = (float)(isfinite(sxx) ? sxx * scale : nan);
    if (pyy) pyy[o] = (float)(isfinite(syy) ? syy * scale : nan);
    if (pxy) {
        pxy[2 * o] = (float)(cross_ok ? sre * scale : nan);
        pxy[2 * o + 1] = (float)(cross_ok ? sim * scale : nan);
    }
    if (cxy) cxy[o] = (float)((sre * sre + sim * sim) / (sxx * syy));
}

// Completion word for a polling host (FinalizeArgs.host_seq; round 5).  Called by EVERY thread of the block after its
// last output store (the outputs of such a launch are pinned host memory).  Every wave that stored outputs makes them
// visible at system scope with a RELEASE fence (L2 write-back + wait for the wave's stores; no acquire: an acquire would
// also invalidate the XCD's L2 under the blocks that are still reading partial rows - the first form of this, a full
// __threadfence_system() in all four waves of every block, took the 256-block finalize from 4.4 to ~28 us), the block
// barrier collects the waves where more than wave 0 stores (ALL_WAVES), and thread 0 arrives on the device counter.
// Whoever arrives last has, through that counter, every other block's fence before it: it re-arms the counter for the
// next launch and publishes the sequence value with a system-scope release store.  The host (oth_welch_exec / _poll /
// _wait in abi_welch.hip) reads the word with acquire semantics and then the rows.
template <bool ALL_WAVES>
__device__ __forceinline__ void finalize_signal(const FinalizeArgs &a) {
    if (!a.host_seq) return;      // launch-uniform
    if (ALL_WAVES || threadIdx.x < 64) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (ALL_WAVES) __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned nblocks = gridDim.x * gridDim.y;
        const unsigned prev = __hip_atomic_fetch_add(a.done_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == nblocks - 1) {
            // the one acquire of the scheme: this block has read every other block's arrival; their release fences now
            // happen-before the publication below (an invalidate in ONE block, after everybody has read the partial rows)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(a.done_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.host_seq, a.seq_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// 256 threads = 32 consecutive bins x 8 slices of the workgroup axis: slice_sums on the NCH rows of every workgroup, so the
// result does not depend on scheduling.
template <int NCH>
__global__ __launch_bounds__(256) void finalize_kernel(FinalizeArgs a) {
    if (a.queue_reset && blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < a.queue_n) a.queue_reset[threadIdx.x] = 0u;
    // threads walk partial-sum POSITIONS (coalesced reads); the bin and output slot follow
    const int pos = blockIdx.x * 32 + (threadIdx.x & 31), stream = blockIdx.y;
    const int k = bin_pos(pos, a.layout, a.l1, a.l2);
    int i;
    const bool live = out_slot(a.out, a.nfft, k, i) && pos < a.nfft;
    const float *base = a.partial + (size_t)stream * a.W * NCH * a.nfft + pos;
    double s[NCH];
    if (slice_sums<NCH>(live, a.W, [&](int w, int c) { return base[((size_t)w * NCH + c) * a.nfft]; }, s)) {
        const size_t o = (size_t)stream * a.out.nout + i;
        if constexpr (NCH == 1) store_psd(a.out0, o, s[0], a.scale, a.accumulate, a.out);
        else csd_store(s[0], s[1], s[2], s[3], a.scale, o, a.out0, a.out1, a.out2, a.out3);
    }
    finalize_signal<false>(a);      // the stores above are wave 0's (slice 0)
}

// One-launch form for many partial rows (the headline Welch path; NCH = 4: the two-channel path, round 4 - it went
// through reduce_partials_kernel + finalize_kernel, two launches): 256 threads = POS / 4 float4 columns (POS consecutive
// positions) x 1024 / POS row slices; slice sums in double, combined in a fixed order.  POS = 16 gives nfft / 16 blocks
// (one per CU at nfft = 4096).  Rows are [w][channel][nfft].
template <int POS, int NCH>
__global__ __launch_bounds__(256) void finalize_wide_kernel(FinalizeArgs a) {
    constexpr int COLS = POS / 4, SLICES = 256 / COLS;
    __shared__ double red[NCH][SLICES][POS + 1];
    if (a.queue_reset && blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < a.queue_n) a.queue_reset[threadIdx.x] = 0u;
    const int col = threadIdx.x % COLS, slice = threadIdx.x / COLS;
    const int stream = blockIdx.y;
    const float *base = a.partial + (size_t)stream * a.W * NCH * a.nfft + blockIdx.x * POS + col * 4;
    double s[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c) s[c][0] = s[c][1] = s[c][2] = s[c][3] = 0.0;
    for (int w = slice; w < a.W; w += SLICES) {      // (four rows of every channel in flight per trip: measured, no faster)
        float4 v[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = *reinterpret_cast<const float4 *>(base + ((size_t)w * NCH + c) * a.nfft);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            s[c][0] += v[c].x;
            s[c][1] += v[c].y;
            s[c][2] += v[c].z;
            s[c][3] += v[c].w;
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[c][slice][col * 4 + e] = s[c][e];
    __syncthreads();
    // The SLICES slice sums of a position in two steps (round 6): every thread adds SLICES / GROUPS of them (fixed order),
    // then the first POS threads add the GROUPS group sums.  One thread walking all 64 slices of four channels was 256
    // LDS reads that the compiler unrolled into 512 registers (the code object reported 536) - 8.9 us for the
    // four-channel form against 5.5 for one channel.
    constexpr int GROUPS = 256 / POS, PER = SLICES / GROUPS;
    static_assert(SLICES % GROUPS == 0, "slices per group");
    __shared__ double red2[NCH][GROUPS][POS + 1];
    {
        const int p = threadIdx.x % POS, g = threadIdx.x / POS;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < PER; ++q) t += red[c][g * PER + q][p];
            red2[c][g][p] = t;
        }
    }
    __syncthreads();
    const int pos = blockIdx.x * POS + threadIdx.x;
    const int k = bin_pos(pos, a.layout, a.l1, a.l2);
    int i;
    if (out_slot(a.out, a.nfft, k, i) && threadIdx.x < POS) {
        double t[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            t[c] = 0.0;
#pragma unroll 4
            for (int q = 0; q < GROUPS; ++q) t[c] += red2[c][q][threadIdx.x];
        }
        const size_t o = (size_t)stream * a.out.nout + i;
        if constexpr (NCH == 1) {
            store_psd(a.out0, o, t[0], a.scale, a.accumulate, a.out);
        } else {      // as finalize_kernel: Pxx, Pyy, Pxy, Cxy
            csd_store(t[0], t[1], t[2], t[3], a.scale, o, a.out0, a.out1, a.out2, a.out3);
        }
    }
    finalize_signal<false>(a);      // the stores above are wave 0's (threads < POS)
}

// (Determinism note: the group sums below are rounded to float32 before the second stage adds them in double, so a launch
// that takes this stage - W >= 1024 rows of 256 ... 1024 points, or W > 32 rows of the four-channel path - differs from the
// one-stage form by up to ~6e-8 relative per group: results are bit-reproducible for a given launch shape, not across the
// W threshold.  Far inside the parity tolerance; stated so that "fixed order" is not read as "one order for every shape".)
// Stage 1 of the cross-workgroup reduction when there are many partial rows: row group g of
// kReduceGroups sums its rows (fixed order) into scratch[stream][g][ch][nfft]; finalize_kernel then
// runs over the kReduceGroups rows.  256 threads = 64 float4 columns x 4 row lanes.
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float *partial, float *scratch, int W, int nch,
                                                              int nfft, int rows_per_group) {
    __shared__ double red[4][64][4];
    const int q = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + q) * 4;
    const int g = blockIdx.y, G = gridDim.y;
    const int stream = blockIdx.z / nch, ch = blockIdx.z % nch;
    const int w0 = g * rows_per_group, w1 = min(W, w0 + rows_per_group);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    const float *base = partial + (((size_t)stream * W) * nch + ch) * nfft + col;
    for (int w = w0 + j; w < w1; w += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(base + (size_t)w * nch * nfft);
        s0 += v.x;
        s1 += v.y;
        s2 += v.z;
        s3 += v.w;
    }
    red[j][q][0] = s0;
    red[j][q][1] = s1;
    red[j][q][2] = s2;
    red[j][q][3] = s3;
    __syncthreads();
    if (j) return;
    float4 o;
    o.x = (float)(red[0][q][0] + red[1][q][0] + red[2][q][0] + red[3][q][0]);
    o.y = (float)(red[0][q][1] + red[1][q][1] + red[2][q][1] + red[3][q][1]);
    o.z = (float)(red[0][q][2] + red[1][q][2] + red[2][q][2] + red[3][q][2]);
    o.w = (float)(red[0][q][3] + red[1][q][3] + red[2][q][3] + red[3][q][3]);
    *reinterpret_cast<float4 *>(scratch + ((((size_t)stream * G) + g) * nch + ch) * nfft + col) = o;
}

// ROW_X1_16K (welch16k1x, 16384 points, one channel): position 1024 k2 + 4 (16 k0 + k1) + q holds bin
// k0 + 16 k1 + 256 k2 + 4096 bitrev2(q), so ONE float4 at position 1024 k2 + 4 t (t = 16 k0 + k1) carries the four k3 of
// (k0, k1, k2).  A block takes one k2: 256 threads read W rows of 4 KiB each as float4 (coalesced), sum in double (fixed
// order), turn t = 16 k0 + k1 into k0 + 16 k1 through LDS and write four runs of 256 consecutive bins (1 KiB each) -
// reads and writes both coalesced.  The general finalize_kernel scatters 4-byte stores across the row for this layout:
// 21-24 us for the 64 x 16384 rows of BASELINE config 5 next to a 450 us transform kernel; this one 4-5 us.
__global__ __launch_bounds__(256) void finalize_l4_kernel(FinalizeArgs a) {
    __shared__ double red[4][256];
    if (a.queue_reset && blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < a.queue_n) a.queue_reset[threadIdx.x] = 0u;
    const int t = threadIdx.x, k2 = blockIdx.x, stream = blockIdx.y;
    const float *base = a.partial + (size_t)stream * a.W * a.nfft + 1024 * k2 + 4 * t;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int w = 0;
    for (; w + 4 <= a.W; w += 4) {      // four rows in flight (config 5 has exactly four per stream); same order of addition
        float4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const float4 *>(base + (size_t)(w + i) * a.nfft);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s0 += v[i].x;
            s1 += v[i].y;
            s2 += v[i].z;
            s3 += v[i].w;
        }
    }
    for (; w < a.W; ++w) {
        const float4 v = *reinterpret_cast<const float4 *>(base + (size_t)w * a.nfft);
        s0 += v.x;
        s1 += v.y;
        s2 += v.z;
        s3 += v.w;
    }
    const int u = (t >> 4) + 16 * (t & 15);      // k0 + 16 k1
    red[0][u] = s0;                              // q = 0 -> k3 = 0
    red[2][u] = s1;                              // q = 1 -> k3 = 2
    red[1][u] = s2;                              // q = 2 -> k3 = 1
    red[3][u] = s3;                              // q = 3 -> k3 = 3
    __syncthreads();
#pragma unroll
    for (int k3 = 0; k3 < 4; ++k3) {
        int i;
        if (!out_slot(a.out, a.nfft, t + 256 * k2 + 4096 * k3, i)) continue;
        store_psd(a.out0, (size_t)stream * a.out.nout + i, red[k3][t], a.scale, a.accumulate, a.out);
    }
    finalize_signal<true>(a);
}

hipError_t launch_finalize(const FinalizeArgs &a_in, int nstreams, hipStream_t s) {
    FinalizeArgs a = a_in;
    if (a.layout == ROW_X1_16K && a.nch == 1 && a.nfft == 16384 && a.W <= 64) {
        hipLaunchKernelGGL(finalize_l4_kernel, dim3(16, nstreams), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (const int groups = a.scratch ? finalize_row_groups(a.nfft, a.W, a.nch) : 0) {
        // many short rows: 256 workgroups sum them into `groups` rows first (fixed order inside a group and across groups)
        const int rpg = (a.W + groups - 1) / groups;
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(a.nfft / 256, groups, nstreams), dim3(256), 0, s, a.partial, a.scratch,
                           a.W, 1, a.nfft, rpg);
        a.partial = a.scratch;
        a.W = groups;
    }
    if (a.nch == 1 && a.W >= 64 && (a.nfft % 16) == 0) {
        // 16 positions per block: 5.2 us for 512 rows of 4096 against 6.8 us with 32 (half as many blocks)
        hipLaunchKernelGGL((finalize_wide_kernel<16, 1>), dim3(a.nfft / 16, nstreams), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.nch == 4 && a.W >= 64 && (a.nfft % 16) == 0 && !a.accumulate && !a.out.db) {
        hipLaunchKernelGGL((finalize_wide_kernel<16, 4>), dim3(a.nfft / 16, nstreams), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.W > 2 * kReduceGroups && a.scratch && (a.nfft % 256) == 0) {
        const int rpg = (a.W + kReduceGroups - 1) / kReduceGroups;
        const dim3 g1(a.nfft / 256, kReduceGroups, nstreams * a.nch);
        hipLaunchKernelGGL(reduce_partials_kernel, g1, dim3(256), 0, s, a.partial, a.scratch, a.W, a.nch, a.nfft,
                           rpg);
        a.partial = a.scratch;
        a.W = kReduceGroups;
    }
    const dim3 grid((a.nfft + 31) / 32, nstreams);
    if (a.nch == 1) hipLaunchKernelGGL(finalize_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(finalize_kernel<4>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

__global__ void scale_kernel(const float *sum, float *out, int nfft, double scale, OutStage stage) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stage.nout) return;
    out[i] = psd_value(stage, finite_power((double)sum[in_bin(stage, nfft, i)] * scale));      // (the rule of store_psd)
}

hipError_t launch_scale(const float *sum, float *out, int nfft, double scale, const OutStage &stage, hipStream_t s) {
    hipLaunchKernelGGL(scale_kernel, dim3((stage.nout + 255) / 256), dim3(256), 0, s, sum, out, nfft, scale, stage);
    return hipGetLastError();
}

// Summed partials of the two-channel path (time-sharded form): sums = [sum|X|^2][sum|Y|^2][sum conj(X)Y re,im]
// in natural bin order -> scaled Pxx, Pyy, Pxy, Cxy with the plan's shift / trim.
__global__ void csd_scale_kernel(const float *sums, int nfft, double scale, OutStage stage, float *pxx, float *pyy, float *pxy,
                                 float *cxy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stage.nout) return;
    const int k = in_bin(stage, nfft, i);
    const double xx = sums[k], yy = sums[nfft + k], re = sums[2 * nfft + 2 * k], im = sums[2 * nfft + 2 * k + 1];
    csd_store(xx, yy, re, im, scale, (size_t)i, pxx, pyy, pxy, cxy);
}

hipError_t launch_csd_scale(const float *sums, int nfft, double scale, const OutStage &stage, float *pxx, float *pyy, float *pxy,
                            float *cxy, hipStream_t s) {
    hipLaunchKernelGGL(csd_scale_kernel, dim3((stage.nout + 255) / 256), dim3(256), 0, s, sums, nfft, scale, stage, pxx, pyy, pxy, cxy);
    return hipGetLastError();
}

// One thread per bin walks the rows in time order.
__global__ void rows_epilogue_kernel(float *rows, long long nrows, int nfft, float alpha, float kdb,
                                     float *iir_state, float *peak_state, int *peak_init, int do_iir, int do_peak) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nfft) return;
    float y = do_iir ? iir_state[k] : 0.f;
    const bool have_peak = do_peak && (*peak_init != 0);
    float pk = have_peak ? peak_state[k] : 0.f;
    for (long long r = 0; r < nrows; ++r) {
        float v = rows[(size_t)r * nfft + k];
        if (do_peak) pk = (have_peak || r > 0) ? peak_max(pk, v) : v;
        if (do_iir) {
            y = fmaf(alpha, v, (1.0f - alpha) * y);
            rows[(size_t)r * nfft + k] = 10.0f * log10f(y) + kdb;
        }
    }
    if (do_iir) iir_state[k] = y;
    if (do_peak && nrows > 0) peak_state[k] = pk;
}

__global__ void set_flag_kernel(int *flag, int v) { *flag = v; }

// ---- closing a fused chain launch (segfft.hip) ------------------------------------------------------------
// The launch leaves W per-team accumulator rows (natural bin order): weighted sums for the IIR form, maxima for
// peak hold - about 12.6 MB at every transform size (48 / 24 / 12 / 6 / 3 teams per CU x 256 CUs rows of nfft floats).
// They become the new IIR / peak state (kept in ROW order, i.e. after the optional fftshift), and the raw rows the
// launch stored for the caller go through the last steps of the recursion in time order.
//   acc_mode 1  y = (1-alpha)^nbase y0 + alpha sum_w partial[w][k];  per raw row: y = alpha x + (1-alpha) y,
//               rows_out = 10 log10(y) + kdb      (single_pole_iir_filter_ff + nlog10_ff, local_worker.py:66-69)
//   acc_mode 2  peak = max(state, max_w partial[w][k])                (psd_logger.py:85); rows were written raw
// Two launches, both wide (the one-launch form of round 2 walked all W rows in nfft / 256 workgroups: 174-3313 us):
//   chain_reduce_kernel   grid (nfft / 256, G): group g of the rows -> scratch[g][nfft]; 256 threads = 64 float4
//                         columns x 4 row lanes; sums in double, fixed order
//   chain_state_kernel    grid nfft / 16: the G group rows (or the W rows themselves when there are few) -> state,
//                         16 positions x 64 row slices per block like finalize_wide_kernel, then the raw rows
// 5 + 5 us, each at the floor of a small kernel.  Tried and dropped: ONE launch in which the last block of a column
// block to finish reduces the group rows - with __threadfence() it took 60 us (an agent-scope release / acquire
// writes back / invalidates the XCD's whole L2 from each of ~1000 workgroups), with agent-scope atomic stores / loads
// for the group rows instead of fences 10-20 us.
template <bool MAX>
__global__ __launch_bounds__(256) void chain_reduce_kernel(const float *partial, float *scratch, int W, int nfft, int rows_per_group) {
    __shared__ double red[3][64][4];
    const int q = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + q) * 4;
    const int g = blockIdx.y;
    const int w0 = g * rows_per_group, w1 = min(W, w0 + rows_per_group);
    const float *base = partial + col;
    if constexpr (MAX) {      // peak hold: the maximum of the bit patterns (peak_max, fft_lds.hip.h: a NaN stays)
        unsigned(*redu)[64][4] = reinterpret_cast<unsigned(*)[64][4]>(red);
        uint4 m = make_uint4(0u, 0u, 0u, 0u);
        for (int w = w0 + j; w < w1; w += 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(base + (size_t)w * nfft);
            m.x = peak_max(m.x, v.x), m.y = peak_max(m.y, v.y), m.z = peak_max(m.z, v.z), m.w = peak_max(m.w, v.w);
        }
        if (j) redu[j - 1][q][0] = m.x, redu[j - 1][q][1] = m.y, redu[j - 1][q][2] = m.z, redu[j - 1][q][3] = m.w;
        __syncthreads();
        if (j) return;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            m.x = peak_max(m.x, redu[r][q][0]), m.y = peak_max(m.y, redu[r][q][1]), m.z = peak_max(m.z, redu[r][q][2]),
            m.w = peak_max(m.w, redu[r][q][3]);
        *reinterpret_cast<uint4 *>(scratch + (size_t)g * nfft + col) = m;
        return;
    }
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int w = w0 + j; w < w1; w += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(base + (size_t)w * nfft);
        s0 += v.x, s1 += v.y, s2 += v.z, s3 += v.w;
    }
    if (j) {
        red[j - 1][q][0] = s0;
        red[j - 1][q][1] = s1;
        red[j - 1][q][2] = s2;
        red[j - 1][q][3] = s3;
    }
    __syncthreads();
    if (j) return;
#pragma unroll
    for (int r = 0; r < 3; ++r) s0 += red[r][q][0], s1 += red[r][q][1], s2 += red[r][q][2], s3 += red[r][q][3];
    *reinterpret_cast<float4 *>(scratch + (size_t)g * nfft + col) = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
}

struct ChainStateArgs {
    const float *rows;      // [nrows][nfft] group rows (or the team rows); bin order by `layout` (bin_pos)
    int nrows, nfft, fftshift, acc_mode;
    RowLayout layout;
    long long nbase;
    double decay;           // (1 - alpha)^nbase, computed on the host (a device pow() in double is a long routine)
    float alpha, kdb;
    float *iir_state, *peak_state;
    const float *raw_rows;  // [nraw][nfft] row order
    long long nraw;         // rows taken through the recursion here (0 when chain_rows_kernel follows)
    float *rows_out;
};

__global__ __launch_bounds__(256) void chain_state_kernel(ChainStateArgs a) {
    constexpr int POS = 16, COLS = POS / 4, SLICES = 256 / COLS;
    __shared__ double red[SLICES][POS + 1];
    const int col = threadIdx.x % COLS, slice = threadIdx.x / COLS;
    const float *base = a.rows + blockIdx.x * POS + col * 4;
    if (a.acc_mode == 2) {      // peak hold (launch-uniform): the maximum of the bit patterns, a NaN stays (peak_max)
        unsigned(*redu)[POS + 1] = reinterpret_cast<unsigned(*)[POS + 1]>(red);
        uint4 m = make_uint4(0u, 0u, 0u, 0u);
        for (int w = slice; w < a.nrows; w += SLICES) {
            const uint4 v = *reinterpret_cast<const uint4 *>(base + (size_t)w * a.nfft);
            m.x = peak_max(m.x, v.x), m.y = peak_max(m.y, v.y), m.z = peak_max(m.z, v.z), m.w = peak_max(m.w, v.w);
        }
        redu[slice][col * 4] = m.x;
        redu[slice][col * 4 + 1] = m.y;
        redu[slice][col * 4 + 2] = m.z;
        redu[slice][col * 4 + 3] = m.w;
        __syncthreads();
        if (threadIdx.x >= POS) return;
        const int k = bin_pos(blockIdx.x * POS + threadIdx.x, a.layout);
        const int i = a.fftshift ? shifted(k, a.nfft) : k;
        unsigned t = 0u;
        for (int q = 0; q < SLICES; ++q) t = peak_max(t, redu[q][threadIdx.x]);
        // |X| and |X|^2 are >= 0 or NaN and the state starts at 0: no "initialised" flag needed
        a.peak_state[i] = peak_max(__builtin_bit_cast(float, t), a.peak_state[i]);
        return;
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int w = slice; w < a.nrows; w += SLICES) {
        const float4 v = *reinterpret_cast<const float4 *>(base + (size_t)w * a.nfft);
        s0 += v.x, s1 += v.y, s2 += v.z, s3 += v.w;
    }
    red[slice][col * 4] = s0;
    red[slice][col * 4 + 1] = s1;
    red[slice][col * 4 + 2] = s2;
    red[slice][col * 4 + 3] = s3;
    __syncthreads();
    if (threadIdx.x >= POS) return;
    const int k = bin_pos(blockIdx.x * POS + threadIdx.x, a.layout);                // bin held at this position of a row
    const int i = a.fftshift ? shifted(k, a.nfft) : k;                              // row position
    double t = 0.0;
    for (int q = 0; q < SLICES; ++q) t += red[q][threadIdx.x];
    float y = a.iir_state[i];
    if (a.nbase > 0) y = (float)((double)y * a.decay + (double)a.alpha * t);
    for (long long r = 0; r < a.nraw; ++r) {
        y = fmaf(a.alpha, a.raw_rows[(size_t)r * a.nfft + i], (1.0f - a.alpha) * y);
        a.rows_out[(size_t)r * a.nfft + i] = 10.0f * log10f(y) + a.kdb;
    }
    a.iir_state[i] = y;
}

// many raw rows (a caller that wants more than the latest few): one thread per row position walks them in time order
__global__ __launch_bounds__(64) void chain_rows_kernel(int nfft, float alpha, float kdb, float *iir_state, const float *raw_rows,
                                                        long long nraw, float *rows_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= nfft) return;
    float y = iir_state[i];
    for (long long r = 0; r < nraw; ++r) {
        y = fmaf(alpha, raw_rows[(size_t)r * nfft + i], (1.0f - alpha) * y);
        rows_out[(size_t)r * nfft + i] = 10.0f * log10f(y) + kdb;
    }
    iir_state[i] = y;
}

// rows of scratch the two-launch form needs for W team rows (0: the state kernel reads the team rows directly)
int chain_tail_groups(int W, int nfft) {
    if (W <= 128) return 0;
    // 8192 / 16384 points: the state kernel alone has 512 / 1024 workgroups and 8 / 4 team rows per thread - one launch
    // instead of two (same-box A/B: -0.5 ... -1 % of the push; at 2048 / 4096 points the direct form is 1.4-4 % SLOWER)
    if (nfft >= 8192 && W <= 1536) return 0;
    // ~12 rows per group gives nfft / 256 x G ~ 1024 workgroups at every size; at most 256 groups, so that the state
    // kernel (nfft / 16 workgroups) never walks more than four rows per thread
    int g = (W + 11) / 12;
    const int gmax = nfft >= 1024 ? 1024 * 256 / nfft : 256;
    if (g > gmax) g = gmax;
    return g < 1 ? 1 : g;
}

hipError_t launch_chain_tail(const float *partial, float *scratch, int W, int nfft, RowLayout layout, int fftshift, int acc_mode, long long nbase,
                             float alpha, float kdb, float *iir_state, float *peak_state, const float *raw_rows,
                             long long nraw, float *rows_out, hipStream_t s) {
    ChainStateArgs a;
    a.rows = partial;
    a.nrows = W;
    const int G = scratch ? chain_tail_groups(W, nfft) : 0;
    if (G) {
        const int rpg = (W + G - 1) / G;
        const dim3 grid(nfft / 256, G);
        if (acc_mode == 2) hipLaunchKernelGGL(chain_reduce_kernel<true>, grid, dim3(256), 0, s, partial, scratch, W, nfft, rpg);
        else hipLaunchKernelGGL(chain_reduce_kernel<false>, grid, dim3(256), 0, s, partial, scratch, W, nfft, rpg);
        a.rows = scratch;
        a.nrows = G;
    }
    const bool rows_apart = acc_mode == 1 && nraw > 8;
    a.nfft = nfft;
    a.layout = layout;
    a.fftshift = fftshift;
    a.acc_mode = acc_mode;
    a.nbase = nbase;
    a.decay = nbase > 0 ? pow(1.0 - (double)alpha, (double)nbase) : 1.0;
    a.alpha = alpha;
    a.kdb = kdb;
    a.iir_state = iir_state;
    a.peak_state = peak_state;
    a.raw_rows = raw_rows;
    a.nraw = (acc_mode == 1 && !rows_apart) ? nraw : 0;
    a.rows_out = rows_out;
    hipLaunchKernelGGL(chain_state_kernel, dim3(nfft / 16), dim3(256), 0, s, a);
    if (rows_apart)
        hipLaunchKernelGGL(chain_rows_kernel, dim3((nfft + 63) / 64), dim3(64), 0, s, nfft, alpha, kdb, iir_state, raw_rows, nraw,
                           rows_out);
    return hipGetLastError();
}

hipError_t launch_set_flag(int *flag, int v, hipStream_t s) {
    hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1), 0, s, flag, v);
    return hipGetLastError();
}

hipError_t launch_rows_epilogue(float *rows, long long nrows, int nfft, float alpha, float kdb, float *iir_state,
                                float *peak_state, int *peak_init, int do_iir, int do_peak, hipStream_t s) {
    hipLaunchKernelGGL(rows_epilogue_kernel, dim3((nfft + 255) / 256), dim3(256), 0, s, rows, nrows, nfft, alpha,
                       kdb, iir_state, peak_state, peak_init, do_iir, do_peak);
    if (do_peak && nrows > 0) hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1), 0, s, peak_init, 1);
    return hipGetLastError();
}

__global__ void group_mean_kernel(const float *rows, long long ngroups, int nfft, int group, float *out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const long long g = blockIdx.y;
    if (k >= nfft || g >= ngroups) return;
    double s = 0.0;
    for (int r = 0; r < group; ++r) s += (double)rows[((size_t)g * group + r) * nfft + k];
    out[(size_t)g * nfft + k] = (float)(s / group);
}

hipError_t launch_group_mean(const float *rows, long long ngroups, int nfft, int group, float *out, hipStream_t s) {
    hipLaunchKernelGGL(group_mean_kernel, dim3((nfft + 255) / 256, (unsigned)ngroups), dim3(256), 0, s, rows,
                       ngroups, nfft, group, out);
    return hipGetLastError();
}

// min() that keeps a NaN, as numpy's min / amin do (fminf drops it): the noise floor of a row with a NaN bin is NaN
// and its mask all zero, like the reference's movingaverage(...).min()
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || a < b) ? a : b; }

// movingaverage(): np.convolve(psd, ones(M)/sb, 'same'), M = int(sb):
// same[i] = (1/sb) * sum_{j<M} psd[i + (M-1)/2 - j]  (terms outside [0,N) dropped), then abs.
// blockIdx.y = PSD row (batched scanner: one row per channel stream).
__global__ void movavg_kernel(const float *psd, int nfft, double srch_bins, double *movavg, float *movavg_f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nfft) return;
    const size_t row = (size_t)blockIdx.y * nfft;
    const int M = (int)srch_bins;
    const int top = i + (M - 1) / 2;
    double s = 0.0;
    for (int j = 0; j < M; ++j) {
        const int n = top - j;
        if (n >= 0 && n < nfft) s += (double)psd[row + n];
    }
    s = fabs(s / srch_bins);
    movavg[row + i] = s;
    if (movavg_f) movavg_f[row + i] = (float)s;
}

__global__ void channel_sum_kernel(const double *movavg, int nfft, int nch, const int *lo, const int *hi, float *power) {
    const int c = blockIdx.x;
    const double *row = movavg + (size_t)blockIdx.y * nfft;
    double s = 0.0;
    for (int i = lo[c] + threadIdx.x; i < hi[c]; i += 64) s += row[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) power[(size_t)blockIdx.y * nch + c] = (float)s;
}

hipError_t launch_channel_power(const float *psd, int nrows, int nfft, double srch_bins, int nch, const int *lo,
                                const int *hi, double *movavg, float *power, float *movavg_f, hipStream_t s) {
    hipLaunchKernelGGL(movavg_kernel, dim3((nfft + 255) / 256, nrows), dim3(256), 0, s, psd, nfft, srch_bins, movavg,
                       movavg_f);
    hipLaunchKernelGGL(channel_sum_kernel, dim3(nch, nrows), dim3(64), 0, s, movavg, nfft, nch, lo, hi, power);
    return hipGetLastError();
}

// Per-bin threshold: one workgroup per PSD row; noise = min over bins of the moving average.
__global__ __launch_bounds__(256) void bin_threshold_kernel(const float *psd, int nfft, double srch_bins, float thr,
                                                            unsigned char *mask, float *noise_out) {
    __shared__ float red[4];
    const float *row = psd + (size_t)blockIdx.x * nfft;
    const int M = (int)srch_bins;
    float mn = INFINITY;
    for (int i = threadIdx.x; i < nfft; i += 256) {
        const int top = i + (M - 1) / 2;
        double s = 0.0;
        for (int j = 0; j < M; ++j) {
            const int n = top - j;
            if (n >= 0 && n < nfft) s += (double)row[n];
        }
        mn = nan_min(mn, (float)fabs(s / srch_bins));
    }
    // (spelled out: through wave_reduce() of fft_lds.hip.h this kernel comes out with other registers)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = nan_min(mn, __shfl_xor(mn, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
    __syncthreads();
    const float noise = nan_min(nan_min(red[0], red[1]), nan_min(red[2], red[3]));
    if (threadIdx.x == 0 && noise_out) noise_out[blockIdx.x] = noise;
    const float level = noise * thr;
    for (int i = threadIdx.x; i < nfft; i += 256) mask[(size_t)blockIdx.x * nfft + i] = row[i] > level ? 1 : 0;
}

// Same decision from an already computed moving average (the batched decision stage runs movavg_kernel once for the
// channel sums and the noise floor): noise = min_k movavg[k], mask[k] = psd[k] > thr * noise.
__global__ __launch_bounds__(256) void bin_threshold_ma_kernel(const float *psd, const double *movavg, int nfft, float thr,
                                                               unsigned char *mask, float *noise_out) {
    __shared__ float red[4];
    const float *row = psd + (size_t)blockIdx.x * nfft;
    const double *ma = movavg + (size_t)blockIdx.x * nfft;
    float mn = INFINITY;
    for (int i = threadIdx.x; i < nfft; i += 256) mn = nan_min(mn, (float)ma[i]);
    // (spelled out: through wave_reduce() of fft_lds.hip.h this kernel comes out with other registers)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = nan_min(mn, __shfl_xor(mn, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
    __syncthreads();
    const float noise = nan_min(nan_min(red[0], red[1]), nan_min(red[2], red[3]));
    if (threadIdx.x == 0 && noise_out) noise_out[blockIdx.x] = noise;
    if (!mask) return;
    const float level = noise * thr;
    for (int i = threadIdx.x; i < nfft; i += 256) mask[(size_t)blockIdx.x * nfft + i] = row[i] > level ? 1 : 0;
}

// ---- decision stage of the batched scanner, many rows (oth_scan_decide_dev*) ------------------------------------------
// movingaverage (ofdm_cr_tools.py:168-170) as a SLIDING sum: a thread forms the M-tap sum of its first output directly
// and moves on by + x[in] - x[out] for the others of its run; a dozen adds per output instead of M = 163 at config 5's search
// bandwidth.  A double sum of M float32 values is EXACT - and the sliding sum then IS the direct one - while the taps of
// a window span less than 2^(28 - log2 M) in magnitude (62 dB of power at M = 163).  Beyond that every add / subtract
// of a large tap rounds at 2^-53 of it, and what a strong carrier leaves behind when it slides out of the window stays in
// the sum for the rest of the run: at most 2 (kMaRun - 1) 2^-53 max|tap| - which matters exactly where the row's noise
// floor (its minimum, the most sensitive output) sits right next to a carrier more than ~90 dB above it.  So the run
// keeps the largest tap it has seen and forms an output directly again whenever the sliding sum has fallen below
// 2^-24 of it (advisor, round 4): the result then never differs from the direct sum by more than 2^-24 relative.  The row minimum (the noise floor of
// spectrum_sensor_v2.py:465-467, per row) is taken on the way: every block leaves the minimum of its tile in
// tile_min[row][tile], and scan_post_kernel takes the minimum of a row's few tiles (round 4: an atomicMin on a word the
// launcher had to preset cost a fill launch per call).
// The 4096 + M - 1 inputs of a block's 4096 outputs are staged in LDS first (coalesced; one pad word per 16 so that
// the per-thread runs, 16 apart, fall into different banks): the taps then cost LDS reads, not dependent global loads
// (35 us -> 5 us for 64 rows of 16384 at M = 163).
// kMaRun outputs per thread: 8.9 us for config 5's 64 rows of 16384 against 11.2 at 16 and 15.4 at 32 (tile 4096; tiles of
// 1024 / 2048 at 4-16 per thread: 7.8-10.3 us - the kernel is a latency chain, tools/archive/decide_probe.py)
constexpr int kMaTile = 4096, kMaRun = 8, kMaMaxM = 1024, kMaThreads = kMaTile / kMaRun;
// movavg_run_kernel holds 67.6 KB of STATIC LDS: more than the 64 KB a workgroup may have on every target but gfx950
// (160 KB per CU) - this library is built for gfx950 only (Makefile ARCH); a change of --offload-arch must shrink the tile
static_assert((kMaTile + kMaMaxM) * 5 / 4 * sizeof(float) + (kMaTile * 9 / 8) * sizeof(double) <= 160 * 1024, "movavg_run_kernel's LDS");
__device__ __forceinline__ int ma_pad(int k) { return k + k / kMaRun; }      // one pad word per run: a thread stride of kMaRun + 1 words
__global__ __launch_bounds__(kMaThreads) void movavg_run_kernel(const float *psd, int nfft, double srch_bins, double *movavg,
                                                         float *tile_min) {
    __shared__ float xs[(kMaTile + kMaMaxM) + (kMaTile + kMaMaxM) / kMaRun + 1];
    __shared__ double ys[kMaTile + kMaTile / kMaRun];      // the outputs, written back coalesced (a thread's own run of 16
                                                       // doubles is 64 different cache lines per store instruction)
    __shared__ float red[kMaThreads / 64];
    // sums / largest magnitudes of the staged inputs in blocks of kMaRun (round 5): a thread's run starts on a block
    // boundary, so its first M-tap sum is M / kMaRun block sums + M % kMaRun taps - 23 LDS reads at M = 163 where the
    // tap-by-tap sum made 163 in 21 dependent trips (measured: no faster by itself - the kernel's 9-11 us are launch,
    // staging and write-back latency, see kMaRun).  A double sum of float32 taps is exact over the same range as before, so the order in
    // which it is formed does not show.
    constexpr int kMaBlocks = (kMaTile + kMaMaxM) / kMaRun + 1;
    __shared__ double bsum[kMaBlocks];
    __shared__ float bmax[kMaBlocks];
    const float *x = psd + (size_t)blockIdx.y * nfft;
    double *out = movavg + (size_t)blockIdx.y * nfft;
    const int M = (int)srch_bins, half = (M - 1) / 2;
    const double inv = 1.0 / srch_bins;      // np.convolve(x, ones(M) / sb): the taps are 1 / sb there too; 16 double divisions less
    const int base = blockIdx.x * kMaTile;
    const int lo = base + half - M + 1, count = kMaTile + M - 1;      // inputs n = lo + k, k in [0, count)
    for (int k0 = threadIdx.x; k0 < count; k0 += 8 * kMaThreads) {          // eight independent loads per thread and trip
        float a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int n = lo + k0 + kMaThreads * u;
            a[u] = (k0 + kMaThreads * u < count && n >= 0 && n < nfft) ? x[n] : 0.f;      // out-of-range taps are skipped = add 0
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + kMaThreads * u < count) xs[ma_pad(k0 + kMaThreads * u)] = a[u];
    }
    __syncthreads();
    for (int b = threadIdx.x; b * kMaRun < count; b += kMaThreads) {      // taps behind `count` were never staged: skip them
        float a[kMaRun];
#pragma unroll
        for (int u = 0; u < kMaRun; ++u) a[u] = (b * kMaRun + u < count) ? xs[ma_pad(b * kMaRun + u)] : 0.f;
        double d = 0.0;
        float m = 0.f;
#pragma unroll
        for (int u = 0; u < kMaRun; u += 4) {
            d += ((double)a[u] + a[u + 1]) + ((double)a[u + 2] + a[u + 3]);
            m = fmaxf(fmaxf(m, fmaxf(fabsf(a[u]), fabsf(a[u + 1]))), fmaxf(fabsf(a[u + 2]), fabsf(a[u + 3])));
        }
        bsum[b] = d;
        bmax[b] = m;
    }
    __syncthreads();
    const int t0 = threadIdx.x * kMaRun, i0 = base + t0;              // output i0 + r takes xs[t0 + r .. t0 + r + M - 1]
    float mn = INFINITY;
    if (i0 < nfft) {
        double s = 0.0;
        float big = 0.f;                  // largest |tap| this run has added so far
        auto direct = [&](int first) {    // M-tap sum of xs[first ..]: eight independent LDS reads per trip (one read per
            double d = 0.0;               // trip waited ~100 cycles each)
            int jj = 0;
            for (; jj + 8 <= M; jj += 8) {
                float a[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] = xs[ma_pad(first + jj + u)];
#pragma unroll
                for (int u = 0; u < 8; ++u) big = fmaxf(big, fabsf(a[u]));
                d += (((double)a[0] + a[1]) + ((double)a[2] + a[3])) + (((double)a[4] + a[5]) + ((double)a[6] + a[7]));
            }
            for (; jj < M; ++jj) {
                const float a = xs[ma_pad(first + jj)];
                big = fmaxf(big, fabsf(a));
                d += (double)a;
            }
            return d;
        };
        {   // the run's first output from the block sums (the lambda above serves the rare re-start in mid-run)
            const int nb = M / kMaRun;
            for (int b = 0; b < nb; ++b) {
                s += bsum[threadIdx.x + b];
                big = fmaxf(big, bmax[threadIdx.x + b]);
            }
            for (int jj = nb * kMaRun; jj < M; ++jj) {
                const float a = xs[ma_pad(t0 + jj)];
                big = fmaxf(big, fabsf(a));
                s += (double)a;
            }
        }
        double v = fabs(s * inv);
        ys[ma_pad(t0)] = v;
        mn = (float)v;
        // the taps that enter and leave over the run, read in one batch: inside the loop each pair of LDS reads was waited
        // for on its own (the re-start branch keeps the compiler from moving them up), ~500 cycles per output
        float tin[kMaRun], tout[kMaRun];
#pragma unroll
        for (int r = 1; r < kMaRun; ++r) {
            tin[r] = xs[ma_pad(t0 + r + M - 1)];
            tout[r] = xs[ma_pad(t0 + r - 1)];
        }
#pragma unroll
        for (int r = 1; r < kMaRun; ++r) {
            const float in = tin[r];
            big = fmaxf(big, fabsf(in));
            s += (double)in;
            s -= (double)tout[r];
            // a carrier > 2^24 x the window's content has just left - or the sum is not finite: an inf / NaN tap stays in a
            // sliding sum (inf - inf) after it has left the window, in a direct sum it leaves with its window, as in
            // np.convolve
            if (!(fabs(s) >= (double)big * (1.0 / 16777216.0))) {
                big = 0.f;
                s = direct(t0 + r);
            }
            v = fabs(s * inv);
            ys[ma_pad(t0 + r)] = v;
            if (i0 + r < nfft) mn = nan_min(mn, (float)v);        // (a cut last run: ys[] behind the row's end is never
        }                                                          // copied out)
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kMaTile && base + k < nfft; k += kMaThreads) out[base + k] = ys[ma_pad(k)];
    // (spelled out: through wave_reduce() of fft_lds.hip.h this kernel comes out with other registers)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = nan_min(mn, __shfl_xor(mn, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = red[0];
#pragma unroll
        for (int w = 1; w < kMaThreads / 64; ++w) m = nan_min(m, red[w]);
        tile_min[blockIdx.y * gridDim.x + blockIdx.x] = m;
    }
}

// What follows the moving average, one launch (round 4: mask and channel sums were two, behind a fill): the row's noise
// floor = the minimum of its tile minima; blocks [0, nmb) write mask[k] = psd[k] > thr * noise for 1024 bins each (the
// one-workgroup-per-row form left 192 of 256 CUs idle at 64 rows), blocks behind them take four channel slices each,
// one wave per slice (ofdm_cr_tools.py:232-249: sums of the moving average over [lo, hi)).
__global__ __launch_bounds__(256) void scan_post_kernel(const float *psd, const double *movavg, const float *tile_min,
                                                        int ntiles, int nfft, float thr, int nmb, int nch, const int *lo,
                                                        const int *hi, unsigned char *mask, float *noise, float *power) {
    float floor_ = tile_min[blockIdx.y * ntiles];
    for (int k = 1; k < ntiles; ++k) floor_ = nan_min(floor_, tile_min[blockIdx.y * ntiles + k]);
    if (blockIdx.x == 0 && threadIdx.x == 0) noise[blockIdx.y] = floor_;
    if ((int)blockIdx.x < nmb) {
        if (!mask) return;
        const size_t row = (size_t)blockIdx.y * nfft;
        const float level = floor_ * thr;
        const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
        if (i + 3 < nfft) {
            const float4 v = *reinterpret_cast<const float4 *>(psd + row + i);
            uchar4 m;
            m.x = v.x > level ? 1 : 0;
            m.y = v.y > level ? 1 : 0;
            m.z = v.z > level ? 1 : 0;
            m.w = v.w > level ? 1 : 0;
            *reinterpret_cast<uchar4 *>(mask + row + i) = m;
        } else {
            for (int k = i; k < nfft; ++k) mask[row + k] = psd[row + k] > level ? 1 : 0;
        }
        return;
    }
    const int c = ((int)blockIdx.x - nmb) * 4 + (threadIdx.x >> 6);
    if (c >= nch) return;
    const double *row = movavg + (size_t)blockIdx.y * nfft;
    double s = 0.0;
    for (int i = lo[c] + (threadIdx.x & 63); i < hi[c]; i += 64) s += row[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) power[(size_t)blockIdx.y * nch + c] = (float)s;
}

int scan_decide_tiles(int nfft) { return (nfft + kMaTile - 1) / kMaTile; }

// Two doors: the tiled run kernels above take rows of a multiple of four bins at 16-byte aligned addresses (float4 /
// uchar4 mask stores) with int(srch_bins) <= kMaMaxM (the halo in LDS); every other call takes the direct form
// (movavg_kernel, channel_sum_kernel, bin_threshold_ma_kernel).  Both compute the same thing.
hipError_t launch_scan_decide(const float *psd, int nrows, int nfft, double srch_bins, float thr, int nch, const int *lo,
                              const int *hi, double *movavg, float *tile_min, unsigned char *mask, float *noise, float *power,
                              hipStream_t s) {
    if ((nfft & 3) == 0 && (reinterpret_cast<uintptr_t>(psd) & 15) == 0 && (!mask || (reinterpret_cast<uintptr_t>(mask) & 3) == 0) &&
        (int)srch_bins <= kMaMaxM) {
        const int ntiles = scan_decide_tiles(nfft), nmb = (nfft + 1023) / 1024, ncb = (nch > 0 && power) ? (nch + 3) / 4 : 0;
        hipLaunchKernelGGL(movavg_run_kernel, dim3(ntiles, nrows), dim3(kMaThreads), 0, s, psd, nfft, srch_bins, movavg, tile_min);
        hipLaunchKernelGGL(scan_post_kernel, dim3(nmb + ncb, nrows), dim3(256), 0, s, psd, movavg, tile_min, ntiles, nfft, thr,
                           nmb, ncb ? nch : 0, lo, hi, mask, noise, power);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(movavg_kernel, dim3((nfft + 255) / 256, nrows), dim3(256), 0, s, psd, nfft, srch_bins, movavg,
                       (float *)nullptr);
    if (nch > 0 && power)
        hipLaunchKernelGGL(channel_sum_kernel, dim3(nch, nrows), dim3(64), 0, s, movavg, nfft, nch, lo, hi, power);
    hipLaunchKernelGGL(bin_threshold_ma_kernel, dim3(nrows), dim3(256), 0, s, psd, movavg, nfft, thr, mask, noise);
    return hipGetLastError();
}

hipError_t launch_bin_threshold(const float *psd, int nrows, int nfft, double srch_bins, float thr,
                                unsigned char *mask, float *noise, hipStream_t s) {
    hipLaunchKernelGGL(bin_threshold_kernel, dim3(nrows), dim3(256), 0, s, psd, nfft, srch_bins, thr, mask, noise);
    return hipGetLastError();
}

// ---- synthetic IQ -----------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct ToneSet {
    float amp[8];
    float freq[8];
    int n;
};

__global__ void synth_kernel(float2 *iq, size_t n, uint64_t seed, ToneSet tones, float dc_re, float dc_im) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t h = splitmix64(seed * 0xD1342543DE82EF95ull + i);
        const float u1 = ((uint32_t)(h >> 40) + 1) * (1.0f / 16777216.0f);   // (0, 1]
        const float u2 = (uint32_t)(h & 0xFFFFFF) * (1.0f / 16777216.0f);    // [0, 1)
        // unit-power complex Gaussian: sqrt(-ln u1) * exp(2 pi i u2)
        const float r = sqrtf(-logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);
        double re = r * cs + dc_re, im = r * sn + dc_im;
        for (int t = 0; t < tones.n; ++t) {
            double ph = (double)tones.freq[t] * (double)i;
            ph -= floor(ph);
            double s, c;
            sincospi(2.0 * ph, &s, &c);
            re += tones.amp[t] * c;
            im += tones.amp[t] * s;
        }
        iq[i] = make_float2((float)re, (float)im);
    }
}

hipError_t launch_synth(float2 *iq, size_t n, uint64_t seed, int ntones, const float *amp, const float *freq,
                        float dc_re, float dc_im, hipStream_t s) {
    ToneSet t;
    t.n = ntones > 8 ? 8 : ntones;
    for (int i = 0; i < t.n; ++i) {
        t.amp[i] = amp[i];
        t.freq[i] = freq[i];
    }
    hipLaunchKernelGGL(synth_kernel, dim3(4096), dim3(256), 0, s, iq, n, seed, t, dc_re, dc_im);
    return hipGetLastError();
}

// ---- probes -----------------------------------------------------------------
// Streaming-read probe (the second roofline denominator): every workgroup walks contiguous 32 KiB tiles, eight
// non-temporal 16-byte loads in flight per thread - the shape that reads fastest on this part
// (tools/ubench/read_peak.hip: 7.1 TB/s; grid-stride loads 5.5-6.2, the same tiles without the non-temporal hint 6.3).
__global__ __launch_bounds__(256) void read_probe_kernel(const float4 *p, size_t n4, float *sink) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = 8;
    const size_t tile = 256 * U, ntiles = n4 / tile;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const f4 *q = reinterpret_cast<const f4 *>(p) + t * tile + threadIdx.x;
        f4 v[U];
#pragma unroll
        for (int j = 0; j < U; ++j) v[j] = __builtin_nontemporal_load(q + 256 * j);
#pragma unroll
        for (int j = 0; j < U; ++j) acc += v[j];
    }
    for (size_t i = ntiles * tile + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 a = p[i];
        acc += f4{a.x, a.y, a.z, a.w};
    }
    const float v = acc.x + acc.y + acc.z + acc.w;
    if (v == 1.2345e-30f) sink[0] = v;   // keeps the loads alive, practically never stores
}

// the same stream read 8 bytes per lane (global_load_dwordx2, the access width of the FFT kernels' sample loads)
__global__ __launch_bounds__(256) void read_probe8_kernel(const float2 *p, size_t n2, float *sink) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 acc = {0.f, 0.f};
    constexpr int U = 16;
    const size_t tile = 256 * U, ntiles = n2 / tile;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const f2 *q = reinterpret_cast<const f2 *>(p) + t * tile + threadIdx.x;
        f2 v[U];
#pragma unroll
        for (int j = 0; j < U; ++j) v[j] = __builtin_nontemporal_load(q + 256 * j);
#pragma unroll
        for (int j = 0; j < U; ++j) acc += v[j];
    }
    for (size_t i = ntiles * tile + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        acc.x += p[i].x;
        acc.y += p[i].y;
    }
    const float v = acc.x + acc.y;
    if (v == 1.2345e-30f) sink[0] = v;
}

hipError_t launch_read_probe8(const void *p, size_t bytes, float *sink, hipStream_t s) {
    hipLaunchKernelGGL(read_probe8_kernel, dim3(256 * 16), dim3(256), 0, s, (const float2 *)p, bytes / 8, sink);
    return hipGetLastError();
}

hipError_t launch_read_probe(const void *p, size_t bytes, float *sink, hipStream_t s) {
    hipLaunchKernelGGL(read_probe_kernel, dim3(256 * 8), dim3(256), 0, s, (const float4 *)p, bytes / 16, sink);
    return hipGetLastError();
}

__global__ void iq_power_kernel(const float2 *iq, size_t n, double *acc4) {
    double sr = 0, si = 0, sp = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float2 v = iq[i];
        sr += v.x;
        si += v.y;
        sp += (double)v.x * v.x + (double)v.y * v.y;
    }
    // (spelled out: through wave_sum() of fft_lds.hip.h this kernel comes out with other registers)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sr += __shfl_xor(sr, off, 64);
        si += __shfl_xor(si, off, 64);
        sp += __shfl_xor(sp, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&acc4[0], sr);
        atomicAdd(&acc4[1], si);
        atomicAdd(&acc4[2], sp);
    }
}

// Pilot of the constant detrend (WelchArgs.pilot): per stream (and per channel of a pair) the means of kPilotProbes
// segments spread evenly over the launch - segment (nseg - 1) k / 7 for probe k; load_pilot() averages them, so the pilot
// is near the stream's mean also when the stream opens with a transient or its offset drifts.  One 1024-thread block
// per probe, double accumulation, four independent loads per thread and trip (at nperseg = 4096 every load of the block
// is in flight at once).  Its value only has to be NEAR the mean: any constant comes off exactly.
__global__ __launch_bounds__(1024) void pilot_mean_kernel(const float2 *x, const float2 *y, size_t stream_stride, int n,
                                                          long long step, long long nseg, int nstreams, float2 *out) {
    __shared__ double red[2][16];
    const int probe = blockIdx.x % kPilotProbes, sc = blockIdx.x / kPilotProbes;
    const int stream = sc % nstreams, ch = sc / nstreams;
    const float2 *src = (ch ? y : x) + (size_t)stream * stream_stride + (size_t)(((nseg - 1) * probe) / (kPilotProbes - 1)) * step;
    double sr = 0.0, si = 0.0;
    for (int i = threadIdx.x; i < n; i += 4096) {
        float2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i + 1024 * k < n) ? src[i + 1024 * k] : make_float2(0.f, 0.f);
        sr += ((double)v[0].x + v[1].x) + ((double)v[2].x + v[3].x);
        si += ((double)v[0].y + v[1].y) + ((double)v[2].y + v[3].y);
    }
    // (spelled out: through wave_sum() of fft_lds.hip.h this kernel comes out with other registers)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sr += __shfl_xor(sr, off, 64);
        si += __shfl_xor(si, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sr;
        red[1][threadIdx.x >> 6] = si;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        sr = threadIdx.x < 16 ? red[0][threadIdx.x] : 0.0;
        si = threadIdx.x < 16 ? red[1][threadIdx.x] : 0.0;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            sr += __shfl_xor(sr, off, 64);
            si += __shfl_xor(si, off, 64);
        }
        if (threadIdx.x == 0) out[blockIdx.x] = make_float2((float)(sr / n), (float)(si / n));
    }
}

hipError_t launch_pilot_mean(const float2 *x, const float2 *y, size_t stream_stride, int n, long long step, long long nseg,
                             int nstreams, float2 *out, hipStream_t s) {
    hipLaunchKernelGGL(pilot_mean_kernel, dim3(nstreams * (y ? 2 : 1) * kPilotProbes), dim3(1024), 0, s, x, y, stream_stride,
                       n, step, nseg, nstreams, out);
    return hipGetLastError();
}

hipError_t launch_iq_power(const float2 *iq, size_t n, double *acc4, hipStream_t s) {
    hipLaunchKernelGGL(iq_power_kernel, dim3(2048), dim3(256), 0, s, iq, n, acc4);
    return hipGetLastError();
}

}  // namespace oth
