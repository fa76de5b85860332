// The output stage every finalize kernel shares - natural bin -> fftshift -> trim -> output slot (out_slot; in_bin the other
// way round), then sum * scale -> optional 10 log10 -> store or accumulate (psd_value, store_psd) - and the finalize stage of
// the per-bin statistics (ftest_, sk_, jack_, adapt_, cyc_, lag_ and mat_finalize_kernel): 256 threads = 32 consecutive bins x 8 slices
// of the workgroup axis.  Such a kernel maps its bin to the output slot, adds its R rows of the W workgroups' partial sums
// in double in a fixed order (slice_sums: a result depends on the launch shape only), and keeps for itself the statistic's
// own formula and its degenerate-bin rules.
#pragma once
#include "oth_internal.h"

namespace oth {

// np.fft.fftshift for any length: bin k lands at (k + n / 2) mod n (integer division: n odd included)
__device__ __forceinline__ int shifted(int k, int n) {
    const int p = k + n / 2;
    return p >= n ? p - n : p;
}
// ... and its inverse: the bin at shifted position ks
__device__ __forceinline__ int unshifted(int ks, int n) {
    const int p = ks + n - n / 2;
    return p >= n ? p - n : p;
}

// natural bin k -> index i into the output row under the plan's shift and trim; false: the bin is trimmed away (or past nfft)
__device__ __forceinline__ bool out_slot(const OutStage &o, int nfft, int k, int &i) {
    const int ks = o.fftshift ? shifted(k, nfft) : k;
    i = ks - o.trim;
    return k < nfft && i >= 0 && i < o.nout;
}
// ... and the natural bin that lands at index i < nout of the output row
__device__ __forceinline__ int in_bin(const OutStage &o, int nfft, int i) { return o.fftshift ? unshifted(i + o.trim, nfft) : i + o.trim; }

// a PSD value leaves linear, or as dB
__device__ __forceinline__ float psd_value(const OutStage &o, double v) { return o.db ? (float)(10.0 * log10(v)) : (float)v; }

// The one-channel rule for sums that are not finite (include/ofdm_tools_hip.h, oth_welch_exec; csd_store in kernels_misc.hip
// is its two-channel twin): a scaled power that float32 cannot hold - an inf or NaN sum, or one that overflows on the way
// out - leaves as NaN, linear or dB, never as inf.  An inf sample leaves NaN in every bin of SciPy's transform but inf in
// some bins of the register-butterfly kernels, and a float32 sum of |X|^2 that overflowed reads inf in every kernel.  It is
// applied here and not in psd_value, which the per-bin statistics share.  Zero stays zero (-inf in dB, numpy's 10 log10(0)).
__device__ __forceinline__ double finite_power(double v) { return isfinite((float)v) ? v : __builtin_nan(""); }

// a summed bin into slot o of `out` by FinalizeArgs.accumulate: 0 scaled, through finite_power and psd_value; 1 added raw to
// the running sums there (the streaming form); 2 stored raw, non-finite or not (the time-sharded sums)
__device__ __forceinline__ void store_psd(float *out, size_t o, double sum, double scale, int accumulate, const OutStage &stage) {
    if (accumulate == 1) out[o] += (float)sum;
    else if (accumulate) out[o] = (float)sum;
    else out[o] = psd_value(stage, finite_power(sum * scale));
}

// t[r] = sum over the W workgroups of load(w, r), r < R: slice `slice` adds w = slice, slice + 8, ... in double, then the
// first slice adds the eight slice sums 0 ... 7.  Every thread of the workgroup calls it; true in the threads that go on to
// write (first slice, live bin), which hold the sums.
template <int R, typename Load> __device__ __forceinline__ bool slice_sums(bool live, int W, Load load, double (&t)[R]) {
    __shared__ double red[R][8][32];
    const int lane = threadIdx.x & 31, slice = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < R; ++r) t[r] = 0.0;
    if (live) {
        for (int w = slice; w < W; w += 8)
#pragma unroll
            for (int r = 0; r < R; ++r) t[r] += (double)load(w, r);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) red[r][slice][lane] = t[r];
    __syncthreads();
    if (slice != 0 || !live) return false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        t[r] = 0.0;
        for (int q = 0; q < 8; ++q) t[r] += red[r][q][lane];
    }
    return true;
}

// one workgroup per 32 bins, stream and - where nz > 1 - z index
template <auto K, typename Args> hipError_t launch_stat_finalize(const Args &a, int nstreams, int nz, hipStream_t s) {
    const dim3 grid((a.nfft + 31) / 32, nstreams, nz);
    hipLaunchKernelGGL(K, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace oth
