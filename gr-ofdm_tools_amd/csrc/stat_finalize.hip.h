// The finalize stage the per-bin statistics share (ftest_, sk_, jack_, adapt_ and cyc_finalize_kernel): 256 threads = 32
// consecutive bins x 8 slices of the workgroup axis.  A kernel maps its bin to the output slot (out_slot), adds its R rows
// of the W workgroups' partial sums in double in a fixed order (slice_sums: a result depends on the launch shape only),
// and keeps for itself the statistic's own formula and its degenerate-bin rules; a PSD row leaves through psd_value.
#pragma once
#include "oth_internal.h"

namespace oth {

// natural bin k -> index i into the output row under the plan's shift and trim; false: the bin is trimmed away (or past nfft)
__device__ __forceinline__ bool out_slot(const OutStage &o, int nfft, int k, int &i) {
    int ks = k;
    if (o.fftshift) {
        ks = k + nfft / 2;
        if (ks >= nfft) ks -= nfft;
    }
    i = ks - o.trim;
    return k < nfft && i >= 0 && i < o.nout;
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

// the PSD output stage (finalize_kernel's): linear, or dB of the scaled value
__device__ __forceinline__ float psd_value(const OutStage &o, double v) { return o.db ? (float)(10.0 * log10(v)) : (float)v; }

// one workgroup per 32 bins, stream and - where nz > 1 - z index
template <auto K, typename Args> hipError_t launch_stat_finalize(const Args &a, int nstreams, int nz, hipStream_t s) {
    const dim3 grid((a.nfft + 31) / 32, nstreams, nz);
    hipLaunchKernelGGL(K, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace oth
