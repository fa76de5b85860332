// The bin order of a partial-sum row as a data format: a transform kernel leaves the sums of its bins at the positions its
// butterflies end in, and whoever reads the rows (the finalize kernels and chain_state_kernel, kernels_misc.hip) asks
// bin_pos for the bin at a position.  Host and device; no HIP header, so a plain C++ compiler takes it too (the CPU suite
// checks every layout below to be a permutation).
#pragma once

#ifdef __HIPCC__
#define OTH_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define OTH_HOST_DEVICE inline
#endif

namespace oth {

// The numbers are the recipe text's `layout=`.  Per value: who writes it, and the bin at a position.
enum RowLayout : int {
    ROW_NATURAL = 0,   // the generic kernels, segfft.hip, the taper loops, fft_any.hip's one-level routes: position k holds bin k
    ROW_W4096 = 1,     // welch4096 / csd4096[ws]: position 16 k0 + k1 + 256 k2 holds bin k0 + 16 k1 + 256 k2 (its own inverse)
    ROW_W16K = 2,      // welch16k, 16384 points: position 4096 k' + (ROW_W4096 position of q) holds bin k' + 4 q
    ROW_W8K = 3,       // welch16k, 8192 points: the same with bin k' + 2 q
    ROW_X1_16K = 4,    // welch16k1x, 16384 points: position 1024 k2 + 64 k0 + 4 k1 + q holds bin k0 + 16 k1 + 256 k2 + 4096 bitrev2(q)
    ROW_X1_8K = 5,     // its 8-wave form, 8192 points: position 512 k2 + 64 (k0 >> 1) + 4 (8 (k0 & 1) + k1) + q holds
                       // bin k0 + 16 k1 + 128 k2 + 2048 bitrev2(q)
    ROW_TWOLEVEL = 6,  // fft_any.hip / fft_tl.hip, two-level route L = l1 l2: position k1 l2 + k2 holds bin k1 + l1 k2
    ROW_W32K = 7,      // welch32k, 32768 points: halves A | B of 16384 positions in ROW_X1_16K each; A holds bin 2 k, B bin 2 k + 1
    ROW_W64K = 8,      // its 65536-point pair: halves of 32768 positions in ROW_W32K each, the first the even bins, the second the odd
};

// bin held at position `pos` of a partial-sum row (l1, l2: ROW_TWOLEVEL only)
OTH_HOST_DEVICE int bin_pos(int pos, RowLayout layout, int l1 = 0, int l2 = 0) {
    if (layout == ROW_NATURAL) return pos;
    if (layout == ROW_TWOLEVEL) {
        const int k1 = pos / l2;
        return k1 + l1 * (pos - k1 * l2);
    }
    if (layout == ROW_X1_16K || layout == ROW_W32K || layout == ROW_W64K) {
        const int h8 = layout == ROW_W64K ? pos >> 15 : 0;
        if (layout == ROW_W64K) pos &= 32767;
        const int h7 = layout != ROW_X1_16K ? pos >> 14 : 0;
        if (layout != ROW_X1_16K) pos &= 16383;
        int k = ((pos >> 6) & 15) + 16 * ((pos >> 2) & 15) + 256 * (pos >> 10) + 4096 * (((pos & 1) << 1) | ((pos >> 1) & 1));
        if (layout != ROW_X1_16K) k = 2 * k + h7;
        return layout == ROW_W64K ? 2 * k + h8 : k;
    }
    if (layout == ROW_X1_8K)      // pos = 512 k2 + 64 k0' + 4 (8 h + k1) + q holds bin (2 k0' + h) + 16 k1 + 128 k2 + 2048 bitrev2(q)
        return 2 * ((pos >> 6) & 7) + ((pos >> 5) & 1) + 16 * ((pos >> 2) & 7) + 128 * (pos >> 9) + 2048 * (((pos & 1) << 1) | ((pos >> 1) & 1));
    const int r = pos & 4095;
    const int q = ((r & 15) << 4) | ((r >> 4) & 15) | (r & ~255);
    return layout == ROW_W4096 ? q : (pos >> 12) + (layout == ROW_W16K ? 4 : 2) * q;
}

// what a writer with more than one layout leaves at a size it runs
inline RowLayout w16k_layout(int nfft) { return nfft == 16384 ? ROW_W16K : ROW_W8K; }            // welch16k.hip
inline RowLayout x1_layout(int nfft) { return nfft == 16384 ? ROW_X1_16K : ROW_X1_8K; }          // welch16k1x.hip
inline RowLayout w32k_layout(int L) { return L == 65536 ? ROW_W64K : ROW_W32K; }                 // welch32k.hip

}  // namespace oth
