// Polyphase channelizer (oth_channelizer): M channels, hop D (M, M / 2 or M / 4), a real prototype h of L = P M taps.  With
// frame m of a push covering the samples m D ... m D + L - 1 of tail ++ x (the samples earlier pushes left, then the new ones),
//   u_m[r]                 = sum_{p < P} h[r + p M] x[m D + r + p M]      r < M     welchpfb.hip's fold, no detrend, p ascending
//   v_m[(r + j D) mod M]   = u_m[r]                                        j = frames before this push + m: the absolute frame
//   out[k][m]              = FFT_M(v_m)[k]                                  natural order, no scale
// which is y_k[j] = sum_n h[n] x[j D + n] e^{-j 2 pi k (j D + n) / M}: channel k mixed to DC by the phase of the absolute
// sample index, filtered by h, every D-th output kept.  The circular shift is what keeps the phase continuous between hops:
// D divides M, so (j D) mod M = (j mod (M / D)) D and the host hands down rot0 = (frames before this push) mod (M / D).
//
// The body is welch_pfb_kernel's (a whole frame per work item, one LDS buffer, fft_lds): thread tid owns the points
// r = tid + q T, loads x[r + p M] and h[r + p M] for p = 0 ... P - 1, both coalesced, and writes the fold to LDS at the
// rotated index - a rotation moves every lane by the same amount, so the write stays free of bank conflicts.
//
// The store decides the design: frame-major results leave channel-major.  A workgroup takes its frames in tiles of
// F = kChanTile = 8 consecutive frames, aligned on the push's column 0, and keeps its bins of the tile's frames in registers
// (F M / T complex values per thread); after the tile's last transform a thread writes, for each of its channels, the F
// consecutive outputs of the row: 64 contiguous bytes, as four 16-byte stores where the row is 16-byte aligned (an even
// out_stride on a 16-byte aligned buffer), as eight 8-byte stores otherwise and in the push's last, partial tile.  T = M / 4
// from 256 channels on (64 below), so M / T <= 4 and a tile is at most 32 complex registers whatever the size: every build
// comes out without scratch inside the 128 registers of a 1024-thread workgroup (tests/test_channelizer_cpu.py reads the
// code objects).  Not built: the transpose of a larger tile through a second LDS buffer, which would let a row's piece grow
// past 64 bytes ([F][M] fits next to the transform buffer for F M <= 8192).
//
// A push's tiles go to W workgroups in contiguous runs of whole tiles.  A result depends on the absolute frame index alone -
// not on the tile, on W or on where the pushes were cut: the fold adds p ascending and the transform is fft_lds's fixed
// sequence.
//
// What a workgroup reads.  Sample i of tail ++ x is tail[i] for i < pending and x[i - pending] behind.  The host counts
// nframes so that the furthest sample of the last frame, (nframes - 1) D + L - 1, is below pending + the new samples: that
// is the bound of every load here.  A frame with m D >= pending lies wholly in x and takes the loop without a per-sample
// test; the frames in front (fewer than L / D of a push) select per sample.  h is read at r + p M < L.  What it writes:
// rows k < M, columns m < nframes <= out_stride.
//
// Degenerate input.  All-zero input gives exact zeros.  A NaN or +-inf sample makes u of the frames that cover it
// non-finite, and every bin of a transform depends on every point: exactly those frames are non-finite, in every channel;
// the other frames share no sum with them.  A power-of-two gain scales every product and sum exactly.
#include "fft_lds.hip.h"
#include "oth_internal.h"
#include "launch.h"

#include <type_traits>

namespace oth {
namespace {

constexpr int chan_threads(int n) { return n >= 256 ? n / 4 : 64; }

// the fold of one frame whose sample i is xs[i] (SPLIT: tail[i] for i < pending, xs[i] behind - xs = x - pending)
template <int N, int T, bool SPLIT>
__device__ __forceinline__ void chan_fold(float2 (&y)[N / T], const float2 *__restrict__ xs, const float2 *__restrict__ tail,
                                          long long first, long long pending, const float *__restrict__ h, int P, int tid) {
    const float *__restrict__ hp = h + tid;
    long long i0 = first + tid;
    for (int t = 0; t < P; ++t, i0 += N, hp += N) {
#pragma unroll
        for (int q = 0; q < N / T; ++q) {
            const long long i = i0 + q * T;
            const float2 r = SPLIT && i < pending ? tail[i] : xs[i];
            const float hv = hp[q * T];
            y[q].x = fmaf(hv, r.x, y[q].x);
            y[q].y = fmaf(hv, r.y, y[q].y);
        }
    }
}

template <int N, int T, int F> __global__ __launch_bounds__(T) void chan_pfb_kernel(ChanPfbArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *buf = reinterpret_cast<float2 *>(smem);
    constexpr int NQ = N / T;
    static_assert(F % 2 == 0, "a tile leaves in 16-byte pieces");
    const int tid0 = threadIdx.x;
    const long long W = p.wg_count, wg = blockIdx.x;
    const long long ntiles = (p.nframes + F - 1) / F;
    const long long t0 = (ntiles * wg) / W, t1 = (ntiles * (wg + 1)) / W;
    const int P = p.ntaps, D = p.decim;
    const int rmask = N / D - 1;
    const float2 *xs = p.x - p.pending;      // sample i of tail ++ x for i >= pending (never read below)
    const bool wide = ((reinterpret_cast<size_t>(p.out) & 15) == 0) && ((p.out_stride & 1) == 0);

    for (long long t = t0; t < t1; ++t) {
        const long long m0 = t * F;
        float2 Y[F][NQ];
#pragma unroll
        for (int f = 0; f < F; ++f) {
            long long m = m0 + f;
            asm volatile("" : "+s"(m));      // opaque too: the F unrolled frames' scalar addresses are formed one frame at a time
#pragma unroll
            for (int q = 0; q < NQ; ++q) Y[f][q] = make_float2(0.f, 0.f);
            if (m < p.nframes) {      // uniform: the barriers below are met by the whole workgroup or by nobody
                int tid = tid0;       // an opaque copy, as in welch_pfb_kernel: a frame's index arithmetic is not hoisted
                asm volatile("" : "+v"(tid));
                const long long first = m * D;
                float2 y[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) y[q] = make_float2(0.f, 0.f);
                if (first >= p.pending) chan_fold<N, T, false>(y, xs, p.tail, first, p.pending, p.h, P, tid);
                else chan_fold<N, T, true>(y, xs, p.tail, first, p.pending, p.h, P, tid);
                const int rot = (int)((p.rot0 + m) & rmask) * D;
#pragma unroll
                for (int q = 0; q < NQ; ++q) buf[(tid + q * T + rot) & (N - 1)] = y[q];
                __syncthreads();
                fft_lds<N, T>(buf, p.tw, tid);
#pragma unroll
                for (int q = 0; q < NQ; ++q) Y[f][q] = buf[tid + q * T];
                __syncthreads();      // buf is the next frame's
            }
        }
        const bool whole = m0 + F <= p.nframes;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float2 *row = p.out + (size_t)(tid0 + q * T) * p.out_stride + m0;
            if (whole && wide) {
                float4 *row4 = reinterpret_cast<float4 *>(row);
#pragma unroll
                for (int f = 0; f < F; f += 2) row4[f / 2] = make_float4(Y[f][q].x, Y[f][q].y, Y[f + 1][q].x, Y[f + 1][q].y);
            } else {
#pragma unroll
                for (int f = 0; f < F; ++f)
                    if (m0 + f < p.nframes) row[f] = Y[f][q];
            }
        }
    }
}

#define OTH_CHAN_FOR_EACH_N(X) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)

template <typename R, typename Fn> R chan_for_size(int nchan, R otherwise, Fn f) {
    switch (nchan) {
#define X(N) \
    case N: return f(std::integral_constant<int, N>{});
        OTH_CHAN_FOR_EACH_N(X)
#undef X
        default: return otherwise;
    }
}

}  // namespace

#define OTH_CHAN_KERNEL(N) chan_pfb_kernel<N, chan_threads(N), kChanTile>

int chan_pfb_blocks_per_cu(int nchan) {
    return chan_for_size(nchan, 0, [](auto n) {
        constexpr int N = decltype(n)::value;
        return resident_blocks<OTH_CHAN_KERNEL(N)>(chan_threads(N), sizeof(float2) * N, 0);
    });
}

hipError_t launch_chan_pfb(int nchan, const ChanPfbArgs &a, hipStream_t s) {
    return chan_for_size(nchan, hipErrorInvalidValue, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return launch_lds<OTH_CHAN_KERNEL(N)>(dim3(a.wg_count), dim3(chan_threads(N)), sizeof(float2) * N, s, a);
    });
}

}  // namespace oth
