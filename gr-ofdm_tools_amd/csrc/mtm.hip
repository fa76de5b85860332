// Multitaper (Thomson) PSD: per segment K orthogonal tapers on the SAME samples, sum_k c_k |FFT((x - mean) v_k)|^2, for
// every power-of-two size 64..16384 on the LDS Stockham FFT of fft_lds.hip.h.
//
// The shape is the opposite of Welch's: few segments (often one: a work()-sized vector, one row per scanner channel), many
// streams, K transforms per segment.  The work items of a stream are its (segment, taper) pairs, taper index fastest; a
// workgroup walks one contiguous run of them, so a single segment with K tapers spreads over K workgroups and a long
// launch over about the resident capacity, each workgroup loading a segment once for all of its tapers.
//
// Per segment (only when the run enters a new one): a pilot - the mean of the segment's first 64 samples, formed by the
// first wave - comes off every sample, then the residual mean (a block sum) comes off.  Taken directly in float32 the
// mean of a segment under a 35-sigma offset leaves up to 2.8e-4 of relative bin error (4096 points, NW 2, K 3); with the
// pilot the sums run over values of the noise's size and the worst bin reads 1.1e-5.
// Per item: taper product into LDS, fft_lds, acc += c_k |X|^2 in registers.  The run's row goes to
// partial[stream][workgroup][N] in natural bin order (finalize layout 0); the finalize kernels add the rows in a fixed
// order, so a result depends on the launch shape only - bit-identical from run to run.
//
// KEEP (below 8192 points): the detrended samples of the segment stay in registers across its tapers (N / T complex values
// per thread).  At 16384 points (1024 threads, 128 registers per lane) they do not fit next to the butterflies' operands
// without scratch (28 bytes per lane), and at 8192 points they cost the second resident workgroup of a CU (134 registers
// against 82): those builds keep the pilot and the residual mean instead and read the samples again per taper - from L2,
// one tile against the fourteen tile passes a transform moves through LDS.  Measured on one session, alternating: 8192 points
// 1.07 against 1.21 ms for 2^25 samples with K 4 and 0.062 against 0.069 ms for 64 single segments with K 7 in favour of
// re-reading; 4096 points 1.77 against 1.54 ms for 2^26 samples with K 4 in favour of the registers (three workgroups per
// CU against four).  profiles/mtm_keep_ab.txt.
#include "mtm_common.hip.h"
#include "oth_internal.h"
#include "launch.h"

namespace oth {
namespace {

template <int N, int T, bool KEEP> __global__ __launch_bounds__(T) void mtm_kernel(MtmArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *buf = reinterpret_cast<float2 *>(smem);
    float2 *red = buf + N;      // [0] the pilot, [1 ...] the block sum's wave rows
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y, K = p.ntapers;
    const long long items = p.nseg * K;
    const long long i0 = (items * wg) / W, i1 = (items * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;

    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    float2 v[KEEP ? NQ : 1];
    float2 pil = make_float2(0.f, 0.f), mean = make_float2(0.f, 0.f);      // of the current segment

    long long s = i0 / K, cur = -1;
    int k = (int)(i0 - s * K);
    for (long long i = i0; i < i1; ++i) {
        // an opaque copy of the thread index per item: the index arithmetic of the seven passes is a handful of integer
        // instructions, and hoisted out of this loop it would hold registers that the butterflies need
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step;
        if (s != cur) {
            cur = s;
            if (p.detrend) pil = mtm_pilot(xs, p.nperseg, red, tid);
            float2 sum = make_float2(0.f, 0.f);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int n = tid + q * T;
                const float2 r = (n < p.nperseg) ? csub(xs[n], pil) : make_float2(0.f, 0.f);
                if constexpr (KEEP) v[q] = r;
                sum = cadd(sum, r);
            }
            if (p.detrend) {
                const float2 tot = block_sum<T>(sum, red, tid, 1);
                const float inv = 1.0f / (float)p.nperseg;
                mean = make_float2(tot.x * inv, tot.y * inv);
            }
            if constexpr (KEEP) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int n = tid + q * T;
                    v[q] = (n < p.nperseg) ? csub(v[q], mean) : make_float2(0.f, 0.f);
                }
            }
        }
        const float *__restrict__ w = p.tapers + (size_t)k * N;      // zero-extended to N
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int n = tid + q * T;
            float2 r;
            if constexpr (KEEP) {
                r = v[q];
            } else {
                r = (n < p.nperseg) ? csub(csub(xs[n], pil), mean) : make_float2(0.f, 0.f);      // the same arithmetic as KEEP
            }
            const float wn = w[n];
            buf[n] = make_float2(r.x * wn, r.y * wn);
        }
        __syncthreads();
        fft_lds<N, T>(buf, p.tw, tid);
        const float c = p.coef[k];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float2 X = buf[tid + q * T];
            acc[q] = fmaf(c, fmaf(X.x, X.x, X.y * X.y), acc[q]);
        }
        __syncthreads();
        if (++k == K) {
            k = 0;
            ++s;
        }
    }
    float *dst = p.partial + ((size_t)stream * W + wg) * N;
#pragma unroll
    for (int q = 0; q < NQ; ++q) dst[tid0 + q * T] = acc[q];
}

}  // namespace

#define OTH_MTM_KERNEL(N) mtm_kernel<N, generic_threads(N), mtm_keep(N)>

int mtm_blocks_per_cu(int nfft) {
    return mtm_for_size(nfft, 0, [](auto n) {
        constexpr int N = decltype(n)::value;
        return resident_blocks<OTH_MTM_KERNEL(N)>(generic_threads(N), stat_lds_bytes(N), 0);
    });
}

hipError_t launch_mtm(int nfft, const MtmArgs &a, hipStream_t s) {
    const dim3 grid(a.wg_per_stream, a.nstreams);
    return mtm_for_size(nfft, hipErrorInvalidValue, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return launch_lds<OTH_MTM_KERNEL(N)>(grid, dim3(generic_threads(N)), stat_lds_bytes(N), s, a);
    });
}

}  // namespace oth
