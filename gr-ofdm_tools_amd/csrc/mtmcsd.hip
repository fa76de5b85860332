// Two-channel multitaper: per segment K orthogonal tapers on the SAME samples of both channels,
//   sum_k c_k |X_k|^2, sum_k c_k |Y_k|^2, sum_k c_k conj(X_k) Y_k,   X_k = FFT((x - m_x) v_k), Y_k = FFT((y - m_y) v_k),
// for every power-of-two size 64..16384 on the LDS Stockham FFT of fft_lds.hip.h - the taper loop of mtm.hip with a second
// channel: the same work split ((segment, taper) items, taper index fastest, a workgroup walks one contiguous run and
// forms a segment's samples, pilot and residual mean once per channel when the run enters it), the same pilot arithmetic
// (mtm_common.hip.h), each channel with `red` slots of its own so that a NaN in one never reaches the other.
//
// Per item both spectra have to exist at once, next to four rows of sums (in the order of welch_generic_kernel<..., true>:
// |X|^2, |Y|^2, Re conj(X) Y, Im conj(X) Y).  What was chosen per size, and why:
//   64 ... 8192 points   TWO LDS buffers (2 x 8 N bytes: 64 KiB at 4096, 128 KiB + the reduction slots at 8192): both taper
//                        products are written, both transforms run, the sums read both buffers.  Nothing of a spectrum
//                        sits in registers - the coverage kernel's shape (X parked in N / T float2 registers) would add
//                        them to the 4 N / T accumulators, which stay in registers across the run's transforms.
//   4096, 8192 points    twice mtm_kernel's threads (512, 1024), so N / T = 8.  At 4096 points the LDS bound is two workgroups
//                        per CU whatever the registers; measured in one session (profiles/mtm_csd_ab.txt), 64 single
//                        segments with K 7 / 2^24 samples with K 4:  256 threads, samples re-read (148 registers)
//                        2.44 / 1.09 ms;  512 threads, re-read (90) 1.91 / 0.92 ms;  512 threads, samples kept (126)
//                        1.76 / 0.80 ms - the build;  1024 threads, kept (79; one workgroup per CU) 1.67 / 1.07 ms.
//                        1024 threads at 8192 points is by that analogy, not by a measurement of its own.
//   16384 points         one 128 KiB buffer is all that fits in 160 KiB.  X's spectrum goes through a row of 16384 float2
//                        in global memory that belongs to the workgroup (MtmCsdArgs.ws): every thread writes the N / T
//                        bins it will sum and reads the same addresses back after Y's transform - written once, read
//                        once per item by the thread that wrote them, so it needs no barrier and stays in L2.  64
//                        accumulators next to the butterflies' operands do not fit the 128 registers of a 1024-thread
//                        build (296 bytes of scratch), so the four rows live in the workgroup's own partial rows: the
//                        first item of a run stores them, every later one reads, adds and stores - again each thread
//                        its own addresses.  A single segment (W = K, one item per workgroup) never reads them back.
// Samples: kept in registers across a segment's tapers below 8192 points, read again per taper from L2 from there on
// (mtm.hip's KEEP and its line), both channels alike.
// Scalar registers: behind 128 KiB of tile the reduction slots' addresses do not fit a DS offset field, and as 2 x 17
// scalar constants they were hoisted out of the item loop and spilled; they hang off one opaque vector register instead.
// The thread index is opaque per transform, not only per item as in mtm_kernel: shared between an item's two transforms
// the passes' index arithmetic cost 24 registers at 16384 points.
//
// Arithmetic the tests rely on: Re conj(X) Y = fma(Xr, Yr, Xi Yi) has the expression shape of |X|^2 = fma(Xr, Xr, Xi Xi),
// so a channel against itself gives three bit-identical rows and Cxy = 1 exactly; Im conj(X) Y is cross_im's two rounded
// products, exactly 0 for identical channels.  Every sum runs in a fixed order: a result depends on the launch shape only.
#include "mtm_common.hip.h"
#include "oth_internal.h"
#include "launch.h"

#include <type_traits>

namespace oth {
namespace {

constexpr bool mtmcsd_two_buffers(int n) { return n <= 8192; }

// one channel's segment on entry: pilot, residual mean and (KEEP) the detrended samples
template <int N, int T, bool KEEP>
__device__ __forceinline__ void mtmcsd_enter(const float2 *__restrict__ xs, int nperseg, int detrend, float2 *red, int tid,
                                             float2 &pil, float2 &mean, float2 (&v)[KEEP ? N / T : 1]) {
    constexpr int NQ = N / T;
    if (detrend) pil = mtm_pilot(xs, nperseg, red, tid);
    float2 sum = make_float2(0.f, 0.f);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int n = tid + q * T;
        const float2 r = (n < nperseg) ? csub(xs[n], pil) : make_float2(0.f, 0.f);
        if constexpr (KEEP) v[q] = r;
        sum = cadd(sum, r);
    }
    if (detrend) {
        const float2 tot = block_sum<T>(sum, red, tid, 1);
        const float inv = 1.0f / (float)nperseg;
        mean = make_float2(tot.x * inv, tot.y * inv);
    }
    if constexpr (KEEP) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int n = tid + q * T;
            v[q] = (n < nperseg) ? csub(v[q], mean) : make_float2(0.f, 0.f);
        }
    }
}

template <int N, int T, bool KEEP, bool TWO, bool ACCREG> __global__ __launch_bounds__(T) void mtmcsd_kernel(MtmCsdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MtmArgs &p = a.m;
    float2 *bufx = reinterpret_cast<float2 *>(smem);
    float2 *bufy = TWO ? bufx + N : bufx;
    // per channel: [0] the pilot, [1 ...] the block sum's wave rows; off an opaque vector register (file header)
    int red0 = 0;
    asm volatile("" : "+v"(red0));
    float2 *redx = bufy + N + red0, *redy = redx + kMtmRedSlots;
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y, K = p.ntapers;
    const long long items = p.nseg * K;
    const long long i0 = (items * wg) / W, i1 = (items * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    const float2 *yb = a.y + (size_t)stream * p.stream_stride;
    float2 *ws = TWO ? nullptr : a.ws + ((size_t)stream * W + wg) * N;

    float *dst = p.partial + ((size_t)stream * W + wg) * 4 * N;
    float acc[ACCREG ? 4 : 1][ACCREG ? NQ : 1];
    if constexpr (ACCREG) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[c][q] = 0.f;
    }
    float2 vx[KEEP ? NQ : 1], vy[KEEP ? NQ : 1];
    float2 pilx = make_float2(0.f, 0.f), meanx = pilx, pily = pilx, meany = pilx;      // of the current segment

    long long s = i0 / K;
    int k = (int)(i0 - s * K);
    bool first = true;      // of the run: it enters its segment whatever k is, and its sums start from zero
    for (long long left = i1 - i0; left > 0; --left) {
        int tid = tid0;      // an opaque copy per item, as in mtm_kernel: the passes' index arithmetic is not hoisted
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step, *ys = yb + s * p.step;
        if (first || k == 0) {
            mtmcsd_enter<N, T, KEEP>(xs, p.nperseg, p.detrend, redx, tid, pilx, meanx, vx);
            mtmcsd_enter<N, T, KEEP>(ys, p.nperseg, p.detrend, redy, tid, pily, meany, vy);
        }
        const float *__restrict__ w = p.tapers + (size_t)k * N;      // zero-extended to N
        mtm_taper_product<N, T, KEEP>(xs, w, p.nperseg, tid, pilx, meanx, vx, bufx);
        if constexpr (TWO) {
            mtm_taper_product<N, T, KEEP>(ys, w, p.nperseg, tid, pily, meany, vy, bufy);
            __syncthreads();
            fft_lds<N, T>(bufx, p.tw, tid);
            asm volatile("" : "+v"(tid));      // (nor shared between the two transforms)
            fft_lds<N, T>(bufy, p.tw, tid);
        } else {
            __syncthreads();
            fft_lds<N, T>(bufx, p.tw, tid);
#pragma unroll
            for (int q = 0; q < NQ; ++q) ws[tid + q * T] = bufx[tid + q * T];      // this thread's bins, read back below
            __syncthreads();
            mtm_taper_product<N, T, KEEP>(ys, w, p.nperseg, tid, pily, meany, vy, bufy);
            __syncthreads();
            asm volatile("" : "+v"(tid));
            fft_lds<N, T>(bufy, p.tw, tid);
        }
        const float c = p.coef[k];
        // LOAD: the sums so far come from the registers or, with the rows in memory, from this thread's own stores of the
        // item before (four bins at a time there, so that the loads in flight do not outgrow the registers); the first
        // item of such a run only stores - a uniform branch, not a select per bin
        auto sum = [&](auto load) {
#pragma unroll ACCREG ? NQ : 4
            for (int q = 0; q < NQ; ++q) {
                const float2 X = TWO ? bufx[tid + q * T] : ws[tid + q * T];
                const float2 Y = bufy[tid + q * T];
                float r[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (decltype(load)::value) {
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) r[ch] = ACCREG ? acc[ACCREG ? ch : 0][ACCREG ? q : 0] : dst[ch * N + tid + q * T];
                }
                r[0] = fmaf(c, fmaf(X.x, X.x, X.y * X.y), r[0]);
                r[1] = fmaf(c, fmaf(Y.x, Y.x, Y.y * Y.y), r[1]);
                r[2] = fmaf(c, fmaf(X.x, Y.x, X.y * Y.y), r[2]);      // conj(X) Y
                r[3] = fmaf(c, cross_im(X, Y), r[3]);
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    if constexpr (ACCREG) acc[ch][q] = r[ch];
                    else dst[ch * N + tid + q * T] = r[ch];
                }
            }
        };
        if (ACCREG || !first) sum(std::true_type{});
        else sum(std::false_type{});
        __syncthreads();
        first = false;
        if (++k == K) {
            k = 0;
            ++s;
        }
    }
    if constexpr (ACCREG) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < NQ; ++q) dst[c * N + tid0 + q * T] = acc[c][q];
    }
}

size_t mtmcsd_lds_bytes(int nfft) { return stat_lds_bytes(nfft, mtmcsd_two_buffers(nfft) ? 2 : 1, 2); }

// (file header: twice the coverage kernels' threads at 4096 and 8192 points)
#define OTH_MTMCSD_KERNEL(N) mtmcsd_kernel<N, stat_threads(N), mtm_keep(N), mtmcsd_two_buffers(N), mtmcsd_two_buffers(N)>

}  // namespace

size_t mtmcsd_ws_points(int nfft) { return mtmcsd_two_buffers(nfft) ? 0 : (size_t)nfft; }

int mtmcsd_blocks_per_cu(int nfft) {
    return mtm_for_size(nfft, 0, [](auto n) {
        constexpr int N = decltype(n)::value;
        return resident_blocks<OTH_MTMCSD_KERNEL(N)>(stat_threads(N), mtmcsd_lds_bytes(N), 0);
    });
}

hipError_t launch_mtmcsd(int nfft, const MtmCsdArgs &a, hipStream_t s) {
    const dim3 grid(a.m.wg_per_stream, a.m.nstreams);
    return mtm_for_size(nfft, hipErrorInvalidValue, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return launch_lds<OTH_MTMCSD_KERNEL(N)>(grid, dim3(stat_threads(N)), mtmcsd_lds_bytes(N), s, a);
    });
}

}  // namespace oth
