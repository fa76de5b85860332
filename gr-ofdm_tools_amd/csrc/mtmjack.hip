// Jackknife (Thomson & Chave) of a multitaper plan over its M = K nseg (segment, taper) items: the second of two passes.
// The first pass is the plan's own averaging launch and reduction and leaves the totals per bin - S = sum_i p_i for one
// channel, Sxx, Syy, Sxy for two.  Given them an item's delete-one estimate depends on no other item, so this pass walks
// the items exactly as mtm_kernel / mtmcsd_kernel do ((segment, taper) pairs, taper index fastest, contiguous runs over W
// workgroups; segment entry and taper product are mtm_common.hip.h's) and adds per owned bin
//   one channel    l = log1p(-min(p / S, CL)),  CL = 1 - 2^-24              ->  sum l, sum l^2
//   two channels   lx, ly as above; with Ci = |Sxy - r|^2 / ((Sxx - p)(Syy - q)) - each factor kept at 2^-24 of its total
//                  at least, which is the clamp of p / Sxx at CL - and z(c) = atanh(min(sqrt(c), CL)):
//                  d = z(Ci) - z(C)                                          ->  sum lx, lx^2, ly, ly^2, d, d^2
// The deviation from the full estimate is what is summed: a sum of squares of z(Ci) itself cancels in float32.  A bin
// whose total is not positive adds zeros.  The rows leave as partial[stream][wg][2 or 6][N] in natural bin order;
// jack_finalize_kernel adds them in double in a fixed order and forms (M - 1) / M (sum a^2 - (sum a)^2 / M), clamped at 0,
// and its root, with the plan's shift and trim.
//
// (Sxx - p)(Syy - q) against |Sxy - r|^2: for a channel against itself the three totals and the three item terms are the
// same bits (mtmcsd.hip's header), numerator and denominator are one product and Ci = 1 exactly, as C is - every d is 0.
// The exception is a bin in which one item holds all but 2^-24 of a total (a pure line on three items or fewer): the floor
// acts on the denominator's factors and not on the numerator, as the clamp of the definition does, so Ci < 1 = C there.
//
// Where the running sums live (mtmftest.hip's and mtmcsd.hip's precedents):
//   one channel    64 ... 8192 points: registers (2 N / T), the samples too below 8192 points (mtm.hip's KEEP);
//                  16384 points (1024 threads, 128 registers): the workgroup's own partial rows - the first item of a run
//                  stores, every later one reads, adds and stores, each thread its own addresses.
//   two channels   64 ... 2048 points: registers (6 N / T <= 48) next to both channels' samples; from 4096 points on the
//                  partial rows.  Threads and LDS as mtmcsd_kernel's: two buffers up to 8192 points, one at 16384 with
//                  X's spectrum through the workgroup's own global workspace row.
// The totals are read again per item (L2), never held.
#include "mtm_common.hip.h"
#include "out_stage.hip.h"
#include "launch.h"

#include <type_traits>

namespace oth {
namespace {

constexpr float kJackCl = 0.99999994f;        // 1 - 2^-24
constexpr float kJackFloor = 5.9604645e-8f;   // 2^-24

// log1p(-min(p / S, CL)); 0 where the total is not positive
__device__ __forceinline__ float jack_l(float p, float S) {
    const float t = fminf(p / S, kJackCl);
    return S > 0.f ? log1pf(-t) : 0.f;
}
__device__ __forceinline__ float jack_z(float c) { return atanhf(fminf(sqrtf(c), kJackCl)); }

template <int N, int T, bool KEEP, bool ACCREG> __global__ __launch_bounds__(T) void mtm_jack_kernel(MtmJackArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MtmArgs &p = a.m;
    float2 *buf = reinterpret_cast<float2 *>(smem);
    float2 *red = buf + N;      // [0] the pilot, [1 ...] the block sum's wave rows
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y, K = p.ntapers;
    const long long items = p.nseg * K;
    const long long i0 = (items * wg) / W, i1 = (items * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    const float *__restrict__ tot = a.totals + (size_t)stream * N;
    float *dst = p.partial + ((size_t)stream * W + wg) * 2 * N;      // [0] sum l, [1] sum l^2

    float s1[ACCREG ? NQ : 1], s2[ACCREG ? NQ : 1];
    if constexpr (ACCREG) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) s1[q] = s2[q] = 0.f;
    }
    float2 v[KEEP ? NQ : 1];
    float2 pil = make_float2(0.f, 0.f), mean = pil;      // of the current segment

    long long s = i0 / K;
    int k = (int)(i0 - s * K);
    bool first = true;      // of the run: it enters its segment whatever k is, and its sums start from zero
    for (long long left = i1 - i0; left > 0; --left) {
        int tid = tid0;      // an opaque copy per item, as in mtm_kernel: the passes' index arithmetic is not hoisted
        asm volatile("" : "+v"(tid));
        const float2 *xs = xb + s * p.step;
        if (first || k == 0) mtm_segment_entry<N, T, KEEP>(xs, p.nperseg, p.detrend != 0, red, tid, v, pil, mean);
        mtm_taper_product<N, T, KEEP>(xs, p.tapers + (size_t)k * N, p.nperseg, tid, pil, mean, v, buf);
        __syncthreads();
        fft_lds<N, T>(buf, p.tw, tid);
        const float c = p.coef[k];
        if constexpr (ACCREG) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int j = tid + q * T;
                const float2 X = buf[j];
                const float l = jack_l(c * fmaf(X.x, X.x, X.y * X.y), tot[j]);
                s1[q] += l;
                s2[q] = fmaf(l, l, s2[q]);
            }
        } else {
            // the partial rows: four bins at a time, so that the loads in flight do not outgrow the registers
#pragma unroll 4
            for (int q = 0; q < NQ; ++q) {
                const int j = tid + q * T;
                const float2 X = buf[j];
                const float l = jack_l(c * fmaf(X.x, X.x, X.y * X.y), tot[j]);
                float a1 = 0.f, a2 = 0.f;
                if (!first) {
                    a1 = dst[j];
                    a2 = dst[N + j];
                }
                dst[j] = a1 + l;
                dst[N + j] = fmaf(l, l, a2);
            }
        }
        __syncthreads();
        first = false;
        if (++k == K) {
            k = 0;
            ++s;
        }
    }
    if constexpr (ACCREG) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            dst[tid0 + q * T] = s1[q];
            dst[N + tid0 + q * T] = s2[q];
        }
    }
}

template <int N, int T, bool KEEP, bool TWO, bool ACCREG> __global__ __launch_bounds__(T) void mtmcsd_jack_kernel(MtmCsdJackArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MtmArgs &p = g.c.m;
    float2 *bufx = reinterpret_cast<float2 *>(smem);
    float2 *bufy = TWO ? bufx + N : bufx;
    // per channel: [0] the pilot, [1 ...] the block sum's wave rows; off an opaque vector register (mtmcsd.hip's header)
    int red0 = 0;
    asm volatile("" : "+v"(red0));
    float2 *redx = bufy + N + red0, *redy = redx + kMtmRedSlots;
    constexpr int NQ = N / T;
    const int tid0 = threadIdx.x;
    const int wg = blockIdx.x, W = p.wg_per_stream, stream = blockIdx.y, K = p.ntapers;
    const long long items = p.nseg * K;
    const long long i0 = (items * wg) / W, i1 = (items * (wg + 1)) / W;
    const float2 *xb = p.x + (size_t)stream * p.stream_stride;
    const float2 *yb = g.c.y + (size_t)stream * p.stream_stride;
    float2 *ws = TWO ? nullptr : g.c.ws + ((size_t)stream * W + wg) * N;
    // totals of the stream: [Sxx][Syy][Sxy re, im interleaved]
    const float *__restrict__ txx = g.totals + (size_t)stream * 4 * N, *__restrict__ tyy = txx + N;
    const float2 *__restrict__ txy = reinterpret_cast<const float2 *>(txx + 2 * N);
    float *dst = p.partial + ((size_t)stream * W + wg) * 6 * N;      // sum lx, lx^2, ly, ly^2, d, d^2

    float acc[ACCREG ? 6 : 1][ACCREG ? NQ : 1];
    if constexpr (ACCREG) {
#pragma unroll
        for (int c = 0; c < 6; ++c)
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
            mtm_segment_entry<N, T, KEEP>(xs, p.nperseg, p.detrend != 0, redx, tid, vx, pilx, meanx);
            mtm_segment_entry<N, T, KEEP>(ys, p.nperseg, p.detrend != 0, redy, tid, vy, pily, meany);
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
        // LOAD: as mtmcsd_kernel's - the sums so far from the registers or this thread's own stores of the item before;
        // the first item of a run with the rows in memory only stores (a uniform branch)
        auto sum = [&](auto load) {
#pragma unroll ACCREG ? NQ : 2
            for (int q = 0; q < NQ; ++q) {
                const int j = tid + q * T;
                const float2 X = TWO ? bufx[j] : ws[j];
                const float2 Y = bufy[j];
                const float sxx = txx[j], syy = tyy[j];
                const float2 sxy = txy[j];
                float pp = c * fmaf(X.x, X.x, X.y * X.y), qq = c * fmaf(Y.x, Y.x, Y.y * Y.y);
                float rr = c * fmaf(X.x, Y.x, X.y * Y.y), ri = c * cross_im(X, Y);      // conj(X) Y
                // opaque, as cross_im's products: contracted into the subtractions below (-ffp-contract=fast) Sxy - r and
                // Sxx - p would round differently, and a channel against itself would not read C_i = 1
                asm("" : "+v"(pp), "+v"(qq), "+v"(rr), "+v"(ri));
                const float lx = jack_l(pp, sxx), ly = jack_l(qq, syy);
                float d = 0.f;
                if (sxx > 0.f && syy > 0.f) {
                    const float zc = jack_z(fmaf(sxy.x, sxy.x, sxy.y * sxy.y) / (sxx * syy));
                    const float er = sxy.x - rr, ei = sxy.y - ri;
                    const float dx = fmaxf(sxx - pp, sxx * kJackFloor), dy = fmaxf(syy - qq, syy * kJackFloor);
                    d = jack_z(fmaf(er, er, ei * ei) / (dx * dy)) - zc;
                }
                const float t[6] = {lx, lx * lx, ly, ly * ly, d, d * d};
#pragma unroll
                for (int ch = 0; ch < 6; ++ch) {
                    float r = 0.f;
                    if constexpr (decltype(load)::value) r = ACCREG ? acc[ACCREG ? ch : 0][ACCREG ? q : 0] : dst[ch * N + j];
                    r += t[ch];
                    if constexpr (ACCREG) acc[ch][q] = r;
                    else dst[ch * N + j] = r;
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
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int q = 0; q < NQ; ++q) dst[c * N + tid0 + q * T] = acc[c][q];
    }
}

// The shared finalize stage (out_stage.hip.h) on the 2 npairs rows sum l, sum l^2; then the variances in double and
// their rows.  The Cxy row is the first pass's (its reduction formed it from the double sums, natural order): it only takes
// the shift and trim here.
template <int NP> __device__ __forceinline__ void jack_finalize(const JackFinalizeArgs &a) {
    const int k = blockIdx.x * 32 + (threadIdx.x & 31), stream = blockIdx.y;
    int i;
    const bool live = out_slot(a.out, a.nfft, k, i);
    constexpr int R = 2 * NP;
    const float *base = a.partial + (size_t)stream * a.W * R * a.nfft + k;
    double t[R];
    if (!slice_sums<R>(live, a.W, [&](int w, int r) { return base[((size_t)w * R + r) * a.nfft]; }, t)) return;
    const size_t o = (size_t)stream * a.out.nout + i;
#pragma unroll
    for (int pr = 0; pr < NP; ++pr) {
        const double t1 = t[2 * pr], t2 = t[2 * pr + 1];
        const double var = a.mm1_over_m * (t2 - t1 * t1 / a.m);
        if (a.sd_out[pr]) a.sd_out[pr][o] = var > 0.0 ? (float)sqrt(var) : 0.f;      // (a NaN reads 0 as well)
    }
    if (a.cxy_out) a.cxy_out[o] = a.cxy_nat[(size_t)stream * a.nfft + k];
}

// npairs is 1 (one channel) or 3 (two): the same for every thread of the launch
__global__ __launch_bounds__(256) void jack_finalize_kernel(JackFinalizeArgs a) {
    if (a.npairs == 1) jack_finalize<1>(a);
    else jack_finalize<3>(a);
}

constexpr bool jack_accreg(int n) { return n < 16384; }

// mtmcsd.hip's threads, buffers and workspace
constexpr bool jackcsd_two_buffers(int n) { return n <= 8192; }
constexpr bool jackcsd_accreg(int n) { return n <= 2048; }
size_t jackcsd_lds_bytes(int nfft) { return stat_lds_bytes(nfft, jackcsd_two_buffers(nfft) ? 2 : 1, 2); }

}  // namespace

#define OTH_JACK_KERNEL(N) mtm_jack_kernel<N, generic_threads(N), mtm_keep(N), jack_accreg(N)>
#define OTH_JACKCSD_KERNEL(N) mtmcsd_jack_kernel<N, stat_threads(N), mtm_keep(N), jackcsd_two_buffers(N), jackcsd_accreg(N)>

size_t mtmcsd_jack_ws_points(int nfft) { return jackcsd_two_buffers(nfft) ? 0 : (size_t)nfft; }

int mtm_jack_blocks_per_cu(int nfft) {
    return mtm_for_size(nfft, 0, [](auto n) {
        constexpr int N = decltype(n)::value;
        return resident_blocks<OTH_JACK_KERNEL(N)>(generic_threads(N), stat_lds_bytes(N), 0);
    });
}

hipError_t launch_mtm_jack(int nfft, const MtmJackArgs &a, hipStream_t s) {
    const dim3 grid(a.m.wg_per_stream, a.m.nstreams);
    return mtm_for_size(nfft, hipErrorInvalidValue, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return launch_lds<OTH_JACK_KERNEL(N)>(grid, dim3(generic_threads(N)), stat_lds_bytes(N), s, a);
    });
}

int mtmcsd_jack_blocks_per_cu(int nfft) {
    return mtm_for_size(nfft, 0, [](auto n) {
        constexpr int N = decltype(n)::value;
        return resident_blocks<OTH_JACKCSD_KERNEL(N)>(stat_threads(N), jackcsd_lds_bytes(N), 0);
    });
}

hipError_t launch_mtmcsd_jack(int nfft, const MtmCsdJackArgs &a, hipStream_t s) {
    const dim3 grid(a.c.m.wg_per_stream, a.c.m.nstreams);
    return mtm_for_size(nfft, hipErrorInvalidValue, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return launch_lds<OTH_JACKCSD_KERNEL(N)>(grid, dim3(stat_threads(N)), jackcsd_lds_bytes(N), s, a);
    });
}

hipError_t launch_jack_finalize(const JackFinalizeArgs &a, int nstreams, hipStream_t s) {
    return launch_stat_finalize<jack_finalize_kernel>(a, nstreams, 1, s);
}

}  // namespace oth
