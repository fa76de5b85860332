// median.hip: the median over segments of every bin of every stream - scipy.signal.welch(average='median') before the
// bias division - as an exact radix select over the float bit patterns of the periodogram rows.
//
// Every value is |X|^2 >= +0, so its uint32 bit pattern orders like the float (the sign bit is masked off: -0 counts as
// +0; patterns above 0x7f800000 are NaN and mark the bin).  Four passes of 8-bit digits from the top:
//   histogram  a workgroup owns kMedianTile contiguous bins (one per lane: a wave reads 256 contiguous bytes of a row)
//              and a chunk of segments; its four waves walk the chunk and count, into an LDS histogram [digit][bin]
//              (bank = lane: every ds_add_u32 is conflict-free), the values whose higher digits equal the bin's prefix.
//              The non-zero counts go to [stream][bin][256] with integer atomics (64 consecutive digits of one bin per
//              wave instruction: two cache lines).
//   scan       one wave per bin: prefix sum of the 256 counts, the digit that holds the remaining rank, the new prefix
//              and rank; the counts are zeroed behind it for the next pass.
// Counts are integers, so the result is the same bits under any schedule and any workgroup order.  Even nseg needs ranks k
// and k + 1: only k is carried through the passes; the last pass also records the smallest key above k's 24-bit bucket,
// and rank k + 1 is then k's own value (the bucket's count allows it), the next digit of the last histogram, or that key.
#include "fft_lds.hip.h"
#include "oth_internal.h"

namespace oth {
namespace {

constexpr int kMedBlock = 256;      // four waves per histogram workgroup
constexpr int kMedUnroll = 16;      // row loads in flight per wave

__global__ __launch_bounds__(256) void median_init_kernel(MedianArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.nstreams * a.nfft) return;
    a.state[2 * i] = 0u;
    a.state[2 * i + 1] = (unsigned)((a.nseg - 1) >> 1);      // rank k of the (lower) middle value
    a.above[i] = 0xffffffffu;
    a.nanflag[i] = 0u;
}

// KIND 0: first pass (every value counts; NaN flags), 1: middle passes, 2: last pass (+ smallest key above the bucket)
template <int KIND>
__global__ __launch_bounds__(kMedBlock) void median_hist_kernel(MedianArgs a, int shift) {
    __shared__ unsigned hist[256 * kMedianTile];      // [digit][bin of the tile]
    for (int i = threadIdx.x; i < 256 * kMedianTile / 4; i += kMedBlock) reinterpret_cast<uint4 *>(hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = blockIdx.x * kMedianTile + lane, stream = blockIdx.z;
    const bool live = bin < a.nfft;
    const size_t sb = (size_t)stream * a.nfft + (live ? bin : 0);
    const unsigned prefix = KIND == 0 ? 0u : a.state[2 * sb];
    const unsigned hmask = KIND == 0 ? 0u : (0xffffffffu << (shift + 8));
    const unsigned top = prefix | ~hmask;      // largest key of the bin's bucket
    const long long s0 = a.seg_per_wg * (long long)blockIdx.y;
    const long long s1 = s0 + a.seg_per_wg < a.nseg ? s0 + a.seg_per_wg : a.nseg;
    const unsigned *base = a.rows + (size_t)stream * (size_t)a.nseg * a.nfft + (live ? bin : 0);
    unsigned *h = hist + lane;
    bool nan = false;
    unsigned above = 0xffffffffu;
    auto count = [&](unsigned key) {
        key &= 0x7fffffffu;
        if (KIND == 0) nan = nan || key > 0x7f800000u;
        if ((key & hmask) == prefix) atomicAdd(h + ((key >> shift) & 255u) * kMedianTile, 1u);
        if (KIND == 2 && key > top) above = key < above ? key : above;
    };
    if (live) {
        long long s = s0 + wave;
        for (; s + 4 * (kMedUnroll - 1) < s1; s += 4 * kMedUnroll) {
            unsigned k[kMedUnroll];
#pragma unroll
            for (int u = 0; u < kMedUnroll; ++u) k[u] = base[(size_t)(s + 4 * u) * a.nfft];
#pragma unroll
            for (int u = 0; u < kMedUnroll; ++u) count(k[u]);
        }
        for (; s < s1; s += 4) count(base[(size_t)s * a.nfft]);
        if (KIND == 0 && nan) atomicOr(a.nanflag + sb, 1u);
        if (KIND == 2 && above != 0xffffffffu) atomicMin(a.above + sb, above);
    }
    __syncthreads();
    // flush: a wave takes 64 consecutive digits of one bin (coalesced atomics; the LDS reads of the flush conflict, once
    // per workgroup)
    for (int i = threadIdx.x; i < 256 * kMedianTile; i += kMedBlock) {
        const int d = i & 255, b = i >> 8;
        const unsigned cnt = hist[d * kMedianTile + b];
        const int gb = blockIdx.x * kMedianTile + b;
        if (cnt && gb < a.nfft) atomicAdd(a.counts + ((size_t)stream * a.nfft + gb) * 256 + d, cnt);
    }
}

// one wave per (stream, bin); LAST: the pass of the lowest digit - writes the median
template <bool LAST>
__global__ __launch_bounds__(256) void median_scan_kernel(MedianArgs a, int shift) {
    const int lane = threadIdx.x & 63;
    const size_t sb = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sb >= (size_t)a.nstreams * a.nfft) return;      // (wave-uniform)
    uint4 *cp = reinterpret_cast<uint4 *>(a.counts + sb * 256) + lane;
    const uint4 c4 = *cp;
    *cp = make_uint4(0u, 0u, 0u, 0u);      // clean for the next pass / call
    const unsigned cnt[4] = {c4.x, c4.y, c4.z, c4.w};
    const unsigned tot = c4.x + c4.y + c4.z + c4.w;
    unsigned incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const unsigned excl = incl - tot;
    const unsigned prefix = a.state[2 * sb], rank = a.state[2 * sb + 1];
    const bool mine = rank >= excl && rank < incl;
    unsigned d = 0, r = rank - excl, cd = 0;
    if (mine) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (r < cnt[j]) {
                d = 4 * lane + j;
                cd = cnt[j];
                break;
            }
            r -= cnt[j];
        }
    }
    const unsigned long long m = __ballot(mine);
    const int src = m ? __ffsll((long long)m) - 1 : 0;
    d = __shfl(d, src, 64);
    r = __shfl(r, src, 64);
    cd = __shfl(cd, src, 64);
    if (!LAST) {
        if (lane == 0) {
            a.state[2 * sb] = prefix | (d << shift);
            a.state[2 * sb + 1] = r;
        }
        return;
    }
    // rank k + 1 (even nseg): the same value, the next digit present in this bucket, or the smallest key above it
    unsigned nxt = 256u;
#pragma unroll
    for (int j = 3; j >= 0; --j)
        if (4u * lane + j > d && cnt[j]) nxt = 4u * lane + j;
    nxt = wave_reduce(nxt, [](unsigned v, unsigned w) { return w < v ? w : v; });
    if (lane == 0) {
        const unsigned klo = prefix | d;
        const unsigned khi = r + 1 < cd ? klo : (nxt < 256u ? (prefix | nxt) : a.above[sb]);
        float v;
        if (a.nanflag[sb] || !m) {
            v = __builtin_nanf("");
        } else if (a.nseg & 1) {
            v = __uint_as_float(klo);
        } else {
            v = (__uint_as_float(klo) + __uint_as_float(khi)) * 0.5f;      // np.median: the mean of the two
        }
        a.med[sb] = v;
    }
}

}  // namespace

size_t median_scratch_words(int nfft, int nstreams) { return (size_t)nstreams * nfft * (256 + 2 + 1 + 1); }

void median_bind_scratch(MedianArgs &a, unsigned *scratch) {
    const size_t n = (size_t)a.nstreams * a.nfft;
    a.counts = scratch;
    a.state = scratch + 256 * n;
    a.above = a.state + 2 * n;
    a.nanflag = a.above + n;
}

// segments per histogram workgroup: about four workgroups per CU over the launch (fewer chunks = fewer count atomics),
// at least 256 segments each
long long median_seg_per_wg(long long nseg, int nfft, int nstreams, int cu_count) {
    const long long tiles = (long long)((nfft + kMedianTile - 1) / kMedianTile) * nstreams;
    long long chunks = (4LL * cu_count + tiles - 1) / tiles;
    const long long most = (nseg + 255) / 256;
    if (chunks > most) chunks = most;
    if (chunks > 65535) chunks = 65535;
    if (chunks < 1) chunks = 1;
    return (nseg + chunks - 1) / chunks;
}

hipError_t launch_median_select(const MedianArgs &a, hipStream_t s) {
    const size_t n = (size_t)a.nstreams * a.nfft;
    hipError_t e = hipMemsetAsync(a.counts, 0, sizeof(unsigned) * 256 * n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(median_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    const dim3 hg((unsigned)((a.nfft + kMedianTile - 1) / kMedianTile), (unsigned)((a.nseg + a.seg_per_wg - 1) / a.seg_per_wg),
                  (unsigned)a.nstreams);
    const dim3 sg((unsigned)((n + 3) / 4));
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (pass == 0) hipLaunchKernelGGL(median_hist_kernel<0>, hg, dim3(kMedBlock), 0, s, a, shift);
        else if (pass < 3) hipLaunchKernelGGL(median_hist_kernel<1>, hg, dim3(kMedBlock), 0, s, a, shift);
        else hipLaunchKernelGGL(median_hist_kernel<2>, hg, dim3(kMedBlock), 0, s, a, shift);
        if (pass < 3) hipLaunchKernelGGL(median_scan_kernel<false>, sg, dim3(256), 0, s, a, shift);
        else hipLaunchKernelGGL(median_scan_kernel<true>, sg, dim3(256), 0, s, a, shift);
    }
    return hipGetLastError();
}

}  // namespace oth
