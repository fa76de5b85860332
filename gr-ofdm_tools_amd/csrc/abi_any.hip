// C ABI, host side.
#include "abi_state.h"

// ---- the any-length route (fft_any.hip, round 6) -----------------------------------------------------------------------
// Lengths the power-of-two kernels do not take: any_describe() picks direct / two-level / Bluestein; the tables below are
// built once per plan or chain, any_run() drives the launches of one averaging (or periodogram-row) request.

namespace {
// workspace of a chunk: it and the chunk's samples stay in the Infinity Cache (OTH_ANY_WS_MB: A/B of the chunk size)
size_t any_ws_bytes() {
    const char *e = getenv("OTH_ANY_WS_MB");      // (read per call: the tests shrink it to cross chunk boundaries on small inputs)
    const long mb = e ? atol(e) : 0;
    return (size_t)(mb > 0 ? mb : 128) << 20;
}
constexpr int kAnyRowTile = 16;                // rows of L2 points a K2 workgroup transforms together

// Forward transform of ONE length-L vector, natural order in and out, in place in `data` (L points); L is a power of two
// or smooth (kind ANY_DIRECT / ANY_TWOLEVEL of `sh`); tmp: L points (the two-level route's reordering).
int any_fft_nat_inner(oth_ctx *c, const AnyShape &sh, const float2 *tw, float2 *data, float2 *tmp) {
    AnyArgs a{};
    a.nseg = 1;
    a.ws = data;
    a.load_op = 0;
    if (sh.kind == ANY_DIRECT) {
        any_make_desc(sh.L, 1, tw, sh.L, &a.f);
        a.es = 1, a.cs = 1, a.inv_n = 1.0f / (float)sh.L;
        HIPCHK(c, launch_any_fft(a, 1, 1, 1, 0, c->stream));
        return OTH_OK;
    }
    AnyArgs k1 = a;
    any_make_desc(sh.L1, sh.C, tw, sh.L, &k1.f);
    k1.es = sh.L2, k1.tile_stride = sh.C, k1.cs = 1, k1.inv_n = 1.0f / (float)sh.L1;
    k1.twbig = tw;
    k1.tw_t = sh.C, k1.tw_c = 1;
    HIPCHK(c, launch_any_fft(k1, sh.L2 / sh.C, 1, 1, 0, c->stream));
    AnyArgs k2 = a;
    any_make_desc(sh.L2, kAnyRowTile, tw, sh.L, &k2.f);
    k2.es = 1, k2.tile_stride = kAnyRowTile * sh.L2, k2.cs = sh.L2, k2.inv_n = 1.0f / (float)sh.L2;
    HIPCHK(c, launch_any_fft(k2, sh.L1 / kAnyRowTile, 1, 1, 0, c->stream));
    HIPCHK(c, launch_any_ew(3, tmp, data, nullptr, nullptr, sh.L, sh.L, sh.L1, sh.L2, c->stream));      // [k1][k2] -> k1 + L1 k2
    HIPCHK(c, hipMemcpyAsync(data, tmp, sizeof(float2) * (size_t)sh.L, hipMemcpyDeviceToDevice, c->stream));
    return OTH_OK;
}
}  // namespace

namespace oth {
void host_fft_pow2(std::vector<double> &re, std::vector<double> &im) {      // in place, forward, n a power of two
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(re[i], re[j]);
            std::swap(im[i], im[j]);
        }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double ang = -2.0 * M_PI / (double)len;
        for (size_t j = 0; j < len / 2; ++j) {
            const double c = cos(ang * (double)j), sn = sin(ang * (double)j);
            for (size_t i = j; i < n; i += len) {
                const size_t b = i + len / 2;
                const double tr = re[b] * c - im[b] * sn, ti = re[b] * sn + im[b] * c;
                re[b] = re[i] - tr;
                im[b] = im[i] - ti;
                re[i] += tr;
                im[i] += ti;
            }
        }
    }
}

// tables of a length-nfft transform; the caller synchronises the stream before the host vectors die (done here)
int any_tables_init(oth_ctx *c, int nfft, AnyTables *t) {
    if (any_describe(nfft, &t->sh))
        return fail(c, OTH_ERR_UNSUPPORTED, "transform length outside [1, 1048576] (lengths that are not 2-3-5-7-smooth or exceed "
                                            "16384 without being a power of two run as Bluestein transforms of 2^ceil(log2(2 n - 1)) "
                                            "<= 1048576 points: n <= 524288)");
    int rc = get_twiddles(c, t->sh.L, &t->tw);
    if (rc) return rc;
    if (t->sh.kind == ANY_BLUESTEIN || t->sh.kind == ANY_BLUESTEIN2) {
        const int N = nfft, M = t->sh.L;
        std::vector<float2> ch(N), mt(M);
        std::vector<double> bre(M, 0.0), bim(M, 0.0);
        for (int n = 0; n < N; ++n) {
            const long long q = ((long long)n * (long long)n) % (2LL * N);      // the chirp's phase, reduced exactly
            const double a = M_PI * (double)q / (double)N;
            ch[n] = make_float2((float)cos(a), (float)-sin(a));                  // c[n] = exp(-i pi n^2 / N)
            bre[n] = cos(a);                                                     // b[n] = conj(c[n]), b[M - n] = b[n]
            bim[n] = sin(a);
            if (n) {
                bre[M - n] = bre[n];
                bim[M - n] = bim[n];
            }
        }
        host_fft_pow2(bre, bim);
        for (int k = 0; k < M; ++k) mt[k] = make_float2((float)(bre[k] / M), (float)(bim[k] / M));
        hipError_t e = t->chirp.upload(c, ch.data(), sizeof(float2) * N);
        if (e == hipSuccess) e = t->midtab.upload(c, mt.data(), sizeof(float2) * M);
        hipError_t es = hipStreamSynchronize(c->stream);      // also after a failure: the host vectors die here
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) {
            *t = AnyTables{};
            return fail(c, OTH_ERR_HIP, std::string("any-length tables: ") + hipGetErrorString(e));
        }
    }
    return OTH_OK;
}

// partial rows (per stream) an averaging launch of this shape leaves; pure host logic (the recipe text carries it)
int any_partial_rows(const AnyShape &sh, long long nseg, int cu_count) {
    long long w;
    if (sh.kind == ANY_DIRECT || sh.kind == ANY_BLUESTEIN) {
        // workgroups per CU by LDS footprint (tile + the staged twiddles where any_make_desc puts them there), at most 16:
        // the single-column builds hold ~100 registers, five 64-thread workgroups per SIMD
        const long long tile = (long long)sh.L * 8, both = 2 * tile;
        const long long lds = (both <= 64 * 1024 || (tile > 64 * 1024 && both <= 150 * 1024)) ? both : tile;
        long long occ = (150 * 1024) / lds;
        occ = occ < 1 ? 1 : (occ > 16 ? 16 : occ);
        w = (long long)cu_count * occ;
    } else {
        static const char *e = getenv("OTH_ANY_TL_W");      // (A/B of the partial-row count of the two-level routes)
        w = e && atoi(e) > 0 ? atoi(e) : 64;
    }
    if (w > nseg) w = nseg;
    if (w > 65535) w = 65535;
    return (int)(w < 1 ? 1 : w);
}

// nseg segments starting at x[first + s seg_step] (nperseg samples, window win, optional constant detrend) -> either the
// W x nch partial rows of |X|^2 (cross) sums (rows == nullptr; ROW_NATURAL, or ROW_TWOLEVEL = [k1][k2] for the two-level route), or one
// periodogram row per segment (rows != nullptr: epilogue / scale / fftshift as PgramArgs).  nbins = t.sh.nfft.
int any_run(oth_ctx *c, AnyTables &t, const float2 *x, const float2 *y, long long first, long long seg_step, int nperseg,
            const float *win, bool detrend, long long nseg, float *partial, int W, float *rows, int epilogue, float scale,
            int fftshift, bool coverage_only) {
    const AnyShape &sh = t.sh;
    const int nch = y ? 2 : 1, N = sh.nfft, L = sh.L;
    const bool two = sh.kind == ANY_TWOLEVEL || sh.kind == ANY_BLUESTEIN2, blu = sh.kind == ANY_BLUESTEIN || sh.kind == ANY_BLUESTEIN2;
    const int acc_store = y ? 2 : 1;
    long long B = two ? (long long)(any_ws_bytes() / (sizeof(float2) * (size_t)L * nch)) : (1LL << 20);
    if (B < 1) B = 1;
    if (B > nseg) B = nseg;
    int rc;
    if (two && (rc = t.ws.ensure(c, sizeof(float2) * (size_t)L * nch * (size_t)B))) return rc;
    // (the fast two-level route keeps sub-block sums there instead: at most B * seg_step / kTlSub + nperseg / kTlSub of them)
    const size_t nsums = nch * ((size_t)B * (size_t)(seg_step / kTlSub + 1) + (size_t)(nperseg / kTlSub) + 1);
    if (detrend && (rc = t.mean.ensure(c, sizeof(float4) * std::max(nch * (size_t)B, nsums)))) return rc;
    AnyFftDesc d_one{}, d_col{}, d_row{};
    if (two) {
        any_make_desc(sh.L1, sh.C, t.tw, L, &d_col);
        any_make_desc(sh.L2, kAnyRowTile, t.tw, L, &d_row);
    } else {
        any_make_desc(L, 1, t.tw, L, &d_one);
    }
    for (long long s0 = 0; s0 < nseg; s0 += B) {
        const long long nb = nseg - s0 < B ? nseg - s0 : B;
        const long long cfirst = first + s0 * seg_step;
        AnyArgs a{};
        // what every launch of the chunk shares
        a.nseg = nb;
        a.x = x;
        a.y = y;
        a.first = cfirst;
        a.seg_step = seg_step;
        a.nperseg = nperseg;
        a.win = win;
        a.mean = detrend ? t.mean.get() : nullptr;
        a.mean_ch_stride = (size_t)B;
        a.ws = t.ws.get();
        a.ws_seg_stride = (size_t)L;
        a.ws_ch_stride = (size_t)L * (size_t)B;
        a.midtab = t.midtab.get();
        a.partial = partial;
        a.nbins = N;
        a.first_chunk = s0 == 0;
        a.conj_out = blu ? 1 : 0;
        a.rows = rows ? rows + (size_t)s0 * N : nullptr;
        a.epilogue = epilogue;
        a.scale = scale;
        a.fftshift = fftshift;
        const int gy_rows = (int)(nb < 65535 ? nb : 65535);
        if (sh.kind == ANY_TWOLEVEL && tl_supported(L) && !rows && !coverage_only) {
            // 32768 / 65536 points, averages (one or two channels): the register radix-16 kernels of fft_tl.hip
            const bool blocks = detrend && nperseg % kTlSub == 0 && seg_step % kTlSub == 0;      // (t.mean holds B float4 = B double2)
            TlArgs ta{};
            ta.x = x, ta.y = y, ta.first = cfirst, ta.seg_step = seg_step, ta.nperseg = nperseg, ta.win = win;
            ta.ws = t.ws.get(), ta.ws_seg_stride = (size_t)L, ta.ws_ch_stride = (size_t)L * (size_t)B, ta.nseg = nb, ta.tw = t.tw;
            ta.partial = partial, ta.first_chunk = s0 == 0;
            if (blocks) {
                ta.nsub = nperseg / kTlSub, ta.sub_step = (int)(seg_step / kTlSub);
                const long long nblk = (nb - 1) * ta.sub_step + ta.nsub;
                ta.aux_ch_stride = (size_t)nblk;
                ta.bsum = reinterpret_cast<const double2 *>(t.mean.get());
                for (int ch = 0; ch < nch; ++ch)
                    HIPCHK(c, launch_tl_blocksum(ch ? y : x, cfirst, nblk, reinterpret_cast<double2 *>(t.mean.get()) + (size_t)ch * nblk, c->stream));
            } else if (detrend) {
                ta.mean = t.mean.get();
                ta.aux_ch_stride = (size_t)B;
                for (int ch = 0; ch < nch; ++ch)
                    HIPCHK(c, launch_tl_mean(ch ? y : x, cfirst, seg_step, nperseg, nb, t.mean.get() + (size_t)ch * B, c->stream));
            }
            HIPCHK(c, launch_tl_k1(L, ta, c->stream));
            HIPCHK(c, launch_tl_k2(L, ta, W, c->stream));
            continue;
        }
        if (detrend) HIPCHK(c, launch_any_mean(x, y, cfirst, seg_step, nperseg, nb, t.mean.get(), (size_t)B, c->stream));
        if (!two) {
            // one launch: a workgroup per segment (rows W of the partial buffer), nothing leaves LDS
            a.f = d_one;
            a.es = 1, a.tile_stride = 0, a.cs = 1, a.inv_n = 1.0f / (float)L;
            a.load_op = 1;
            a.chirp = blu ? t.chirp.get() : nullptr;
            a.mid_op = blu ? 1 : 0;
            a.nat_i = 1, a.pp_i = 1;
            HIPCHK(c, launch_any_fft(a, 1, rows ? gy_rows : W, 1, rows ? 3 : acc_store, c->stream));
            continue;
        }
        // K1: tiles of C columns (stride L2) of every segment, transform along L1, x W_L^(k1 n2), into the workspace
        AnyArgs k1 = a;
        k1.f = d_col;
        k1.es = sh.L2, k1.tile_stride = sh.C, k1.cs = 1, k1.inv_n = 1.0f / (float)sh.L1;
        k1.load_op = 1;
        k1.chirp = blu ? t.chirp.get() : nullptr;
        k1.twbig = t.tw;
        k1.tw_t = sh.C, k1.tw_c = 1;
        HIPCHK(c, launch_any_fft(k1, sh.L2 / sh.C, gy_rows, nch, 0, c->stream));
        // K2: tiles of kAnyRowTile rows k1 (L2 contiguous points each), transform along L2: bins k1 + L1 k2
        AnyArgs k2 = a;
        k2.f = d_row;
        k2.es = 1, k2.tile_stride = kAnyRowTile * sh.L2, k2.cs = sh.L2, k2.inv_n = 1.0f / (float)sh.L2;
        k2.load_op = 0;
        k2.nat_i = sh.L1, k2.nat_t = kAnyRowTile, k2.nat_c = 1;
        if (!blu) {
            k2.pp_i = 1, k2.pp_t = kAnyRowTile * sh.L2, k2.pp_c = sh.L2;      // partial rows in [k1][k2] order (ROW_TWOLEVEL)
            HIPCHK(c, launch_any_fft(k2, sh.L1 / kAnyRowTile, rows ? gy_rows : W, 1, rows ? 3 : acc_store, c->stream));
            continue;
        }
        // Bluestein: K2 = row transform, x B / M, conj, row transform, x W_L^(n2 k1), in place ...
        k2.mid_op = 1;
        k2.twbig = t.tw;
        k2.tw_t = kAnyRowTile, k2.tw_c = 1;
        HIPCHK(c, launch_any_fft(k2, sh.L1 / kAnyRowTile, gy_rows, nch, 0, c->stream));
        // ... K3 = column transform along L1 -> natural order n1 L2 + n2; the first nfft outputs are (conj of) X
        AnyArgs k3 = a;
        k3.f = d_col;
        k3.es = sh.L2, k3.tile_stride = sh.C, k3.cs = 1, k3.inv_n = 1.0f / (float)sh.L1;
        k3.load_op = 0;
        k3.nat_i = sh.L2, k3.nat_t = sh.C, k3.nat_c = 1;
        k3.pp_i = sh.L2, k3.pp_t = sh.C, k3.pp_c = 1;
        HIPCHK(c, launch_any_fft(k3, sh.L2 / sh.C, rows ? gy_rows : W, 1, rows ? 3 : acc_store, c->stream));
    }
    return OTH_OK;
}

// np.fft.fft of one length-nfft vector in `data` (natural order, in place) for every route; scratch as above
int any_fft_nat(oth_ctx *c, const AnyTables &t, float2 *data, float2 *scratch) {
    const AnyShape &sh = t.sh;
    if (sh.kind == ANY_DIRECT || sh.kind == ANY_TWOLEVEL) return any_fft_nat_inner(c, sh, t.tw, data, scratch);
    AnyShape in{};
    if (any_describe(sh.L, &in)) return fail(c, OTH_ERR_INTERNAL, "Bluestein length has no route");
    float2 *A = scratch, *tmp = scratch + sh.L;
    int rc;
    HIPCHK(c, launch_any_ew(0, A, data, nullptr, t.chirp.get(), sh.L, sh.nfft, 0, 0, c->stream));      // a = x c, zero padded to M
    if ((rc = any_fft_nat_inner(c, in, t.tw, A, tmp))) return rc;
    HIPCHK(c, launch_any_ew(1, A, A, nullptr, t.midtab.get(), sh.L, sh.L, 0, 0, c->stream));            // conj(A B / M)
    if ((rc = any_fft_nat_inner(c, in, t.tw, A, tmp))) return rc;
    HIPCHK(c, launch_any_ew(2, data, A, nullptr, t.chirp.get(), sh.nfft, sh.nfft, 0, 0, c->stream));    // X = conj(.) c
    return OTH_OK;
}
}  // namespace oth
