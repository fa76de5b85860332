// The body of mateig.hip's kernels, included once per kernel: mat_eig_kernel<CC, T, VEC>(MatEigArgs a) with
// OTH_MAT_EIG_BASIS 0, and mat_eig_basis_kernel<CC, T>(MatEigArgs a, double *basis) with OTH_MAT_EIG_BASIS 1 and VEC = true,
// which shares everything up to the end of the sweep loop and then stores the ranked decomposition to `basis`.  It is text,
// not a function: the body as an inlined device function gave the six builds of mat_eig_kernel another register allocation
// (130 VGPRs for 106 at (8, vector)), and their code objects are to stay what they were.  No include guard.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int P = CC * (CC + 1) / 2;
    const int t = threadIdx.x, k = blockIdx.x * T + t, C = a.nchan;
    double *are = reinterpret_cast<double *>(smem) + t, *aim = are + P * T;      // [entry] at entry * T
    double *vre = aim + P * T, *vim = vre + (VEC ? CC * CC * T : 0);             // [row CC + column], with VEC only
    int i;
    if (!out_slot(a.out, a.nfft, k, i)) return;      // no barrier below: a thread works in its own column
    const size_t n = (size_t)a.nfft, nout = (size_t)a.out.nout;
    const double *tot = a.totals + k;
    bool empty = false, bad = false;
    for (int c = 0; c < C; ++c) {
        const double d = tot[(size_t)(c * C + c) * n];
        if (!isfinite(d)) bad = true;
        else if (d <= 0.0) empty = true;
    }
    if (bad) {
#if OTH_MAT_EIG_BASIS      // the direction stage reads the bin's NaN off its first eigenvalue
        basis[k] = __builtin_nan("");
#else
        const float nanf32 = __builtin_nanf("");
        for (int c = 0; c < C; ++c) {
            if (a.eig_out) a.eig_out[c * nout + i] = nanf32;
            if (VEC) a.vec_out[2 * (c * nout + i)] = a.vec_out[2 * (c * nout + i) + 1] = nanf32;
        }
#endif
        return;
    }
    const bool ofg = a.of != 0;
#pragma unroll
    for (int r = 0; r < CC; ++r) {
        if (r < C) {      // uniform
            const double trr = tot[(size_t)(r * C + r) * n];
#pragma unroll
            for (int c = r; c < CC; ++c) {
                if (c < C) {
                    const double tcc = tot[(size_t)(c * C + c) * n];
                    const double re = tot[(size_t)(r * C + c) * n], im = c > r ? tot[(size_t)(c * C + r) * n] : 0.0;
                    double xr, xi;
                    if (ofg) {
                        const double inv = empty ? 0.0 : 1.0 / sqrt(trr * tcc);
                        xr = c == r ? 1.0 : empty ? 0.0 : re * inv;
                        xi = c == r || empty ? 0.0 : im * inv;
                    } else {
                        const bool zero = trr <= 0.0 || tcc <= 0.0;
                        xr = zero ? 0.0 : re * a.s_scale;
                        xi = zero || c == r ? 0.0 : im * a.s_scale;
                    }
                    are[eig_at<CC>(r, c) * T] = xr;
                    aim[eig_at<CC>(r, c) * T] = xi;
                }
            }
        }
    }
    if constexpr (VEC) {
#pragma unroll
        for (int r = 0; r < CC; ++r)
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (r < C && c < C) {
                    vre[(r * CC + c) * T] = r == c ? 1.0 : 0.0;
                    vim[(r * CC + c) * T] = 0.0;
                }
    }

    for (int sweep = 0; sweep < kMatEigSweepCap; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int r = 0; r < CC; ++r) {
            if (r < C) {
                const double d = are[eig_at<CC>(r, r) * T];
                diag += d * d;
#pragma unroll
                for (int c = r + 1; c < CC; ++c) {
                    if (c < C) {
                        const double x = are[eig_at<CC>(r, c) * T], y = aim[eig_at<CC>(r, c) * T];
                        off += x * x + y * y;
                    }
                }
            }
        }
        if (2.0 * off <= kMatEigTol * diag) break;
#pragma unroll
        for (int p = 0; p < CC - 1; ++p) {
#pragma unroll
            for (int q = p + 1; q < CC; ++q) {
                if (q < C) {      // uniform
                    const double x = are[eig_at<CC>(p, q) * T], y = aim[eig_at<CC>(p, q) * T];
                    const double g = sqrt(x * x + y * y);
                    if (g != 0.0) {
                        const double app = are[eig_at<CC>(p, p) * T], aqq = are[eig_at<CC>(q, q) * T];
                        const double tau = (aqq - app) / (2.0 * g);
                        const double tt = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = tt * cs;
                        const double sr = sn * (x / g), si = sn * (y / g);      // s e^(i phi)
                        are[eig_at<CC>(p, p) * T] = app - tt * g;
                        are[eig_at<CC>(q, q) * T] = aqq + tt * g;
                        are[eig_at<CC>(p, q) * T] = 0.0;
                        aim[eig_at<CC>(p, q) * T] = 0.0;
#pragma unroll
                        for (int r = 0; r < CC; ++r) {
                            if (r != p && r != q && r < C) {
                                // a_rp and a_rq from the upper triangle: the stored entry, or its conjugate below the diagonal
                                const int ip = (r < p ? eig_at<CC>(r, p) : eig_at<CC>(p, r)) * T;
                                const int iq = (r < q ? eig_at<CC>(r, q) : eig_at<CC>(q, r)) * T;
                                const double fp = r < p ? 1.0 : -1.0, fq = r < q ? 1.0 : -1.0;
                                const double pr = are[ip], pi = fp * aim[ip], qr = are[iq], qi = fq * aim[iq];
                                const double npr = cs * pr - (sr * qr + si * qi), npi = cs * pi - (sr * qi - si * qr);
                                const double nqr = (sr * pr - si * pi) + cs * qr, nqi = (sr * pi + si * pr) + cs * qi;
                                are[ip] = npr;
                                aim[ip] = fp * npi;
                                are[iq] = nqr;
                                aim[iq] = fq * nqi;
                            }
                        }
                        if constexpr (VEC) {
#pragma unroll
                            for (int r = 0; r < CC; ++r) {
                                if (r < C) {
                                    const int ip = (r * CC + p) * T, iq = (r * CC + q) * T;
                                    const double pr = vre[ip], pi = vim[ip], qr = vre[iq], qi = vim[iq];
                                    vre[ip] = cs * pr - (sr * qr + si * qi);
                                    vim[ip] = cs * pi - (sr * qi - si * qr);
                                    vre[iq] = (sr * pr - si * pi) + cs * qr;
                                    vim[iq] = (sr * pi + si * pr) + cs * qi;
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    // every eigenvalue to the row of its rank, descending; the largest one's index (the lowest of equals) picks V's column
    int top = 0;
#pragma unroll
    for (int j = 0; j < CC; ++j) {
        if (j < C) {
            const double d = are[eig_at<CC>(j, j) * T];
            int rank = 0;
#pragma unroll
            for (int m = 0; m < CC; ++m) {
                if (m < C && m != j) {
                    const double e = are[eig_at<CC>(m, m) * T];
                    rank += (e > d || (e == d && m < j)) ? 1 : 0;
                }
            }
            if (rank == 0) top = j;
#if OTH_MAT_EIG_BASIS      // the eigenvalue and column j of V to the rows of their rank
            basis[(size_t)rank * n + k] = d < 0.0 ? 0.0 : d;
#pragma unroll
            for (int r = 0; r < CC; ++r) {
                if (r < C) {
                    basis[(size_t)mat_basis_at(CC, rank, r) * n + k] = vre[(r * CC + j) * T];
                    basis[(size_t)(mat_basis_at(CC, rank, r) + 1) * n + k] = vim[(r * CC + j) * T];
                }
            }
#else
            if (a.eig_out) a.eig_out[rank * nout + i] = (float)(d < 0.0 ? 0.0 : d);
#endif
        }
    }
#if OTH_MAT_EIG_BASIS
    (void)top, (void)nout, (void)i;
#else
    if constexpr (VEC) {
        const double zr = vre[top * T], zi = vim[top * T];      // component 0
        const double z = sqrt(zr * zr + zi * zi);
        const double ur = z != 0.0 ? zr / z : 1.0, ui = z != 0.0 ? -zi / z : 0.0;      // conj(v_0) / |v_0|
#pragma unroll
        for (int r = 0; r < CC; ++r) {
            if (r < C) {
                const double xr = vre[(r * CC + top) * T], xi = vim[(r * CC + top) * T];
                double wr = xr * ur - xi * ui, wi = xr * ui + xi * ur;
                if (r == 0 && z != 0.0) wr = z, wi = 0.0;
                a.vec_out[2 * (r * nout + i)] = (float)wr;
                a.vec_out[2 * (r * nout + i) + 1] = (float)wi;
            }
        }
    }
#endif
