// The Kolmogorov-Smirnov tail of rare classes as device code (tsfa_ks_matrix_tails and ks_tail = TSFA_KS_TAIL_DEVICE_MATRIX of
// tsfa_relevance_tails_*, include/tsfresh_amd.h): the cells rel_ks_large.h leaves as TSFA_ROUTE_HOST_KS although a sample is
// longer than RK_MAX_ROWS, because scipy.stats.kstwo.sf(d, n), n = round(n1 n2 / (n1 + n2)), takes Durbin's matrix or
// Pomeranz's recursion there.  Restated from scipy/stats/_ksstats.py (1.15): _kolmogn, _kolmogn_DMTW, _kolmogn_Pomeranz and
// _pomeranz_compute_j1j2, in float64 (1e-6 relative to the host's value, not bit for bit).
//
// With x = d, t = n x and nxsq = t x, formed in float64 exactly so (-ffp-contract=off), _kolmogn(n, x, cdf=False) takes
//   n <= 140:   x >= 1 -> 0,  x <= 0 -> 1,  t <= 0.5 -> 1
//               t <= 1            1 - prod_{i = 1 .. n} (i (1 / n)) (2 t - 1)      (the product, not the Stirling form)
//               t >= n - 1        2 (1 - x)^n
//               x >= 0.5          2 P(D+ >= x)                                     (ksl_smirnov of rel_ks_large.h)
//               nxsq <= 0.754693  1 - cdf by Durbin's matrix                       (KSM_DURBIN_SMALL: m = 2 k - 1 <= 21)
//               nxsq <= 4         1 - cdf by Pomeranz's recursion                  (KSM_POMERANZ)
//               otherwise         2 P(D+ >= x)
//   141 <= n <= 100 000:  only the cell ksl_branch leaves for this reason: 1 < t < n - 1, x < 0.5, nxsq < 2.2 and
//               n x^1.5 <= 1.4    1 - cdf by Durbin's matrix                       (KSM_DURBIN_LARGE: m <= 117)
// ksm_branch uses ksl_branch's own expressions in ksl_branch's order, so a cell at a seam falls to exactly one stage.
// The sum's shift L = -2 nxsq (rel_ks_large.h) needs exp(-2 nxsq) <= 1/2, nxsq >= 0.347: here the sum serves nxsq > 4, or
// x >= 0.5 with 1 < t < n - 1, which needs n >= 3 and so nxsq >= 0.75.
//
// Durbin's matrix (Marsaglia, Tsang and Wang 2003): with k = ceil(n x), h = k - n x, m = 2 k - 1, cdf = (n! / n^n) (H^n)[k-1][k-1]
// for the m x m matrix H of ksm_h_at.  H is squared bit by bit of n; of the running power only ROW k - 1 is kept, a vector
// r <- r H before every squaring that the bit of n asks for.  Scaling as _kolmogn_DMTW: H by 2^-128 whenever its entry
// [k-1][k-1] exceeds 2^128 after a squaring, the exponent carried as an integer.  (r is scaled the same way, which scipy does
// not need in float64's range and which changes no bit: a power of two.)  The squaring after the last bit of n is not made.
//   ksm_durbin_small   ONE WAVEFRONT per cell: H and its square ping-pong in the wavefront's 8 KB of LDS, lane = entry; then
//                      the loop p <- i p / n with its scaling, ldexp and clip(1 - cdf), as scipy
//   ksm_durbin_large   ONE WORKGROUP of 512 per cell: H padded to M = 16 T <= 128 rows of M + 2 doubles in LDS (at most
//                      133 KB: a second matrix does not fit), squared IN PLACE: the T^2 tiles of 16 x 16 are dealt over the 8
//                      wavefronts, tile q to wavefront q mod 8, each accumulated in 4 registers a lane by
//                      v_mfma_f64_16x16x4_f64 (operands as k_cwt_gemm: A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15],
//                      D[i = 4 v + (lane >> 4)][j]); barrier; the tiles are stored over H; barrier.  n! / n^n by the Stirling
//                      series of rel_ks_large.h in place of up to 100 000 dependent divisions: cdf <= 0.1 in this branch, so
//                      its 1e-11 does not show in 1 - cdf.
// Pomeranz's recursion: 2 n + 1 rows V_i of at most npwrs = 2 (floor(t) + 1) <= 48 entries; row i is the previous one
// convolved with one of three tables (g / n)^j / j!, (2 g / n)^j / j!, ((1 - 2 g) / n)^j / j!, g = min(f, 1 - f), f the
// fractional part of t.  ONE WAVEFRONT per cell: lane = entry of the row (a register), the tables in 1.2 KB of LDS; term a of
// the convolution is lane a's entry broadcast, times the lane's own table entry, a ascending.  Window ends j1, j2, the
// offsets V0s / V1s, the 2^128 scaling when the row's maximum falls below 2^-128 and the final n! loop are scipy's.
//
// A cell's bits depend on (n, x) alone: every sum has a fixed order, a lane's or a tile's share is fixed by (n, x), and the
// work lists only say which wavefront or workgroup evaluates a cell.
//
// Compiled two ways like rel_ks_large.h (hipcc for gfx950; g++ -DTSFA_EMUL with the lanes looped), except ksm_durbin_large,
// which is device code only.
#ifndef TSFA_REL_KS_MATRIX_H
#define TSFA_REL_KS_MATRIX_H

#include "rel_ks_large.h"

#define KSM_SMALL_N 140.0        // _kolmogn: up to here Durbin / Pomeranz / the sum, whatever nxsq is
#define KSM_MAX_N 100000.0       // _kolmogn: Durbin's matrix only up to here
#define KSM_SM 21                // largest m of KSM_DURBIN_SMALL: k = ceil(sqrt(140 * 0.754693)) = 11
#define KSM_SMALL_LDS (2 * KSM_SM * KSM_SM + 4 * KSM_SM)   // doubles a wavefront: H, its square, w, v, r, r'
#define KSM_LG_NT 512            // threads of KSM_DURBIN_LARGE's workgroup
#define KSM_LG_MAX_K 64          // m = 2 k - 1 <= 127 fits 128 rows; _kolmogn's bound is k <= 59
#define KSM_PZ 48                // widest row of KSM_POMERANZ: floor(sqrt(4 * 140)) = 23
#define KSM_EP128 3.4028236692093846e38    // 2^128
#define KSM_EM128 2.9387358770557188e-39   // 2^-128

// what ksm_branch found
enum { KSM_LEAVE = 0,
       KSM_ZERO = 1, KSM_ONE = 2, KSM_PRODUCT = 3, KSM_RUBEN_HIGH = 4,                          // closed: ksm_closed
       KSM_SMIRNOV = 5, KSM_DURBIN_SMALL = 6, KSM_POMERANZ = 7, KSM_DURBIN_LARGE = 8 };         // the four work lists
#define KSM_LISTS 4
#define KSM_LIST_OF(branch) ((branch) - KSM_SMIRNOV)

// the serve rule and the branch of kstwo.sf(d, n) for the samples n1, n2; *n_out = n
RT_HD int ksm_branch(int64_t n1, int64_t n2, double x, double *n_out) {
    if (n1 < 1 || n2 < 1 || x != x) return KSM_LEAVE;
    const double big = (double)((n1 > n2) ? n1 : n2), small = (double)((n1 > n2) ? n2 : n1);
    if (big <= (double)RK_MAX_ROWS) return KSM_LEAVE;
    const double n = rint(big * small / (big + small));
    *n_out = n;
    if (!(n >= 1.0 && n <= KSM_MAX_N)) return KSM_LEAVE;
    const double t = n * x, nxsq = t * x;
    if (n >= KSL_MIN_N) {   // the one cell ksl_branch leaves below KSM_MAX_N, by its expressions
        if (x >= 1.0 || x <= 0.0 || t <= 1.0 || t >= n - 1.0 || x >= 0.5 || nxsq >= 2.2) return KSM_LEAVE;
        if (!(n * pow(x, 1.5) <= 1.4) || ceil(t) > (double)KSM_LG_MAX_K) return KSM_LEAVE;
        return KSM_DURBIN_LARGE;
    }
    if (x >= 1.0) return KSM_ZERO;
    if (x <= 0.0) return KSM_ONE;
    if (t <= 1.0) return (t <= 0.5) ? KSM_ONE : KSM_PRODUCT;
    if (t >= n - 1.0) return KSM_RUBEN_HIGH;
    if (x >= 0.5) return KSM_SMIRNOV;
    if (nxsq <= 0.754693) return KSM_DURBIN_SMALL;
    return (nxsq <= 4.0) ? KSM_POMERANZ : KSM_SMIRNOV;
}

// the value of a closed branch
RT_HD double ksm_closed(int branch, double n, double x) {
    if (branch == KSM_ZERO) return 0.0;
    if (branch == KSM_ONE) return 1.0;
    if (branch == KSM_RUBEN_HIGH) return ksl_clip(2.0 * pow(1.0 - x, n));
    const double rn = 1.0 / n, c = 2.0 * (n * x) - 1.0;   // np.prod(np.arange(1, n + 1) * (1.0 / n) * (2 * t - 1))
    double prob = 1.0;
    for (int i = 1; i <= (int)n; ++i) prob *= ((double)i * rn) * c;
    return ksl_clip(1.0 - prob);
}

// ---- Durbin's matrix ----
// _kolmogn_DMTW's w[j] = 1 / j! and v[j] = (1 - h^(j+1)) / (j + 1)!, v[m-1] = (1 + tt) / m!, by its divisions in its order
RT_HD void ksm_tables(int m, double h, double *w, double *v) {
    double fac = 1.0;
    for (int j = 1; j <= m; ++j) {
        w[j - 1] = fac;
        fac /= (double)j;
        v[j - 1] = (1.0 - pow(h, (double)j)) * fac;
    }
    const double c = 2.0 * h - 1.0, tt = pow((c > 0.0) ? c : 0.0, (double)m) - 2.0 * pow(h, (double)m);
    v[m - 1] = (1.0 + tt) * fac;
}
// H[r][c]: the last row is v reversed, the first column v, column c >= 1 holds w from row c - 1 down, the rest is zero
RT_HD double ksm_h_at(int r, int c, int m, const double *w, const double *v) {
    if (r == m - 1) return v[m - 1 - c];
    if (c == 0) return v[r];
    return (r >= c - 1) ? w[r - c + 1] : 0.0;
}

#if RT_GPU
#define KSM_SYNC() __syncthreads()   // ksm_durbin_small and ksm_pomeranz run in workgroups of ONE wavefront
#else
#define KSM_SYNC() ((void)0)
#endif

// clip(1 - cdf), n <= 140 and m <= KSM_SM; called by the 64 lanes of a one-wavefront workgroup with the same arguments, every
// lane returns the value.  lds: KSM_SMALL_LDS doubles.
RT_DEV double ksm_durbin_small(double n, double x, double *lds) {
    const double nd = n * x;
    const int k = (int)ceil(nd), m = 2 * k - 1, mm = m * m;
    const double h = (double)k - nd;
    double *A = lds, *B = A + KSM_SM * KSM_SM, *w = B + KSM_SM * KSM_SM, *v = w + KSM_SM, *r0 = v + KSM_SM, *r1 = r0 + KSM_SM;
    KSM_SYNC();   // the cell before is done with the slice
    RT_LANES(l) if (l == 0) ksm_tables(m, h, w, v);
    KSM_SYNC();
    RT_LANES(l) {
        for (int e = l; e < mm; e += 64) A[e] = ksm_h_at(e / m, e % m, m, w, v);
        if (l < m) r0[l] = (l == k - 1) ? 1.0 : 0.0;
    }
    KSM_SYNC();
    int expnt = 0, hexpnt = 0;
    for (int nn = (int)n; nn > 0;) {
        if (nn & 1) {
            RT_LANES(l) if (l < m) {
                double s = 0.0;
                for (int i = 0; i < m; ++i) s += r0[i] * A[i * m + l];
                r1[l] = s;
            }
            KSM_SYNC();
            double *t = r0; r0 = r1; r1 = t;
            expnt += hexpnt;
            if (r0[k - 1] > KSM_EP128) {
                KSM_SYNC();
                RT_LANES(l) if (l < m) r0[l] *= KSM_EM128;
                expnt += 128;
                KSM_SYNC();
            }
        }
        nn >>= 1;
        if (!nn) break;
        RT_LANES(l) for (int e = l; e < mm; e += 64) {
            const int i = e / m, j = e - i * m;
            double s = 0.0;
            for (int q = 0; q < m; ++q) s += A[i * m + q] * A[q * m + j];
            B[e] = s;
        }
        KSM_SYNC();
        double *t = A; A = B; B = t;
        hexpnt *= 2;
        if (fabs(A[(k - 1) * m + k - 1]) > KSM_EP128) {
            KSM_SYNC();
            RT_LANES(l) for (int e = l; e < mm; e += 64) A[e] *= KSM_EM128;
            hexpnt += 128;
            KSM_SYNC();
        }
    }
    double p = r0[k - 1];
    for (int i = 1; i <= (int)n; ++i) {   // times n! / n^n
        p = (double)i * p / n;
        if (fabs(p) < KSM_EM128) { p *= KSM_EP128; expnt -= 128; }
    }
    if (expnt != 0) p = ldexp(p, expnt);
    return ksl_clip(1.0 - ksl_clip(p));
}

#if RT_GPU
typedef double ksm_d4 __attribute__((ext_vector_type(4)));

RT_HD int ksm_large_pad(int k) { return ((2 * k - 1 + 15) / 16) * 16; }
// the doubles of LDS a workgroup needs for cells of up to k_max: H [M][M + 2], w, v, r, r'
RT_HD size_t ksm_large_lds(int k_max) { const size_t M = (size_t)ksm_large_pad(k_max); return M * (M + 2) + 4 * M; }

// clip(1 - cdf), 141 <= n <= 100 000 and k <= KSM_LG_MAX_K; called by the KSM_LG_NT threads of a workgroup with the same
// arguments, every thread returns the value.  lds: ksm_large_lds(k) doubles or more.
__device__ __forceinline__ double ksm_durbin_large(double n, double x, double *lds) {
    const double nd = n * x;
    const int k = (int)ceil(nd), m = 2 * k - 1, M = ksm_large_pad(k), T = M / 16, LD = M + 2;
    const double h = (double)k - nd;
    double *H = lds, *w = H + M * LD, *v = w + M, *r0 = v + M, *r1 = r0 + M;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    __syncthreads();   // the cell before is done with the LDS
    if (tid == 0) ksm_tables(m, h, w, v);
    __syncthreads();
    for (int e = tid; e < M * M; e += KSM_LG_NT) {   // the pad rows and columns are zero, and stay so under squaring
        const int i = e / M, j = e - i * M;
        H[i * LD + j] = (i < m && j < m) ? ksm_h_at(i, j, m, w, v) : 0.0;
    }
    if (tid < M) r0[tid] = (tid == k - 1) ? 1.0 : 0.0;
    __syncthreads();
    // tile q = wave + 8 u = (ti, tj): where the lane reads A[ti 16 + r][kq], B[kq][tj 16 + r] and stores D[ti 16 + kq][tj 16 + r]
    int a_at[8], b_at[8], d_at[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int q = wave + 8 * u, ti = q / T, tj = q - ti * T;
        a_at[u] = (ti * 16 + r) * LD + kq;
        b_at[u] = kq * LD + tj * 16 + r;
        d_at[u] = (ti * 16 + kq) * LD + tj * 16 + r;
    }
    int expnt = 0, hexpnt = 0;
    for (int nn = (int)n; nn > 0;) {
        if (nn & 1) {
            if (tid < M) {
                double s = 0.0;
                for (int i = 0; i < m; ++i) s += r0[i] * H[i * LD + tid];
                r1[tid] = s;
            }
            __syncthreads();
            double *t = r0; r0 = r1; r1 = t;
            expnt += hexpnt;
            if (r0[k - 1] > KSM_EP128) {
                __syncthreads();
                if (tid < M) r0[tid] *= KSM_EM128;
                expnt += 128;
                __syncthreads();
            }
        }
        nn >>= 1;
        if (!nn) break;
        ksm_d4 acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = (ksm_d4){0.0, 0.0, 0.0, 0.0};
        for (int ks = 0; ks < M; ks += 4) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (wave + 8 * u < T * T) {   // wave-uniform
                    const double a = H[a_at[u] + ks], b = H[b_at[u] + ks * LD];
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
                }
            }
        }
        __syncthreads();   // every tile has read all it needs of H
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (wave + 8 * u < T * T) {
#pragma unroll
                for (int e = 0; e < 4; ++e) H[d_at[u] + 4 * e * LD] = acc[u][e];
            }
        }
        __syncthreads();
        hexpnt *= 2;
        if (fabs(H[(k - 1) * LD + k - 1]) > KSM_EP128) {
            __syncthreads();
            for (int e = tid; e < M * M; e += KSM_LG_NT) {
                const int i = e / M, j = e - i * M;
                H[i * LD + j] *= KSM_EM128;
            }
            hexpnt += 128;
            __syncthreads();
        }
    }
    const double cdf = exp((log(r0[k - 1]) + (double)expnt * M_LN2) + ksl_log_nfact_div_n_pow_n(n));
    return ksl_clip(1.0 - ksl_clip(cdf));
}
#endif

// ---- Pomeranz's recursion ----
// _pomeranz_compute_j1j2: the window of row i
RT_HD void ksm_pomeranz_j1j2(int i, int n, int ll, int ceilf, int roundf, int *j1_out, int *j2_out) {
    int j1, j2;
    if (i == 0) {
        j1 = -ll - ceilf - 1; j2 = ll + ceilf - 1;
    } else {
        const int ip1div2 = (i + 1) / 2, ip1mod2 = (i + 1) % 2;
        if (ip1mod2 == 0) {
            if (ip1div2 == n + 1) { j1 = n - ll - ceilf - 1; j2 = n + ll + ceilf - 1; }
            else { j1 = ip1div2 - 1 - ll - roundf - 1; j2 = ip1div2 + ll - 1 + ceilf - 1; }
        } else {
            j1 = ip1div2 - 1 - ll - 1; j2 = ip1div2 + ll + roundf - 1;
        }
    }
    *j1_out = (j1 + 2 > 0) ? j1 + 2 : 0;
    *j2_out = (j2 < n) ? j2 : n;
}

RT_DEV double ksm_wave_max(const double *v) {
#if RT_GPU
    double x = v[0];
    for (int s = 32; s > 0; s >>= 1) x = fmax(x, __shfl_xor(x, s, 64));
    return x;
#else
    double x = v[0];
    for (int l = 1; l < 64; ++l) x = fmax(x, v[l]);
    return x;
#endif
}

// clip(1 - cdf), n <= 140 and 0.754693 < nxsq <= 4; called by the 64 lanes of a one-wavefront workgroup with the same
// arguments, every lane returns the value.  lds: 3 * KSM_PZ doubles.
RT_DEV double ksm_pomeranz(double nf, double x, double *lds) {
    const int n = (int)nf;
    const double t = nf * x;
    const int ll = (int)floor(t);
    const double f = t - (double)ll, g = (f < 1.0 - f) ? f : 1.0 - f;
    const int ceilf = (f > 0.0) ? 1 : 0, roundf = (f > 0.5) ? 1 : 0, npwrs = 2 * (ll + 1);
    double *gpower = lds, *twogpower = lds + KSM_PZ, *onem2gpower = lds + 2 * KSM_PZ;
    KSM_SYNC();   // the cell before is done with the slice
    RT_LANES(l) if (l == 0) {
        const double g_over_n = g / nf, two_g_over_n = 2.0 * g / nf, one_minus_two_g_over_n = (1.0 - 2.0 * g) / nf;
        gpower[0] = twogpower[0] = onem2gpower[0] = 1.0;
        for (int j = 1; j < npwrs; ++j) {
            gpower[j] = gpower[j - 1] * g_over_n / (double)j;
            twogpower[j] = twogpower[j - 1] * two_g_over_n / (double)j;
            onem2gpower[j] = onem2gpower[j - 1] * one_minus_two_g_over_n / (double)j;
        }
    }
    KSM_SYNC();
    double V0[RT_NL], V1[RT_NL];   // V1: the row just made, lane = entry
    RT_LANES(l) { V0[RT_AT(l)] = 0.0; V1[RT_AT(l)] = (l == 0) ? 1.0 : 0.0; }
    int V0s = 0, V1s = 0, expnt = 0, j1, j2;
    ksm_pomeranz_j1j2(0, n, ll, ceilf, roundf, &j1, &j2);
    for (int i = 1; i < 2 * n + 2; ++i) {
        const int k1 = j1;
        RT_LANES(l) { V0[RT_AT(l)] = V1[RT_AT(l)]; V1[RT_AT(l)] = 0.0; }
        { const int s = V0s; V0s = V1s; V1s = s; }
        ksm_pomeranz_j1j2(i, n, ll, ceilf, roundf, &j1, &j2);
        const double *pwrs = (i == 1 || i == 2 * n + 1) ? gpower : ((i % 2) ? twogpower : onem2gpower);
        const int ln2 = j2 - k1 + 1;
        if (ln2 <= 0) continue;
        // np.convolve(V0[k1 - V0s : k1 - V0s + ln2], pwrs[:ln2])[j1 - k1 : j2 + 1 - k1]: both slices end with the arrays
        const int off = k1 - V0s, conv_start = j1 - k1, conv_len = j2 - j1 + 1, nb = (ln2 < npwrs) ? ln2 : npwrs;
        const int na = (ln2 < npwrs - off) ? ln2 : npwrs - off;
        for (int a = 0; a < na; ++a) {
            const double va = rt_wave_get(V0, off + a);
            RT_LANES(l) {
                const int b = conv_start + l - a;
                if (l < conv_len && b >= 0 && b < nb) V1[RT_AT(l)] += va * pwrs[b];
            }
        }
        const double top = ksm_wave_max(V1);
        if (top > 0.0 && top < KSM_EM128) {
            RT_LANES(l) V1[RT_AT(l)] *= KSM_EP128;
            expnt -= 128;
        }
        V1s = V0s + j1 - k1;
    }
    double ans = rt_wave_get(V1, n - V1s);
    for (int j = 1; j <= n; ++j) {   // times n!
        if (fabs(ans) > KSM_EP128) { ans *= KSM_EM128; expnt += 128; }
        ans *= (double)j;
    }
    if (expnt != 0) ans = ldexp(ans, expnt);
    return ksl_clip(1.0 - ksl_clip(ans));
}

// ---- the cells ----
// one lane per cell: a TSFA_ROUTE_HOST_KS cell of a closed branch gets its p and TSFA_ROUTE_KS_MATRIX -> KSM_LEAVE (also for a
// cell of another route), the closed branch served, or the work list the cell belongs to; *k_out: k of a KSM_DURBIN_LARGE cell
RT_HD int ksm_route_cell(const RkCells &s, int64_t cell, double *p, unsigned char *route, int *k_out) {
    if (route[cell] != TSFA_ROUTE_HOST_KS) return KSM_LEAVE;
    int64_t n1, n2;
    double d, n = 0.0;
    rk_cell_args(s, cell, &n1, &n2, &d);
    const int branch = ksm_branch(n1, n2, d, &n);
    if (branch == KSM_DURBIN_LARGE) *k_out = (int)ceil(n * d);
    if (branch == KSM_LEAVE || branch >= KSM_SMIRNOV) return branch;
    p[cell] = ksm_closed(branch, n, d);
    route[cell] = TSFA_ROUTE_KS_MATRIX;
    return branch;
}

// one wavefront (KSM_DURBIN_LARGE: one workgroup) per cell of the work list `branch`; lds: what the branch's function asks for
RT_DEV void ksm_list_cell(const RkCells &s, int64_t cell, int branch, double *lds, double *p, unsigned char *route) {
    int64_t n1, n2;
    double d, n = 0.0, v;
    rk_cell_args(s, cell, &n1, &n2, &d);
    if (ksm_branch(n1, n2, d, &n) != branch) return;   // (the list holds no such cell)
    if (branch == KSM_SMIRNOV) v = ksl_smirnov(n, d);
    else if (branch == KSM_DURBIN_SMALL) v = ksm_durbin_small(n, d, lds);
    else if (branch == KSM_POMERANZ) v = ksm_pomeranz(n, d, lds);
#if RT_GPU
    else v = ksm_durbin_large(n, d, lds);
    if (threadIdx.x != 0 && (branch == KSM_DURBIN_LARGE || (threadIdx.x & 63) != 0)) return;
#else
    else return;
#endif
    p[cell] = v;
    route[cell] = TSFA_ROUTE_KS_MATRIX;
}

#endif
