// The Kolmogorov-Smirnov tail beyond 10 000 rows as device code (tsfa_ks_large_tails and ks_tail = TSFA_KS_TAIL_DEVICE_LARGE
// of tsfa_relevance_tails_*, include/tsfresh_amd.h): the cells rel_ks.h leaves as TSFA_ROUTE_HOST_KS because a sample is
// longer than RK_MAX_ROWS, where significance_tests.py ks_2samp_pvalue calls scipy.stats.kstwo.sf(d, n) with
// n = round(n1 n2 / (n1 + n2)).
//
// kstwo.sf is the survival function of the two-sided one-sample statistic as R. Simard and P. L'Ecuyer, "Computing the
// Two-Sided Kolmogorov-Smirnov Distribution", J. Stat. Softw. 39(11), 2011, lay it out.  With x = d, t = n x and
// nxsq = t x, formed in float64 exactly so (-ffp-contract=off), the branches are taken in this order:
//   x >= 1 -> 0,  x <= 0 -> 1,  t <= 0.5 -> 1
//   t <= 1          1 - n! (2 t - 1)^n / n^n                     (Ruben and Gambino 1982; n!/n^n by the Stirling series)
//   t >= n - 1      2 (1 - x)^n                                  (Ruben and Gambino 1982)
//   x >= 0.5        2 P(D+ >= x)                                 (the one-sided sum below; exact there)
//   n <= 140        Durbin's matrix / Pomeranz: NOT SERVED
//   nxsq >= 370     0
//   nxsq >= 2.2     clip(2 P(D+ >= x))
//   n <= 100 000 and n x^1.5 <= 1.4   Durbin's matrix: NOT SERVED
//   otherwise       clip(1 - cdf), cdf by Pelz and Good (1976): K0(z) + K1(z) / sqrt(n) + K2(z) / n + K3(z) / n^1.5, z = sqrt(n) x
// The one-sided tail is the sum of Birnbaum and Tingey (1951), all of whose terms are positive:
//   P(D+ >= x) = sum_{j = 0 .. floor(n (1 - x))}  C(n, j) x (x + j/n)^(j-1) (1 - x - j/n)^(n-j).
//
//   ksl_branch / ksl_closed   the serve rule, the branch and every closed branch: ONE LANE per cell
//   ksl_smirnov               the sum: ONE WAVEFRONT per cell.  Wavefronts never meet: no barrier, no LDS.
//
// The sum.  Term j is exp(l_j), l_j = log C(n, j) + log x + (j - 1) log(x + j/n) + (n - j) log1p(-(x + j/n)).  The terms are
// cut into runs of KSL_RUN consecutive j; run r belongs to lane r mod 64.  At the head of a run log C(n, j) comes from the
// Lanczos log-gamma of tsfa_common.h (tsfa_lgamma_pos: three values, one of them per cell), inside the run it advances by
// log((n - j) / (j + 1)), kept as a separate small sum so that what a run carries is at most KSL_RUN roundings of a number
// below KSL_RUN log n, whatever n is.  Every term is evaluated; none is skipped.
// Terms are accumulated as exp(l_j - L) against the cell's reference exponent L = -2 nxsq.  By Massart's form of the
// Dvoretzky-Kiefer-Wolfowitz inequality (Ann. Probab. 18, 1990) P(D+ >= x) <= exp(-2 n x^2) whenever that bound is at most
// 1/2, i.e. nxsq >= 0.35, which every cell of this branch satisfies (nxsq >= 2.2, or x >= 0.5 with n >= 141).  Every term is
// at most the sum, so l_j - L <= 0: no overflow; and a cell whose value is a normal double has l_j - L >= -708 + 2 nxsq - log 2
// for the terms that matter, so they are normal doubles too and a p near 1e-300 keeps its relative accuracy.
// p = clip(2 exp(L) S).  L needs no pass over the terms and depends on (n, x) alone.
// The lanes' sums are added by the four DPP steps inside a row and the fixed tree of the four row totals (wave_sum of
// tsfa_common.h); a lane adds its runs in ascending order.  So a cell's bits depend on (n, x) only: not on the grid, the other
// cells of the call or the cell's place in the work list.
//
// Compiled two ways like rel_ks.h (hipcc for gfx950; g++ -DTSFA_EMUL, tests/emul/emul_rel_ks_large.cpp, lanes looped, the
// additions of the reduction in the order of the DPP steps; log / log1p / exp / pow are glibc's there and ocml's here).
#ifndef TSFA_REL_KS_LARGE_H
#define TSFA_REL_KS_LARGE_H

#include "rel_ks.h"
#include "tsfa_common.h"   // tsfa_lgamma_pos, wave_sum

#define KSL_MIN_N 141.0       // below, kstwo.sf takes Durbin's matrix or Pomeranz's recursion
#define KSL_MAX_N 1000000.0   // above, scipy's smirnov leaves the sum for an approximation of its own
#define KSL_RUN 16            // consecutive terms a lane evaluates from one log-gamma head

// what ksl_branch found
enum { KSL_LEAVE = 0,      // not served: the cell stays with the caller
       KSL_ZERO = 1, KSL_ONE = 2, KSL_RUBEN_LOW = 3, KSL_RUBEN_HIGH = 4, KSL_PELZ_GOOD = 5,   // closed: ksl_closed
       KSL_SMIRNOV = 6 };  // ksl_smirnov

// the serve rule and the branch of kstwo.sf(d, n) for the samples n1, n2; *n_out = n
RT_HD int ksl_branch(int64_t n1, int64_t n2, double x, double *n_out) {
    if (n1 < 1 || n2 < 1 || x != x) return KSL_LEAVE;
    const double big = (double)((n1 > n2) ? n1 : n2), small = (double)((n1 > n2) ? n2 : n1);
    if (big <= (double)RK_MAX_ROWS) return KSL_LEAVE;
    const double n = rint(big * small / (big + small));   // np.round(en): both round half to even
    *n_out = n;
    if (!(n >= KSL_MIN_N && n <= KSL_MAX_N)) return KSL_LEAVE;
    if (x >= 1.0) return KSL_ZERO;
    if (x <= 0.0) return KSL_ONE;
    const double t = n * x;
    if (t <= 1.0) return (t <= 0.5) ? KSL_ONE : KSL_RUBEN_LOW;
    if (t >= n - 1.0) return KSL_RUBEN_HIGH;
    if (x >= 0.5) return KSL_SMIRNOV;
    const double nxsq = t * x;
    if (nxsq >= 370.0) return KSL_ZERO;
    if (nxsq >= 2.2) return KSL_SMIRNOV;
    if (n <= 100000.0 && n * pow(x, 1.5) <= 1.4) return KSL_LEAVE;
    return KSL_PELZ_GOOD;
}

RT_HD double ksl_clip(double p) { return (p < 0.0) ? 0.0 : ((p > 1.0) ? 1.0 : p); }

// log(n! / n^n): Stirling's series with n log n taken out, log(n) / 2 - n + log(2 pi) / 2 + sum B_2j / (2j (2j - 1) n^(2j-1))
RT_HD double ksl_log_nfact_div_n_pow_n(double n) {
    const double c[8] = {-2.955065359477124183e-2, 6.4102564102564102564e-3, -1.9175269175269175269e-3, 8.4175084175084175084e-4,
                         -5.952380952380952381e-4, 7.9365079365079365079e-4, -2.7777777777777777778e-3, 8.3333333333333333333e-2};
    const double rn = 1.0 / n, y = rn / n;
    double s = c[0];
    for (int i = 1; i < 8; ++i) s = s * y + c[i];
    return log(n) / 2.0 - n + log(2.0 * M_PI) / 2.0 + rn * s;
}

// Pelz and Good's cdf at z = sqrt(n) x: the four K_i as theta-function sums suited to small z, each a Horner sum in
// q^(8k) over the odd integers 2k - 1, k = ceil(16 z / pi) .. 1, and the two sums over all integers that K2 and K3 add
RT_HD double ksl_pelz_good_cdf(double n, double x) {
    const double pi2 = M_PI * M_PI, pi4 = pi2 * pi2, pi6 = pi4 * pi2, sqrt2pi = sqrt(2.0 * M_PI);
    const double z = sqrt(n) * x;
    const double z2 = z * z, z3 = z2 * z, z4 = z2 * z2, z6 = z4 * z2, z7 = z6 * z, z8 = z4 * z4, z10 = z8 * z2;
    const double qlog = -pi2 / 8.0 / z2;
    if (qlog < -708.0) return 0.0;
    double q = exp(qlog);
    const double k1a = -z2, k1b = pi2 / 4.0;
    const double k2a = 6.0 * z6 + 2.0 * z4, k2b = (2.0 * z4 - 5.0 * z2) * pi2 / 4.0, k2c = pi4 * (1.0 - 2.0 * z2) / 16.0;
    const double k3d = pi6 * (5.0 - 30.0 * z2) / 64.0, k3c = pi4 * (-60.0 * z2 + 212.0 * z4) / 16.0;
    const double k3b = pi2 * (135.0 * z4 - 96.0 * z6) / 4.0, k3a = -30.0 * z6 - 90.0 * z8;
    const int maxk = (int)ceil(16.0 * z / M_PI);
    double K0 = 0.0, K1 = 0.0, K2 = 0.0, K3 = 0.0;
    for (int k = maxk; k > 0; --k) {
        const double m = (double)(2 * k - 1), m2 = m * m, m4 = m2 * m2, m6 = m4 * m2;
        const double qp = pow(q, 8.0 * (double)k);
        K0 = K0 * qp + 1.0;
        K1 = K1 * qp + (k1a + k1b * m2);
        K2 = K2 * qp + (k2a + k2b * m2 + k2c * m4);
        K3 = K3 * qp + (k3a + k3b * m2 + k3c * m4 + k3d * m6);
    }
    K0 = K0 * q * sqrt2pi / z;
    K1 = K1 * q * sqrt2pi / (6.0 * z4);
    K2 = K2 * q * sqrt2pi / (72.0 * z7);
    K3 = K3 * q * sqrt2pi / (6480.0 * z10);
    q = exp(-pi2 / 2.0 / z2);
    const double sqrt3z = sqrt(3.0) * z;
    double e2 = 0.0, e3 = 0.0;
    for (int k = maxk; k > 0; --k) {
        const double kk = (double)k, k2 = kk * kk, kpi = M_PI * kk, qp = pow(q, k2);
        e2 += k2 * qp;
        e3 += (sqrt3z + kpi) * (sqrt3z - kpi) * k2 * qp;
    }
    K2 += e2 * (pi2 * sqrt2pi / (-36.0 * z3));
    K3 += e3 * (pi2 * sqrt2pi / (216.0 * z6));
    return K0 + K1 / sqrt(n) + K2 / n + K3 / (n * sqrt(n));
}

// the value of a closed branch
RT_HD double ksl_closed(int branch, double n, double x) {
    if (branch == KSL_ZERO) return 0.0;
    if (branch == KSL_ONE) return 1.0;
    if (branch == KSL_RUBEN_LOW) return ksl_clip(1.0 - exp(ksl_log_nfact_div_n_pow_n(n) + n * log(2.0 * (n * x) - 1.0)));
    if (branch == KSL_RUBEN_HIGH) return ksl_clip(2.0 * pow(1.0 - x, n));
    return ksl_clip(1.0 - ksl_pelz_good_cdf(n, x));
}

// the lanes' partial sums -> the total, in every lane: wave_sum's order (four butterfly steps inside each row of 16 lanes,
// then (row 0 + row 1) + (row 2 + row 3))
RT_DEV double ksl_wave_sum(const double *v) {
#if RT_GPU
    return wave_sum(v[0]);
#else
    double t[64], u[64];
    for (int l = 0; l < 64; ++l) t[l] = v[l];
    for (int step = 0; step < 4; ++step) {
        for (int l = 0; l < 64; ++l) {
            // quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
            const int src = (step == 0) ? (l ^ 1) : ((step == 1) ? (l ^ 2) : ((step == 2) ? (l ^ 7) : (l ^ 15)));
            u[l] = t[l] + t[src];
        }
        for (int l = 0; l < 64; ++l) t[l] = u[l];
    }
    return (t[0] + t[16]) + (t[32] + t[48]);
#endif
}

// clip(2 P(D+ >= x)) for n samples; called by all 64 lanes of a wavefront with the same arguments, every lane returns the
// value.  141 <= n <= KSL_MAX_N, 0 < x < 1 and nxsq >= 0.35 (see the head of the file).
RT_DEV double ksl_smirnov(double n, double x) {
    const int64_t n_terms = (int64_t)floor(n * (1.0 - x)) + 1;
    const int64_t n_runs = (n_terms + KSL_RUN - 1) / KSL_RUN;
    const double lgn1 = tsfa_lgamma_pos(n + 1.0), logx = log(x), L = -2.0 * ((n * x) * x);
    double acc[RT_NL];
    RT_LANES(l) {
        double s = 0.0;
        for (int64_t run = l; run < n_runs; run += 64) {
            const int64_t j0 = run * KSL_RUN, j1 = (j0 + KSL_RUN < n_terms) ? j0 + KSL_RUN : n_terms;
            const double head = lgn1 - tsfa_lgamma_pos((double)j0 + 1.0) - tsfa_lgamma_pos(n - (double)j0 + 1.0);   // log C(n, j0)
            double step = 0.0;   // log C(n, j) - log C(n, j0)
            for (int64_t j = j0; j < j1; ++j) {
                const double fj = (double)j, a = x + fj / n;
                if (a < 1.0) s += exp((((head + step) + logx) + ((fj - 1.0) * log(a) + (n - fj) * log1p(-a))) - L);
                step += log((n - fj) / (fj + 1.0));
            }
        }
        acc[RT_AT(l)] = s;
    }
    return ksl_clip(2.0 * exp(L) * ksl_wave_sum(acc));
}

// ---- the cells ----
// one lane per cell: a TSFA_ROUTE_HOST_KS cell of a closed branch gets its p and TSFA_ROUTE_KS_KOLMOGN -> KSL_LEAVE (also for
// a cell of another route), KSL_SMIRNOV (the cell is the sum's), or the closed branch served
RT_HD int ksl_route_cell(const RkCells &s, int64_t cell, double *p, unsigned char *route) {
    if (route[cell] != TSFA_ROUTE_HOST_KS) return KSL_LEAVE;
    int64_t n1, n2;
    double d, n = 0.0;
    rk_cell_args(s, cell, &n1, &n2, &d);
    const int branch = ksl_branch(n1, n2, d, &n);
    if (branch == KSL_LEAVE || branch == KSL_SMIRNOV) return branch;
    p[cell] = ksl_closed(branch, n, d);
    route[cell] = TSFA_ROUTE_KS_KOLMOGN;
    return branch;
}

// one wavefront per cell of the work list ksl_route_cell's callers filled
RT_DEV void ksl_smirnov_cell(const RkCells &s, int64_t cell, double *p, unsigned char *route) {
    int64_t n1, n2;
    double d, n = 0.0;
    rk_cell_args(s, cell, &n1, &n2, &d);
    if (ksl_branch(n1, n2, d, &n) != KSL_SMIRNOV) return;   // (the list holds no such cell)
    const double v = ksl_smirnov(n, d);
#if RT_GPU
    if ((threadIdx.x & 63) != 0) return;
#endif
    p[cell] = v;
    route[cell] = TSFA_ROUTE_KS_KOLMOGN;
}

#endif
