// p-value tails and the FDR step-up of the feature selection, as device code (tsfa_relevance_tails_* / tsfa_relevance_fdr /
// tsfa_compact_mask, include/tsfresh_amd.h).
//
// The statistics sweep of tsfa_relevance.hip leaves, per column (and class), the sufficient statistics of the reference's
// univariate tests in HBM.  The functions here restate tsfresh_amd/feature_selection/significance_tests.py on them in
// float64, in the operation order of the Python text (-ffp-contract=off), so that the device-resident chain never copies
// the statistics to the host:
//   rt_mwu_normal   mannwhitney_pvalue, the branch of the normal approximation (tie and continuity correction)
//   rt_kendall      kendall_pvalue (tau-b, asymptotic)
//   rt_fisher       fisher_exact_pvalue, two-sided: ONE WAVEFRONT per cell, lanes stride the support
//   rt_fdr_*        fdr_reject: the step-up rule on sorted p-values, and _relevance_table's combination of the tables
//   rt_compact_*    mask -> ascending indices
// Every cell carries a route byte (enum below).  The two HOST routes are not served here: the exact Mann-Whitney
// distribution is a big-integer recurrence and the Kolmogorov-Smirnov tail a lattice walk (tsfa_ks_outer_prob) or
// scipy's kstwo; the kernel writes NaN there and the caller fills those cells in before the FDR step.  (rel_ks.h serves the
// lattice walk on the device where the caller asks for it: TSFA_ROUTE_KS_EXACT.)
//
// Compiled two ways like roll_device.h / pack_dense.h: by hipcc for gfx950 and by g++ -DTSFA_EMUL
// (tests/emul/emul_rel_tails.cpp).  In the emulation one host thread is a workgroup and the lanes are looped: a per-lane
// value is an array of RT_NL = 64 cells (one cell on the GPU), a wavefront operation (scan, sum, broadcast) takes the
// array, and does the additions in the order of the GPU's shuffle steps, so the emulated Fisher tail is the GPU's bit for
// bit up to the math library (lgamma / log / exp: glibc there, ocml here).
#ifndef TSFA_REL_TAILS_H
#define TSFA_REL_TAILS_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_GPU 1
#define RT_HD __host__ __device__ __forceinline__
#define RT_DEV __device__ __forceinline__
#define RT_NL 1
#else
#define RT_GPU 0
#define RT_HD static inline
#define RT_DEV static inline
#define RT_NL 64
#endif

#include "../../include/tsfresh_amd.h"  // enum tsfa_route

#define RT_ROUTE_IS_HOST(r) ((r) == TSFA_ROUTE_HOST_MWU_EXACT || (r) == TSFA_ROUTE_HOST_KS)

#define RT_NAN (__builtin_nan(""))
#define RT_INF (__builtin_inf())

RT_HD unsigned char rt_type_of(int64_t n_unique) { return (unsigned char)(n_unique == 1 ? 0 : (n_unique == 2 ? 1 : 2)); }

// ---- routes ----
RT_HD unsigned char rt_route_class_cell(unsigned char type, int with_ks, int64_t n1, int64_t n0, double tie_term) {
    if (type == 0) return TSFA_ROUTE_NONE;
    if (type == 1) return TSFA_ROUTE_FISHER;
    if (with_ks) return TSFA_ROUTE_HOST_KS;
    return ((n1 > 8 && n0 > 8) || tie_term > 0.0) ? TSFA_ROUTE_MWU_NORMAL : TSFA_ROUTE_HOST_MWU_EXACT;
}
RT_HD unsigned char rt_route_real_cell(unsigned char type) {
    return (unsigned char)(type == 0 ? TSFA_ROUTE_NONE : (type == 1 ? TSFA_ROUTE_HOST_KS : TSFA_ROUTE_KENDALL));
}

// ---- closed forms: one lane per cell ----
// significance_tests.py mannwhitney_pvalue, branch (n1 > 8 and n2 > 8) or tie_term > 0
RT_HD double rt_mwu_normal(double rank_sum_1, int64_t n1, int64_t n2, double tie_term) {
    const double u1 = rank_sum_1 - (double)(n1 * (n1 + 1)) / 2.0;
    const double u2 = (double)(n1 * n2) - u1;
    const double u = (u1 > u2) ? u1 : u2;  // max(u1, u2)
    const int64_t n = n1 + n2;
    const double mu = (double)(n1 * n2) / 2.0;
    const double var = (double)(n1 * n2) / 12.0 * ((double)(n + 1) - tie_term / ((double)n * ((double)n - 1.0)));
    const double s = (var > 0.0) ? sqrt(var) : 0.0;
    const double num = u - mu - 0.5;
    double z;
    if (s == 0.0) z = (num != 0.0) ? copysign(RT_INF, num) : RT_NAN;
    else z = num / s;
    if (z != z) return RT_NAN;
    const double p = erfc(z / sqrt(2.0));  // 2 * norm.sf(z)
    return (p < 0.0) ? 0.0 : ((p > 1.0) ? 1.0 : p);
}

// significance_tests.py kendall_pvalue
RT_HD double rt_kendall(int64_t n, int64_t dis, int64_t xtie, int64_t ntie, double x0, double x1, int64_t ytie, double y0,
                        double y1) {
    const int64_t tot = n * (n - 1) / 2;
    if (xtie == tot || ytie == tot) return RT_NAN;
    const int64_t con_minus_dis = tot - xtie - ytie + ntie - 2 * dis;
    const double m = (double)n * ((double)n - 1.0);
    const double var = ((m * (double)(2 * n + 5) - x1 - y1) / 18.0 + (2.0 * (double)xtie * (double)ytie) / m +
                        x0 * y0 / (9.0 * m * (double)(n - 2)));
    const double z = (double)con_minus_dis / sqrt(var);
    return erfc(fabs(z) / sqrt(2.0));
}

// ---- wavefront operations on a per-lane value (GPU: v[0] of every lane; emulation: the 64 cells of one array) ----
// inclusive scan, Hillis-Steele: at step s lane l adds the value lane l - s held before the step
RT_DEV void rt_wave_scan(double *v) {
#if RT_GPU
    const int lane = (int)(threadIdx.x & 63);
    double x = v[0];
    for (int s = 1; s < 64; s <<= 1) {
        const double t = __shfl_up(x, s, 64);
        if (lane >= s) x += t;
    }
    v[0] = x;
#else
    for (int s = 1; s < 64; s <<= 1)
        for (int l = 63; l >= s; --l) v[l] += v[l - s];
#endif
}
// butterfly sum: every lane receives the total (lane l adds lane l ^ s at every step)
RT_DEV double rt_wave_sum(const double *v) {
#if RT_GPU
    double x = v[0];
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
#else
    double t[64];
    for (int l = 0; l < 64; ++l) t[l] = v[l];
    for (int s = 32; s > 0; s >>= 1) {
        double u[64];
        for (int l = 0; l < 64; ++l) u[l] = t[l] + t[l ^ s];
        for (int l = 0; l < 64; ++l) t[l] = u[l];
    }
    return t[0];
#endif
}
RT_DEV double rt_wave_get(const double *v, int src) {
#if RT_GPU
    return __shfl(v[0], src, 64);
#else
    return v[src];
#endif
}
#if RT_GPU
#define RT_LANES(l) for (int l = (int)(threadIdx.x & 63), rt_once_ = 1; rt_once_; rt_once_ = 0)
#define RT_AT(l) ((void)(l), 0)
#else
#define RT_LANES(l) for (int l = 0; l < 64; ++l)
#define RT_AT(l) (l)
#endif

// log pmf(k + 1) - log pmf(k) of the hypergeometric distribution, as fisher_exact_pvalue writes it
RT_HD double rt_fisher_log_ratio(double k, double n1, double n2, double n) {
    return log((n1 - k) * (n - k)) - log((k + 1.0) * (n2 - n + k + 1.0));
}

// One pass over the support lo .. hi in chunks of 64: element j (value k = lo + j) gets pm_j = exp(log0 + the cumulative
// sum of the log ratios below it), the scan carried from chunk to chunk.  pass 1 (S = 0): returns sum pm_j and leaves
// pm_{obs} in *pobs.  pass 2 (S > 0): returns sum of pm_j / S over the j with pm_j / S <= limit.
RT_DEV double rt_fisher_pass(double log0, int64_t lo, int64_t len, int64_t obs, double n1, double n2, double n, double S,
                             double limit, double *pobs) {
    double acc[RT_NL], cum[RT_NL], held[RT_NL];
    RT_LANES(l) { acc[RT_AT(l)] = 0.0; held[RT_AT(l)] = 0.0; }
    double carry = 0.0;
    for (int64_t j0 = 0; j0 < len; j0 += 64) {
        RT_LANES(l) {
            const int64_t j = j0 + l;
            cum[RT_AT(l)] = (j > 0 && j < len) ? rt_fisher_log_ratio((double)(lo + j - 1), n1, n2, n) : 0.0;
        }
        rt_wave_scan(cum);
        RT_LANES(l) {
            const int64_t j = j0 + l;
            cum[RT_AT(l)] = carry + cum[RT_AT(l)];
            if (j < len) {
                const double pm = exp(log0 + cum[RT_AT(l)]);
                if (S > 0.0) {
                    const double q = pm / S;
                    if (q <= limit) acc[RT_AT(l)] += q;
                } else {
                    acc[RT_AT(l)] += pm;
                    if (j == obs) held[RT_AT(l)] = pm;
                }
            }
        }
        carry = rt_wave_get(cum, 63);
    }
    if (pobs) *pobs = rt_wave_sum(held);  // one lane holds it, the others 0.0
    return rt_wave_sum(acc);
}

// significance_tests.py fisher_exact_pvalue([[a, b], [c, d]]); called by all 64 lanes of a wavefront with the same
// arguments (wave-uniform control flow), every lane returns the value
RT_DEV double rt_fisher(int64_t a, int64_t b, int64_t c, int64_t d) {
    const int64_t n1 = a + b, n2 = c + d, n = a + c;
    if (n1 == 0 || n2 == 0 || n == 0 || (b + d) == 0) return 1.0;
    const int64_t lo = (n - n2 > 0) ? n - n2 : 0, hi = (n1 < n) ? n1 : n;
    const double f1 = (double)n1, f2 = (double)n2, fn = (double)n, fl = (double)lo;
    const double log0 = (lgamma(f1 + 1.0) - lgamma(fl + 1.0) - lgamma(f1 - fl + 1.0) + lgamma(f2 + 1.0) - lgamma(fn - fl + 1.0) -
                         lgamma(f2 - fn + fl + 1.0) - (lgamma(f1 + f2 + 1.0) - lgamma(fn + 1.0) - lgamma(f1 + f2 - fn + 1.0)));
    double pobs = 0.0;
    const double S = rt_fisher_pass(log0, lo, hi - lo + 1, a - lo, f1, f2, fn, 0.0, 0.0, &pobs);
    const double limit = (pobs / S) * (1.0 + 1e-7);
    const double p = rt_fisher_pass(log0, lo, hi - lo + 1, a - lo, f1, f2, fn, S, limit, nullptr);
    return (p < 1.0) ? p : 1.0;  // min(., 1)
}

// ---- the cells of the tables ----
// class tables, one lane per cell (column c, class k) = c * n_classes + k: type and route, the closed form or NaN; the
// Fisher cells' p is rt_tails_fisher_cell's.  Returns 1 for a HOST-route cell.
RT_HD int rt_tails_classes_cell(const tsfa_relevance_col *cols, const double *rank_sums, const int64_t *class_n, int64_t n_rows,
                                int n_classes, int with_ks, int64_t cell, double *p, unsigned char *route, unsigned char *type) {
    const int64_t c = cell / n_classes;
    const int k = (int)(cell - c * n_classes);
    const unsigned char ty = rt_type_of(cols[c].n_unique);
    if (k == 0) type[c] = ty;
    const int64_t n1 = class_n[k], n0 = n_rows - n1;
    const unsigned char r = rt_route_class_cell(ty, with_ks, n1, n0, cols[c].tie_term);
    route[cell] = r;
    if (r == TSFA_ROUTE_FISHER) return 0;
    p[cell] = (r == TSFA_ROUTE_MWU_NORMAL) ? rt_mwu_normal(rank_sums[cell], n1, n0, cols[c].tie_term) : RT_NAN;
    return RT_ROUTE_IS_HOST(r) ? 1 : 0;
}
// class tables, one wavefront per cell: the Fisher cells (two-valued columns); the others leave at once
RT_DEV void rt_tails_fisher_cell(const tsfa_relevance_col *cols, const int64_t *hi_counts, const int64_t *class_n, int64_t n_rows,
                                 int n_classes, int64_t cell, double *p) {
    const int64_t c = cell / n_classes;
    const int k = (int)(cell - c * n_classes);
    if (cols[c].n_unique != 2) return;
    long long hi_total = 0;  // rows of the column that hold its larger value (an integer sum: any order)
#if RT_GPU
    const int lane = (int)(threadIdx.x & 63);
    for (int q = lane; q < n_classes; q += 64) hi_total += hi_counts[c * n_classes + q];
    for (int s = 32; s > 0; s >>= 1) hi_total += __shfl_xor(hi_total, s, 64);
#else
    const int lane = 0;
    for (int q = 0; q < n_classes; ++q) hi_total += hi_counts[c * n_classes + q];
#endif
    // [[y1 & x1, y1 & x0], [y0 & x1, y0 & x0]], x1 = the larger of the column's two values
    const int64_t n1 = class_n[k], n0 = n_rows - n1, a = hi_counts[cell], cc = hi_total - a;
    const double v = rt_fisher(a, n1 - a, cc, n0 - cc);
    if (lane == 0) p[cell] = v;
}
// the table of a real target, one lane per column.  Returns 1 for a HOST-route cell.
RT_HD int rt_tails_real_cell(const tsfa_relevance_real_col *cols, int64_t n_rows, int64_t ytie, double y0, double y1, int64_t c,
                             double *p, unsigned char *route, unsigned char *type) {
    const tsfa_relevance_real_col o = cols[c];
    const unsigned char ty = rt_type_of(o.n_unique);
    const unsigned char r = rt_route_real_cell(ty);
    type[c] = ty;
    route[c] = r;
    p[c] = (r == TSFA_ROUTE_KENDALL) ? rt_kendall(n_rows, o.dis, o.xtie, o.ntie, o.x0, o.x1, ytie, y0, y1) : RT_NAN;
    return RT_ROUTE_IS_HOST(r) ? 1 : 0;
}

// ---- FDR (significance_tests.py fdr_reject, relevance.py _relevance_table) ----
// the sort key of a p-value: constant columns and NaN go behind every number (numpy's argsort puts NaN last; a p-value
// is at most 1, so +inf is free), and `+inf <= threshold` never holds
RT_HD double rt_fdr_key(double p, unsigned char type) { return (type != 0 && p == p) ? p : RT_INF; }
// threshold of the sorted position k = 1 .. m: (np.arange(1, m + 1) / float(m) / c_m) * alpha, in that order
RT_HD double rt_fdr_threshold(int64_t k, int64_t m, double c_m, double alpha) { return (((double)k / (double)m) / c_m) * alpha; }

// one column over its n_tables tables (p and the per-table flags are [n_cols, n_tables])
RT_HD void rt_fdr_combine(const double *p, const unsigned char *rel_t, int32_t n_tables, unsigned char type, int32_t multiclass,
                          int32_t n_significant, unsigned char *relevant, int32_t *n_sig_out, double *p_min) {
    int32_t cnt = 0;
    double mn = RT_NAN;
    if (type != 0)
        for (int32_t t = 0; t < n_tables; ++t) {
            cnt += rel_t[t] ? 1 : 0;
            const double v = p[t];
            if (v == v && !(mn <= v)) mn = v;  // the smallest number; NaN only when every table is NaN
        }
    *n_sig_out = cnt;
    *relevant = (unsigned char)(multiclass ? (cnt >= n_significant) : (cnt > 0));
    *p_min = mn;
}

// ---- compaction of a byte mask to ascending indices: thread t of nt owns the contiguous slice [t * chunk, (t + 1) * chunk) ----
RT_HD int64_t rt_compact_chunk(int64_t n, int nt) { return (n + nt - 1) / nt; }
RT_HD int32_t rt_compact_count(const unsigned char *mask, int64_t n, int t, int nt) {
    const int64_t chunk = rt_compact_chunk(n, nt), p0 = (int64_t)t * chunk, p1 = (p0 + chunk < n) ? p0 + chunk : n;
    int32_t c = 0;
    for (int64_t p = p0; p < p1; ++p) c += mask[p] ? 1 : 0;
    return c;
}
RT_HD void rt_compact_write(const unsigned char *mask, int64_t n, int t, int nt, int32_t base, int32_t *indices) {
    const int64_t chunk = rt_compact_chunk(n, nt), p0 = (int64_t)t * chunk, p1 = (p0 + chunk < n) ? p0 + chunk : n;
    for (int64_t p = p0; p < p1; ++p)
        if (mask[p]) indices[base++] = (int32_t)p;
}

#endif
