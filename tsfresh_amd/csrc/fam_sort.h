// Family SORT: features that need the order statistics of the series (in-LDS bitonic sort) plus the
// histogram-of-ordinal-patterns and Langevin-polynomial features that reuse its scratch.
#ifndef TSFA_FAM_SORT_H
#define TSFA_FAM_SORT_H

#include "tsfa_common.h"
#include "fam_langevin_dd.h"

// np.quantile(sorted, q, method="linear")   (numpy/lib/_function_base_impl.py: _compute_virtual_index,
// _get_indexes, _get_gamma, _lerp -- the exact expression order matters for tie-sensitive callers)
template <class S>
TSFA_DEV double np_quantile_sorted(S s, int n, double q) {
    const double vi = (double)(n - 1) * q;  // _QuantileMethods["linear"]: get_virtual_index = (n - 1) * quantiles
    int prev, next;
    double pf = floor(vi);
    if (vi >= (double)(n - 1)) {
        prev = next = n - 1;
        pf = -1.0;
    } else if (vi < 0.0) {
        prev = next = 0;
        pf = 0.0;
    } else {
        prev = (int)pf;
        next = prev + 1;
    }
    const double gamma = vi - pf;
    const double a = s(prev), c = s(next);
    const double diff = c - a;
    double r = a + diff * gamma;
    if (gamma >= 0.5) r = c - diff * (1.0 - gamma);
    return r;
}

// pandas Series.quantile(q) as used by pd.qcut: np.percentile(values, q * 100.0) -> q' = (q*100)/100
template <class S>
TSFA_DEV double pd_quantile_sorted(S s, int n, double q) {
    const double qq = (q * 100.0) / 100.0;
    return np_quantile_sorted(s, n, qq);
}

// Minimum-norm least squares  min |A c - y|  for a small dense A (rows x cols, column-major, lda = rows)
// by Householder QR (of A, or of A^T when rows < cols).  Serial; called by one thread.  A and y are
// overwritten; `c` receives cols coefficients; `tmp` >= max(rows, cols) doubles.
TSFA_DEV void small_lstsq(double *A, int rows, int cols, double *y, double *c, double *tmp) {
    if (rows >= cols) {
        for (int k = 0; k < cols; ++k) {
            double nrm = 0.0;
            for (int i = k; i < rows; ++i) nrm += A[i + k * rows] * A[i + k * rows];
            nrm = sqrt(nrm);
            if (nrm == 0.0) { tmp[k] = 0.0; continue; }
            const double alpha = (A[k + k * rows] > 0.0) ? -nrm : nrm;
            const double v0 = A[k + k * rows] - alpha;
            // v = (v0, A[k+1..,k]);  H = I - 2 v v^T / (v^T v)
            double vtv = v0 * v0;
            for (int i = k + 1; i < rows; ++i) vtv += A[i + k * rows] * A[i + k * rows];
            for (int j = k + 1; j < cols; ++j) {
                double d = v0 * A[k + j * rows];
                for (int i = k + 1; i < rows; ++i) d += A[i + k * rows] * A[i + j * rows];
                d = 2.0 * d / vtv;
                A[k + j * rows] -= d * v0;
                for (int i = k + 1; i < rows; ++i) A[i + j * rows] -= d * A[i + k * rows];
            }
            double d = v0 * y[k];
            for (int i = k + 1; i < rows; ++i) d += A[i + k * rows] * y[i];
            d = 2.0 * d / vtv;
            y[k] -= d * v0;
            for (int i = k + 1; i < rows; ++i) y[i] -= d * A[i + k * rows];
            A[k + k * rows] = alpha;
        }
        for (int k = cols - 1; k >= 0; --k) {
            double sacc = y[k];
            for (int j = k + 1; j < cols; ++j) sacc -= A[k + j * rows] * c[j];
            c[k] = sacc / A[k + k * rows];
        }
    } else {
        // underdetermined: B = A^T (cols x rows) = Q R;  A c = y  ->  R^T z = y,  c = Q [z; 0]
        // build B column-major in place is awkward; use tmp-free access B(i, j) = A[j + i * rows]
        // Householder vectors are stored in the strictly-lower part of B, i.e. in A[j + i*rows], i > j.
        double v0s[8];
        double vtvs[8];
        for (int k = 0; k < rows; ++k) {
            double nrm = 0.0;
            for (int i = k; i < cols; ++i) nrm += A[k + i * rows] * A[k + i * rows];
            nrm = sqrt(nrm);
            const double akk = A[k + k * rows];
            const double alpha = (akk > 0.0) ? -nrm : nrm;
            const double v0 = akk - alpha;
            double vtv = v0 * v0;
            for (int i = k + 1; i < cols; ++i) vtv += A[k + i * rows] * A[k + i * rows];
            v0s[k] = v0;
            vtvs[k] = vtv;
            if (vtv != 0.0) {
                for (int j = k + 1; j < rows; ++j) {
                    double d = v0 * A[j + k * rows];
                    for (int i = k + 1; i < cols; ++i) d += A[k + i * rows] * A[j + i * rows];
                    d = 2.0 * d / vtv;
                    A[j + k * rows] -= d * v0;
                    for (int i = k + 1; i < cols; ++i) A[j + i * rows] -= d * A[k + i * rows];
                }
            }
            tmp[k] = alpha;  // R(k, k)
        }
        // R(k, j) for j > k is B(k, j) = A[j + k*rows];  solve R^T z = y (forward)
        for (int k = 0; k < rows; ++k) {
            double sacc = y[k];
            for (int j = 0; j < k; ++j) sacc -= A[k + j * rows] * c[j];
            c[k] = sacc / tmp[k];
        }
        for (int k = rows; k < cols; ++k) c[k] = 0.0;
        // c = H_0 H_1 ... H_{rows-1} [z; 0]
        for (int k = rows - 1; k >= 0; --k) {
            if (vtvs[k] == 0.0) continue;
            double d = v0s[k] * c[k];
            for (int i = k + 1; i < cols; ++i) d += A[k + i * rows] * c[i];
            d = 2.0 * d / vtvs[k];
            c[k] -= d * v0s[k];
            for (int i = k + 1; i < cols; ++i) c[i] -= d * A[k + i * rows];
        }
    }
}

// max(real(np.roots(c)))  for a polynomial of degree <= 3, coefficients highest power first.
TSFA_DEV double max_real_root_deg3(const double *cin, int ncoef) {
    for (int i = 0; i < ncoef; ++i)
        if (cin[i] != cin[i] || isinf(cin[i])) return TSFA_NAN;  // LinAlgError in eigvals
    int lo = 0, hi = ncoef - 1;
    while (lo <= hi && cin[lo] == 0.0) ++lo;   // strip leading zeros
    if (lo > hi) return TSFA_NAN;              // all zero: np.roots -> [] -> max of empty raises -> NaN
    int tz = 0;
    while (hi > lo && cin[hi] == 0.0) { --hi; ++tz; }  // trailing zeros are roots at 0
    const int deg = hi - lo;
    double best = (tz > 0) ? 0.0 : -TSFA_INF;
    bool any = (tz > 0);
    const double *c = cin + lo;
    if (deg == 1) {
        best = fmax(best, -c[1] / c[0]);
        any = true;
    } else if (deg == 2) {
        const double a = c[0], bq = c[1], cc = c[2];
        const double disc = bq * bq - 4.0 * a * cc;
        if (disc < 0.0) {
            best = fmax(best, -bq / (2.0 * a));
        } else {
            const double sq = sqrt(disc);
            const double q = -0.5 * (bq + (bq >= 0.0 ? sq : -sq));
            double r1 = q / a, r2 = (q != 0.0) ? cc / q : r1;
            best = fmax(best, fmax(r1, r2));
        }
        any = true;
    } else if (deg == 3) {
        // monic: x^3 + a x^2 + b x + c
        const double a = c[1] / c[0], bb = c[2] / c[0], cc = c[3] / c[0];
        const double Q = (a * a - 3.0 * bb) / 9.0;
        const double R = (2.0 * a * a * a - 9.0 * a * bb + 27.0 * cc) / 54.0;
        double r1;
        const double R2 = R * R, Q3 = Q * Q * Q;
        if (R2 < Q3) {
            const double th = acos(R / sqrt(Q3));
            const double sq = -2.0 * sqrt(Q);
            const double x0 = sq * cos(th / 3.0) - a / 3.0;
            const double x1 = sq * cos((th + 2.0 * M_PI) / 3.0) - a / 3.0;
            const double x2 = sq * cos((th - 2.0 * M_PI) / 3.0) - a / 3.0;
            r1 = fmax(x0, fmax(x1, x2));
            // Newton polish on the largest root
            for (int it = 0; it < 4; ++it) {
                const double f = ((r1 + a) * r1 + bb) * r1 + cc;
                const double fp = (3.0 * r1 + 2.0 * a) * r1 + bb;
                if (fp == 0.0) break;
                r1 -= f / fp;
            }
            best = fmax(best, r1);
        } else {
            const double A = -((R >= 0.0) ? 1.0 : -1.0) * cbrt(fabs(R) + sqrt(R2 - Q3));
            const double B = (A != 0.0) ? Q / A : 0.0;
            r1 = (A + B) - a / 3.0;
            for (int it = 0; it < 4; ++it) {
                const double f = ((r1 + a) * r1 + bb) * r1 + cc;
                const double fp = (3.0 * r1 + 2.0 * a) * r1 + bb;
                if (fp == 0.0) break;
                r1 -= f / fp;
            }
            // complex pair: sum of roots = -a
            const double re = 0.5 * (-a - r1);
            best = fmax(best, fmax(r1, re));
        }
        any = true;
    } else if (deg == 0) {
        // constant: no non-zero roots
    }
    return any ? best : TSFA_NAN;
}

// Lehmer code of the (stable) ordinal pattern of a[0..D-1]: c_j = #{l > j : a[l] < a[j]}, mixed radix D!/(D-j)!...
// The window is read into registers once for the usual embedding dimensions.
template <int DD, class AT>
TSFA_DEV int perm_code_fixed(const AT *a, int fact) {
    double r[DD];
#pragma unroll
    for (int j = 0; j < DD; ++j) r[j] = (double)a[j];
    int code = 0, f = fact;
#pragma unroll
    for (int j = 0; j < DD - 1; ++j) {
        int c = 0;
#pragma unroll
        for (int l = j + 1; l < DD; ++l) c += (r[l] < r[j]) ? 1 : 0;
        f /= (DD - j);
        code += c * f;
    }
    return code;
}
template <class AT>
TSFA_DEV int perm_code(const AT *a, int D, int fact) {
    switch (D) {
    case 2: return perm_code_fixed<2>(a, fact);
    case 3: return perm_code_fixed<3>(a, fact);
    case 4: return perm_code_fixed<4>(a, fact);
    case 5: return perm_code_fixed<5>(a, fact);
    case 6: return perm_code_fixed<6>(a, fact);
    case 7: return perm_code_fixed<7>(a, fact);
    default: break;
    }
    int code = 0, f = fact;
    for (int j = 0; j < D - 1; ++j) {
        int c = 0;
        for (int l = j + 1; l < D; ++l) c += ((double)a[l] < (double)a[j]) ? 1 : 0;
        f /= (D - j);
        code += c * f;
    }
    return code;
}

#define TSFA_FRIEDRICH_MAX_R 64
#define TSFA_FRIEDRICH_MAX_M 3

// Where friedrich_coeffs leaves an ill-conditioned fit for the double-double pass (fam_langevin_dd.h).  The device
// build records it for k_langevin_dd; the single-thread emulation (no second kernel) redoes the fit in place.
struct FrDefer {
    double *buf;        // the plan's buffer of deferred fits: records of slot_doubles doubles (tsfa_pf_slot_doubles)
    int *count;         // number of records (zeroed before the launch)
    int slot_doubles;
    long long sidx;     // row of this series in the output matrix
    int spec;           // index of the spec that asked for the fit (the pass reads m and r from it)
    int cap;            // records the buffer holds (n_series x distinct (m, r) fits of the plan); a record beyond it is dropped
};

// Exact bin sums.  A value v with |v| < 2^E is split as v = hi 2^-S1 + lo, hi = rint(v 2^S1), S1 = 60 - bits - E (2^bits
// >= the number of addends: the integer sum stays below 2^60), and lo -- exact in float64 -- as rint(lo 2^S2) with S2 =
// S1 + 59 - bits.  Both parts are added as 64-bit integers (LDS atomics on the device): associative, hence independent
// of the order in which the threads arrive, and EXACT for every addend above 2^-50 of the largest (below: to 2^-100
// of the largest).  pandas' groupby mean adds with Kahan compensation, i.e. also returns the (nearly always correctly)
// rounded exact sum; float atomics differed from run to run, a single 2^-50 grid lost the small deltas of a series with
// a large offset.
struct FxScale {
    int s1, s2;
};
TSFA_DEV FxScale fx_scale(double amax, int bits) {
    int e2 = 0;
    (void)frexp(amax, &e2);   // amax < 2^e2
    FxScale f;
    f.s1 = 60 - bits - e2;
    f.s2 = f.s1 + 59 - bits;
    return f;
}
TSFA_DEV void fx_split(double v, FxScale f, long long &hi, long long &lo) {
    const double h = rint(ldexp(v, f.s1));
    hi = (long long)h;
    lo = (long long)rint(ldexp(v - ldexp(h, -f.s1), f.s2));
}
TSFA_DEV double fx_value(long long hi, long long lo, FxScale f) {
    // 64-bit integers do not fit a float64: 26 low bits apart, the four pieces added in double-double
    const long long hh = hi >> 26, hl = hi - hh * 67108864LL, lh = lo >> 26, ll = lo - lh * 67108864LL;
    const double a = ldexp((double)hh, 26 - f.s1), bq = ldexp((double)hl, -f.s1);
    const double c = ldexp((double)lh, 26 - f.s2), d = ldexp((double)ll, -f.s2);
    // a >> bq >> c >> d in magnitude classes: two_sum cascade, smallest first
    double s = c + d;
    double e = d - (s - c);
    double s2 = bq + s;
    double bb = s2 - bq;
    double e2 = (bq - (s2 - bb)) + (s - bb);
    double s3 = a + s2;
    bb = s3 - a;
    double e3 = (a - (s3 - bb)) + (s2 - bb);
    return s3 + (e3 + (e2 + e));
}

// The quantile bins of fc.py:131-160 -- pd.qcut(x[:-1], r), then per bin the sums of x[t] and of x[t + 1] - x[t] and the count:
//   fw[r + 1 ..) = sum x per bin (r), sum delta per bin (r), count per bin (r) as float64; fw[0 .. r] = the bin edges.
//   fw: >= 6 r + 2 doubles (any pointer: LDS in k_sort, an HBM slot in k_general).  Any r.
// Returns false (uniformly) when the series is too short or the bin edges are not unique (qcut raises, the reference returns NaN).
template <class XS, class S1>
TSFA_DEV bool friedrich_bin_means(const Blk &b, XS xs, int n, S1 srt1, int r, double *fw) {
    const int ns = n - 1;
    if (ns < 1 || r < 1) return false;
    double *edges = fw;                 // r + 1
    double *sx = fw + (r + 1);          // r
    double *sy = sx + r;                // r
    double *cnt = sy + r;               // r
    double *lows = cnt + r + 1;         // 2 r: the low parts of the bin sums, until the float64 sums exist
    ar_sync(b);
    // pd.qcut(signal, r): edges = signal.quantile(np.linspace(0, 1, r + 1))
    for (int j = b.tid; j <= r; j += b.nt) {
        const double q = np_linspace_at(0.0, 1.0, r + 1, j);
        edges[j] = pd_quantile_sorted(srt1, ns, q);
    }
    long long *isx = (long long *)(void *)sx, *isy = (long long *)(void *)sy, *icnt = (long long *)(void *)cnt,
              *isxl = (long long *)(void *)lows, *isyl = isxl + r;
    for (int j = b.tid; j < r; j += b.nt) { isx[j] = 0; isy[j] = 0; icnt[j] = 0; isxl[j] = 0; isyl[j] = 0; }
    ar_sync(b);
    double bad = 0.0;
    for (int j = b.tid; j < r; j += b.nt) bad += (edges[j] < edges[j + 1]) ? 0.0 : 1.0;  // "Bin edges must be unique"
    bad = blk_sum(b, bad);
    if (bad > 0.0) return false;
    // bin index = #{edges < x} - 1, with x == edges[0] -> bin 0  (pandas _bins_to_cuts, right=True, include_lowest)
    {
        double amax = fmax(fabs(srt1(0)), fabs(srt1(ns - 1)));
        amax = fmax(amax, fabs(xs[n - 1]));
        int bits = 1;
        while ((1 << bits) < n) ++bits;
        const FxScale fx = fx_scale(amax, bits), fy = fx_scale(2.0 * amax, bits);   // |delta| <= 2 max|x|
        for (int i = b.tid; i < ns; i += b.nt) {
            const double x = xs[i];
            int lo = 0, hi = r + 1;  // count of edges < x
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (edges[mid] < x) lo = mid + 1; else hi = mid;
            }
            int bin = lo - 1;
            if (x == edges[0]) bin = 0;
            if (bin < 0 || bin >= r) continue;
            const double dlt = xs[i + 1] - xs[i];
            long long xh, xl, yh, yl;
            fx_split(x, fx, xh, xl);
            fx_split(dlt, fy, yh, yl);
#if TSFA_GPU
            atomicAdd((unsigned long long *)&isx[bin], (unsigned long long)xh);
            atomicAdd((unsigned long long *)&isy[bin], (unsigned long long)yh);
            if (xl != 0) atomicAdd((unsigned long long *)&isxl[bin], (unsigned long long)xl);
            if (yl != 0) atomicAdd((unsigned long long *)&isyl[bin], (unsigned long long)yl);
            atomicAdd((unsigned long long *)&icnt[bin], 1ULL);
#else
            isx[bin] += xh; isy[bin] += yh; isxl[bin] += xl; isyl[bin] += yl; icnt[bin] += 1;
#endif
        }
        ar_sync(b);
        for (int j = b.tid; j < r; j += b.nt) {  // back to float64 sums
            const double vx = fx_value(isx[j], isxl[j], fx), vy = fx_value(isy[j], isyl[j], fy);
            const double vc = (double)icnt[j];
            sx[j] = vx; sy[j] = vy; cnt[j] = vc;
        }
        ar_sync(b);
    }
    return true;
}

// fc.py:131 _estimate_friedrich_coefficients(x, m, r) -> coeff[0..m] (highest power first), NaN on failure.
//   srt1  : functor, the first n-1 samples sorted ascending (signal = x[:-1])
//   fw    : LDS double scratch >= 6*r + 16 + (r)*(m+1)
// every thread returns the coefficients in `coef`; an ill-conditioned fit is ALSO recorded in df for the second pass,
// which overwrites the columns this one wrote (fam_langevin_dd.h)
template <class XS, class S1>
TSFA_DEV void friedrich_coeffs(const Blk &b, XS xs, int n, S1 srt1, int m, int r,
                               double *fw, double *coef, const FrDefer &df) {
    for (int k = 0; k <= m; ++k) coef[k] = TSFA_NAN;
    const int ns = n - 1;
    if (ns < 1 || r < 1 || r > TSFA_FRIEDRICH_MAX_R || m < 1 || m > TSFA_FRIEDRICH_MAX_M) return;
    double *sx = fw + (r + 1);          // r
    double *sy = sx + r;                // r
    double *cnt = sy + r;               // r
    double *flag = cnt + r;             // 1
    double *A = flag + 1;               // r * (m+1)   (the low parts of the bin sums live here until the means exist)
    double *yv = A + r * (m + 1);       // r
    double *cc = yv + r;                // m + 1
    double *tmp = cc + (m + 1);         // r
    if (!friedrich_bin_means(b, xs, n, srt1, r, fw)) return;
    if (b.tid == 0) flag[0] = 0.0;
    ar_sync(b);
    const int rmax = (df.slot_doubles - TSFA_PF_HDR) / 2;
#if TSFA_GPU
    // np.polyfit(x_mean, y_mean, deg=m): scaled Vandermonde + least squares.  The r <= 64 bins are the lanes of
    // wavefront 0: every lane keeps its row of the design in registers and the Householder reflections are
    // wavefront reductions (the serial LDS version below costs ~1500 dependent LDS round trips).
    if (b.tid < 64) {
        const int lane = b.tid;
        const bool has = (lane < r) && (cnt[lane < r ? lane : 0] > 0.0);
        const unsigned long long mask = __ballot(has);
        const int k = __popcll(mask);
        const int cols = m + 1;
        const int row = has ? __popcll(mask & ((1ull << lane) - 1ull)) : 1000;
        const double xm = has ? sx[lane] / cnt[lane] : 0.0;
        const double ym = has ? sy[lane] / cnt[lane] : 0.0;
        bool defer = (k < cols);    // fewer bins than coefficients: the minimum-norm fit of the second pass
        if (k >= cols) {
            double yrow = ym;
            double a[TSFA_FRIEDRICH_MAX_M + 1], scale[TSFA_FRIEDRICH_MAX_M + 1], R[TSFA_FRIEDRICH_MAX_M + 1][TSFA_FRIEDRICH_MAX_M + 1],
                qy[TSFA_FRIEDRICH_MAX_M + 1];
#pragma unroll
            for (int c = 0; c <= TSFA_FRIEDRICH_MAX_M; ++c) {
                a[c] = 0.0;
                scale[c] = 1.0;
                if (c < cols) {
                    double pw = 1.0;
                    for (int e = 0; e < m - c; ++e) pw *= xm;
                    pw = has ? pw : 0.0;
                    scale[c] = sqrt(wave_sum(pw * pw));
                    a[c] = pw / scale[c];
                    if (!has) a[c] = 0.0;
                }
            }
            double rmin = TSFA_INF, rbig = 0.0;
#pragma unroll
            for (int kk = 0; kk <= TSFA_FRIEDRICH_MAX_M; ++kk) {
                if (kk < cols) {
                    const bool below = has && (row >= kk);
                    const double nrm = sqrt(wave_sum(below ? a[kk] * a[kk] : 0.0));
                    const double akk = wave_sum((row == kk) ? a[kk] : 0.0);
                    if (nrm != 0.0) {
                        const double alpha = (akk > 0.0) ? -nrm : nrm;
                        const double v0 = akk - alpha;
                        const double vi = (row == kk) ? v0 : ((has && row > kk) ? a[kk] : 0.0);
                        const double vtv = wave_sum(vi * vi);
#pragma unroll
                        for (int j = 0; j <= TSFA_FRIEDRICH_MAX_M; ++j) {
                            if (j > kk && j < cols) {
                                const double d = 2.0 * wave_sum(vi * a[j]) / vtv;
                                a[j] -= d * vi;
                            }
                        }
                        const double d = 2.0 * wave_sum(vi * yrow) / vtv;
                        yrow -= d * vi;
                        R[kk][kk] = alpha;
                    } else {
                        R[kk][kk] = akk;
                    }
                    rmin = fmin(rmin, fabs(R[kk][kk]));
                    rbig = fmax(rbig, fabs(R[kk][kk]));
#pragma unroll
                    for (int j = 0; j <= TSFA_FRIEDRICH_MAX_M; ++j)
                        if (j > kk && j < cols) R[kk][j] = wave_sum((row == kk) ? a[j] : 0.0);
                    qy[kk] = wave_sum((row == kk) ? yrow : 0.0);
                }
            }
            double sol[TSFA_FRIEDRICH_MAX_M + 1];
#pragma unroll
            for (int kk = TSFA_FRIEDRICH_MAX_M; kk >= 0; --kk) {
                sol[kk] = 0.0;
                if (kk < cols) {
                    double sacc = qy[kk];
#pragma unroll
                    for (int j = 0; j <= TSFA_FRIEDRICH_MAX_M; ++j)
                        if (j > kk && j < cols) sacc -= R[kk][j] * sol[j];
                    sol[kk] = sacc / R[kk][kk];
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c <= TSFA_FRIEDRICH_MAX_M; ++c)
                    if (c < cols) cc[c] = sol[c] / scale[c];
                flag[0] = 1.0;
            }
            defer = (rmin < TSFA_PF_FLAG * rbig);   // false for NaN: a non-finite fit stays what it is
        }
        if (defer && k >= 1) {
            if (df.buf != nullptr && r <= rmax) {
                int slot = 0;
                if (lane == 0) slot = atomicAdd(df.count, 1);
                slot = __shfl(slot, 0);
                if (slot < df.cap) {   // (cannot fail: the plan evaluates each distinct (m, r) once per series)
                    double *rec = df.buf + (size_t)slot * (size_t)df.slot_doubles;
                    if (lane == 0) { rec[0] = (double)df.sidx; rec[1] = (double)df.spec; rec[2] = (double)k; }
                    if (has) { rec[TSFA_PF_HDR + row] = xm; rec[TSFA_PF_HDR + rmax + row] = ym; }
                }
            }   // (no buffer: the float64 fit stands; the library always passes one)
        }
    }
#else
    if (b.tid == 0) {
        // np.polyfit(x_mean, y_mean, deg=m): scaled Vandermonde + lstsq
        int k = 0;
        double ysave[TSFA_FRIEDRICH_MAX_R];
        for (int j = 0; j < r; ++j) {
            if (cnt[j] > 0.0) {
                tmp[k] = sx[j] / cnt[j];
                yv[k] = sy[j] / cnt[j];
                ysave[k] = yv[k];
                ++k;
            }
        }
        const int cols = m + 1;
        double scale[TSFA_FRIEDRICH_MAX_M + 1];
        for (int c = 0; c < cols; ++c) {
            double ss = 0.0;
            for (int i = 0; i < k; ++i) {
                double pw = 1.0;
                for (int e = 0; e < m - c; ++e) pw *= tmp[i];
                A[i + c * k] = pw;
                ss += pw * pw;
            }
            scale[c] = sqrt(ss);
            for (int i = 0; i < k; ++i) A[i + c * k] /= scale[c];
        }
        bool defer = (k < cols);
        if (k >= cols) {
            double xsave[TSFA_FRIEDRICH_MAX_R];
            for (int i = 0; i < k; ++i) xsave[i] = tmp[i];
            small_lstsq(A, k, cols, yv, cc, tmp);
            for (int c = 0; c < cols; ++c) cc[c] = cc[c] / scale[c];
            flag[0] = 1.0;
            double rmin = TSFA_INF, rbig = 0.0;
            for (int c = 0; c < cols; ++c) {   // the diagonal of R
                rmin = fmin(rmin, fabs(A[c + c * k]));
                rbig = fmax(rbig, fabs(A[c + c * k]));
            }
            defer = (rmin < TSFA_PF_FLAG * rbig);
            for (int i = 0; i < k; ++i) tmp[i] = xsave[i];
        }
        if (defer && k >= 1) {
            (void)rmax;
            double cf[TSFA_PF_MAXC];
            const double *tx = tmp;
            polyfit_svd_dd([=](int i) { return tx[i]; }, [=](int i) { return ysave[i]; }, k, m, cf);
            for (int c = 0; c < cols; ++c) cc[c] = cf[c];
            flag[0] = 1.0;
        }
    }
#endif
    ar_sync(b);
    if (flag[0] != 0.0)
        for (int c = 0; c <= m; ++c) coef[c] = cc[c];
    ar_sync(b);
}

// Evaluate the SORT specs of one series.
//   xs   : series (LDS, n doubles)
//   srt  : LDS, >= next_pow2(n) doubles (sorted copy)
//   w    : LDS, >= 768 doubles (Langevin-fit scratch)
//   iw   : LDS, >= 2520 ints (ordinal-pattern histogram, two 16-bit counters per word); may alias w
// change_quantiles (fc.py:1511), every corridor of the plan, four per sweep, ONE pass over the samples per sweep.
// cq[5 * k ..] = count, mean, mean |.|, var, var |.| of corridor k.
//   * The corridor edges -- pd.qcut's quantiles, 2 per corridor -- are evaluated once, lane = edge (until round 6 every sweep
//     evaluated its eight edges one after the other on all lanes: 30 dependent chains of two LDS reads, 22 k of the
//     calculator's 115 k cycles per 1024-sample series); a sweep reads its eight back as wave-uniform values.
//   * The variances come from the same pass as the means: sums of (d - s) and (d - s)^2 about a shift known before the pass,
//     s = the mean change of the whole series (x[n-1] - x[0]) / (n - 1), and |s| for the absolute changes:
//         mean = s + S1 / c,   var = S2 / c - (S1 / c)^2.
//     The cancellation in `var` costs eps * (mean - s)^2 <= eps * (4 max|x|)^2, seven decades below the parity bar's absolute
//     floor for a quadratic feature (tests/parity.py: 1e-9 max|x|^2); a second masked pass about each corridor's own mean
//     (what np.var does, and what this function did until round 6) doubled the predicate evaluations and the sample reads.
//   * That floor is no bound where the changes inside a corridor are nearly constant (a sawtooth's rising flank: the
//     corridor's mean change is the slope, far from the series' mean change s, and the variance a jitter twelve decades
//     below slope^2).  The relative error of the one-pass form is K eps R, R = (S2 / c) / var the cancellation ratio; K
//     measured 7 .. 20 on 300 .. 8197 samples (profiles/shift_invariance.md: 5.4e-10 at R = 3.4e5, 1.4e-5 at 3.4e9, 7e-2
//     at 3.3e13).  A corridor whose one-pass variance comes out below TSFA_CQ_REFINE = 2^-20 of S2 / c (R > 1e6: the
//     one-pass error reaches 5e-9 there, 200 times inside the 1e-6 bar, and the gate itself is read from a variance that is
//     still good to 5e-9) is swept again about its own mean.  Noise never asks: R is 1 + mean^2 / var, below 3 for the absolute changes
//     of iid normal samples, 1 for the signed ones (tests/test_shift_invariance.py counts the sweeps of a batch: none), and
//     a corridor that does not ask keeps its bits.  What does ask besides a jittered flank: two or more changes inside a
//     corridor that are EXACTLY equal while their mean differs from s (a piecewise-linear series) -- the one-pass variance is
//     then 0 or round-off, indistinguishable from a cancelled 1e-20, and the sweep is paid to return 0; a corridor holding
//     a single change is left alone.
#define TSFA_CQ_REFINE 9.5367431640625e-07   // 2^-20
#ifdef TSFA_EMUL
static long long g_tsfa_cq_refined = 0;   // the emulation counts the second sweeps (tsfa_emul_cq_refined)
#define TSFA_CQ_REFINE_NOTE() (++g_tsfa_cq_refined)
#else
#define TSFA_CQ_REFINE_NOTE() ((void)0)
#endif
// The second sweep of one corridor [l, h]: the variances of the changes and of the absolute changes about the corridor's own
// means mu1, mu2 (c changes inside), in the corrected two-pass form -- the sums of the residuals are the round-off of the means
// and take it out again.  Block-uniform: every thread calls it.
struct CqRefined { double v, va; };
template <class XS>
TSFA_DEVN CqRefined cq_refine_corridor(const Blk &b, XS xs, int n, double l, double h, double mu1, double mu2, double c) {
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = b.tid; i < n - 1; i += b.nt) {
        const double x0 = xs[i], x1 = xs[i + 1];
        if (x0 >= l && x0 <= h && x1 >= l && x1 <= h) {
            const double d = x1 - x0;
            const double e1 = d - mu1, e2 = fabs(d) - mu2;
            e[0] += e1;
            e[1] += e1 * e1;
            e[2] += e2;
            e[3] += e2 * e2;
        }
    }
    blk_sum_multi<4>(b, e);
    CqRefined r;
    r.v = (e[1] - e[0] * e[0] / c) / c;
    r.va = (e[3] - e[2] * e[2] / c) / c;
    return r;
}
template <class XS, class SS>
TSFA_DEV void cq_fill_all(const Blk &b, XS xs, SS srt, int n, const TsfaCqPlan &plan, double *cq) {
    TSFA_TICKER(tkq, 0);
    // pd.qcut(x, [ql, qh], labels=False) == 0  <=>  lo <= x <= hi  (right-closed, include_lowest)
    for (int e0 = 0; e0 < 2 * plan.n; e0 += b.nt) {
        const int e = e0 + b.tid;
        double q = 0.0;
#if TSFA_GPU
        // (the plan is a by-value kernel argument: a lane-indexed read would move it to scratch memory)
        for (int c = 0; c < plan.n; ++c) {
            q = (e == c) ? plan.ql[c] : q;
            q = (e == plan.n + c) ? plan.qh[c] : q;
        }
#else
        if (e < 2 * plan.n) q = (e < plan.n) ? plan.ql[e] : plan.qh[e - plan.n];
#endif
        if (e < 2 * plan.n) {
            const double v = pd_quantile_sorted([=](int i) { return srt[i]; }, n, q);
            if (e < plan.n) cq[5 * e] = v; else cq[5 * (e - plan.n) + 1] = v;
        }
    }
    ar_sync(b);
    double s = (n > 1) ? (xs[n - 1] - xs[0]) / (double)(n - 1) : 0.0;
    if (!(fabs(s) <= 1.7976931348623157e308)) s = 0.0;   // an infinite end sample must not reach the corridors that exclude it
    const double sa = fabs(s);
    TSFA_TICK(tkq, b, 220);
    for (int k0 = 0; k0 < plan.n; k0 += 4) {
        const int ng = (plan.n - k0 < 4) ? (plan.n - k0) : 4;
        double lo[4], hi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // (wave-uniform: the edges stay in scalar registers for the sweep; as vector operands they measured 20 % slower
            // for the whole kernel)
            const int k = (j < ng) ? (k0 + j) : k0;
            double l = cq[5 * k], h = cq[5 * k + 1];
#if TSFA_GPU
            l = readlane_f64(l, 0);
            h = readlane_f64(h, 0);
#endif
            lo[j] = (j < ng) ? l : TSFA_INF;
            hi[j] = (j < ng) ? h : -TSFA_INF;
        }
        double a[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) a[k] = 0.0;
        for (int i = b.tid; i < n - 1; i += b.nt) {
            const double x0 = xs[i], x1 = xs[i + 1];
            const double d = x1 - x0;
            const double dd = d - s, ad = fabs(d) - sa;
            const double dd2 = dd * dd, ad2 = ad * ad;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (x0 >= lo[j] && x0 <= hi[j] && x1 >= lo[j] && x1 <= hi[j]) {
                    a[5 * j] += 1.0;
                    a[5 * j + 1] += dd;
                    a[5 * j + 2] += ad;
                    a[5 * j + 3] += dd2;
                    a[5 * j + 4] += ad2;
                }
            }
        }
        TSFA_TICK(tkq, b, 221);
        blk_sum_multi<20>(b, a);
        TSFA_TICK(tkq, b, 222);
        // The refinement.  Every thread holds the block's sums, so the gate is block-uniform: bit j asks for the signed
        // variance of corridor j about its own mean, bit 4 + j for that of the absolute changes (c^2 times the gate above,
        // no division; a NaN or an empty corridor asks for nothing).
        int refine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double c = a[5 * j], q1 = a[5 * j + 3] * c, q2 = a[5 * j + 4] * c;
            const bool many = c > 1.0;   // (a single change has the variance 0 in either form)
            refine |= (many && q1 - a[5 * j + 1] * a[5 * j + 1] < TSFA_CQ_REFINE * q1) ? (1 << j) : 0;
            refine |= (many && q2 - a[5 * j + 2] * a[5 * j + 2] < TSFA_CQ_REFINE * q2) ? (16 << j) : 0;
        }
#if TSFA_GPU
        refine = __builtin_amdgcn_readfirstlane(refine);   // a scalar branch around the sweep and its barriers
#endif
        for (int j = 0; refine != 0 && j < ng; ++j) {
            if (((refine >> j) & 0x11) == 0) continue;
            TSFA_CQ_REFINE_NOTE();
            double l = lo[0], h = hi[0], c = a[0], t1 = a[1], t2 = a[2];
#pragma unroll
            for (int jj = 1; jj < 4; ++jj) {   // (selects between wave-uniform values: lo[j] would move the arrays to scratch)
                l = (jj == j) ? lo[jj] : l;
                h = (jj == j) ? hi[jj] : h;
                c = (jj == j) ? a[5 * jj] : c;
                t1 = (jj == j) ? a[5 * jj + 1] : t1;
                t2 = (jj == j) ? a[5 * jj + 2] : t2;
            }
            // (a call, not inline code: the sweep that every series runs keeps the registers it had without the refinement)
            const CqRefined w = cq_refine_corridor(b, xs, n, l, h, s + t1 / c, sa + t2 / c, c);
            const double w1 = w.v, w2 = w.va;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                a[5 * jj + 3] = (jj == j && ((refine >> jj) & 1)) ? w1 : a[5 * jj + 3];
                a[5 * jj + 4] = (jj == j && ((refine >> jj) & 16)) ? w2 : a[5 * jj + 4];
            }
        }
        ar_sync(b);   // every thread has read this sweep's edges
        if (b.tid == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < ng) {
                    double *o = cq + 5 * (k0 + j);
                    const double c = a[5 * j];
                    const bool any = c > 0.0;
                    const double m1 = any ? a[5 * j + 1] / c : 0.0, m2 = any ? a[5 * j + 2] / c : 0.0;
                    o[0] = c;
                    o[1] = any ? s + m1 : 0.0;
                    o[2] = any ? sa + m2 : 0.0;
                    double v1 = a[5 * j + 3] / c - m1 * m1, v2 = a[5 * j + 4] / c - m2 * m2;
                    v1 = ((refine >> j) & 1) ? a[5 * j + 3] : v1;     // (refined: the slot holds the variance itself)
                    v2 = ((refine >> j) & 16) ? a[5 * j + 4] : v2;
                    o[3] = any ? ((v1 < 0.0) ? 0.0 : v1) : 0.0;   // (a NaN stays a NaN: inf - inf changes inside the corridor)
                    o[4] = any ? ((v2 < 0.0) ? 0.0 : v2) : 0.0;
                }
            }
        }
    }
    ar_sync(b);
}

// Per-series values the epilogue columns of the family read (LDS, TSFA_SORT_CTX doubles)
enum { TSFA_SCTX_SYM = 0, TSFA_SCTX_NUNIQUE, TSFA_SCTX_MULTI_VALS, TSFA_SCTX_MULTI_PTS, TSFA_SCTX_SUM_VALS, TSFA_SCTX_SUM_PTS,
       TSFA_SORT_CTX = 8 };

// Columns [first, nspecs) with lane = column: order statistics of the sorted copy and reads of the caches.
template <class SS>
TSFA_DEV void sort_epilogue(const Blk &b, const TsfaSpec *specs, int first, int nspecs, int n, SS srt, const double *ctx,
                            const double *cq, double *out_row) {
    const double dn = (double)n;
    const double vmin = srt[0], vmax = srt[n - 1];
    for (int s = first + b.tid; s < nspecs; s += b.nt) {
        const TsfaSpec sp = specs[s];
        const double p0 = sp.p[0];
        double v = TSFA_NAN;
        switch (sp.calc) {
        case TSFA_C_MEDIAN: v = (n & 1) ? srt[(n - 1) / 2] : (0.0 + srt[n / 2 - 1] + srt[n / 2]) / 2.0; break;
        case TSFA_C_QUANTILE: v = np_quantile_sorted([=](int i) { return srt[i]; }, n, p0); break;
        case TSFA_C_SYMMETRY_LOOKING: v = (ctx[TSFA_SCTX_SYM] < p0 * (vmax - vmin)) ? 1.0 : 0.0; break;
        case TSFA_C_CHANGE_QUANTILES: {
            if (sp.p[1] != -2.0) { v = 0.0; break; }  // ql >= qh
            const double *o = cq + 5 * (((int)p0) & 127);
            const bool isabs = (sp.p[2] != 0.0);
            if (o[0] == 0.0) v = 0.0;
            else if ((int)sp.p[3] == TSFA_AGG_MEAN) v = isabs ? o[2] : o[1];
            else v = isabs ? o[4] : o[3];
        } break;
        case TSFA_C_HAS_DUPLICATE: v = (ctx[TSFA_SCTX_NUNIQUE] != dn) ? 1.0 : 0.0; break;
        case TSFA_C_RATIO_VALUE_NUMBER: v = ctx[TSFA_SCTX_NUNIQUE] / dn; break;
        case TSFA_C_PCT_REOCC_VALUES: v = ctx[TSFA_SCTX_MULTI_VALS] / ctx[TSFA_SCTX_NUNIQUE]; break;
        case TSFA_C_PCT_REOCC_DATAPOINTS: v = ctx[TSFA_SCTX_MULTI_PTS] / dn; break;
        case TSFA_C_SUM_REOCC_VALUES: v = ctx[TSFA_SCTX_SUM_VALS]; break;
        case TSFA_C_SUM_REOCC_DATA_POINTS: v = ctx[TSFA_SCTX_SUM_PTS]; break;
        default: break;
        }
        out_row[sp.col] = v;
    }
}

// The sorted series as a 16-bit ORDER beside the resident samples instead of a sorted copy: srt[i] is read as xs[ord[i]] --
// two bytes per sample in LDS where the copy takes four or eight (tsfa_layout.h: SortLds, what puts 16 one-wavefront series
// of 1024 float32 samples on a CU), the same values in the same places, and a second, dependent LDS read per access.
template <class ST>
struct OrdView {
    const ST *p;
    const unsigned short *o;
    TSFA_MEM double operator[](int i) const { return (double)p[o[i]]; }
};
template <class ST, bool ORD> struct SortedView { typedef XsView<ST> type; };
template <class ST> struct SortedView<ST, true> { typedef OrdView<ST> type; };

// ST: element type of the LDS-resident series and of its sorted copy (the input precision; read as float64)
// ORD: srt_raw holds the 16-bit sample order (OrdView; n entries) and not a sorted copy.  Only with perm_in -- the order
//      is the one another family established -- and with pe_hint != 0: permutation_entropy of a dimension >= 8 borrows the
//      sorted copy's storage, and such a plan keeps the copy (tsfa_api.cpp decides; the kernel is told, it does not choose).
template <class ST, bool ORD = false>
TSFA_DEV void fam_sort_series(const Blk &b, const ST *xs_raw, int n, const TsfaSpec *specs, int nspecs,
                              double *out_row, ST *srt_raw, double *w, int *iw, const TsfaCqPlan &cqplan, double *cq,
                              TsfaSpec *stage, int n_loop = -1, double *ctx = nullptr, int w_doubles = 1280,
                              FrDefer df = FrDefer{nullptr, nullptr, TSFA_PF_HDR + 2 * TSFA_FRIEDRICH_MAX_R, 0, 0},
                              const unsigned short *perm_in = nullptr, const double *stats = nullptr, int pe_hint = 0) {
    // iw aliases w: 32-bit words of the ordinal-pattern histogram.  Where the numpy-order scratch has storage of its own, its
    // leaf sums (idle here) hold the table of logarithms; in the one-wavefront layout that scratch shares w or is absent
    // (SortLds), and the table takes the last 64 doubles of w
    const bool own_np = (b.np != nullptr) && ((const void *)b.np != (const void *)w);
    const int hist_words = own_np ? 2 * w_doubles : 2 * (w_doubles - 64);
    // n_loop columns go through the column loop; the rest are evaluated by sort_epilogue (lane = column)
    const int nloop = (n_loop >= 0 && ctx != nullptr) ? n_loop : nspecs;
    typedef typename SortedView<ST, ORD>::type SV;
    const XsView<ST> xs{xs_raw};
    unsigned short *ord = (unsigned short *)(void *)srt_raw;
    (void)ord;
    SV srt;
    if constexpr (ORD) { srt.p = xs_raw; srt.o = ord; } else { srt.p = srt_raw; }
    const int np2 = next_pow2(n);
    TSFA_TICKER(tk, 0);
    ar_sync(b);
    // perm_in: the sample order another family of the same plan already established (k_entropy_bits sorts the samples
    // for its ranges and leaves the permutation in HBM, 2 bytes per sample): the sorted copy is then a gather from the
    // resident series instead of a second sort of the same keys (62 k of this kernel's cycles per series)
    // (a function: permutation_entropy of dimension >= 8 borrows srt_raw for its sorted pattern codes and rebuilds the copy)
    auto build_sorted_copy = [&]() {
        if constexpr (ORD) {
            if (n >= 3) {
                for (int i = b.tid; i < n; i += b.nt) ord[i] = perm_in[i];
            } else if (b.tid == 0) {   // (the order's owner leaves none for a series of fewer than three samples)
                const bool swap = (n == 2) && (xs_raw[1] < xs_raw[0]);
                ord[0] = swap ? 1 : 0;
                if (n == 2) ord[1] = swap ? 0 : 1;
            }
            ar_sync(b);
        } else
        if (perm_in != nullptr && n >= 3) {
            for (int i = b.tid; i < np2; i += b.nt) srt_raw[i] = (i < n) ? xs_raw[perm_in[i]] : (ST)TSFA_INF;
            ar_sync(b);
        } else
#if TSFA_GPU
        if (!blk_sorted_copy_regs(b, xs_raw, n, srt_raw, np2))
#endif
        {
            for (int i = b.tid; i < np2; i += b.nt) srt_raw[i] = (i < n) ? xs_raw[i] : (ST)TSFA_INF;
            blk_bitonic_sort(b, srt_raw, np2);
        }
    };
    build_sorted_copy();
    TSFA_TICK(tk, b, 104);
    const double dn = (double)n;
    const double vmin = srt[0], vmax = srt[n - 1];

    // one-entry caches: consecutive specs of the reference's parameter grids share their expensive part
    bool have_sym = false, cq_valid = false, fr_valid = false;
    double sym_dist = 0.0, cq_ql = 0.0, cq_qh = 0.0, cq_cnt = 0.0, cq_mean = 0.0, cq_mean_abs = 0.0, cq_var = 0.0, cq_var_abs = 0.0;
    int fr_m = 0, fr_r = 0;
    double fr_coef[TSFA_FRIEDRICH_MAX_M + 1];

    // run structure of the sorted array (np.unique / value_counts)
    double n_unique = 0.0, n_multi_vals = 0.0, n_multi_pts = 0.0, sum_multi_vals = 0.0, sum_multi_pts = 0.0;
    bool have_runs = false;

    for (int s = 0; s < nloop; ++s) {
        const TsfaSpec sp = spec_fetch(b, specs, nspecs, s, stage);
        const double p0 = sp.p[0], p1 = sp.p[1], p2 = sp.p[2], p3 = sp.p[3];
        double v = TSFA_NAN;
        switch (sp.calc) {
        case TSFA_C_MEDIAN:                                              // fc.py:663 np.median
            v = (n & 1) ? srt[(n - 1) / 2] : (0.0 + srt[n / 2 - 1] + srt[n / 2]) / 2.0;
            break;
        case TSFA_C_QUANTILE:                                            // fc.py:1963
            v = np_quantile_sorted([=](int i) { return srt[i]; }, n, p0);
            break;
        case TSFA_C_SYMMETRY_LOOKING: {                                  // fc.py:299
            if (!have_sym) {
                // (stats: the record k_basic left for this series, TSFA_STATS_*: the same numpy-order mean)
                const double mean = stats ? stats[TSFA_STATS_MEAN] : np_sum(b, n, [=](int i) { return xs[i]; }) / dn;
                const double med = (n & 1) ? srt[(n - 1) / 2] : (0.0 + srt[n / 2 - 1] + srt[n / 2]) / 2.0;
                sym_dist = fabs(mean - med);
                have_sym = true;
                if (nloop < nspecs && b.tid == 0) ctx[TSFA_SCTX_SYM] = sym_dist;
            }
            v = (sym_dist < p0 * (vmax - vmin)) ? 1.0 : 0.0;
        } break;
        case TSFA_C_MEAN_N_ABSOLUTE_MAX: {                               // fc.py:1643
            const int k = (int)p0;
            double r = TSFA_NAN;
            if (b.tid == 0 && n > k) {
                int lo = 0, hi = n - 1;
                double acc = 0.0;
                for (int t = 0; t < k; ++t) {  // k largest |x| sit at the two ends of the sorted array
                    const double a = fabs(srt[lo]), c = fabs(srt[hi]);
                    if (a > c) { acc += a; ++lo; } else { acc += c; --hi; }
                }
                r = acc / (double)k;
            }
            v = blk_bcast0(b, r);
        } break;
        case TSFA_C_CHANGE_QUANTILES: {                                  // fc.py:1511
            const double ql = p0, qh = p1;
            const bool isabs = (p2 != 0.0);
            const int agg = (int)p3;
            if (cqplan.n > 0 && p1 == -2.0) {  // indexed corridor: the first such column evaluates them all
                if ((int)p0 >= 128) cq_fill_all(b, xs, srt, n, cqplan, cq);
                const double *o = cq + 5 * (((int)p0) & 127);
                if (o[0] == 0.0) v = 0.0;
                else if (agg == TSFA_AGG_MEAN) v = isabs ? o[2] : o[1];
                else v = isabs ? o[4] : o[3];
                break;
            }
            if (ql >= qh) { v = 0.0; break; }
            if (!(cq_valid && cq_ql == ql && cq_qh == qh)) {
                // one scan per corridor serves its four columns (isabs x {mean, var})
                // pd.qcut(x, [ql, qh], labels=False) == 0  <=>  lo <= x <= hi  (right-closed, include_lowest)
                const double lo = pd_quantile_sorted([=](int i) { return srt[i]; }, n, ql);
                const double hi = pd_quantile_sorted([=](int i) { return srt[i]; }, n, qh);
                double c = 0.0, a = 0.0, aa = 0.0;
                for (int i = b.tid; i < n - 1; i += b.nt) {
                    const double x0 = xs[i], x1 = xs[i + 1];
                    if (x0 >= lo && x0 <= hi && x1 >= lo && x1 <= hi) {
                        const double d = x1 - x0;
                        c += 1.0;
                        a += d;
                        aa += fabs(d);
                    }
                }
                c = blk_sum(b, c);
                a = blk_sum(b, a);
                aa = blk_sum(b, aa);
                cq_cnt = c;
                cq_mean = (c > 0.0) ? a / c : 0.0;
                cq_mean_abs = (c > 0.0) ? aa / c : 0.0;
                double ss = 0.0, ssa = 0.0;
                if (c > 0.0) {
                    const double m1 = cq_mean, m2 = cq_mean_abs;
                    for (int i = b.tid; i < n - 1; i += b.nt) {
                        const double x0 = xs[i], x1 = xs[i + 1];
                        if (x0 >= lo && x0 <= hi && x1 >= lo && x1 <= hi) {
                            const double d = x1 - x0;
                            ss += (d - m1) * (d - m1);
                            ssa += (fabs(d) - m2) * (fabs(d) - m2);
                        }
                    }
                    ss = blk_sum(b, ss);
                    ssa = blk_sum(b, ssa);
                }
                cq_var = (c > 0.0) ? ss / c : 0.0;
                cq_var_abs = (c > 0.0) ? ssa / c : 0.0;
                cq_valid = true;
                cq_ql = ql;
                cq_qh = qh;
            }
            if (cq_cnt == 0.0) v = 0.0;
            else if (agg == TSFA_AGG_MEAN) v = isabs ? cq_mean_abs : cq_mean;
            else v = isabs ? cq_var_abs : cq_var;
        } break;
        case TSFA_C_HAS_DUPLICATE:
        case TSFA_C_RATIO_VALUE_NUMBER:
        case TSFA_C_PCT_REOCC_VALUES:
        case TSFA_C_PCT_REOCC_DATAPOINTS:
        case TSFA_C_SUM_REOCC_VALUES:
        case TSFA_C_SUM_REOCC_DATA_POINTS: {
            if (!have_runs) {
                double nu = 0.0, mv = 0.0, mp = 0.0, sv = 0.0, spn = 0.0;
                for (int i = b.tid; i < n; i += b.nt) {
                    const double x = srt[i];
                    const bool eq_prev = (i > 0) && (srt[i - 1] == x);
                    const bool eq_next = (i < n - 1) && (srt[i + 1] == x);
                    if (!eq_prev) {
                        nu += 1.0;
                        if (eq_next) { mv += 1.0; sv += x; }
                    }
                    if (eq_prev || eq_next) { mp += 1.0; spn += x; }
                }
                double r5[5] = {nu, mv, mp, sv, spn};  // reduced together: one barrier pair
                blk_sum_multi<5>(b, r5);
                n_unique = r5[0]; n_multi_vals = r5[1]; n_multi_pts = r5[2]; sum_multi_vals = r5[3]; sum_multi_pts = r5[4];
                have_runs = true;
                if (nloop < nspecs && b.tid == 0) {
                    ctx[TSFA_SCTX_NUNIQUE] = n_unique; ctx[TSFA_SCTX_MULTI_VALS] = n_multi_vals;
                    ctx[TSFA_SCTX_MULTI_PTS] = n_multi_pts; ctx[TSFA_SCTX_SUM_VALS] = sum_multi_vals;
                    ctx[TSFA_SCTX_SUM_PTS] = sum_multi_pts;
                }
            }
            if (sp.calc == TSFA_C_HAS_DUPLICATE) v = (n_unique != dn) ? 1.0 : 0.0;             // fc.py:355
            else if (sp.calc == TSFA_C_RATIO_VALUE_NUMBER) v = n_unique / dn;                   // fc.py:1045
            else if (sp.calc == TSFA_C_PCT_REOCC_VALUES) v = n_multi_vals / n_unique;           // fc.py:933
            else if (sp.calc == TSFA_C_PCT_REOCC_DATAPOINTS) v = n_multi_pts / dn;              // fc.py:961
            else if (sp.calc == TSFA_C_SUM_REOCC_VALUES) v = sum_multi_vals;                    // fc.py:992
            else v = sum_multi_pts;                                                              // fc.py:1020
        } break;
        case TSFA_C_PERMUTATION_ENTROPY: {                               // fc.py:1866
            const int tau = (int)p0, D = (int)p1;
            // pe_hint: the launch left every permutation_entropy column of the plan to k_perm (fam_perm.h)
            if (ORD || pe_hint != 0) { TSFA_TICK(tk, b, sp.calc); continue; }
            const int num = (n >= D) ? ((n - D) / tau + 1) : 0;
            if (num <= 0) { v = TSFA_NAN; break; }
            int fact = 1;
            for (int k = 2; k <= D; ++k) fact *= k;
            // Two 16-bit counters per LDS word (at most n <= 65535 windows).  The histogram only has room for
            // 2 * hist_words patterns: the pattern space is swept in ranges of that size (one pass for D <= 6 at the
            // usual sizes, four for D = 7 with a 2.5 KB scratch).  With <= 8 windows per thread their codes are
            // computed ONCE and stay in registers for all passes (the code of a D = 7 window is 21 compares).
            // ... a series of more than 65 535 windows (the long-series build, round 5) counts in whole words: a constant or
            // monotone series puts every window into ONE pattern
            const bool wide = num > 65535;
            const int per_pass = wide ? hist_words : 2 * hist_words;
            if (!ORD && fact > 16 * per_pass && sizeof(ST) >= sizeof(int)) {
                // Dimensions 8 .. 10 (40 320 .. 3 628 800 patterns; the reference takes any dimension, round-5 VERDICT missing #2):
                // sweeping the pattern space through the LDS histogram would take thousands of passes.  Instead the windows'
                // codes are SORTED -- in the storage of the sorted copy of the series, np2 elements of at least four bytes,
                // which is rebuilt afterwards -- and the runs of equal codes counted: sum over the runs of (c / num) log(c / num),
                // the run's end found by bisection from its first element.  Only plans that ask for such a dimension pay.
                int *codes_s = (int *)(void *)srt_raw;
                const int cp2 = next_pow2(num);
                ar_sync(b);
                for (int t = b.tid; t < cp2; t += b.nt) codes_s[t] = (t < num) ? perm_code(xs_raw + t * tau, D, fact) : 0x7FFFFFFF;
                blk_bitonic_sort(b, codes_s, cp2);
                double es = 0.0;
                for (int t = b.tid; t < num; t += b.nt) {
                    const int c0 = codes_s[t];
                    if (t > 0 && codes_s[t - 1] == c0) continue;   // not the first of its run
                    int lo = t + 1, hi = num;                      // first index with a larger code
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (codes_s[mid] > c0) hi = mid; else lo = mid + 1; }
                    const double pr = (double)(lo - t) / (double)num;
                    es += pr * log(pr);
                }
                v = -blk_sum(b, es);
                ar_sync(b);
                build_sorted_copy();
                break;
            }
            const bool in_regs = (num <= 8 * b.nt);
            TSFA_TICKER(tp, 0);
            int codes[8];
            if (in_regs) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int t = b.tid + u * b.nt;
                    codes[u] = (t < num) ? perm_code(xs_raw + t * tau, D, fact) : -1;
                }
            }
            // log(c / num) of the small counts from a table (one float64 logarithm, ~150 instructions, per lane of ONE
            // evaluation instead of one per bin / window: for D >= 5 nearly every count is below the table's end)
            TSFA_TICK(tp, b, 236);
            const int LT = 64;
            double *ltab = own_np ? b.np->leaf_sum : w + (w_doubles - 64);  // (the numpy-order scratch is idle here)
            ar_sync(b);
            for (int c = b.tid; c < LT; c += b.nt) ltab[c] = (c > 0) ? log((double)c / (double)num) : 0.0;
            ar_sync(b);
            TSFA_TICK(tp, b, 237);
            double e = 0.0;
            for (int base = 0; base < fact; base += per_pass) {
                const int top = (fact - base < per_pass) ? (fact - base) : per_pass;  // patterns of this pass
                ar_sync(b);
                for (int k = b.tid; k < (wide ? top : (top + 1) >> 1); k += b.nt) iw[k] = 0;
                ar_sync(b);
                if (in_regs) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int c = codes[u] - base;
                        if (codes[u] >= 0 && c >= 0 && c < top) {
#if TSFA_GPU
                            if (wide) atomicAdd(&iw[c], 1); else atomicAdd(&iw[c >> 1], (c & 1) ? 0x10000 : 1);
#else
                            if (wide) iw[c] += 1; else iw[c >> 1] += (c & 1) ? 0x10000 : 1;
#endif
                        }
                    }
                } else {
                    for (int t = b.tid; t < num; t += b.nt) {
                        const int c = perm_code(xs_raw + t * tau, D, fact) - base;
                        if (c >= 0 && c < top) {
#if TSFA_GPU
                            if (wide) atomicAdd(&iw[c], 1); else atomicAdd(&iw[c >> 1], (c & 1) ? 0x10000 : 1);
#else
                            if (wide) iw[c] += 1; else iw[c >> 1] += (c & 1) ? 0x10000 : 1;
#endif
                        }
                    }
                }
                ar_sync(b);
                if (fact <= num) {  // sum over the patterns
                    for (int k = b.tid; k < top; k += b.nt) {
                        const unsigned wv = (unsigned)iw[wide ? k : (k >> 1)];
                        const int c = wide ? (int)wv : ((k & 1) ? (int)(wv >> 16) : (int)(wv & 0xffffu));
                        if (c > 0) {
                            const double pr = (double)c / (double)num;
                            e += pr * ((c < LT) ? ltab[c] : log(pr));
                        }
                    }
                } else {  // more patterns than windows: sum_k c_k log(c_k / num) = sum over windows of log(c(window) / num)
                    double acc = 0.0;
                    if (in_regs) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int c = codes[u] - base;
                            if (codes[u] >= 0 && c >= 0 && c < top) {
                                const unsigned wv = (unsigned)iw[wide ? c : (c >> 1)];
                                const int cc = wide ? (int)wv : ((c & 1) ? (int)(wv >> 16) : (int)(wv & 0xffffu));
                                acc += (cc < LT) ? ltab[cc] : log((double)cc / (double)num);
                            }
                        }
                    } else {
                        for (int t = b.tid; t < num; t += b.nt) {
                            const int c = perm_code(xs_raw + t * tau, D, fact) - base;
                            if (c >= 0 && c < top) {
                                const unsigned wv = (unsigned)iw[wide ? c : (c >> 1)];
                                const int cc = wide ? (int)wv : ((c & 1) ? (int)(wv >> 16) : (int)(wv & 0xffffu));
                                acc += (cc < LT) ? ltab[cc] : log((double)cc / (double)num);
                            }
                        }
                    }
                    e += acc / (double)num;
                }
            }
            TSFA_TICK(tp, b, 238);
            v = -blk_sum(b, e);
            TSFA_TICK(tp, b, 239);
        } break;
        case TSFA_C_FRIEDRICH_COEFFICIENTS:                              // fc.py:2082
        case TSFA_C_MAX_LANGEVIN_FIXED_POINT: {                          // fc.py:2134
            int coeff, m, r;
            if (sp.calc == TSFA_C_FRIEDRICH_COEFFICIENTS) { coeff = (int)p0; m = (int)p1; r = (int)p2; }
            else { coeff = -1; m = (int)p0; r = (int)p1; }
            if (!(fr_valid && fr_m == m && fr_r == r)) {
                // sorted x[:-1] = the sorted series with one occurrence of x[n-1] removed
                int pos = 0;
                {
                    const double xl = xs[n - 1];
                    int lo = 0, hi = n;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (srt[mid] < xl) lo = mid + 1; else hi = mid;
                    }
                    pos = lo;
                }
                const SV sr = srt;
                df.spec = s;
                friedrich_coeffs(b, xs, n, [=](int i) { return sr[i < pos ? i : i + 1]; }, m, r, w, fr_coef, df);
                fr_valid = true;
                fr_m = m;
                fr_r = r;
            }
            const double *coef = fr_coef;
            if (sp.calc == TSFA_C_FRIEDRICH_COEFFICIENTS) v = (coeff >= 0 && coeff <= m && m <= TSFA_FRIEDRICH_MAX_M) ? coef[coeff] : TSFA_NAN;
            else v = (m >= 1 && m <= TSFA_FRIEDRICH_MAX_M) ? max_real_root_deg3(coef, m + 1) : TSFA_NAN;
        } break;
        default: break;
        }
        if (b.tid == 0) out_row[sp.col] = v;
        TSFA_TICK(tk, b, sp.calc);
    }
    if (nloop < nspecs) {
        ar_sync(b);
        sort_epilogue(b, specs, nloop, nspecs, n, srt, ctx, cq, out_row);
    }
}

#endif
