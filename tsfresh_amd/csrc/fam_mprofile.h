// matrix_profile with an explicit window (fc.py:2385-2470, the route `mp.compute(x, windows=w)["mp"]`): the exact
// z-normalised self-join matrix profile of Yeh et al. (2016), one workgroup per series (k_mprofile, TSFA_FAM_MPROFILE).
//
// Definition.  For a series x of n samples and a window w let L = n - w + 1; mu_i and sigma_i are the mean and the
// population standard deviation of window i = x[i .. i + w).
//   rho(i, j) = sum_k (x[i+k] - mu_i)(x[j+k] - mu_j) / (w sigma_i sigma_j), clamped to <= 1
//   P[i]      = sqrt(2 w (1 - max_j rho(i, j))),  the maximum over the admissible j: |i - j| > ceil(w / 4)
// (the exclusion zone of the matrixprofile package: its diagonals start at ceil(w / 4) + 1).  A FLAT window -- all samples
// equal, max == min -- has no z-normalisation: its P[i] is non-finite and it is nobody's neighbour.  The reference drops the
// non-finite entries (fc.py:2455) and takes min / max / mean / median / 25 / 75 (np.percentile, linear) of the rest.
// Choices where the package's behaviour is unknown: L <= ceil(w / 4) + 1 (no admissible pair; w > n included) -> NaN, and
// no finite entry -> NaN.
//
// The kernel, per distinct w of the plan (the host sorts the family's columns by w: tsfa_prepare_family):
//   1. prologue  mu_i, inv_i = 1 / sqrt(sum_k (x[i+k] - mu_i)^2) (NaN for a flat window) -- each window summed directly in
//                a fixed order, O(w) per window: sliding sums of x and x^2 cancel where a window's spread is small against
//                its level, and the error would reach rho unchecked; then df[i] = (x[i+w] - x[i]) / 2 and
//                dg[i] = (x[i+w] - mu_{i+1}) + (x[i] - mu_i), the difference arrays of the diagonal recurrence
//                cov(i+1, j+1) = cov(i, j) + df[i] dg[j] + df[j] dg[i].
//   2. sweep     the diagonals d = ceil(w/4)+1 .. L-1, 64 neighbours to a wavefront, lane = diagonal.  The lanes of a
//                wavefront share the row i: the row side of the maximum is reduced across the wavefront (DPP) and written
//                by one lane, the column side (j = i + d: consecutive addresses) by every lane -- both as integer maxima on
//                order-preserving 64-bit keys, so the result does not depend on who arrives first.
//                BOUNDED DRIFT: the covariance of a diagonal is recomputed directly (O(w)) at every row that is a multiple of
//                TSFA_MP_RESTART, a compile-time constant; between two restarts it takes at most TSFA_MP_RESTART - 1 updates,
//                so the error of rho does not grow with n.
//   3. epilogue  keys -> distances, the mean as a fixed-order sum (np_sum) over the window index, the finite entries sorted
//                by the sort family's in-place bitonic network (non-finite ones as +inf behind them), six statistics.
// BATCH INDEPENDENCE: the value of a cell depends on (i, j) and the restart rows only, the maxima are order-free, the sum
// and the sort are fixed: a series gives the same bits whatever the batch, the length class, the workgroup size, and
// whether the working set lies in LDS or in the long-series build's HBM slot.
//
// The same body compiles single-threaded under g++ (tests/emul/emul_mprofile.cpp).
#ifndef TSFA_FAM_MPROFILE_H
#define TSFA_FAM_MPROFILE_H

#include "tsfa_common.h"

#define TSFA_MP_RESTART 256   // rows between two direct recomputations of a diagonal's covariance
#define TSFA_MP_MIN_W 4       // smallest window served (tsfa_validate_spec)
enum { TSFA_MP_MIN = 0, TSFA_MP_MAX = 1, TSFA_MP_MEAN = 2, TSFA_MP_MEDIAN = 3, TSFA_MP_P25 = 4, TSFA_MP_P75 = 5 };

typedef unsigned long long mp_key_t;

TSFA_DEV int mp_excl(int w) { return (w + 3) / 4; }   // ceil(w / 4)

// order-preserving image of a double (0: no neighbour yet -- below the image of every double)
TSFA_DEV mp_key_t mp_enc(double r) {
    union { double d; mp_key_t u; } a;
    a.d = r;
    return (a.u >> 63) ? ~a.u : (a.u | 0x8000000000000000ull);
}
TSFA_DEV double mp_dec(mp_key_t k) {
    union { double d; mp_key_t u; } a;
    a.u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return a.d;
}
TSFA_DEV void mp_key_max(mp_key_t *p, mp_key_t v) {
#if TSFA_GPU
    (void)atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}

// (the long-series build keeps the keys in HBM, where the maxima are formed in L2: the read must not be served by a line
//  the CU's vector cache kept from an earlier series)
TSFA_DEV mp_key_t mp_key_load(const mp_key_t *p) {
#if TSFA_GPU
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}

// the working set of one series; every array holds maxn entries (tsfa_layout.h: MpLds)
struct MpWork {
    double *mu, *inv, *df, *dg;   // df | dg are contiguous: the epilogue sorts the distances in their storage
    mp_key_t *key;
};

template <class XV>
TSFA_DEV double mp_cov_direct(const XV &x, int i, int j, int w, double mi, double mj) {
    double c = 0.0;
    for (int k = 0; k < w; ++k) c += (x[i + k] - mi) * (x[j + k] - mj);
    return c;
}

template <class XV>
TSFA_DEV void mp_prologue(const Blk &b, const XV &x, int n, int w, const MpWork &W) {
    const int L = n - w + 1;
    for (int i = b.tid; i < L; i += b.nt) {
        const double x0 = x[i];
        double s = 0.0;
        bool flat = true;
        for (int k = 0; k < w; ++k) {
            const double v = x[i + k];
            s += v;
            flat = flat && (v == x0);
        }
        const double m = s / (double)w;
        double q = 0.0;
        for (int k = 0; k < w; ++k) {
            const double d = x[i + k] - m;
            q += d * d;
        }
        W.mu[i] = m;
        W.inv[i] = (flat || !(q > 0.0) || !(q < TSFA_INF)) ? TSFA_NAN : 1.0 / sqrt(q);
        W.key[i] = 0ull;
    }
    blk_sync();
    for (int i = b.tid; i < L; i += b.nt) {
        const bool in = i + 1 < L;   // (the last window has no successor: its differences are never used in a result)
        W.df[i] = in ? (x[i + w] - x[i]) / 2.0 : 0.0;
        W.dg[i] = in ? (x[i + w] - W.mu[i + 1]) + (x[i] - W.mu[i]) : 0.0;
    }
    blk_sync();
}

template <class XV>
TSFA_DEV void mp_sweep(const Blk &b, const XV &x, int n, int w, const MpWork &W) {
    const int L = n - w + 1;
    const int dmin = mp_excl(w) + 1;
    if (L <= dmin) return;
#if TSFA_GPU
    const int lanes = 64, lane = b.tid & 63, wv = b.tid >> 6, nw = b.nt >> 6;
#else
    const int lanes = 1, lane = 0, wv = 0, nw = 1;
#endif
    const int ngroups = (L - dmin + lanes - 1) / lanes;
    // groups of `lanes` neighbouring diagonals, dealt to the wavefronts back and forth (a group's work falls with d)
    for (int r = 0; r * nw < ngroups; ++r) {
        const int g = r * nw + ((r & 1) ? nw - 1 - wv : wv);
        if (g >= ngroups) continue;
        const int d0 = dmin + g * lanes;
        const int d = d0 + lane;
        const int rows = L - d0;   // of the group's longest diagonal
        for (int i0 = 0; i0 < rows; i0 += TSFA_MP_RESTART) {
            const int i1 = (i0 + TSFA_MP_RESTART < rows) ? i0 + TSFA_MP_RESTART : rows;
            double c = 0.0;
            if (i0 + d < L) c = mp_cov_direct(x, i0, i0 + d, w, W.mu[i0], W.mu[i0 + d]);
            for (int i = i0; i < i1; ++i) {
                const int j = i + d;
                double rho = -TSFA_INF;
                if (j < L) {
                    const double dfi = W.df[i], dgi = W.dg[i], dfj = W.df[j], dgj = W.dg[j];
                    double v = c * W.inv[i] * W.inv[j];
                    c = c + dfi * dgj + dfj * dgi;
                    if (v > 1.0) v = 1.0;
                    if (v == v) {   // (a flat window's inverse norm is NaN: no neighbour, nobody's neighbour)
                        rho = v;
                        mp_key_max(&W.key[j], mp_enc(v));
                    }
                }
#if TSFA_GPU
                const double rmax = wave_max(rho);
                if (lane == 0 && rmax > -TSFA_INF) mp_key_max(&W.key[i], mp_enc(rmax));
#else
                if (rho > -TSFA_INF) mp_key_max(&W.key[i], mp_enc(rho));
#endif
            }
        }
    }
    blk_sync();
}

// np.percentile(a, 100 q) of the sorted a[0 .. m), method "linear" (numpy/lib/_function_base_impl.py: _lerp)
TSFA_DEV double mp_percentile(const double *a, int m, double q) {
    const double vi = (double)m * q + (1.0 + q * -1.0) - 1.0;
    int lo = (int)floor(vi);
    if (lo < 0) lo = 0;
    if (lo > m - 1) lo = m - 1;
    const int hi = (lo + 1 < m) ? lo + 1 : m - 1;
    const double t = vi - (double)lo, lo_v = a[lo], hi_v = a[hi];
    const double diff = hi_v - lo_v;
    return (t >= 0.5) ? hi_v - diff * (1.0 - t) : lo_v + diff * t;
}

// every matrix_profile column of a plan for one series.  specs: sorted by window (p0); p1: TSFA_MP_*.
template <class XV>
TSFA_DEV void fam_mprofile_series(const Blk &b, const XV &x, int n, const TsfaSpec *specs, int nspecs, double *out_row,
                                  const MpWork &W) {
    int cur_w = -1, m = 0;
    double mean = TSFA_NAN;
    double *srt = W.df;   // df | dg: 2 maxn doubles >= the power of two above L
    for (int s = 0; s < nspecs; ++s) {
        const TsfaSpec sp = specs[s];
        const int w = (int)sp.p[0];
        if (w != cur_w) {
            cur_w = w;
            m = 0;
            mean = TSFA_NAN;
            const int L = n - w + 1;
            blk_sync();
            if (w >= TSFA_MP_MIN_W && L > mp_excl(w) + 1) {
                mp_prologue(b, x, n, w, W);
                mp_sweep(b, x, n, w, W);
                // distances: sorted in df | dg's storage (non-finite ones as +inf behind the others); mu is dead and holds
                // them by window (non-finite: 0) for the fixed-order sum
                const double w2 = 2.0 * (double)w;
                const int np2 = next_pow2(L);
                double cnt = 0.0;
                for (int i = b.tid; i < np2; i += b.nt) {
                    const mp_key_t k = (i < L) ? mp_key_load(&W.key[i]) : 0ull;
                    const double p = k ? sqrt(w2 * (1.0 - mp_dec(k))) : TSFA_INF;
                    const bool fin = p < TSFA_INF;   // (false for NaN too)
                    srt[i] = fin ? p : TSFA_INF;
                    if (i < L) W.mu[i] = fin ? p : 0.0;
                    cnt += fin ? 1.0 : 0.0;
                }
                m = (int)blk_sum(b, cnt);
                blk_sync();
                const double *pm = W.mu;
                const double total = np_sum(b, L, [=](int i) { return pm[i]; });
                blk_bitonic_sort(b, srt, np2);
                if (m > 0) mean = total / (double)m;
            }
        }
        double v = TSFA_NAN;
        if (m > 0) {
            switch ((int)sp.p[1]) {
            case TSFA_MP_MIN: v = srt[0]; break;
            case TSFA_MP_MAX: v = srt[m - 1]; break;
            case TSFA_MP_MEAN: v = mean; break;
            case TSFA_MP_MEDIAN: v = (m & 1) ? srt[m / 2] : (srt[m / 2 - 1] + srt[m / 2]) / 2.0; break;
            case TSFA_MP_P25: v = mp_percentile(srt, m, 0.25); break;
            case TSFA_MP_P75: v = mp_percentile(srt, m, 0.75); break;
            default: break;
            }
        }
        if (b.tid == 0) out_row[sp.col] = v;
    }
}

#endif
