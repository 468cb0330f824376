// The exact two-sample Kolmogorov-Smirnov tail of the feature selection as device code (tsfa_ks_tails and the ks_tail
// variants of tsfa_relevance_tails_*, include/tsfresh_amd.h): what rel_tails.h leaves to the caller as TSFA_ROUTE_HOST_KS.
//
// Restates significance_tests.py ks_2samp_pvalue for max(n1, n2) <= 10 000, in float64 and in the operation order of the
// Python text (-ffp-contract=off):
//   rk_plan        the route rule, g / lcm / h = rint(d * lcm), h == 0, and for n1 == n2 the Horner form: ONE LANE per cell
//   rk_ks_lattice  n1 != n2, tsfa_ks_outer_prob's lattice: ONE WAVEFRONT per cell, walked by anti-diagonals
// A value outside [0, 1] is not served: the cell keeps TSFA_ROUTE_HOST_KS and the caller falls through to kstwo, as the
// Python text does.  Beyond 10 000 rows (scipy's kstwo.sf) nothing is served here.
//
// The lattice.  With m >= n, mg = m / g, ng = n / g, row i of tsfa_ks_outer_prob holds the columns minj(i) <= j < maxj(i),
//   minj(i) = clip(floor((ng i - h) / mg) + 1, 0, n),   maxj(i) = min(ceil((ng i + h) / mg), n + 1),
// which is the set 0 <= j <= n with |j mg - i ng| < h (j > (ng i - h) / mg  <=>  j mg - i ng > -h; the clip at n never
// acts, since ng i - h < ng m = n mg).  A point is one expression of its upper and left neighbour,
//   A(i, j) = (A(i-1, j) * (double)i + A(i, j-1) * (double)j) / (double)(i + j),
// with 1.0 for a neighbour outside the band, 0.0 for the left neighbour of column 0, and A(0, j) = 0.0 inside the band;
// so every order that respects the two dependencies gives the host's value bit for bit.  Here the order is the
// anti-diagonal s = i + j: lane = column, in 64-column chunks ALIGNED to the column index, from high columns to low.  The
// latest value of every column lives in a ring of chunks (slot = chunk mod ring size, element = lane): a lane reads and
// writes only its own elements, the left neighbour comes by __shfl_up, and lane 0 takes lane 63 of the chunk below, which
// is loaded before it is overwritten.  No value is handed from lane to lane through memory, so the walk needs no fence and
// no barrier.  Whether a neighbour lies in the band is decided by the integer test above, never by what the ring holds: a
// stale or never-written element is loaded at most into a register that the test discards.
//
// Ring size.  The columns of diagonal s satisfy |j (mg + ng) - s ng| < h: at most F + 1 of them, F = floor(2 h / (mg + ng)),
// and the diagonals s - 1 and s together span at most F + 2 columns, i.e. at most (F + 1) / 64 + 2 aligned chunks.  Up to
// RK_LDS_CHUNKS chunks the ring is the wavefront's slice of LDS; beyond, a slice of HBM scratch of RK_HBM_CHUNKS chunks
// (n + 1 <= 10 001 columns need at most 158).  The scratch is sized by the wavefronts of the launch, not by the cells.
//
// Integers: under the 10 000-row rule lcm = mg n <= 1e8, so the per-lane products j mg, i ng and their sums with h fit
// int32; the per-diagonal bounds use int64.
//
// Compiled two ways like rel_tails.h (hipcc for gfx950; g++ -DTSFA_EMUL, tests/emul/emul_rel_ks.cpp, lanes looped).
#ifndef TSFA_REL_KS_H
#define TSFA_REL_KS_H

#include "rel_tails.h"

#define RK_MAX_ROWS 10000   // ks_2samp_pvalue: the exact tail serves max(n1, n2) <= 10 000
#define RK_LDS_CHUNKS 16    // 16 chunks of 64 doubles: 8 KB of LDS per wavefront
#define RK_HBM_CHUNKS 256   // 128 KB of scratch per wavefront

// what rk_plan found
enum { RK_LEAVE = 0,      // not served: the cell stays with the caller
       RK_VALUE = 1,      // *value holds the tail (h == 0, or the Horner form)
       RK_LATTICE = 2 };  // n1 != n2: rk_ks_lattice(n1, n2, *g, *h)

RT_HD int64_t rk_gcd(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

// chunks of ring the lattice of (m, n, g, h) needs
RT_HD int64_t rk_ring_chunks(int64_t m, int64_t n, int64_t g, int64_t h) { return ((2 * h) / (m / g + n / g) + 1) / 64 + 2; }

// ks_2samp_pvalue up to the lattice walk, one lane per cell
RT_HD int rk_plan(int64_t n1, int64_t n2, double d, int64_t *g_out, int64_t *h_out, double *value) {
    if (n1 < 1 || n2 < 1 || !(d >= 0.0 && d <= 1.0)) return RK_LEAVE;
    if (((n1 > n2) ? n1 : n2) > RK_MAX_ROWS) return RK_LEAVE;
    const int64_t g = rk_gcd(n1, n2);
    const int64_t lcm = (n1 / g) * n2;
    const int64_t h = (int64_t)rint(d * (double)lcm);   // int(round(d * lcm)): both round half to even
    *g_out = g;
    *h_out = h;
    if (h == 0) { *value = 1.0; return RK_VALUE; }
    if (n1 != n2) return RK_LATTICE;
    double prob = 0.0;
    for (int64_t k = n1 / h; k >= 0; --k) {  // Horner form of 2 * sum (-1)^(k-1) binom(2n, n - k h) / binom(2n, n)
        double p1 = 1.0;
        for (int64_t j = 0; j < h; ++j) p1 = (double)(n1 - k * h - j) * p1 / (double)(n1 + k * h + j + 1);
        prob = p1 * (1.0 - prob);
    }
    *value = 2.0 * prob;
    return RK_VALUE;
}

// `0.0 <= prob <= 1.0` of the Python text: only then is the value the cell's p
RT_HD int rk_in_range(double v) { return (v >= 0.0 && v <= 1.0) ? 1 : 0; }

// ---- wavefront operations ----
RT_DEV int rk_wave_any(const int *f) {
#if RT_GPU
    return __any(f[0]) ? 1 : 0;
#else
    int r = 0;
    for (int l = 0; l < 64; ++l) r |= f[l];
    return r ? 1 : 0;
#endif
}
// out of lane l = cur of lane l - 1; lane 0 receives lane 63 of `low`, the chunk below
RT_DEV void rk_shift_up(const double *cur, const double *low, double *out) {
#if RT_GPU
    const int lane = (int)(threadIdx.x & 63);
    const double a = __shfl_up(cur[0], 1, 64), b = __shfl(low[0], 63, 64);
    out[0] = lane ? a : b;
#else
    for (int l = 63; l > 0; --l) out[l] = cur[l - 1];
    out[0] = low[63];
#endif
}

// tsfa_ks_outer_prob(m, n, g, h), m != n, h >= 1, max(m, n) <= RK_MAX_ROWS; called by all 64 lanes of a wavefront with
// the same arguments, every lane returns the value.  ring: the wavefront's own ring_chunks * 64 doubles (LDS or HBM),
// ring_chunks a power of two >= rk_ring_chunks(m, n, g, h); its contents on entry do not matter.
RT_DEV double rk_ks_lattice(int64_t m, int64_t n, int64_t g, int64_t h, double *ring, int ring_chunks) {
    if (m < n) { const int64_t t = m; m = n; n = t; }
    const int64_t mg = m / g, ng = n / g, q = mg + ng;
    {   // an empty band at any row is the host function's early return; the limits are its integer formulas
        int empty[RT_NL];
        RT_LANES(l) {
            int e = 0;
            for (int64_t i = 1 + l; i <= m; i += 64) {
                const int64_t num = ng * i - h;
                int64_t fl = num / mg;
                if (num % mg != 0 && num < 0) --fl;
                int64_t minj = fl + 1;
                if (minj < 0) minj = 0;
                if (minj > n) minj = n;
                int64_t maxj = (ng * i + h + mg - 1) / mg;
                if (maxj > n + 1) maxj = n + 1;
                if (maxj <= minj) e = 1;
            }
            empty[RT_AT(l)] = e;
        }
        if (rk_wave_any(empty)) return 1.0;
    }
    const int64_t slot_mask = ring_chunks - 1;
    const int img = (int)mg, ing = (int)ng, ih = (int)h, in = (int)n, im = (int)m;
    double cur[RT_NL], low[RT_NL], left[RT_NL], val[RT_NL];
    RT_LANES(l) val[RT_AT(l)] = 0.0;
    // the columns of diagonal s: jlo <= j <= jhi with |j q - s ng| < h, then clipped to the lattice.  From s to s + 1 both
    // limits move by ng / q < 1, so each advances by at most one
    int64_t jlo = 1 - (h + q - 1) / q, jhi = (h - 1) / q;
    for (int64_t s = 0; s <= m + n; ++s) {
        if (s) {
            if ((jhi + 1) * q - s * ng < h) ++jhi;
            if (!(jlo * q - s * ng > -h)) ++jlo;
        }
        int64_t a = (jlo > s - m) ? jlo : s - m, b = (jhi < s) ? jhi : s;
        if (a < 0) a = 0;
        if (b > n) b = n;
        if (a > b) continue;
        const int64_t c_hi = b >> 6, c_lo = a >> 6;
        RT_LANES(l) cur[RT_AT(l)] = ring[(c_hi & slot_mask) * 64 + l];
        for (int64_t c = c_hi; c >= c_lo; --c) {
            RT_LANES(l) low[RT_AT(l)] = (c > 0) ? ring[((c - 1) & slot_mask) * 64 + l] : 0.0;
            rk_shift_up(cur, low, left);
            RT_LANES(l) {
                const int j = (int)(c * 64) + l, i = (int)s - j;
                const int t = j * img - i * ing;
                if (j <= in && i >= 0 && i <= im && t > -ih && t < ih) {
                    double v = 0.0;   // row 0
                    if (i > 0) {
                        const double up = (t + ing < ih) ? cur[RT_AT(l)] : 1.0;
                        const double lf = (j == 0) ? 0.0 : ((t - img > -ih) ? left[RT_AT(l)] : 1.0);
                        v = (up * (double)i + lf * (double)j) / (double)(i + j);
                    }
                    ring[(c & slot_mask) * 64 + l] = v;
                    val[RT_AT(l)] = v;
                }
                cur[RT_AT(l)] = low[RT_AT(l)];
            }
        }
    }
    return rt_wave_get(val, (int)(n & 63));   // the point (m, maxj(m) - 1) = (m, n), alone on the last diagonal
}

// ---- the cells ----
// Where the (n1, n2, d) of cell number `cell` are: the arrays of tsfa_ks_tails; or the class tables (cell = column *
// n_classes + class: class_n[class] against the rest, d = d[cell]); or the real table (cell = column: n_hi and ks_d of the
// sweep's record).
struct RkCells {
    const int64_t *n1, *n2;
    const double *d;
    const int64_t *class_n;
    int64_t n_rows;
    int32_t n_classes;
    const tsfa_relevance_real_col *rcols;
};
RT_HD void rk_cell_args(const RkCells &s, int64_t cell, int64_t *n1, int64_t *n2, double *d) {
    if (s.rcols) {
        *n1 = s.rcols[cell].n_hi;
        *n2 = s.n_rows - *n1;
        *d = s.rcols[cell].ks_d;
    } else if (s.class_n) {
        *n1 = s.class_n[cell % s.n_classes];
        *n2 = s.n_rows - *n1;
        *d = s.d[cell];
    } else {
        *n1 = s.n1[cell];
        *n2 = s.n2[cell];
        *d = s.d[cell];
    }
}

// what rk_closed_cell / rk_lattice_cell report
enum { RK_CELL_NONE = 0, RK_CELL_SERVED = 1, RK_CELL_LATTICE_LDS = 2, RK_CELL_LATTICE_HBM = 3 };

// one lane per cell: a TSFA_ROUTE_HOST_KS cell whose tail is a closed form gets its p and TSFA_ROUTE_KS_EXACT; a lattice
// cell is reported with the storage its ring needs and left to rk_lattice_cell
RT_HD int rk_closed_cell(const RkCells &s, int64_t cell, double *p, unsigned char *route) {
    if (route[cell] != TSFA_ROUTE_HOST_KS) return RK_CELL_NONE;
    int64_t n1, n2, g = 1, h = 0;
    double d, v = RT_NAN;
    rk_cell_args(s, cell, &n1, &n2, &d);
    const int what = rk_plan(n1, n2, d, &g, &h, &v);
    if (what == RK_LATTICE) return (rk_ring_chunks(n1, n2, g, h) <= RK_LDS_CHUNKS) ? RK_CELL_LATTICE_LDS : RK_CELL_LATTICE_HBM;
    if (what != RK_VALUE || !rk_in_range(v)) return RK_CELL_NONE;
    p[cell] = v;
    route[cell] = TSFA_ROUTE_KS_EXACT;
    return RK_CELL_SERVED;
}

// one wavefront per cell: the lattice cells among the TSFA_ROUTE_HOST_KS cells.  lds: the wavefront's RK_LDS_CHUNKS * 64
// doubles; hbm: its RK_HBM_CHUNKS * 64 doubles of scratch, or null when rk_closed_cell reported no cell that needs them
// (such a cell would then stay with the caller).
RT_DEV int rk_lattice_cell(const RkCells &s, int64_t cell, double *lds, double *hbm, double *p, unsigned char *route) {
    if (route[cell] != TSFA_ROUTE_HOST_KS) return RK_CELL_NONE;
    int64_t n1, n2, g = 1, h = 0;
    double d, v = RT_NAN;
    rk_cell_args(s, cell, &n1, &n2, &d);
    if (n1 == n2 || rk_plan(n1, n2, d, &g, &h, &v) != RK_LATTICE) return RK_CELL_NONE;
    const int in_lds = rk_ring_chunks(n1, n2, g, h) <= RK_LDS_CHUNKS;
    if (!in_lds && !hbm) return RK_CELL_NONE;
    // (two calls, so that each inlined copy knows its address space)
    v = in_lds ? rk_ks_lattice(n1, n2, g, h, lds, RK_LDS_CHUNKS) : rk_ks_lattice(n1, n2, g, h, hbm, RK_HBM_CHUNKS);
    if (!rk_in_range(v)) return RK_CELL_NONE;
#if RT_GPU
    if ((threadIdx.x & 63) != 0) return RK_CELL_SERVED;
#endif
    p[cell] = v;
    route[cell] = TSFA_ROUTE_KS_EXACT;
    return RK_CELL_SERVED;
}

#endif
