// The exact Mann-Whitney tail of the feature selection as device code (tsfa_mwu_tails and mwu_tail of
// tsfa_relevance_tails_classes, include/tsfresh_amd.h): what rel_tails.h leaves to the caller as TSFA_ROUTE_HOST_MWU_EXACT.
//
// Restates significance_tests.py mannwhitney_pvalue's exact branch, 2 * _mwu_exact_sf(int(u), n1, n2), in exact integers.
// With m = min(n1, n2) <= 8, n = max(n1, n2), top = m n: c_j, the number of arrangements with statistic j, is the coefficient of
// q^j in the Gaussian binomial [n + m choose m]_q = prod_{i = 1..m} (1 - q^(n + i)) / (1 - q^i), and the tail is S_k / total,
// S_k = sum_{j >= k} c_j, total = S_0 = C(n + m, m), k = clamp(int(u), 0, top + 1).  The coefficients depend on (m, n) alone,
// so they are built ONCE PER TABLE (a class of a classification) and a cell is a lookup and one division:
//   rm_build   ONE WORKGROUP per distinct (m, n), through all 2 m passes and the last sum
//   rm_cell    ONE LANE per cell: S_k and total from the table, long division to the correctly rounded float64
//
// Integers.  A count is RM_LIMBS 64-bit limbs, little-endian, modulo 2^(64 RM_LIMBS): the coefficients between a multiply and
// a divide step are negative, and two's complement carries them exactly, since every finished polynomial has coefficients in
// [0, total].  The limb count follows from the cap TSFA_MWU_EXACT_MAX_TOP on top (rm_total_bits, pinned below).
//
// Layout.  A polynomial of len = top + 1 coefficients is LIMB-PLANAR: limb l of coefficient d at l * len + d, so the lanes
// of an element-wise pass read consecutive 8-byte words.  Two such buffers ping-pong: the multiply pass
// c'[d] = c[d] - c[d - a] reads a snapshot (element-wise, buffer 0 -> 1), the divide pass c'[d] = c[d] + c'[d - i] is i
// independent inclusive prefix sums of stride i (buffer 1 -> 0).  Both buffers live in LDS while len <= RM_LDS_ELEMS, else in a
// block of HBM scratch that the launch sizes.
//
// The divide pass is a three-phase workgroup scan per residue r = d mod i: thread t owns the coefficients
// [t * chunk, (t + 1) * chunk), chunk a multiple of i, and (1) adds up its coefficients of residue r, (2) the RM_NT sums are
// scanned in LDS (Hillis-Steele, two rows that ping-pong), (3) it walks its block again, starting from the sum of the threads
// before it, and writes the running sum.  The residues go one after the other: the scan rows of one residue are 2 * RM_NT counts
// (24 KB), those of 8 residues would not fit beside the buffers.
//
// The tail.  The Gaussian binomial is palindromic, c_j = c_(top - j), so S_k = sum_{j <= top - k} c_j: the table that rm_build
// leaves in HBM is the PREFIX sum P (one more divide pass with i = 1, straight into the table), S_k = P[top - k], total = P[top].
// No reversed scan is needed.
//
// Compiled two ways like rel_tails.h (hipcc for gfx950; g++ -DTSFA_EMUL, tests/emul/emul_rel_mwu.cpp): in the emulation the
// threads of a phase are looped, and a phase ends where the GPU has its barrier.
#ifndef TSFA_REL_MWU_H
#define TSFA_REL_MWU_H

#include "rel_tails.h"

#define RM_MAX_M 8          // scipy's method="auto": the exact distribution when a sample has at most 8 members
#define RM_LIMBS 3
#define RM_NT 512           // threads of the build workgroup: 8 wavefronts, so its barrier waits for the global stores too
#define RM_LDS_ELEMS 2560   // both buffers in LDS up to this many coefficients: 2 * 2560 * 8 * RM_LIMBS = 120 KB
#define RM_SCAN_WORDS (2 * RM_LIMBS * RM_NT)   // the two rows of the scan of the thread sums, limb-planar: 24 KB

// bits of total = C(n + m, m) <= (n + m)^m / m! over every table under the cap: m * ceil(log2(n + m)) - floor(log2(m!))
constexpr int rm_ceil_log2(int64_t v) {
    int b = 0;
    while (((int64_t)1 << b) < v) ++b;
    return b;
}
constexpr int rm_total_bits() {
    int worst = 0;
    int64_t fact = 1;
    for (int m = 1; m <= RM_MAX_M; ++m) {
        fact *= m;
        const int floor_log2_fact = rm_ceil_log2(fact + 1) - 1;
        const int bits = m * rm_ceil_log2(TSFA_MWU_EXACT_MAX_TOP / m + m) - floor_log2_fact;
        worst = bits > worst ? bits : worst;
    }
    return worst;
}
// every count fits, and so does twice a count (the remainder of the long division, shifted)
static_assert(rm_total_bits() + 1 <= 64 * RM_LIMBS && rm_total_bits() + 1 > 64 * (RM_LIMBS - 1), "limbs of an exact Mann-Whitney count");
static_assert(2 * RM_LDS_ELEMS * 8 * RM_LIMBS + RM_SCAN_WORDS * 8 <= 160 * 1024, "LDS of the build workgroup");

struct RmInt { uint64_t w[RM_LIMBS]; };

RT_HD RmInt rm_zero() {
    RmInt z;
    for (int l = 0; l < RM_LIMBS; ++l) z.w[l] = 0;
    return z;
}
RT_HD RmInt rm_add(RmInt a, const RmInt &b) {
    uint64_t carry = 0;
    for (int l = 0; l < RM_LIMBS; ++l) {
        const uint64_t s = a.w[l] + b.w[l], s2 = s + carry;
        carry = (uint64_t)(s < b.w[l]) | (uint64_t)(s2 < s);
        a.w[l] = s2;
    }
    return a;
}
RT_HD RmInt rm_sub(RmInt a, const RmInt &b) {
    uint64_t borrow = 0;
    for (int l = 0; l < RM_LIMBS; ++l) {
        const uint64_t d = a.w[l] - b.w[l], d2 = d - borrow;
        borrow = (uint64_t)(a.w[l] < b.w[l]) | (uint64_t)(d < borrow);
        a.w[l] = d2;
    }
    return a;
}
RT_HD int rm_ge(const RmInt &a, const RmInt &b) {
    for (int l = RM_LIMBS - 1; l >= 0; --l)
        if (a.w[l] != b.w[l]) return a.w[l] > b.w[l];
    return 1;
}
RT_HD RmInt rm_shl1(RmInt a) {
    for (int l = RM_LIMBS - 1; l > 0; --l) a.w[l] = (a.w[l] << 1) | (a.w[l - 1] >> 63);
    a.w[0] <<= 1;
    return a;
}
RT_HD int rm_is_zero(const RmInt &a) {
    uint64_t any = 0;
    for (int l = 0; l < RM_LIMBS; ++l) any |= a.w[l];
    return any == 0;
}
// limb-planar element d of a buffer whose planes are `stride` words apart
RT_HD RmInt rm_load(const uint64_t *buf, int64_t stride, int64_t d) {
    RmInt v;
    for (int l = 0; l < RM_LIMBS; ++l) v.w[l] = buf[(int64_t)l * stride + d];
    return v;
}
RT_HD void rm_store(uint64_t *buf, int64_t stride, int64_t d, const RmInt &v) {
    for (int l = 0; l < RM_LIMBS; ++l) buf[(int64_t)l * stride + d] = v.w[l];
}

// ---- the serve rule ----
RT_HD int rm_served(int64_t n1, int64_t n2) {
    const int64_t m = (n1 < n2) ? n1 : n2, n = (n1 < n2) ? n2 : n1;
    return (m >= 1 && m <= RM_MAX_M && n <= TSFA_MWU_EXACT_MAX_TOP && m * n <= TSFA_MWU_EXACT_MAX_TOP) ? 1 : 0;
}
RT_HD int64_t rm_table_words(int64_t m, int64_t n) { return (int64_t)RM_LIMBS * (m * n + 1); }
RT_HD int rm_in_lds(int64_t m, int64_t n) { return (m * n + 1 <= RM_LDS_ELEMS) ? 1 : 0; }

// ---- the phases of rm_build: what thread t of RM_NT does between two barriers ----
RT_HD void rm_phase_init(int t, uint64_t *buf, int64_t len) {
    for (int64_t d = t; d < len; d += RM_NT)
        for (int l = 0; l < RM_LIMBS; ++l) buf[(int64_t)l * len + d] = (d == 0 && l == 0) ? 1u : 0u;
}
// times (1 - q^a): element-wise from a snapshot
RT_HD void rm_phase_mul(int t, const uint64_t *src, uint64_t *dst, int64_t len, int64_t a) {
    for (int64_t d = t; d < len; d += RM_NT) {
        RmInt v = rm_load(src, len, d);
        if (d >= a) v = rm_sub(v, rm_load(src, len, d - a));
        rm_store(dst, len, d, v);
    }
}
// the coefficients thread t owns in a divide pass by (1 - q^i): chunk is a multiple of i, so residue r starts at t * chunk + r
RT_HD int64_t rm_chunk(int64_t len, int64_t i) { return ((len + RM_NT - 1) / RM_NT + i - 1) / i * i; }
RT_HD void rm_phase_sum(int t, const uint64_t *src, int64_t len, int64_t i, int64_t r, uint64_t *row) {
    const int64_t chunk = rm_chunk(len, i), d0 = (int64_t)t * chunk, d1 = (d0 + chunk < len) ? d0 + chunk : len;
    RmInt acc = rm_zero();
    for (int64_t d = d0 + r; d < d1; d += i) acc = rm_add(acc, rm_load(src, len, d));
    rm_store(row, RM_NT, t, acc);
}
// one Hillis-Steele step over the RM_NT thread sums, from one row into the other
RT_HD void rm_phase_scan(int t, const uint64_t *in, uint64_t *out, int s) {
    RmInt v = rm_load(in, RM_NT, t);
    if (t >= s) v = rm_add(v, rm_load(in, RM_NT, t - s));
    rm_store(out, RM_NT, t, v);
}
// the running sums of residue r in thread t's block, from the inclusive scan of the thread sums
RT_HD void rm_phase_apply(int t, const uint64_t *src, uint64_t *dst, int64_t len, int64_t i, int64_t r, const uint64_t *incl) {
    const int64_t chunk = rm_chunk(len, i), d0 = (int64_t)t * chunk, d1 = (d0 + chunk < len) ? d0 + chunk : len;
    RmInt acc = (t > 0) ? rm_load(incl, RM_NT, t - 1) : rm_zero();
    for (int64_t d = d0 + r; d < d1; d += i) {
        acc = rm_add(acc, rm_load(src, len, d));
        rm_store(dst, len, d, acc);
    }
}

// a phase: every thread of the workgroup runs the body, then all meet.  (An 8-wavefront workgroup: the barrier carries the
// wait for the global stores of the scratch form)
#if RT_GPU
#define RM_PHASE(t) for (int t = (int)threadIdx.x, rm_go_ = 1; rm_go_; rm_go_ = 0, __syncthreads())
#else
#define RM_PHASE(t) for (int t = 0; t < RM_NT; ++t)
#endif

// divided by (1 - q^i): dst[d] = src[d] + dst[d - i].  src and dst hold len coefficients each and are different buffers.
RT_DEV void rm_divide(const uint64_t *src, uint64_t *dst, int64_t len, int64_t i, uint64_t *scan) {
    uint64_t *row0 = scan, *row1 = scan + RM_LIMBS * RM_NT;
    for (int64_t r = 0; r < i; ++r) {
        RM_PHASE(t) rm_phase_sum(t, src, len, i, r, row0);
        uint64_t *in = row0, *out = row1;
        for (int s = 1; s < RM_NT; s <<= 1) {
            RM_PHASE(t) rm_phase_scan(t, in, out, s);
            uint64_t *x = in; in = out; out = x;
        }
        RM_PHASE(t) rm_phase_apply(t, src, dst, len, i, r, in);
    }
}

// The prefix sums P[0 .. m n] of the coefficients of [n + m choose m]_q into table (limb-planar, m n + 1 coefficients); buf0 and
// buf1 hold as much each (LDS or scratch), scan RM_SCAN_WORDS words of LDS.  Called by all RM_NT threads of a workgroup with
// the same arguments; m <= n, rm_served(m, n).
RT_DEV void rm_build(int64_t m, int64_t n, uint64_t *buf0, uint64_t *buf1, uint64_t *scan, uint64_t *table) {
    const int64_t len = m * n + 1;
    RM_PHASE(t) rm_phase_init(t, buf0, len);
    for (int64_t i = 1; i <= m; ++i) {
        RM_PHASE(t) rm_phase_mul(t, buf0, buf1, len, n + i);
        rm_divide(buf1, buf0, len, i, scan);
    }
    rm_divide(buf0, table, len, 1, scan);
}

// ---- the cells ----
// num / den, 0 < num <= den, as the correctly rounded float64 (ties to even: Python's int / int): long division to a 55-bit
// quotient and a sticky bit, by shifts and subtractions on the limbs
RT_HD double rm_ratio(const RmInt &num, const RmInt &den) {
    RmInt rem = num;
    int e = 0;
    // den <= rem < 2 den: num / den = (rem / den) * 2^-e, in [1, 2) * 2^-e.  (The bound on e only ends the loop for a num of 0,
    // which no table holds.)
    while (e < 64 * RM_LIMBS && !rm_ge(rem, den)) { rem = rm_shl1(rem); ++e; }
    uint64_t q = 0;
    for (int b = 0; b < 55; ++b) {
        q <<= 1;
        if (rm_ge(rem, den)) { rem = rm_sub(rem, den); q |= 1u; }
        rem = rm_shl1(rem);
    }
    // q = floor(rem / den * 2^54), 2^54 <= q < 2^55; two bits go: the half bit, and the rest with the remainder
    const uint64_t half = (q >> 1) & 1u, rest = (q & 1u) | (uint64_t)(rm_is_zero(rem) ? 0 : 1);
    uint64_t mant = q >> 2;
    mant += half & (rest | (mant & 1u));
    return ldexp((double)mant, -e - 52);   // mant <= 2^53: exact
}

// a caller's table: its sample sizes, and where its P starts in the block of tables (words), -1 when the table is not served
struct RmTable { int64_t n1, n2, off; };

// where the cells come from: a stand-alone list (tsfa_mwu_tails: table[cell], u[cell]), or the class tables of a sweep
// (table = cell mod n_classes; u from the rank sum as mannwhitney_pvalue takes it)
struct RmCells {
    const int32_t *table;
    const double *u;
    const double *rank_sums;
    const int64_t *class_n;
    int64_t n_rows;
    int32_t n_classes;
};

// one lane per cell -> 1 when the cell was served (p and TSFA_ROUTE_MWU_EXACT written), else nothing is written
RT_HD int rm_cell(const RmCells &s, const RmTable *tables, int32_t n_tables, const uint64_t *tabs, int64_t cell, double *p,
                  unsigned char *route) {
    if (route[cell] != TSFA_ROUTE_HOST_MWU_EXACT) return 0;
    int64_t t;
    double u;
    if (s.table) {
        t = s.table[cell];
        u = s.u[cell];
    } else {
        t = cell % s.n_classes;
        const int64_t n1 = s.class_n[t], n2 = s.n_rows - n1;
        const double u1 = s.rank_sums[cell] - (double)(n1 * (n1 + 1)) / 2.0;
        const double u2 = (double)(n1 * n2) - u1;
        u = (u1 > u2) ? u1 : u2;
    }
    if (t < 0 || t >= n_tables || !(u == u)) return 0;
    const RmTable tb = tables[t];
    if (tb.off < 0) return 0;
    const int64_t top = tb.n1 * tb.n2;
    // k = max(0, min(int(u), top + 1)); int() truncates towards zero
    const int64_t k = (u < 1.0) ? 0 : ((u >= (double)(top + 1)) ? top + 1 : (int64_t)u);
    double v = 0.0;
    if (k <= top) {
        const uint64_t *P = tabs + tb.off;
        v = 2.0 * rm_ratio(rm_load(P, top + 1, top - k), rm_load(P, top + 1, top));
        v = (v < 0.0) ? 0.0 : ((v > 1.0) ? 1.0 : v);
    }
    p[cell] = v;
    route[cell] = TSFA_ROUTE_MWU_EXACT;
    return 1;
}

#endif
