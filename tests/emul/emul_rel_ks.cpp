// TEST INFRASTRUCTURE ONLY: the exact Kolmogorov-Smirnov tail of tsfresh_amd/csrc/tsfa_relevance.hip without the device.
// The bodies live in tsfresh_amd/csrc/rel_ks.h and are compiled here by g++ -DTSFA_EMUL: the 64 lanes of a wavefront are
// looped (a per-lane value is an array of 64; the shift by one lane is a copy), the two kernels are loops over the cells, and
// the rings are heap blocks of EXACTLY the sizes the driver gives a wavefront (RK_LDS_CHUNKS * 64 doubles of LDS,
// RK_HBM_CHUNKS * 64 of scratch), allocated per call, so that a step outside a ring is AddressSanitizer's to find.
// The product never loads this; tests/test_select_ks_emul.py compares it with the row walk and with scipy.
// With -DRK_EMUL_MAIN the file is a stand-alone program: the form an AddressSanitizer / UBSan run of the bodies takes.
#include <stdint.h>

#include <vector>

#include "../../tsfresh_amd/csrc/rel_ks.h"

extern "C" int64_t tsfa_emul_ks_ring_chunks(int64_t m, int64_t n, int64_t g, int64_t h) { return rk_ring_chunks(m, n, g, h); }
extern "C" int32_t tsfa_emul_ks_lds_chunks() { return RK_LDS_CHUNKS; }

// rk_ks_lattice on the ring the driver would choose (storage 0), on the LDS-sized ring (1) or on the scratch-sized one (2).
// The ring starts out as NaN: a value taken from an element that was never written would show in the result.
extern "C" double tsfa_emul_ks_lattice(int64_t m, int64_t n, int64_t g, int64_t h, int32_t storage) {
    const int64_t need = rk_ring_chunks(m, n, g, h);
    const int chunks = (storage == 1 || (storage == 0 && need <= RK_LDS_CHUNKS)) ? RK_LDS_CHUNKS : RK_HBM_CHUNKS;
    if (need > chunks) return -1.0;
    std::vector<double> ring((size_t)chunks * 64, RT_NAN);
    return rk_ks_lattice(m, n, g, h, ring.data(), chunks);
}

// the two kernels over the cells of a table whose route bytes rel_tails.h has written -> the cells served.
// class tables: class_n, n_rows, n_classes, d = ks_d [n_cells]; real table: rcols, n_rows; stand-alone: n1, n2, d.
extern "C" int64_t tsfa_emul_ks_stage(const int64_t *n1, const int64_t *n2, const double *d, const int64_t *class_n, int64_t n_rows,
                                      int32_t n_classes, const tsfa_relevance_real_col *rcols, int64_t n_cells, double *p,
                                      unsigned char *route) {
    RkCells s;
    s.n1 = n1; s.n2 = n2; s.d = d; s.class_n = class_n; s.n_rows = n_rows; s.n_classes = n_classes; s.rcols = rcols;
    int64_t served = 0;
    bool need_hbm = false;
    for (int64_t cell = 0; cell < n_cells; ++cell) {
        const int r = rk_closed_cell(s, cell, p, route);
        served += (r == RK_CELL_SERVED) ? 1 : 0;
        need_hbm = need_hbm || r == RK_CELL_LATTICE_HBM;
    }
    std::vector<double> lds((size_t)RK_LDS_CHUNKS * 64, RT_NAN), hbm;
    if (need_hbm) hbm.assign((size_t)RK_HBM_CHUNKS * 64, RT_NAN);
    for (int64_t cell = 0; cell < n_cells; ++cell)
        served += (rk_lattice_cell(s, cell, lds.data(), need_hbm ? hbm.data() : nullptr, p, route) == RK_CELL_SERVED) ? 1 : 0;
    return served;
}

// tsfa_ks_tails: every cell starts as TSFA_ROUTE_HOST_KS with p = NaN -> the cells left to the caller
extern "C" int64_t tsfa_emul_ks_tails(const int64_t *n1, const int64_t *n2, const double *d, int64_t n_cells, double *p,
                                      unsigned char *route) {
    for (int64_t c = 0; c < n_cells; ++c) { p[c] = RT_NAN; route[c] = TSFA_ROUTE_HOST_KS; }
    return n_cells - tsfa_emul_ks_stage(n1, n2, d, nullptr, 0, 0, nullptr, n_cells, p, route);
}

#ifdef RK_EMUL_MAIN
#include <stdio.h>

// tsfa_ks_outer_prob's row walk (tsfresh_amd/csrc/tsfa_relevance.hip), restated: what the walk by diagonals must equal
static double row_walk(int64_t m, int64_t n, int64_t g, int64_t h) {
    if (m < n) { const int64_t t = m; m = n; n = t; }
    const int64_t mg = m / g, ng = n / g;
    int64_t minj = 0, maxj = (h + mg - 1) / mg;
    if (maxj > n + 1) maxj = n + 1;
    int64_t curlen = maxj - minj;
    std::vector<double> A((size_t)n + 4, 1.0);
    for (int64_t j = minj; j < maxj; ++j) A[(size_t)j] = 0.0;
    for (int64_t i = 1; i <= m; ++i) {
        const int64_t lastminj = minj, lastlen = curlen;
        const int64_t num = ng * i - h;
        int64_t fl = num / mg;
        if (num % mg != 0 && num < 0) --fl;
        minj = fl + 1;
        if (minj < 0) minj = 0;
        if (minj > n) minj = n;
        maxj = (ng * i + h + mg - 1) / mg;
        if (maxj > n + 1) maxj = n + 1;
        if (maxj <= minj) return 1.0;
        double val = (minj == 0) ? 0.0 : 1.0;
        for (int64_t jj = 0; jj < maxj - minj; ++jj) {
            const int64_t j = jj + minj;
            const int64_t src = jj + minj - lastminj;
            const double up = (src < lastlen) ? A[(size_t)src] : 1.0;
            val = (up * (double)i + val * (double)j) / (double)(i + j);
            A[(size_t)jj] = val;
        }
        curlen = maxj - minj;
    }
    return A[(size_t)(maxj - minj - 1)];
}

int main() {
    int failed = 0;
    struct Case { int64_t m, n, h; };
    // band widths 1 .. 130 around the chunk seams, tiny tails, an empty band, both sides of the LDS / scratch crossover
    const Case cases[] = {{145, 67, 73},     {131, 130, 85},    {131, 130, 4117}, {131, 130, 4159}, {131, 130, 4243}, {131, 130, 8317},
                          {131, 130, 8359},  {131, 130, 8485},  {138, 130, 4423}, {129, 65, 129 * 65}, {250, 100, 450}, {200, 3, 300},
                          {97, 89, 1},       {3, 200, 300},     {1030, 1029, 987290}, {1030, 1029, 987291}, {1999, 1000, 1999000}};
    for (const Case &c : cases) {
        const int64_t g = rk_gcd(c.m, c.n);
        const double want = row_walk(c.m, c.n, g, c.h);
        for (int storage : {0, 2}) {
            const double got = tsfa_emul_ks_lattice(c.m, c.n, g, c.h, storage);
            if (!(got == want)) {
                ++failed;
                fprintf(stderr, "FAILED lattice %lld %lld h %lld storage %d: %.17g != %.17g\n", (long long)c.m, (long long)c.n,
                        (long long)c.h, storage, got, want);
            }
        }
    }
    // the cells: heap arrays of exactly n_cells entries
    {
        const int64_t N = 9;
        std::vector<int64_t> n1 = {5, 5, 7, 131, 10000, 10001, 40, 0, 1030}, n2 = {5, 5, 7, 130, 9999, 3, 60, 4, 1029};
        std::vector<double> d = {0.2, 0.6, 0.0, 0.25, 0.0, 0.5, 0.3, 0.5, 0.995}, p((size_t)N);
        std::vector<unsigned char> route((size_t)N);
        const int64_t left = tsfa_emul_ks_tails(n1.data(), n2.data(), d.data(), N, p.data(), route.data());
        const unsigned char want[] = {TSFA_ROUTE_HOST_KS, TSFA_ROUTE_KS_EXACT, TSFA_ROUTE_KS_EXACT, TSFA_ROUTE_KS_EXACT, TSFA_ROUTE_KS_EXACT,
                                      TSFA_ROUTE_HOST_KS, TSFA_ROUTE_KS_EXACT, TSFA_ROUTE_HOST_KS, TSFA_ROUTE_KS_EXACT};
        int64_t host = 0;
        for (int64_t c = 0; c < N; ++c) {
            host += want[c] == TSFA_ROUTE_HOST_KS ? 1 : 0;
            if (route[(size_t)c] != want[c]) { ++failed; fprintf(stderr, "FAILED route of cell %lld: %d\n", (long long)c, route[(size_t)c]); }
            if ((want[c] == TSFA_ROUTE_HOST_KS) != (p[(size_t)c] != p[(size_t)c])) ++failed;
        }
        if (left != host) ++failed;
    }
    printf("%d failed\n", failed);
    return failed ? 1 : 0;
}
#endif
