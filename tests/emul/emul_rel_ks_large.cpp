// TEST INFRASTRUCTURE ONLY: the Kolmogorov-Smirnov tail beyond 10 000 rows of tsfresh_amd/csrc/tsfa_relevance.hip without the
// device.  The bodies live in tsfresh_amd/csrc/rel_ks_large.h and are compiled here by g++ -DTSFA_EMUL: the 64 lanes of a
// wavefront are looped, the route kernel is a loop over the cells that fills a work list of exactly n_cells entries, and the
// sum's kernel walks that list from its END, so that the order of the list shows if it ever mattered.
// The product never loads this; tests/test_select_ks_large_emul.py compares it with ks_2samp_pvalue.
// With -DKSL_EMUL_MAIN the file is a stand-alone program: the form an AddressSanitizer / UBSan run of the bodies takes.
#include <stdint.h>

#include <vector>

#include "../../tsfresh_amd/csrc/rel_ks_large.h"

extern "C" int32_t tsfa_emul_ksl_run() { return KSL_RUN; }

// tsfa_ks_large_tails: every cell starts as TSFA_ROUTE_HOST_KS with p = NaN -> the cells left to the caller
extern "C" int64_t tsfa_emul_ks_large_tails(const int64_t *n1, const int64_t *n2, const double *d, int64_t n_cells, double *p,
                                            unsigned char *route) {
    RkCells s = {};
    s.n1 = n1; s.n2 = n2; s.d = d;
    std::vector<int32_t> list((size_t)n_cells);
    int64_t n_list = 0, served = 0;
    for (int64_t c = 0; c < n_cells; ++c) { p[c] = RT_NAN; route[c] = TSFA_ROUTE_HOST_KS; }
    for (int64_t c = 0; c < n_cells; ++c) {
        const int r = ksl_route_cell(s, c, p, route);
        if (r == KSL_SMIRNOV) list[(size_t)n_list++] = (int32_t)c;
        else if (r != KSL_LEAVE) ++served;
    }
    for (int64_t i = n_list - 1; i >= 0; --i) ksl_smirnov_cell(s, list[(size_t)i], p, route);
    return n_cells - served - n_list;
}

#ifdef KSL_EMUL_MAIN
#include <stdio.h>

int main() {
    // one cell of every branch and the serve-rule edges, in heap arrays of exactly n_cells entries
    std::vector<int64_t> n1 = {10001, 10001, 10000, 2000000, 2000002, 10001, 20000, 20000, 20000, 20000, 20000, 20000, 10001},
                         n2 = {142, 143, 10000, 2000000, 2000002, 10001, 20000, 20000, 20000, 20000, 20000, 20000, 0};
    std::vector<double> d = {0.3, 0.3, 0.3, 0.002, 0.002, 0.0031, 0.0, 1.0, 0.00008, 0.99995, 0.6, 0.01, 0.3};
    const unsigned char want[] = {5, 8, 5, 8, 5, 5, 8, 8, 8, 8, 8, 8, 5};
    const int64_t N = (int64_t)n1.size();
    std::vector<double> p((size_t)N);
    std::vector<unsigned char> route((size_t)N);
    int failed = 0;
    int64_t host = 0;
    const int64_t left = tsfa_emul_ks_large_tails(n1.data(), n2.data(), d.data(), N, p.data(), route.data());
    for (int64_t c = 0; c < N; ++c) {
        host += want[c] == TSFA_ROUTE_HOST_KS ? 1 : 0;
        const double v = p[(size_t)c];
        if (route[(size_t)c] != want[c]) { ++failed; fprintf(stderr, "FAILED route of cell %lld: %d\n", (long long)c, route[(size_t)c]); }
        if ((want[c] == TSFA_ROUTE_HOST_KS) ? (v == v) : !(v >= 0.0 && v <= 1.0)) { ++failed; fprintf(stderr, "FAILED p of cell %lld: %g\n", (long long)c, v); }
    }
    if (left != host) ++failed;
    printf("%d failed\n", failed);
    return failed ? 1 : 0;
}
#endif
