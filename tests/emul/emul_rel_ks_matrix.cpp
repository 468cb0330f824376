// TEST INFRASTRUCTURE ONLY: the Kolmogorov-Smirnov tail of rare classes of tsfresh_amd/csrc/tsfa_relevance.hip without the
// device.  The bodies live in tsfresh_amd/csrc/rel_ks_matrix.h and are compiled here by g++ -DTSFA_EMUL: the 64 lanes of a
// wavefront are looped, the route kernel is a loop over the cells, and every work list is walked from its END.  The cells of
// the 512-thread MFMA kernel (Durbin's matrix above n = 140) have no emulation: they stay TSFA_ROUTE_HOST_KS here.
// The product never loads this; tests/test_select_ks_matrix_emul.py compares it with ks_2samp_pvalue.
#include <stdint.h>

#include <vector>

#include "../../tsfresh_amd/csrc/rel_ks_matrix.h"

extern "C" int64_t tsfa_emul_ks_matrix_tails(const int64_t *n1, const int64_t *n2, const double *d, int64_t n_cells, double *p,
                                             unsigned char *route) {
    RkCells s = {};
    s.n1 = n1; s.n2 = n2; s.d = d;
    std::vector<int32_t> list[KSM_LISTS];
    std::vector<double> lds(KSM_SMALL_LDS);
    int64_t left = n_cells;
    for (int64_t c = 0; c < n_cells; ++c) { p[c] = RT_NAN; route[c] = TSFA_ROUTE_HOST_KS; }
    for (int64_t c = 0; c < n_cells; ++c) {
        int k = 0;
        const int r = ksm_route_cell(s, c, p, route, &k);
        if (r >= KSM_SMIRNOV) list[KSM_LIST_OF(r)].push_back((int32_t)c);
        else if (r != KSM_LEAVE) --left;
    }
    for (int b = KSM_SMIRNOV; b <= KSM_POMERANZ; ++b) {
        const std::vector<int32_t> &q = list[KSM_LIST_OF(b)];
        for (size_t i = q.size(); i-- > 0; --left) ksm_list_cell(s, q[i], b, lds.data(), p, route);
    }
    return left;
}
