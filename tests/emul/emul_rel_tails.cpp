// TEST INFRASTRUCTURE ONLY: the tails / FDR / compaction kernels of tsfresh_amd/csrc/tsfa_relevance.hip without the device.
// The kernel bodies live in tsfresh_amd/csrc/rel_tails.h and are compiled here by g++ -DTSFA_EMUL: one host thread is a
// workgroup, the 64 lanes of a wavefront are looped (a per-lane value is an array of 64, and the wavefront scan / sum add in
// the order of the GPU's shuffle steps).  The launches are replaced by loops over the cells; the sort of the FDR keys, which on
// the device is k_rel_stage / k_rel_sort (a bitonic network on (key, row) with ties by row), is std::sort with that order.
// The product never loads this; tests/test_select_tensor_emul.py compares it with scipy and with fdr_reject.
// With -DRT_EMUL_MAIN the file is a stand-alone program over heap blocks of exactly the driver's sizes: the form an
// AddressSanitizer / UBSan run of the bodies takes.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../tsfresh_amd/csrc/rel_tails.h"

extern "C" double tsfa_emul_mwu_normal(double rank_sum_1, int64_t n1, int64_t n2, double tie_term) {
    return rt_mwu_normal(rank_sum_1, n1, n2, tie_term);
}

extern "C" double tsfa_emul_kendall(int64_t n, int64_t dis, int64_t xtie, int64_t ntie, double x0, double x1, int64_t ytie,
                                    double y0, double y1) {
    return rt_kendall(n, dis, xtie, ntie, x0, x1, ytie, y0, y1);
}

extern "C" double tsfa_emul_fisher(int64_t a, int64_t b, int64_t c, int64_t d) { return rt_fisher(a, b, c, d); }

// k_tails_classes + k_tails_fisher over all cells -> the number of HOST-route cells
extern "C" int64_t tsfa_emul_tails_classes(const tsfa_relevance_col *cols, const double *rank_sums, const int64_t *hi_counts,
                                           const int64_t *class_n, int64_t n_rows, int64_t n_cols, int32_t n_classes, int32_t with_ks,
                                           double *p, unsigned char *route, unsigned char *type) {
    int64_t n_host = 0;
    for (int64_t cell = 0; cell < n_cols * n_classes; ++cell)
        n_host += rt_tails_classes_cell(cols, rank_sums, class_n, n_rows, n_classes, with_ks, cell, p, route, type);
    for (int64_t cell = 0; cell < n_cols * n_classes; ++cell) rt_tails_fisher_cell(cols, hi_counts, class_n, n_rows, n_classes, cell, p);
    return n_host;
}

// k_tails_real over all columns -> the number of HOST-route cells
extern "C" int64_t tsfa_emul_tails_real(const tsfa_relevance_real_col *cols, int64_t n_rows, int64_t n_cols, int64_t ytie, double y0,
                                        double y1, double *p, unsigned char *route, unsigned char *type) {
    int64_t n_host = 0;
    for (int64_t c = 0; c < n_cols; ++c) n_host += rt_tails_real_cell(cols, n_rows, ytie, y0, y1, c, p, route, type);
    return n_host;
}

// tsfa_relevance_fdr: k_fdr_keys, the sort, k_fdr_stepup per table, k_fdr_combine
extern "C" int tsfa_emul_fdr(const double *p, const unsigned char *type, int64_t n_cols, int32_t n_tables, double alpha, double c_m,
                             int32_t n_significant, int32_t multiclass, unsigned char *rel_t, unsigned char *relevant,
                             int32_t *n_sig, double *p_min) {
    if (n_cols < 0 || n_tables < 1 || !(c_m > 0.0)) return TSFA_ERR_INVALID;
    std::vector<double> keys((size_t)n_cols);
    std::vector<uint32_t> idx((size_t)n_cols);
    int64_t m = 0;
    for (int64_t c = 0; c < n_cols; ++c) m += (type[c] != 0) ? 1 : 0;
    for (int32_t t = 0; t < n_tables; ++t) {
        for (int64_t c = 0; c < n_cols; ++c) {
            keys[(size_t)c] = rt_fdr_key(p[c * n_tables + t], type[c]);
            idx[(size_t)c] = (uint32_t)c;
        }
        std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
            return keys[a] < keys[b] || (keys[a] == keys[b] && a < b);
        });
        int64_t last = -1;
        for (int64_t i = 0; i < m; ++i)
            if (keys[idx[(size_t)i]] <= rt_fdr_threshold(i + 1, m, c_m, alpha)) last = i;
        for (int64_t i = 0; i < n_cols; ++i) rel_t[(int64_t)idx[(size_t)i] * n_tables + t] = (i <= last) ? 1 : 0;
    }
    for (int64_t c = 0; c < n_cols; ++c)
        rt_fdr_combine(p + c * n_tables, rel_t + c * n_tables, n_tables, type[c], multiclass, n_significant, relevant + c, n_sig + c,
                       p_min + c);
    return TSFA_OK;
}

// k_compact_mask with nt threads, phase by phase -> the count
extern "C" int64_t tsfa_emul_compact_mask(const unsigned char *mask, int64_t n, int32_t *indices, int32_t nt) {
    std::vector<int32_t> cnt((size_t)nt);
    for (int t = 0; t < nt; ++t) cnt[(size_t)t] = rt_compact_count(mask, n, t, nt);
    int32_t acc = 0;
    for (int t = 0; t < nt; ++t) { const int32_t v = cnt[(size_t)t]; cnt[(size_t)t] = acc; acc += v; }
    for (int t = 0; t < nt; ++t) rt_compact_write(mask, n, t, nt, cnt[(size_t)t], indices);
    return acc;
}

#ifdef RT_EMUL_MAIN
// Stand-alone form (g++ -DTSFA_EMUL -DRT_EMUL_MAIN -fsanitize=address,undefined): the bodies over heap blocks of EXACTLY the
// sizes the driver allocates, so that a write behind the last cell is the sanitizer's to find.
#include <stdio.h>

int main() {
    int failed = 0;
    // Fisher across the chunk seams of the support: the p-value of every table of a few margins sums sensibly
    for (int64_t n : {1, 2, 62, 63, 64, 127, 128, 129, 700}) {
        const int64_t n1 = n + 3, n2 = n + 5;
        for (int64_t a : {(int64_t)0, n / 3, n / 2, n}) {
            const double p = tsfa_emul_fisher(a, n1 - a, n - a, n2 - (n - a));
            if (!(p >= 0.0 && p <= 1.0))   /* (the far tables underflow to 0, as scipy does) */ { ++failed; fprintf(stderr, "FAILED fisher n %lld a %lld: %g\n", (long long)n, (long long)a, p); }
        }
    }
    if (tsfa_emul_fisher(0, 0, 3, 4) != 1.0) ++failed;
    // FDR and compaction at the sizes around a wavefront and a tile
    for (int64_t m : {1, 2, 63, 64, 65, 2049, 5000}) {
        for (int32_t T : {1, 3}) {
            std::vector<double> p((size_t)(m * T)), pmin((size_t)m);
            std::vector<unsigned char> type((size_t)m), rel_t((size_t)(m * T)), rel((size_t)m);
            std::vector<int32_t> nsig((size_t)m);
            uint64_t s = 12345u + (uint64_t)m;
            for (int64_t i = 0; i < m * T; ++i) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const double u = (double)(s >> 11) / 9007199254740992.0;
                p[(size_t)i] = (i % 11 == 0) ? RT_NAN : u * u * u;
            }
            for (int64_t c = 0; c < m; ++c) type[(size_t)c] = (unsigned char)(c % 7 == 3 ? 0 : 1 + c % 2);
            if (tsfa_emul_fdr(p.data(), type.data(), m, T, 0.1, 1.0, 2, T > 1, rel_t.data(), rel.data(), nsig.data(), pmin.data()) != TSFA_OK) ++failed;
            int64_t want = 0;
            for (int64_t c = 0; c < m; ++c) {
                want += rel[(size_t)c] ? 1 : 0;
                if (type[(size_t)c] == 0 && (rel[(size_t)c] || nsig[(size_t)c] || pmin[(size_t)c] == pmin[(size_t)c])) ++failed;
            }
            std::vector<int32_t> idx((size_t)want);   // exactly `count` cells
            for (int nt : {1024, 64, 3})
                if (tsfa_emul_compact_mask(rel.data(), m, want ? idx.data() : nullptr, nt) != want) ++failed;
            for (int64_t i = 0; i < want; ++i)
                if (!rel[(size_t)idx[(size_t)i]] || (i && idx[(size_t)i] <= idx[(size_t)i - 1])) ++failed;
        }
    }
    printf("%d failed\n", failed);
    return failed ? 1 : 0;
}
#endif
