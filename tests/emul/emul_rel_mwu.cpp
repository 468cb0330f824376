// TEST INFRASTRUCTURE ONLY: the exact Mann-Whitney tail of tsfresh_amd/csrc/tsfa_relevance.hip without the device.
// The bodies live in tsfresh_amd/csrc/rel_mwu.h and are compiled here by g++ -DTSFA_EMUL: the RM_NT threads of a phase are
// looped, a phase ends where the workgroup has its barrier, and the buffers, the scan rows and the table of a job are heap
// blocks of EXACTLY the sizes the driver gives them, allocated per job and filled with a garbage pattern, so that a step
// outside one is AddressSanitizer's to find and a word that was never written shows in the result.
// The product never loads this; tests/test_select_mwu_emul.py compares it with mannwhitney_pvalue.
// With -DRM_EMUL_MAIN the file is a stand-alone program: the form an AddressSanitizer / UBSan run of the bodies takes.
#include <stdint.h>

#include <vector>

#include "../../tsfresh_amd/csrc/rel_mwu.h"

#define GARBAGE 0xA5A5A5A5A5A5A5A5ull

extern "C" int32_t tsfa_emul_mwu_lds_elems() { return RM_LDS_ELEMS; }
extern "C" int32_t tsfa_emul_mwu_served(int64_t n1, int64_t n2) { return rm_served(n1, n2); }

// k_mwu_build's workgroup for one job
static std::vector<uint64_t> build_table(int64_t m, int64_t n) {
    const size_t words = (size_t)rm_table_words(m, n);
    std::vector<uint64_t> buf0(words, GARBAGE), buf1(words, GARBAGE), scan((size_t)RM_SCAN_WORDS, GARBAGE), table(words, GARBAGE);
    rm_build(m, n, buf0.data(), buf1.data(), scan.data(), table.data());
    return table;
}

// mwu_tails_run: the tables served are built one after the other, then the cells are walked -> the cells served.
// stand-alone cells: table[n_cells], u[n_cells]; class tables (table == NULL): n1 = class_n, n_tables = n_classes, rank_sums.
extern "C" int64_t tsfa_emul_mwu_stage(const int64_t *n1, const int64_t *n2, int32_t n_tables, const int32_t *table, const double *u,
                                       const double *rank_sums, int64_t n_rows, int64_t n_cells, double *p, unsigned char *route) {
    std::vector<RmTable> tables((size_t)n_tables);
    std::vector<uint64_t> tabs;
    for (int32_t t = 0; t < n_tables; ++t) {
        tables[(size_t)t] = {n1[t], n2[t], -1};
        if (!rm_served(n1[t], n2[t])) continue;
        const std::vector<uint64_t> one = build_table(n1[t] < n2[t] ? n1[t] : n2[t], n1[t] < n2[t] ? n2[t] : n1[t]);
        tables[(size_t)t].off = (int64_t)tabs.size();
        tabs.insert(tabs.end(), one.begin(), one.end());
    }
    RmCells s = {table, u, rank_sums, n1, n_rows, n_tables};
    int64_t served = 0;
    for (int64_t cell = 0; cell < n_cells; ++cell) served += rm_cell(s, tables.data(), n_tables, tabs.data(), cell, p, route);
    return served;
}

#ifdef RM_EMUL_MAIN
#include <math.h>
#include <stdio.h>

typedef unsigned __int128 u128;

// _mwu_exact_sf's coefficient list, restated with 128-bit integers (tables whose total fits), then summed from the left
static std::vector<u128> prefix_sums(int64_t m, int64_t n) {
    const int64_t top = m * n;
    std::vector<u128> c((size_t)top + 1, 0);
    c[0] = 1;
    for (int64_t i = 1; i <= m; ++i) {
        for (int64_t d = top; d >= n + i; --d) c[(size_t)d] -= c[(size_t)(d - n - i)];
        for (int64_t d = i; d <= top; ++d) c[(size_t)d] += c[(size_t)(d - i)];
    }
    for (int64_t d = 1; d <= top; ++d) c[(size_t)d] += c[(size_t)(d - 1)];
    return c;
}

int main() {
    int failed = 0;
    struct Case { int64_t m, n; };
    // both sides of the LDS / scratch crossover, a chunk smaller than i, counts beyond 2^64, the cap
    const Case cases[] = {{1, 1}, {1, 9}, {2, 3}, {8, 8}, {8, 9}, {3, 2000}, {8, 319}, {8, 320}, {5, 20000}, {8, 262144}};
    for (const Case &c : cases) {
        const std::vector<uint64_t> table = build_table(c.m, c.n);
        if (c.m * c.n > 16000 && c.m > 3) continue;   // the total leaves 128 bits: built for the sanitizers only
        const std::vector<u128> want = prefix_sums(c.m, c.n);
        const int64_t len = c.m * c.n + 1;
        for (int64_t d = 0; d < len; ++d) {
            const RmInt got = rm_load(table.data(), len, d);
            if (got.w[0] != (uint64_t)want[(size_t)d] || got.w[1] != (uint64_t)(want[(size_t)d] >> 64) || got.w[2] != 0) {
                ++failed;
                fprintf(stderr, "FAILED table (%lld, %lld) at %lld\n", (long long)c.m, (long long)c.n, (long long)d);
                break;
            }
        }
    }
    // the division against the hardware's rounding of an integer: num / 2^55 for numerators of 55 bits (every rounding case)
    for (uint64_t low = 0; low < 16; ++low) {
        RmInt num = rm_zero(), den = rm_zero();
        num.w[0] = ((uint64_t)1 << 54) + low;
        den.w[0] = (uint64_t)1 << 55;
        if (rm_ratio(num, den) != ldexp((double)num.w[0], -55)) { ++failed; fprintf(stderr, "FAILED ratio, low bits %d\n", (int)low); }
    }
    {
        RmInt one = rm_zero(), three = rm_zero();
        one.w[0] = 1;
        three.w[2] = 3;   // 1 / (3 * 2^128)
        if (rm_ratio(one, three) != ldexp(1.0 / 3.0, -128)) { ++failed; fprintf(stderr, "FAILED ratio 1 / (3 * 2^128)\n"); }
    }
    // the cells: heap arrays of exactly n_cells entries; an unserved table, another route byte, a bad table index, a NaN
    {
        const int64_t n1[] = {3, 262145, 5}, n2[] = {2000, 8, 20000};
        std::vector<int32_t> table = {0, 0, 1, 2, 2, 3, 0};
        std::vector<double> u = {3000.0, 6001.0, 5.0, 50000.0, 100000.0, 1.0, RT_NAN}, p(7, -1.0);
        std::vector<unsigned char> route = {4, 4, 4, 4, 1, 4, 4};
        const unsigned char want[] = {7, 7, 4, 7, 1, 4, 4};
        const int64_t served = tsfa_emul_mwu_stage(n1, n2, 3, table.data(), u.data(), nullptr, 0, 7, p.data(), route.data());
        for (int c = 0; c < 7; ++c)
            if (route[(size_t)c] != want[c] || (want[c] == 7) != (p[(size_t)c] >= 0.0)) { ++failed; fprintf(stderr, "FAILED cell %d\n", c); }
        if (served != 3 || p[0] != 1.0 || p[1] != 0.0) ++failed;
    }
    printf("%d failed\n", failed);
    return failed ? 1 : 0;
}
#endif
