// TEST INFRASTRUCTURE ONLY: the row packer's kernel bodies (tsfresh_amd/csrc/pack_rows.h) compiled by g++ -DTSFA_EMUL and driven
// work item by work item with ONE thread per workgroup and any number of workgroups, as tsfa_pack_set_rows /
// tsfa_pack_set_hours launch them on the GPU.  The product never loads this; it lets tests/test_pack_rows_emul.py compare the
// rows gather with values[perm] and the hours with data._hours_since_first on a box without a GPU.  The checks, the choice
// of the route and the work items are the shared pr_check / pr_route / pr_plan_work / ph_check of the header.
//
// With -DTSFA_EMUL_MAIN the file is a program of its own (the same drivers under a main that checks them against plain
// loops): the build that runs under -fsanitize=address,undefined.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tsfresh_amd/csrc/pack_rows.h"

// tile_c / tile_t of the tiles route for n_cols columns, and the launch bounds of the two kernels
extern "C" void tsfa_emul_pack_rows_geometry(int64_t n_cols, int32_t *tile_c, int32_t *tile_t, int32_t *rows_max_grid,
                                             int32_t *hours_tile, int32_t *hours_max_grid) {
    *tile_c = pd_tile_c(n_cols);
    *tile_t = PD_TILE_CELLS / *tile_c;
    *rows_max_grid = PR_MAX_GRID;
    *hours_tile = PK_TILE;
    *hours_max_grid = PH_MAX_GRID;
}

template <int TYPE>
static void run_rows(const PrArgs &a, int route, int64_t grid) {
    const PkBlk b{0, 1};
    std::vector<uint32_t> tile(2 * PD_TILE_WORDS), rows(PD_TILE_CELLS / 2);
    for (int64_t wg = 0; wg < grid; ++wg) {
        if (route == PR_ROUTE_TILES) pr_tiles_body<TYPE>(b, wg, grid, a, tile.data(), rows.data());
        else pr_gather_body<TYPE>(b, wg, grid, a);
    }
}

// out: n_cols * n_rows elements of the output type; nan_flags: n_cols words (cleared by the caller).
// n_workgroups: 0 = what the GPU launches (bounded by PR_MAX_GRID), else that many.
// Returns the route (>= 0) or the status tsfa_pack_set_rows reports (< 0).
extern "C" int tsfa_emul_pack_rows(const void *values, int32_t value_type, const uint32_t *perm, int64_t n_rows, int64_t n_cols,
                                   int64_t sr, int64_t sc, void *out, uint32_t *nan_flags, int64_t n_workgroups) {
    const char *why;
    if (int rc = pr_check(values, value_type, n_rows, n_cols, sr, sc, out, &why)) return rc;
    PrArgs a;
    a.values = values; a.perm = perm; a.n_rows = n_rows; a.n_cols = n_cols; a.sr = sr; a.sc = sc; a.out = out;
    a.nan_flags = nan_flags;
    const int route = pr_route(n_cols, sc);
    pr_plan_work(&a, route);
    int64_t grid = a.n_work < PR_MAX_GRID ? a.n_work : PR_MAX_GRID;
    if (n_workgroups > 0) grid = n_workgroups;
#define RUN(T) run_rows<T>(a, route, grid)
    PR_DISPATCH(value_type, RUN)
#undef RUN
    return route;
}

// Returns 0 or the status tsfa_pack_set_hours reports.  offsets: n_groups + 1 over the whole sorted frame.
extern "C" int tsfa_emul_pack_hours(const void *t, int32_t t_type, int64_t ticks_per_second, int64_t stride, const uint32_t *perm,
                                    const int64_t *offsets, int64_t n_rows, int64_t n_groups, double *hours_out,
                                    uint32_t *flags_out, int64_t n_workgroups) {
    const char *why;
    if (int rc = ph_check(t, t_type, ticks_per_second, n_rows, stride, hours_out, flags_out, &why)) return rc;
    PhArgs a;
    a.t = t; a.stride = stride; a.tps = t_type == TSFA_I64 ? (double)ticks_per_second : 1.0;
    a.perm = perm; a.offsets = offsets; a.n_rows = n_rows; a.n_groups = n_groups; a.out = hours_out; a.flags = flags_out;
    a.n_work = (n_rows + PK_TILE - 1) / PK_TILE;
    int64_t grid = a.n_work < PH_MAX_GRID ? a.n_work : PH_MAX_GRID;
    if (n_workgroups > 0) grid = n_workgroups;
    const PkBlk b{0, 1};
    std::vector<uint32_t> starts(PK_TILE);
    int64_t head = 0;
    for (int64_t wg = 0; wg < grid; ++wg) {
        if (t_type == TSFA_I64) ph_hours_body<TSFA_I64>(b, wg, grid, a, starts.data(), &head);
        else ph_hours_body<TSFA_F64>(b, wg, grid, a, starts.data(), &head);
    }
    return 0;
}

#ifdef TSFA_EMUL_MAIN
#include <stdio.h>

// every buffer is a std::vector of exactly the size the driver may touch: the sanitizer sees any access outside
static int check_rows(int64_t n, int64_t c, bool row_major, int64_t grid) {
    std::vector<double> vals((size_t)(n * c)), out((size_t)(n * c));
    std::vector<uint32_t> perm((size_t)n), flags((size_t)c, 0u);
    for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = (uint32_t)((i * 7919 + 3) % n);   // a bijection when gcd(7919, n) = 1
    for (int64_t i = 0; i < n * c; ++i) vals[(size_t)i] = (double)i * 0.5 - 3.0;
    const int64_t sr = row_major ? c : 1, sc = row_major ? 1 : n;
    if (tsfa_emul_pack_rows(vals.data(), TSFA_F64, perm.data(), n, c, sr, sc, out.data(), flags.data(), grid) < 0) return 1;
    for (int64_t k = 0; k < c; ++k)
        for (int64_t p = 0; p < n; ++p)
            if (out[(size_t)(k * n + p)] != vals[(size_t)(perm[(size_t)p] * sr + k * sc)] || flags[(size_t)k]) return 1;
    std::vector<int16_t> iv((size_t)(n * c));
    for (int64_t i = 0; i < n * c; ++i) iv[(size_t)i] = (int16_t)(i * 31 - 20000);
    if (tsfa_emul_pack_rows(iv.data(), TSFA_I16, perm.data(), n, c, sr, sc, out.data(), flags.data(), grid) < 0) return 1;
    for (int64_t k = 0; k < c; ++k)
        for (int64_t p = 0; p < n; ++p)
            if (out[(size_t)(k * n + p)] != (double)iv[(size_t)(perm[(size_t)p] * sr + k * sc)]) return 1;
    std::vector<float> fv((size_t)(n * c)), fo((size_t)(n * c));
    for (int64_t i = 0; i < n * c; ++i) fv[(size_t)i] = (float)i;
    if (tsfa_emul_pack_rows(fv.data(), TSFA_F32, perm.data(), n, c, sr, sc, fo.data(), flags.data(), grid) < 0) return 1;
    for (int64_t k = 0; k < c; ++k)
        for (int64_t p = 0; p < n; ++p)
            if (fo[(size_t)(k * n + p)] != fv[(size_t)(perm[(size_t)p] * sr + k * sc)]) return 1;
    return 0;
}

static int check_hours(int64_t n, int64_t group_len, int64_t grid) {
    std::vector<int64_t> t((size_t)n), offsets;
    std::vector<uint32_t> perm((size_t)n);
    std::vector<double> out((size_t)n);
    for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = (uint32_t)(n - 1 - i);
    for (int64_t i = 0; i < n; ++i) t[(size_t)i] = 1700000000000000000ll + i * 1234567891ll;
    for (int64_t o = 0; o < n; o += group_len) offsets.push_back(o);
    const int64_t ng = (int64_t)offsets.size();
    offsets.push_back(n);
    uint32_t flag = 0;
    if (tsfa_emul_pack_hours(t.data(), TSFA_I64, 1000000000, 1, perm.data(), offsets.data(), n, ng, out.data(), &flag, grid)) return 1;
    for (int64_t g = 0; g < ng; ++g)
        for (int64_t p = offsets[(size_t)g]; p < offsets[(size_t)g + 1]; ++p) {
            const int64_t d = t[perm[(size_t)p]] - t[perm[(size_t)offsets[(size_t)g]]];
            if (out[(size_t)p] != (double)d / 1e9 / 3600.0) return 1;
        }
    return flag ? 1 : 0;
}

int main() {
    int bad = 0;
    const int64_t ns[] = {1, 63, 64, 65, 197, 1031}, cs[] = {1, 2, 3, 31, 32, 33, 65};
    for (int64_t n : ns)
        for (int64_t c : cs)
            for (int rm = 0; rm < 2; ++rm)
                for (int64_t grid : {(int64_t)0, (int64_t)2}) bad += check_rows(n, c, rm != 0, grid);
    const int64_t hn[] = {1, 2, 4095, 4096, 4097, 3 * 4096 + 5}, gl[] = {1, 2, 5, 4096, 100000};
    for (int64_t n : hn)
        for (int64_t g : gl)
            for (int64_t grid : {(int64_t)0, (int64_t)2}) bad += check_hours(n, g, grid);
    printf("emul_pack_rows: %d failures\n", bad);
    return bad ? 1 : 0;
}
#endif
