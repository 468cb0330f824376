// TEST INFRASTRUCTURE ONLY: the pack set's kernel bodies (tsfresh_amd/csrc/pack_device.h) compiled by g++ -DTSFA_EMUL and driven
// tile by tile with ONE thread per workgroup.  The product never loads this; it lets tests/test_pack_set_emul.py compare the
// set with data._pack's host route, kind by kind, on a box without a GPU.  Steps 1-3 (the sort, kind digits included) are
// EmulPkSorter of emul_pack_sort.h, the one emulated twin of the device's PkSorter; this file adds the set's own step 4 on and
// tsfa_pack_set_values.  That the order is the GPU's is held by that one header and by the GPU tests that compare device and
// emulation case by case.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emul_pack_sort.h"

struct EmulPackSet {
    int64_t n = 0, n_groups = 0, n_kinds = 0;
    int32_t flags = 0, n_passes = 0, id_type = 0, sort_type = 0, kind_type = 0;
    std::vector<uint32_t> perm;
    std::vector<int64_t> offsets, rebased, kind_rows, kind_groups;
    std::vector<unsigned char> uniq, kind_vals, sort;
};

extern "C" int tsfa_emul_pack_set_tile(void) { return PK_TILE; }

// Returns NULL for arguments tsfa_pack_set_create refuses.  keep_sort: the packed sort column is kept.
extern "C" EmulPackSet *tsfa_emul_pack_set_create(const void *ids, int32_t id_type, const void *sort, int32_t sort_type,
                                                  const void *kinds, int32_t kind_type, int64_t n, int32_t keep_sort) {
    if (!ids || n < 1 || n > 0xffffffffll || !pk_is_key_type(id_type, false)) return nullptr;
    if (sort && !pk_is_key_type(sort_type, true)) return nullptr;
    if (kinds && !pk_is_key_type(kind_type, false)) return nullptr;
    const int id_size = pk_itemsize(id_type), sort_size = sort ? pk_itemsize(sort_type) : 0, kind_size = kinds ? pk_itemsize(kind_type) : 0;
    EmulPkSorter s;
    s.run(ids, id_type, sort, sort_type, kinds, kind_type, n);
    const PkBlk b = s.b;
    const int64_t n_tiles = s.n_tiles;
    const pk_u64 *hi = s.hi[s.cur].data();
    const uint32_t *idx = s.idx[s.cur].data();
    unsigned int *lds = s.lds.data();
    EmulPackSet *set = new EmulPackSet();
    set->n = n; set->id_type = id_type; set->sort_type = sort ? sort_type : 0; set->kind_type = kinds ? kind_type : 0;
    set->flags = s.in_order ? TSFA_PACK_IN_ORDER : 0;
    set->n_passes = s.n_passes;

    uint32_t *heads = s.counts.data(), *kheads = s.counts.data() + n_tiles;
    for (int64_t t = 0; t < n_tiles; ++t)
        pk_set_heads_count_body(b, t, hi, idx, kinds, kind_type, n, lds, heads, kheads);
    pk_scan_body(b, heads, (size_t)n_tiles, lds, &s.st.n_groups);
    pk_scan_body(b, kheads, (size_t)n_tiles, lds, &s.ks.n_kinds);
    const int64_t ng = set->n_groups = (int64_t)s.st.n_groups, nk = set->n_kinds = (int64_t)s.ks.n_kinds;
    set->offsets.resize((size_t)ng + 1);
    set->uniq.resize((size_t)ng * id_size);
    set->kind_rows.resize((size_t)nk + 1);
    set->kind_groups.resize((size_t)nk + 1);
    set->kind_vals.resize((size_t)nk * kind_size + 1);
    for (int64_t t = 0; t < n_tiles; ++t)
        pk_set_groups_body(b, t, hi, idx, kinds, kind_type, n, heads, kheads, ng, nk, ids, id_size,
                           set->offsets.data(), set->uniq.data(), set->kind_rows.data(), set->kind_groups.data(),
                           set->kind_vals.data(), lds);
    if (nk > 1) {
        set->rebased.resize((size_t)(ng + nk));
        pk_rebase_body(b, 0, 1, set->offsets.data(), set->kind_rows.data(), set->kind_groups.data(), nk, ng + nk, set->rebased.data());
    }
    if (keep_sort && sort) {
        set->sort.resize((size_t)n * sort_size);
        pk_gather_raw_body(b, 0, 1, sort, sort_size, idx, n, set->sort.data());
    }
    set->perm.swap(s.idx[s.cur]);
    return set;
}

extern "C" void tsfa_emul_pack_set_info(const EmulPackSet *set, int64_t *n_groups, int64_t *n_kinds, int32_t *flags, int32_t *n_passes) {
    *n_groups = set->n_groups; *n_kinds = set->n_kinds; *flags = set->flags; *n_passes = set->n_passes;
}

// kind_rows / kind_groups: n_kinds + 1 int64; kind_vals: n_kinds elements of the kind type (or NULL)
extern "C" void tsfa_emul_pack_set_ranges(const EmulPackSet *set, int64_t *kind_rows, int64_t *kind_groups, void *kind_vals) {
    memcpy(kind_rows, set->kind_rows.data(), set->kind_rows.size() * 8);
    memcpy(kind_groups, set->kind_groups.data(), set->kind_groups.size() * 8);
    if (kind_vals && set->kind_type) memcpy(kind_vals, set->kind_vals.data(), (size_t)set->n_kinds * pk_itemsize(set->kind_type));
}

// What pack k of tsfa_pack_set_values sees, as the GPU driver lays the views out: the kind's offsets (its stretch of the rebased
// buffer, or the set's own offsets when there is one kind), its ids and its packed sort keys (NULL: not wanted).
extern "C" void tsfa_emul_pack_set_kind(const EmulPackSet *set, int64_t k, int64_t *offsets, void *ids, void *sort) {
    const int64_t r0 = set->kind_rows[(size_t)k], r1 = set->kind_rows[(size_t)k + 1];
    const int64_t g0 = set->kind_groups[(size_t)k], g1 = set->kind_groups[(size_t)k + 1];
    const int64_t *src = set->rebased.empty() ? set->offsets.data() : set->rebased.data() + g0 + k;
    memcpy(offsets, src, (size_t)(g1 - g0 + 1) * 8);
    const int id_size = pk_itemsize(set->id_type), sort_size = pk_itemsize(set->sort_type);
    memcpy(ids, set->uniq.data() + (size_t)g0 * id_size, (size_t)(g1 - g0) * id_size);
    if (sort && !set->sort.empty()) memcpy(sort, set->sort.data() + (size_t)r0 * sort_size, (size_t)(r1 - r0) * sort_size);
}

// One value column through the stored permutation: out_values holds n elements of *out_type (kind k: rows kind_rows[k] ..).
extern "C" int tsfa_emul_pack_set_values(const EmulPackSet *set, const void *values, int32_t value_type, void *out_values,
                                         int32_t *out_type, int32_t *nan_flag) {
    if (!values || pk_itemsize(value_type) == 0) return -1;
    const PkBlk b{0, 1};
    PkStats st;
    memset(&st, 0, sizeof(st));
    *out_type = pk_out_type(value_type);
    pk_gather_body(b, 0, 1, values, value_type, set->perm.data(), set->n, out_values, &st);
    *nan_flag = st.nan_flag ? 1 : 0;
    return 0;
}

extern "C" void tsfa_emul_pack_set_destroy(EmulPackSet *set) { delete set; }
