// TEST INFRASTRUCTURE ONLY: the device packer's kernel bodies (tsfresh_amd/csrc/pack_device.h) compiled by g++ -DTSFA_EMUL and
// driven tile by tile with ONE thread per workgroup.  The product never loads this; it lets tests/test_pack_device_emul.py
// compare the packer with data._pack's host route on a box without a GPU.  Steps 1-3 (the sort) are EmulPkSorter of
// emul_pack_sort.h, the one emulated twin of the device's PkSorter; this file adds tsfa_pack_device's own step 4 on.  That
// the order is the GPU's is held by that one header and by the GPU tests that compare device and emulation case by case.
#include <stdint.h>
#include <string.h>

#include "emul_pack_sort.h"

extern "C" int tsfa_emul_pack_tile(void) { return PK_TILE; }

// out_values: n_rows elements of *out_type; out_offsets: n_rows + 1 int64; out_ids: n_rows elements of the id type;
// out_sort: n_rows elements of the sort type or NULL.  Returns 0, or -1 for arguments tsfa_pack_device refuses.
extern "C" int tsfa_emul_pack(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *values,
                              int32_t value_type, int64_t n, void *out_values, int32_t *out_type, int64_t *out_offsets,
                              void *out_ids, void *out_sort, int64_t *n_groups, int32_t *flags, int32_t *n_passes) {
    if (!ids || !values || n < 1 || n > 0xffffffffll || !pk_is_key_type(id_type, false) || pk_itemsize(value_type) == 0) return -1;
    if (sort && !pk_is_key_type(sort_type, true)) return -1;
    EmulPkSorter s;
    s.run(ids, id_type, sort, sort_type, nullptr, 0, n);
    const PkBlk b = s.b;
    const int64_t n_tiles = s.n_tiles;
    PkStats &st = s.st;
    const pk_u64 *hi = s.hi[s.cur].data();
    const uint32_t *idx = s.idx[s.cur].data();
    uint32_t *counts = s.counts.data();
    unsigned int *lds = s.lds.data();
    *flags = s.in_order ? TSFA_PACK_IN_ORDER : 0;
    *n_passes = s.n_passes;

    for (int64_t t = 0; t < n_tiles; ++t) pk_heads_count_body(b, t, hi, n, lds, counts);
    pk_scan_body(b, counts, (size_t)n_tiles, lds, &st.n_groups);
    *n_groups = (int64_t)st.n_groups;
    for (int64_t t = 0; t < n_tiles; ++t)
        pk_groups_body(b, t, hi, idx, n, counts, *n_groups, ids, pk_itemsize(id_type), out_offsets, out_ids, lds);
    *out_type = pk_out_type(value_type);
    pk_gather_body(b, 0, 1, values, value_type, idx, n, out_values, &st);
    if (out_sort && sort) pk_gather_raw_body(b, 0, 1, sort, pk_itemsize(sort_type), idx, n, out_sort);
    if (st.nan_flag) *flags |= TSFA_PACK_VALUE_NAN;
    return 0;
}
