// TEST INFRASTRUCTURE ONLY: the device packer's kernel bodies (tsfresh_amd/csrc/pack_device.h) compiled by g++ -DTSFA_EMUL and
// driven tile by tile with ONE thread per workgroup, in the order tsfa_pack_device launches them on the GPU.  The product
// never loads this; it lets tests/test_pack_device_emul.py compare the packer with data._pack's host route on a box
// without a GPU.  The host steps between the launches (pass planning) are the shared pk_plan_passes of the header.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tsfresh_amd/csrc/pack_device.h"

extern "C" int tsfa_emul_pack_tile(void) { return PK_TILE; }

// out_values: n_rows elements of *out_type; out_offsets: n_rows + 1 int64; out_ids: n_rows elements of the id type;
// out_sort: n_rows elements of the sort type or NULL.  Returns 0, or -1 for arguments tsfa_pack_device refuses.
extern "C" int tsfa_emul_pack(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *values,
                              int32_t value_type, int64_t n, void *out_values, int32_t *out_type, int64_t *out_offsets,
                              void *out_ids, void *out_sort, int64_t *n_groups, int32_t *flags, int32_t *n_passes) {
    if (!ids || !values || n < 1 || n > 0xffffffffll || !pk_is_key_type(id_type, false) || pk_itemsize(value_type) == 0) return -1;
    if (sort && !pk_is_key_type(sort_type, true)) return -1;
    const PkBlk b{0, 1};
    const int64_t n_tiles = (n + PK_TILE - 1) / PK_TILE;
    PkStats st;
    pk_stats_init(&st);
    pk_u64 red[5];
    std::vector<unsigned int> lds(16 * PK_RADIX);
    *flags = 0;
    *n_passes = 0;

    pk_minmax_body(b, 0, 1, ids, id_type, sort, sort_type, n, red, &st);
    const bool in_order = st.descents == 0;
    if (in_order) *flags |= TSFA_PACK_IN_ORDER;
    std::vector<pk_u64> hi[2], lo[2];
    std::vector<uint32_t> idx[2];
    for (int k = 0; k < (in_order ? 1 : 2); ++k) {
        hi[k].resize((size_t)n); lo[k].resize((size_t)n); idx[k].resize((size_t)n);
    }
    std::vector<uint32_t> counts((size_t)n_tiles * PK_RADIX);
    pk_keys_body(b, 0, 1, ids, id_type, sort, sort_type, n, st.kmin[0], sort ? st.kmin[1] : 0ull, pk_sig_bytes(st.kmax[0] - st.kmin[0]),
                 sort ? pk_sig_bytes(st.kmax[1] - st.kmin[1]) : 0, in_order ? 0 : 1, hi[0].data(), lo[0].data(), idx[0].data(),
                 lds.data(), &st);
    int cur = 0;
    if (!in_order) {
        int pass_word[16], pass_byte[16];
        const int np = pk_plan_passes(&st, n, sort != nullptr, pass_word, pass_byte);
        for (int p = 0; p < np; ++p) {
            const pk_u64 *key = pass_word[p] ? lo[cur].data() : hi[cur].data();
            const int shift = 8 * pass_byte[p];
            for (int64_t t = 0; t < n_tiles; ++t) pk_hist_body(b, t, n_tiles, key, shift, n, lds.data(), counts.data());
            pk_scan_body(b, counts.data(), (size_t)n_tiles * PK_RADIX, lds.data(), nullptr);
            for (int64_t t = 0; t < n_tiles; ++t)
                pk_scatter_body(b, t, n_tiles, key, shift, n, counts.data(), hi[cur].data(), lo[cur].data(), idx[cur].data(),
                                hi[cur ^ 1].data(), lo[cur ^ 1].data(), idx[cur ^ 1].data(), lds.data());
            cur ^= 1;
        }
        *n_passes = np;
    }
    for (int64_t t = 0; t < n_tiles; ++t) pk_heads_count_body(b, t, hi[cur].data(), n, lds.data(), counts.data());
    pk_scan_body(b, counts.data(), (size_t)n_tiles, lds.data(), &st.n_groups);
    *n_groups = (int64_t)st.n_groups;
    for (int64_t t = 0; t < n_tiles; ++t)
        pk_groups_body(b, t, hi[cur].data(), idx[cur].data(), n, counts.data(), *n_groups, ids, pk_itemsize(id_type), out_offsets,
                       out_ids, lds.data());
    *out_type = pk_out_type(value_type);
    pk_gather_body(b, 0, 1, values, value_type, idx[cur].data(), n, out_values, &st);
    if (out_sort && sort) pk_gather_raw_body(b, 0, 1, sort, pk_itemsize(sort_type), idx[cur].data(), n, out_sort);
    if (st.nan_flag) *flags |= TSFA_PACK_VALUE_NAN;
    return 0;
}
