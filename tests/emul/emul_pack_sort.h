// TEST INFRASTRUCTURE ONLY: steps 1-3 of the device packer on looped kernel bodies (tsfresh_amd/csrc/pack_device.h, g++
// -DTSFA_EMUL, ONE thread per workgroup) -- the emulated twin of PkSorter in tsfresh_amd/csrc/tsfa_pack_device.hip, written
// once for emul_pack.cpp and emul_pack_set.cpp.  Body for launch, it runs what PkSorter::run queues: min / max (and the kinds'),
// the in-order decision, keys (and the kind histogram), the shared pk_plan_passes / pk_plan_kind_passes, and per pass
// histogram, scan, scatter between two buffer sets.  The GPU tests that compare device and emulation hold the two together.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../tsfresh_amd/csrc/pack_device.h"

struct EmulPkSorter {
    const PkBlk b{0, 1};
    int64_t n = 0, n_tiles = 0;   // n_tiles = ceil(n / PK_TILE): the grid of every tile kernel
    PkStats st;
    PkSetStats ks;
    std::vector<pk_u64> hi[2], lo[2];
    std::vector<uint32_t> idx[2];   // set 1 stays empty when the frame is in order
    std::vector<uint32_t> counts;   // n_tiles x PK_RADIX digit counts; step 4 reuses the front for its per-tile head counts
    std::vector<unsigned int> lds = std::vector<unsigned int>(16 * PK_RADIX);
    int cur = 0, n_passes = 0;
    bool in_order = false;

    // kinds: NULL for a frame without a kind column (nothing runs on its behalf)
    void run(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *kinds, int32_t kind_type, int64_t n_rows) {
        n = n_rows;
        n_tiles = (n + PK_TILE - 1) / PK_TILE;
        pk_stats_init(&st);
        pk_set_stats_init(&ks);
        pk_u64 red[5];
        pk_minmax_body(b, 0, 1, ids, id_type, sort, sort_type, n, red, &st);
        if (kinds) pk_kind_minmax_body(b, 0, 1, kinds, kind_type, ids, id_type, sort, sort_type, n, red, &ks);
        const bool inner_in_order = st.descents == 0;                // (id, sort): only the kind passes are left
        in_order = kinds ? ks.descents == 0 : inner_in_order;        // (kind, id, sort): nothing is sorted
        for (int k = 0; k < (in_order ? 1 : 2); ++k) {
            hi[k].resize((size_t)n); lo[k].resize((size_t)n); idx[k].resize((size_t)n);
        }
        counts.resize((size_t)n_tiles * PK_RADIX);
        const int inner_passes = (in_order || inner_in_order) ? 0 : 1;
        pk_keys_body(b, 0, 1, ids, id_type, sort, sort_type, n, st.kmin[0], sort ? st.kmin[1] : 0ull, pk_sig_bytes(st.kmax[0] - st.kmin[0]),
                     sort ? pk_sig_bytes(st.kmax[1] - st.kmin[1]) : 0, inner_passes, hi[0].data(), lo[0].data(), idx[0].data(),
                     lds.data(), &st);
        if (in_order) return;
        if (kinds) pk_kind_hist_body(b, 0, 1, kinds, kind_type, n, ks.kmin, pk_sig_bytes(ks.kmax - ks.kmin), lds.data(), &ks);
        int pass_word[16], pass_byte[16], kind_byte[8];
        const int np = inner_passes ? pk_plan_passes(&st, n, sort != nullptr, pass_word, pass_byte) : 0;
        const int nkp = kinds ? pk_plan_kind_passes(&ks, n, kind_byte) : 0;
        // sort bytes, id bytes, kind bytes, least significant first; a pass sorts set cur into set cur ^ 1.  The plain digit
        // (a key word and a shift) and the kind digit (read through the row index) differ only in the two tile bodies.
        for (int p = 0; p < np + nkp; ++p) {
            const bool plain = p < np;
            pk_u64 *h0 = hi[cur].data(), *l0 = lo[cur].data(), *h1 = hi[cur ^ 1].data(), *l1 = lo[cur ^ 1].data();
            uint32_t *i0 = idx[cur].data(), *i1 = idx[cur ^ 1].data(), *cnt = counts.data();
            const pk_u64 *key = (plain && pass_word[p]) ? l0 : h0;
            const int shift = 8 * (plain ? pass_byte[p] : kind_byte[p - np]);
            const PkKindDigit dg{kinds, kind_type, ks.kmin, i0, shift};
            for (int64_t t = 0; t < n_tiles; ++t) {
                if (plain) pk_hist_body(b, t, n_tiles, key, shift, n, lds.data(), cnt);
                else pk_hist_impl(b, t, n_tiles, dg, n, lds.data(), cnt);
            }
            pk_scan_body(b, cnt, (size_t)n_tiles * PK_RADIX, lds.data(), nullptr);
            for (int64_t t = 0; t < n_tiles; ++t) {
                if (plain) pk_scatter_body(b, t, n_tiles, key, shift, n, cnt, h0, l0, i0, h1, l1, i1, lds.data());
                else pk_scatter_impl(b, t, n_tiles, dg, n, cnt, h0, l0, i0, h1, l1, i1, lds.data());
            }
            cur ^= 1;
        }
        n_passes = np + nkp;
    }
};
