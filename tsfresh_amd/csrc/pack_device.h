// Device packer: kernel bodies of tsfa_pack_device (include/tsfresh_amd.h).
//
// A long frame in ANY row order -> the ragged sample buffer tsfa_extract* consumes, without a host sort: the id and sort
// columns become order-preserving unsigned keys, the row indices are sorted by (id key, sort key) with a stable LSD radix
// sort of 8-bit digits, group boundaries are found along the sorted order and the value column is gathered (and converted
// to float64 where numpy's astype(float64) would convert) through the permutation.
//
// Like the fam_*.h sources this file is compiled two ways: by hipcc for gfx950 (tsfa_pack_device.hip wraps every body in a
// __global__ kernel) and by g++ -DTSFA_EMUL, where every body runs with ONE thread per workgroup (nt = 1, one lane per
// wavefront) -- tests/emul/emul_pack.cpp drives the same bodies tile by tile, so the digit selection, the pass-skipping
// rule, the (digit, tile) scan, the scatter arithmetic, the boundary search and the conversions are checked on a box
// without a GPU.  What the emulation cannot see is the 64-lane multi-split itself (with one lane a rank is always 0).
//
// Scratch (freed before tsfa_pack_device returns):
//     rows x (16 B composite key + 4 B row index) x 2 buffers = 40 B per row
//   + tiles x 256 x 4 B digit counts (one tile = PK_TILE = 4096 rows: 0.25 B per row)
//   + with TSFA_HOST inputs the staged id / sort / value columns.
//
// Pack set (tsfa_pack_set_*): the rows are sorted ONCE by (kind, id, sort) and every value column is gathered through the
// stored permutation.  The kind key does not travel in the scratch record: a kind pass reads its digit through the row
// index (PkKindDigit), so the scratch stays at 40 B per row (+ the staged kind column with TSFA_HOST).  What the set keeps
// after tsfa_pack_set_create: 4 B per row (the permutation), 8 B per group (+ 8 B per group and kind of rebased offsets
// when there are several kinds), the unique ids, and with TSFA_PACK_KEEP_SORT the packed sort column.
//
// Determinism: a pass is three launches (per-tile digit histogram, exclusive scan over (digit, tile), stable scatter).  No
// workgroup ever waits on a word another workgroup writes: no decoupled look-back, no spin of any kind.  Atomics are used
// only where the arrival order cannot matter (counts, min / max, the NaN flag).
#ifndef TSFA_PACK_DEVICE_H
#define TSFA_PACK_DEVICE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/tsfresh_amd.h"
#include "tsfa_common.h"

#define PK_THREADS 256                      /* workgroup of the tile kernels: four wavefronts */
#define PK_ITEMS 16                         /* rows per thread and tile */
#define PK_TILE (PK_THREADS * PK_ITEMS)     /* 4096 rows: 16 rounds of 64 rows per wavefront */
#define PK_RADIX 256
#define PK_SCAN_THREADS 1024                /* the single workgroup of the (digit, tile) scan */

typedef unsigned long long pk_u64;

// helpers the host driver calls as well
#if TSFA_GPU
#define PK_HD __host__ __device__ __forceinline__
#else
#define PK_HD static inline
#endif

// Everything the host reads back between launches; one allocation, initialised by pk_stats_init.
struct PkStats {
    pk_u64 kmin[2], kmax[2];       // [0] id key, [1] sort key (order-preserving images, before the minimum is subtracted)
    pk_u64 descents;               // rows whose composite key is smaller than their predecessor's: 0 = already in order
    unsigned int nan_flag;         // a float value is NaN
    unsigned int n_groups;         // total of the head-flag scan
    unsigned int hist[16][PK_RADIX];  // hist[w * 8 + b]: byte b of word w (0 id, 1 sort) of (key - kmin) over all rows
};

static inline void pk_stats_init(PkStats *s) {
    memset(s, 0, sizeof(*s));
    s->kmin[0] = s->kmin[1] = ~0ull;
}

struct PkBlk {
    int tid, nt;
};
TSFA_DEV int pk_lanes(const PkBlk &b) { return b.nt >= 64 ? 64 : b.nt; }

TSFA_DEV void pk_sync() {
#if TSFA_GPU
    __syncthreads();
#endif
}

// ---- atomics whose arrival order cannot matter (LDS or global) ----
TSFA_DEV void pk_add32(unsigned int *p, unsigned int v) {
#if TSFA_GPU
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
TSFA_DEV void pk_add64(pk_u64 *p, pk_u64 v) {
#if TSFA_GPU
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
TSFA_DEV void pk_min64(pk_u64 *p, pk_u64 v) {
#if TSFA_GPU
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
TSFA_DEV void pk_max64(pk_u64 *p, pk_u64 v) {
#if TSFA_GPU
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
TSFA_DEV void pk_or32(unsigned int *p, unsigned int v) {
#if TSFA_GPU
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

// ---- element types ----
PK_HD int pk_itemsize(int type) {
    switch (type) {
    case TSFA_F64: case TSFA_I64: case TSFA_U64: return 8;
    case TSFA_F32: case TSFA_I32: case TSFA_U32: return 4;
    case TSFA_I16: case TSFA_U16: return 2;
    case TSFA_I8: case TSFA_U8: case TSFA_BOOL: return 1;
    default: return 0;
    }
}
PK_HD bool pk_is_key_type(int type, bool allow_float) {
    if (type == TSFA_F32 || type == TSFA_F64) return allow_float;
    return pk_itemsize(type) != 0 && type != TSFA_BOOL;
}

// Order-preserving image of element i of a key column: a < b  <=>  key(a) < key(b), a == b  <=>  key(a) == key(b).
// Signed integers: the sign bit flipped.  Floats: -0.0 is mapped to +0.0 FIRST (np.lexsort compares them equal and keeps
// the row order; their raw bit patterns differ), then negative values have every bit flipped and the others the sign bit.
TSFA_DEV pk_u64 pk_load_key(const void *col, int type, int64_t i) {
    switch (type) {
    case TSFA_I64: return (pk_u64)((const int64_t *)col)[i] ^ 0x8000000000000000ull;
    case TSFA_U64: return (pk_u64)((const uint64_t *)col)[i];
    case TSFA_I32: return (pk_u64)((uint32_t)((const int32_t *)col)[i] ^ 0x80000000u);
    case TSFA_U32: return (pk_u64)((const uint32_t *)col)[i];
    case TSFA_I16: return (pk_u64)(uint16_t)((uint16_t)((const int16_t *)col)[i] ^ 0x8000u);
    case TSFA_U16: return (pk_u64)((const uint16_t *)col)[i];
    case TSFA_I8: return (pk_u64)(uint8_t)((uint8_t)((const int8_t *)col)[i] ^ 0x80u);
    case TSFA_U8: return (pk_u64)((const uint8_t *)col)[i];
    case TSFA_F32: {
        float v = ((const float *)col)[i];
        if (v == 0.0f) v = 0.0f;
        uint32_t u;
        memcpy(&u, &v, 4);
        return (pk_u64)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
    }
    case TSFA_F64: {
        double v = ((const double *)col)[i];
        if (v == 0.0) v = 0.0;
        pk_u64 u;
        memcpy(&u, &v, 8);
        return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
    }
    default: return 0;
    }
}

TSFA_DEV void pk_copy_raw(void *dst, int64_t di, const void *src, int64_t si, int itemsize) {
    switch (itemsize) {
    case 8: ((uint64_t *)dst)[di] = ((const uint64_t *)src)[si]; break;
    case 4: ((uint32_t *)dst)[di] = ((const uint32_t *)src)[si]; break;
    case 2: ((uint16_t *)dst)[di] = ((const uint16_t *)src)[si]; break;
    default: ((uint8_t *)dst)[di] = ((const uint8_t *)src)[si]; break;
    }
}

// ---------------------------------------------------------------------------------------------
// 1. one read of the id and sort columns: min / max of both keys, descents of the composite key
//    (grid-stride; `red`: 5 pk_u64 of LDS)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void pk_minmax_body(const PkBlk &b, int64_t first, int64_t stride, const void *ids, int id_type, const void *sort,
                             int sort_type, int64_t n, pk_u64 *red, PkStats *st) {
    if (b.tid == 0) {
        red[0] = ~0ull; red[1] = 0; red[2] = ~0ull; red[3] = 0; red[4] = 0;
    }
    pk_sync();
    pk_u64 mn0 = ~0ull, mx0 = 0, mn1 = ~0ull, mx1 = 0, desc = 0;
    for (int64_t i = first + b.tid; i < n; i += stride) {
        const pk_u64 k0 = pk_load_key(ids, id_type, i);
        const pk_u64 k1 = sort ? pk_load_key(sort, sort_type, i) : 0ull;
        mn0 = k0 < mn0 ? k0 : mn0; mx0 = k0 > mx0 ? k0 : mx0;
        mn1 = k1 < mn1 ? k1 : mn1; mx1 = k1 > mx1 ? k1 : mx1;
        if (i > 0) {
            const pk_u64 p0 = pk_load_key(ids, id_type, i - 1);
            const pk_u64 p1 = sort ? pk_load_key(sort, sort_type, i - 1) : 0ull;
            if (k0 < p0 || (k0 == p0 && k1 < p1)) ++desc;
        }
    }
    pk_min64(&red[0], mn0); pk_max64(&red[1], mx0); pk_min64(&red[2], mn1); pk_max64(&red[3], mx1);
    if (desc) pk_add64(&red[4], desc);
    pk_sync();
    if (b.tid == 0) {
        pk_min64(&st->kmin[0], red[0]); pk_max64(&st->kmax[0], red[1]);
        pk_min64(&st->kmin[1], red[2]); pk_max64(&st->kmax[1], red[3]);
        if (red[4]) pk_add64(&st->descents, red[4]);
    }
}

PK_HD int pk_sig_bytes(pk_u64 range) {
    int nb = 0;
    while (range) { ++nb; range >>= 8; }
    return nb;
}

// ---------------------------------------------------------------------------------------------
// 2. the keys with their minimum subtracted (only significant bytes remain), the identity permutation, and -- unless the
//    frame is already in order -- the 256-bin histogram of every significant byte (`lh`: 16 x 256 uint32 of LDS)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void pk_keys_body(const PkBlk &b, int64_t first, int64_t stride, const void *ids, int id_type, const void *sort,
                           int sort_type, int64_t n, pk_u64 min0, pk_u64 min1, int nb0, int nb1, int do_hist, pk_u64 *hi,
                           pk_u64 *lo, uint32_t *idx, unsigned int *lh, PkStats *st) {
    if (do_hist) {
        for (int k = b.tid; k < 16 * PK_RADIX; k += b.nt) lh[k] = 0;
        pk_sync();
    }
    for (int64_t i = first + b.tid; i < n; i += stride) {
        const pk_u64 k0 = pk_load_key(ids, id_type, i) - min0;
        const pk_u64 k1 = sort ? pk_load_key(sort, sort_type, i) - min1 : 0ull;
        hi[i] = k0;
        lo[i] = k1;
        idx[i] = (uint32_t)i;
        if (do_hist) {
            for (int k = 0; k < nb0; ++k) pk_add32(&lh[k * PK_RADIX + (int)((k0 >> (8 * k)) & 255u)], 1u);
            for (int k = 0; k < nb1; ++k) pk_add32(&lh[(8 + k) * PK_RADIX + (int)((k1 >> (8 * k)) & 255u)], 1u);
        }
    }
    if (do_hist) {
        pk_sync();
        for (int k = b.tid; k < 16 * PK_RADIX; k += b.nt)
            if (lh[k]) pk_add32(&st->hist[k >> 8][k & 255], lh[k]);
    }
}

// The passes the sort has to run, least significant first: byte k of word w (1 = sort key, then 0 = id key) is a pass
// unless ONE bin of its histogram holds every row -- a digit that is constant over all rows permutes nothing.  Bytes above
// the significant ones are zero everywhere and never looked at.  Host code (the .hip driver and the emulation share it).
static inline int pk_plan_passes(const PkStats *st, int64_t n_rows, int has_sort, int *pass_word, int *pass_byte) {
    int np = 0;
    for (int w = has_sort ? 1 : 0; w >= 0; --w) {
        const int nb = pk_sig_bytes(st->kmax[w] - st->kmin[w]);
        for (int k = 0; k < nb; ++k) {
            bool constant = false;
            for (int d = 0; d < PK_RADIX; ++d)
                if ((int64_t)st->hist[w * 8 + k][d] == n_rows) { constant = true; break; }
            if (!constant) { pass_word[np] = w; pass_byte[np] = k; ++np; }
        }
    }
    return np;
}

// ---------------------------------------------------------------------------------------------
// Where a pass reads its digit.  PkKeyDigit: byte `shift / 8` of a key word that travels with the row (the id and sort
// passes).  PkKindDigit: the kind key is NOT part of the scratch record; its digit is read through the row index,
// kinds[idx[i]], with the minimum subtracted on the fly (the pack set's kind passes: 0 extra bytes of scratch per row,
// one gathered read of a narrow column per row and launch).
// ---------------------------------------------------------------------------------------------
struct PkKeyDigit {
    const pk_u64 *key;
    int shift;
};
struct PkKindDigit {
    const void *kinds;
    int type;
    pk_u64 kmin;
    const uint32_t *idx;
    int shift;
};
TSFA_DEV int pk_digit(const PkKeyDigit &d, int64_t i) { return (int)((d.key[i] >> d.shift) & 255u); }
TSFA_DEV int pk_digit(const PkKindDigit &d, int64_t i) {
    return (int)(((pk_load_key(d.kinds, d.type, (int64_t)d.idx[i]) - d.kmin) >> d.shift) & 255u);
}

// ---------------------------------------------------------------------------------------------
// 3a. per-tile digit histogram -> counts[digit * n_tiles + tile]   (`lh`: 256 uint32 of LDS)
// ---------------------------------------------------------------------------------------------
template <class D>
TSFA_DEV void pk_hist_impl(const PkBlk &b, int64_t tile, int64_t n_tiles, const D &dg, int64_t n, unsigned int *lh,
                           uint32_t *counts) {
    for (int d = b.tid; d < PK_RADIX; d += b.nt) lh[d] = 0;
    pk_sync();
    const int64_t t0 = tile * PK_TILE;
    for (int k = b.tid; k < PK_TILE; k += b.nt) {
        const int64_t i = t0 + k;
        if (i < n) pk_add32(&lh[pk_digit(dg, i)], 1u);
    }
    pk_sync();
    for (int d = b.tid; d < PK_RADIX; d += b.nt) counts[(size_t)d * (size_t)n_tiles + (size_t)tile] = lh[d];
}
TSFA_DEV void pk_hist_body(const PkBlk &b, int64_t tile, int64_t n_tiles, const pk_u64 *key, int shift, int64_t n,
                           unsigned int *lh, uint32_t *counts) {
    pk_hist_impl(b, tile, n_tiles, PkKeyDigit{key, shift}, n, lh, counts);
}

// exclusive prefix of v over the lower-numbered threads of the workgroup, and the workgroup total (`ws`: 16 uint32 of LDS)
TSFA_DEV uint32_t pk_blk_excl_sum(const PkBlk &b, uint32_t v, unsigned int *ws, uint32_t *total) {
#if TSFA_GPU
    const int lane = b.tid & 63, w = b.tid >> 6, nw = (b.nt + 63) >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t t = __shfl_up(inc, s);
        if (lane >= s) inc += t;
    }
    pk_sync();  // ws of the previous call has been read by everyone
    if (lane == 63 || b.tid == b.nt - 1) ws[w] = inc;
    pk_sync();
    uint32_t base = 0, all = 0;
    for (int k = 0; k < nw; ++k) {
        if (k < w) base += ws[k];
        all += ws[k];
    }
    *total = all;
    return base + inc - v;
#else
    (void)b; (void)ws;
    *total = v;
    return 0;
#endif
}

// ---------------------------------------------------------------------------------------------
// 3b. exclusive scan, in place, of m uint32 by ONE workgroup (the (digit, tile) counts in digit-major order; the head
//     counts per tile).  Four consecutive elements per thread and step.  The total goes to *total_out (may be NULL).
// ---------------------------------------------------------------------------------------------
TSFA_DEV void pk_scan_body(const PkBlk &b, uint32_t *data, size_t m, unsigned int *ws, unsigned int *total_out) {
    uint32_t carry = 0;
    for (size_t base = 0; base < m; base += (size_t)b.nt * 4) {
        const size_t i0 = base + (size_t)b.tid * 4;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i0 + k < m) ? data[i0 + k] : 0u;
        uint32_t tot;
        uint32_t run = carry + pk_blk_excl_sum(b, v[0] + v[1] + v[2] + v[3], ws, &tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < m) data[i0 + k] = run;
            run += v[k];
        }
        carry += tot;
    }
    if (b.tid == 0 && total_out) *total_out = carry;
}

// ---------------------------------------------------------------------------------------------
// 3c. stable scatter of one tile.  Wavefront w owns rows [w * chunk, (w + 1) * chunk) of the tile and walks them in rounds
//     of 64 consecutive rows, so (tile, wavefront, round, lane) is the input order.  wbase[w][d] starts as the scanned
//     global offset of (digit d, this tile) plus the rows of digit d in the tile's earlier wavefronts, and grows by a
//     round's count after every round.  Inside a round the rank of a row among the rows of its digit is a multi-split:
//     eight 64-bit ballots narrow the mask of lanes holding the same digit, rank = popcount of that mask below the lane.
//     (`wbase`: waves x 256 uint32 of LDS = 4 KiB)
// ---------------------------------------------------------------------------------------------
template <class D>
TSFA_DEV void pk_scatter_impl(const PkBlk &b, int64_t tile, int64_t n_tiles, const D &dg, int64_t n, const uint32_t *scanned,
                              const pk_u64 *hi_in, const pk_u64 *lo_in, const uint32_t *idx_in, pk_u64 *hi_out,
                              pk_u64 *lo_out, uint32_t *idx_out, unsigned int *wbase) {
    const int L = pk_lanes(b), W = b.nt / L, lane = b.tid % L, w = b.tid / L;
    const int chunk = PK_TILE / W, rounds = chunk / L;
    const int64_t w0 = tile * PK_TILE + (int64_t)w * chunk;
    unsigned int *mine = wbase + w * PK_RADIX;
    for (int k = b.tid; k < W * PK_RADIX; k += b.nt) wbase[k] = 0;
    pk_sync();
    for (int r = 0; r < rounds; ++r) {
        const int64_t i = w0 + (int64_t)r * L + lane;
        if (i < n) pk_add32(&mine[pk_digit(dg, i)], 1u);
    }
    pk_sync();
    for (int d = b.tid; d < PK_RADIX; d += b.nt) {
        uint32_t run = scanned[(size_t)d * (size_t)n_tiles + (size_t)tile];
        for (int k = 0; k < W; ++k) {
            const uint32_t c = wbase[k * PK_RADIX + d];
            wbase[k * PK_RADIX + d] = run;
            run += c;
        }
    }
    pk_sync();
    for (int r = 0; r < rounds; ++r) {
        const int64_t i = w0 + (int64_t)r * L + lane;
        const bool valid = i < n;
        const int d = valid ? pk_digit(dg, i) : 0;
#if TSFA_GPU
        pk_u64 same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = ((d >> bit) & 1) != 0;
            const pk_u64 bal = __ballot(valid && one);
            same &= one ? bal : ~bal;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        const int cnt = __popcll(same);
#else
        const int rank = 0, cnt = 1;
#endif
        const uint32_t base = valid ? mine[d] : 0u;
        if (valid) {
            const int64_t pos = (int64_t)base + rank;
            if (pos < n) {  // always true for consistent counts; an out-of-range store is never issued
                hi_out[pos] = hi_in[i];
                lo_out[pos] = lo_in[i];
                idx_out[pos] = idx_in[i];
            }
            if (rank == 0) mine[d] = base + (uint32_t)cnt;
        }
        pk_sync();  // the next round reads what this round's leaders wrote
    }
}
TSFA_DEV void pk_scatter_body(const PkBlk &b, int64_t tile, int64_t n_tiles, const pk_u64 *key, int shift, int64_t n,
                              const uint32_t *scanned, const pk_u64 *hi_in, const pk_u64 *lo_in, const uint32_t *idx_in,
                              pk_u64 *hi_out, pk_u64 *lo_out, uint32_t *idx_out, unsigned int *wbase) {
    pk_scatter_impl(b, tile, n_tiles, PkKeyDigit{key, shift}, n, scanned, hi_in, lo_in, idx_in, hi_out, lo_out, idx_out, wbase);
}

// ---------------------------------------------------------------------------------------------
// 4. group boundaries along the sorted order: row i heads a group when its id key differs from row i - 1's -- or, in a
//    pack set with a kind column, when its KIND differs: the last series of kind a and the first series of kind b often
//    carry the same id.  A kind head is a row whose kind differs from its predecessor's (row 0 is both).  The kind of a
//    sorted row is read through the row index.  kinds == NULL: one kind, the id alone decides.
// ---------------------------------------------------------------------------------------------
TSFA_DEV bool pk_kind_head(const void *kinds, int kind_type, const uint32_t *idx, int64_t i) {
    if (i == 0) return true;
    return kinds && pk_load_key(kinds, kind_type, (int64_t)idx[i]) != pk_load_key(kinds, kind_type, (int64_t)idx[i - 1]);
}

// cnt_lds: 2 uint32 of LDS; tile_kheads may be NULL (no kind column)
TSFA_DEV void pk_set_heads_count_body(const PkBlk &b, int64_t tile, const pk_u64 *hi, const uint32_t *idx, const void *kinds,
                                      int kind_type, int64_t n, unsigned int *cnt_lds, uint32_t *tile_heads,
                                      uint32_t *tile_kheads) {
    if (b.tid == 0) cnt_lds[0] = cnt_lds[1] = 0;
    pk_sync();
    const int64_t t0 = tile * PK_TILE;
    unsigned int c = 0, ck = 0;
    for (int k = b.tid; k < PK_TILE; k += b.nt) {
        const int64_t i = t0 + k;
        if (i >= n) continue;
        const bool kh = pk_kind_head(kinds, kind_type, idx, i);
        if (kh) ++ck;
        if (kh || hi[i] != hi[i - 1]) ++c;
    }
    if (c) pk_add32(&cnt_lds[0], c);
    if (ck) pk_add32(&cnt_lds[1], ck);
    pk_sync();
    if (b.tid == 0) {
        tile_heads[tile] = cnt_lds[0];
        if (tile_kheads) tile_kheads[tile] = cnt_lds[1];
    }
}
TSFA_DEV void pk_heads_count_body(const PkBlk &b, int64_t tile, const pk_u64 *hi, int64_t n, unsigned int *cnt_lds,
                                  uint32_t *tile_heads) {
    if (b.tid == 0) *cnt_lds = 0;
    pk_sync();
    const int64_t t0 = tile * PK_TILE;
    unsigned int c = 0;
    for (int k = b.tid; k < PK_TILE; k += b.nt) {
        const int64_t i = t0 + k;
        if (i < n && (i == 0 || hi[i] != hi[i - 1])) ++c;
    }
    if (c) pk_add32(cnt_lds, c);
    pk_sync();
    if (b.tid == 0) tile_heads[tile] = *cnt_lds;
}

// offsets[g] = first sorted row of group g, uniq[g] = its id in the column's own dtype; offsets[n_groups] = n.
// tile_heads: the exclusive scan of the head counts.  (`ws`: 16 uint32 of LDS)
// With a kind column (tile_kheads: the exclusive scan of the kind-head counts) also, for kind number k in ascending order:
// kind_rows[k] = its first sorted row, kind_groups[k] = its first group, kind_vals[k] = its value in the kind column's own
// dtype; kind_rows[n_kinds] = n and kind_groups[n_kinds] = n_groups.  Without one (tile_kheads == NULL) the kind_* outputs
// are not touched.
TSFA_DEV void pk_set_groups_body(const PkBlk &b, int64_t tile, const pk_u64 *hi, const uint32_t *idx, const void *kinds,
                                 int kind_type, int64_t n, const uint32_t *tile_heads, const uint32_t *tile_kheads,
                                 int64_t n_groups, int64_t n_kinds, const void *ids, int id_size, int64_t *offsets, void *uniq,
                                 int64_t *kind_rows, int64_t *kind_groups, void *kind_vals, unsigned int *ws) {
    const int64_t t0 = tile * PK_TILE;
    uint32_t run = tile_heads[tile], krun = tile_kheads ? tile_kheads[tile] : 0u;
    for (int k0 = 0; k0 < PK_TILE; k0 += b.nt) {
        const int64_t i = t0 + k0 + b.tid;
        const bool khead = i < n && pk_kind_head(kinds, kind_type, idx, i);
        const bool head = i < n && (khead || hi[i] != hi[i - 1]);
        uint32_t tot;
        const uint32_t g = run + pk_blk_excl_sum(b, head ? 1u : 0u, ws, &tot);
        if (head && (int64_t)g < n_groups) {
            offsets[g] = i;
            pk_copy_raw(uniq, (int64_t)g, ids, (int64_t)idx[i], id_size);
        }
        if (i == n - 1) offsets[n_groups] = n;
        run += tot;
        if (tile_kheads) {
            uint32_t ktot;
            const uint32_t kk = krun + pk_blk_excl_sum(b, khead ? 1u : 0u, ws, &ktot);
            if (khead && (int64_t)kk < n_kinds) {
                kind_rows[kk] = i;
                kind_groups[kk] = (int64_t)g;
                if (kinds) pk_copy_raw(kind_vals, (int64_t)kk, kinds, (int64_t)idx[i], pk_itemsize(kind_type));
            }
            if (i == n - 1) {
                kind_rows[n_kinds] = n;
                kind_groups[n_kinds] = n_groups;
            }
            krun += ktot;
        }
    }
}
TSFA_DEV void pk_groups_body(const PkBlk &b, int64_t tile, const pk_u64 *hi, const uint32_t *idx, int64_t n,
                             const uint32_t *tile_heads, int64_t n_groups, const void *ids, int id_size, int64_t *offsets,
                             void *uniq, unsigned int *ws) {
    pk_set_groups_body(b, tile, hi, idx, nullptr, 0, n, tile_heads, nullptr, n_groups, 0, ids, id_size, offsets, uniq, nullptr,
                       nullptr, nullptr, ws);
}

// ---------------------------------------------------------------------------------------------
// 4b. the pack set's third key.  One read of the three key columns: min / max of the kind key and the descents of the
//     composite (kind, id, sort) key (grid-stride; `red`: 3 pk_u64 of LDS); then the 256-bin histogram of every
//     significant byte of (kind key - minimum) (`lh`: 8 x 256 uint32 of LDS).
// ---------------------------------------------------------------------------------------------
struct PkSetStats {
    pk_u64 kmin, kmax;            // kind key (order-preserving image, before the minimum is subtracted)
    pk_u64 descents;              // rows whose (kind, id, sort) key is smaller than their predecessor's
    unsigned int n_kinds;         // total of the kind-head scan
    unsigned int hist[8][PK_RADIX];
};

static inline void pk_set_stats_init(PkSetStats *s) {
    memset(s, 0, sizeof(*s));
    s->kmin = ~0ull;
}

TSFA_DEV void pk_kind_minmax_body(const PkBlk &b, int64_t first, int64_t stride, const void *kinds, int kind_type,
                                  const void *ids, int id_type, const void *sort, int sort_type, int64_t n, pk_u64 *red,
                                  PkSetStats *st) {
    if (b.tid == 0) {
        red[0] = ~0ull; red[1] = 0; red[2] = 0;
    }
    pk_sync();
    pk_u64 mn = ~0ull, mx = 0, desc = 0;
    for (int64_t i = first + b.tid; i < n; i += stride) {
        const pk_u64 kk = pk_load_key(kinds, kind_type, i);
        mn = kk < mn ? kk : mn; mx = kk > mx ? kk : mx;
        if (i > 0) {
            const pk_u64 pv = pk_load_key(kinds, kind_type, i - 1);
            bool less = kk < pv;
            if (kk == pv) {
                const pk_u64 k0 = pk_load_key(ids, id_type, i), p0 = pk_load_key(ids, id_type, i - 1);
                less = k0 < p0;
                if (k0 == p0 && sort) less = pk_load_key(sort, sort_type, i) < pk_load_key(sort, sort_type, i - 1);
            }
            if (less) ++desc;
        }
    }
    pk_min64(&red[0], mn); pk_max64(&red[1], mx);
    if (desc) pk_add64(&red[2], desc);
    pk_sync();
    if (b.tid == 0) {
        pk_min64(&st->kmin, red[0]); pk_max64(&st->kmax, red[1]);
        if (red[2]) pk_add64(&st->descents, red[2]);
    }
}

TSFA_DEV void pk_kind_hist_body(const PkBlk &b, int64_t first, int64_t stride, const void *kinds, int kind_type, int64_t n,
                                pk_u64 kmin, int nb, unsigned int *lh, PkSetStats *st) {
    for (int k = b.tid; k < 8 * PK_RADIX; k += b.nt) lh[k] = 0;
    pk_sync();
    for (int64_t i = first + b.tid; i < n; i += stride) {
        const pk_u64 kk = pk_load_key(kinds, kind_type, i) - kmin;
        for (int k = 0; k < nb; ++k) pk_add32(&lh[k * PK_RADIX + (int)((kk >> (8 * k)) & 255u)], 1u);
    }
    pk_sync();
    for (int k = b.tid; k < 8 * PK_RADIX; k += b.nt)
        if (lh[k]) pk_add32(&st->hist[k >> 8][k & 255], lh[k]);
}

// The kind passes, least significant first, by pk_plan_passes' rule.  They run AFTER the sort and id passes: the kind is
// the most significant key.  Host code.
static inline int pk_plan_kind_passes(const PkSetStats *st, int64_t n_rows, int *pass_byte) {
    int np = 0;
    const int nb = pk_sig_bytes(st->kmax - st->kmin);
    for (int k = 0; k < nb; ++k) {
        bool constant = false;
        for (int d = 0; d < PK_RADIX; ++d)
            if ((int64_t)st->hist[k][d] == n_rows) { constant = true; break; }
        if (!constant) pass_byte[np++] = k;
    }
    return np;
}

// ---------------------------------------------------------------------------------------------
// 4c. the offsets of every kind of a pack set, rebased to the kind's first row, in ONE buffer of n_groups + n_kinds int64:
//     kind k owns elements [kind_groups[k] + k, kind_groups[k + 1] + k + 1) = global[kind_groups[k] .. kind_groups[k + 1]]
//     - kind_rows[k].  Element e finds its kind by bisection over the n_kinds starts.  (grid-stride)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void pk_rebase_body(const PkBlk &b, int64_t first, int64_t stride, const int64_t *global, const int64_t *kind_rows,
                             const int64_t *kind_groups, int64_t n_kinds, int64_t total, int64_t *out) {
    for (int64_t e = first + b.tid; e < total; e += stride) {
        int64_t lo = 0, hi = n_kinds - 1;  // the largest k with kind_groups[k] + k <= e
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (kind_groups[mid] + mid <= e) lo = mid;
            else hi = mid - 1;
        }
        out[e] = global[e - lo] - kind_rows[lo];
    }
}

// ---------------------------------------------------------------------------------------------
// 5. gather: out[i] = values[idx[i]].  float32 stays float32, float64 stays float64, every integer type and bool becomes
//    float64 exactly as ndarray.astype(np.float64) does: static_cast<double> of a 64-bit integer is correctly rounded
//    (round to nearest, ties to even) on the host and on gfx950 (the compiler's expansion converts the two 32-bit halves
//    exactly and rounds ONCE, in the final addition), which is what numpy's C cast does; narrower integers are exact.
//    A NaN in a float column raises st->nan_flag (the host turns it into the reference's ValueError).
// ---------------------------------------------------------------------------------------------
PK_HD int pk_out_type(int value_type) { return value_type == TSFA_F32 ? TSFA_F32 : TSFA_F64; }

TSFA_DEV void pk_gather_body(const PkBlk &b, int64_t first, int64_t stride, const void *values, int value_type,
                             const uint32_t *idx, int64_t n, void *out, PkStats *st) {
    bool nan = false;
    for (int64_t i = first + b.tid; i < n; i += stride) {
        const int64_t j = (int64_t)idx[i];
        switch (value_type) {
        case TSFA_F32: { const float v = ((const float *)values)[j]; nan = nan || (v != v); ((float *)out)[i] = v; break; }
        case TSFA_F64: { const double v = ((const double *)values)[j]; nan = nan || (v != v); ((double *)out)[i] = v; break; }
        case TSFA_I64: ((double *)out)[i] = static_cast<double>(((const int64_t *)values)[j]); break;
        case TSFA_U64: ((double *)out)[i] = static_cast<double>(((const uint64_t *)values)[j]); break;
        case TSFA_I32: ((double *)out)[i] = static_cast<double>(((const int32_t *)values)[j]); break;
        case TSFA_U32: ((double *)out)[i] = static_cast<double>(((const uint32_t *)values)[j]); break;
        case TSFA_I16: ((double *)out)[i] = static_cast<double>(((const int16_t *)values)[j]); break;
        case TSFA_U16: ((double *)out)[i] = static_cast<double>(((const uint16_t *)values)[j]); break;
        case TSFA_I8: ((double *)out)[i] = static_cast<double>(((const int8_t *)values)[j]); break;
        case TSFA_U8: ((double *)out)[i] = static_cast<double>(((const uint8_t *)values)[j]); break;
        case TSFA_BOOL: ((double *)out)[i] = ((const uint8_t *)values)[j] ? 1.0 : 0.0; break;
        default: break;
        }
    }
    if (nan) pk_or32(&st->nan_flag, 1u);
}

// the sort column in packed order, element type unchanged (only on request)
TSFA_DEV void pk_gather_raw_body(const PkBlk &b, int64_t first, int64_t stride, const void *col, int itemsize,
                                 const uint32_t *idx, int64_t n, void *out) {
    for (int64_t i = first + b.tid; i < n; i += stride) pk_copy_raw(out, i, col, (int64_t)idx[i], itemsize);
}

#endif /* TSFA_PACK_DEVICE_H */
