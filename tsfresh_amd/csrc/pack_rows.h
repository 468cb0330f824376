// Row packer: kernel bodies of tsfa_pack_set_rows and tsfa_pack_set_hours (include/tsfresh_amd.h).
//
// A pack set (pack_device.h) keeps the permutation `perm` (sorted position -> input row) and the offsets of its (kind, id)
// groups in HBM.  Two things reach the ragged layout through that permutation here:
//
//   rows   a value MATRIX of logical shape (n_rows, n_cols) with any non-negative element strides -- the value columns of a
//          wide frame held as one tensor -- in ONE pass:  out[c * n_rows + p] = convert(values[perm[p] * sr + c * sc]),
//          with pk_gather_body's conversions (float32 stays float32, everything else becomes float64 as
//          ndarray.astype(np.float64) would) and one NaN flag word per column.
//   hours  the stamps of the rows, for every sorted position p of the whole frame:
//          hours[p] = pt_hours(t[perm[p]], t[perm[first position of p's group]])   (pack_times.h's arithmetic, called)
//
// Routes of the rows gather (pr_route, host):
//   PR_ROUTE_TILES    sc == 1 and n_cols > 1 (a row-major matrix): a work item is tile_t consecutive sorted positions.  Their
//                     tile_t permutation entries are staged in LDS ONCE; then, for every tile of tile_c columns, a
//                     [position x column] block is loaded with the lanes running along the columns of a gathered row
//                     (unit stride inside each row), turned in an LDS tile and stored with the lanes running along the
//                     positions of a column (unit stride).  The geometry is pack_dense.h's channels-last route: tile_c the
//                     power of two in [2, 32] that holds n_cols (pd_tile_c), tile_t = PD_TILE_CELLS / tile_c, rows of
//                     `pitch` = tile_t + pd_tile_pad(cw) 32-bit words, a 64-bit output kept as two words in two planes;
//                     the bank argument at the head of pack_dense.h holds word for word (position for time step, column for
//                     channel).  LDS: 12 KiB per plane + 4 KiB of row indices = 16 KiB (float32) or 28 KiB.
//   PR_ROUTE_GATHER   anything else (one column, a column-major or otherwise strided view): one lane per (column,
//                     position), consecutive lanes on consecutive positions of a column; the store is unit-stride, the
//                     load a gather.
// Both walk their work items in a grid-stride loop of at most PR_MAX_GRID workgroups.  Every barrier of the tile route sits
// in loops whose trip counts depend on the work item alone -- the same for every lane of the workgroup --, so every lane
// reaches every barrier.  The only atomic is the OR into a column's flag word, issued by a lane that HAS loaded a NaN.
//
// Hours: a work item is PK_TILE consecutive sorted positions.  ONE bisection of the set's offsets per work item (thread 0)
// finds the group that holds the tile's first position; the offsets of the groups that START inside the tile -- at most
// PK_TILE of them, and they follow that group in the offsets array -- are staged in LDS as 32-bit distances from the tile's
// first position, in rounds of one element per thread that stop at the first round whose first candidate lies beyond the
// tile (a test on one address, the same for every lane).  Every lane then bisects in LDS for the start of its position's
// group; a position in front of the first staged start belongs to the group the work item's bisection found.  LDS: 16 KiB.
// No per-row bisection of the global offsets, no atomic but pt_flag's OR (one per wavefront at most).
//
// Like pack_device.h this file is compiled two ways: by hipcc for gfx950 (tsfa_pack_device.hip wraps every body in a
// __global__ kernel) and by g++ -DTSFA_EMUL with ONE thread per workgroup (tests/emul/emul_pack_rows.cpp drives the same
// bodies work item by work item, with any number of workgroups).  The emulation sees the index arithmetic of both routes,
// the tile and column-tile edges, the staging rounds and their stop rule, both bisections, the conversions, the hours'
// arithmetic on the host's own division, and the flags.  It cannot see what only exists with 64 lanes: the barriers around
// the LDS buffers, the bank behaviour of the pitch, the wavefront vote in front of the flag's atomic, and the device's own
// division and conversion sequences (tests/test_pack_rows_gpu.py compares those bit for bit).
//
// Bounds: perm holds values below n_rows (the set made it), so a load touches values[r * sr + c * sc] with r < n_rows and
// c < n_cols only -- nothing outside the view the caller described; stores go to [0, n_cols * n_rows) of the output and to
// [0, n_rows) of the hours.  The staging reads offsets[g] for g <= n_groups (the array holds n_groups + 1 entries).
#ifndef TSFA_PACK_ROWS_H
#define TSFA_PACK_ROWS_H

#include "pack_times.h"

#define PR_MAX_GRID 2048   /* workgroups of a rows launch; the work items beyond are taken by striding */
#define PH_MAX_GRID 1024   /* workgroups of an hours launch */

enum { PR_ROUTE_TILES = 0, PR_ROUTE_GATHER = 1 };

struct PrArgs {
    const void *values;
    const uint32_t *perm;        // n_rows: sorted position -> input row
    int64_t n_rows, n_cols;
    int64_t sr, sc;              // element strides of values
    void *out;                   // n_cols x n_rows elements of the output type
    unsigned int *nan_flags;     // n_cols words the kernels OR 1 into
    int64_t n_work;              // tiles route: position tiles; gather route: n_cols * n_rows cells
    int64_t tiles_c;             // tiles route: column tiles
    int tile_c, tile_t;          // tiles route: columns and positions of a tile (pd_tile_c), tile_c * tile_t = PD_TILE_CELLS
};

struct PhArgs {
    const void *t;               // n_rows stamps, row-aligned with the set's key columns
    int64_t stride;              // element stride of t
    double tps;                  // ticks per second (TSFA_I64), exact in float64
    const uint32_t *perm;
    const int64_t *offsets;      // n_groups + 1 over the whole sorted frame
    int64_t n_rows, n_groups;
    double *out;
    unsigned int *flags;
    int64_t n_work;              // tiles of PK_TILE positions
};

// Element j of a value column as the bit pattern of its output type (float32 in the low word, or float64), with
// pk_gather_body's conversions; *nan is raised for a float NaN.
template <int TYPE>
TSFA_DEV pk_u64 pr_load(const void *v, int64_t j, bool *nan) {
    if (TYPE == TSFA_F32) {
        const uint32_t u = ((const uint32_t *)v)[j];
        if ((u & 0x7fffffffu) > 0x7f800000u) *nan = true;
        return (pk_u64)u;
    }
    if (TYPE == TSFA_F64) {
        const pk_u64 u = ((const pk_u64 *)v)[j];
        if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) *nan = true;
        return u;
    }
    double d = 0.0;
    switch (TYPE) {
    case TSFA_I64: d = static_cast<double>(((const int64_t *)v)[j]); break;
    case TSFA_U64: d = static_cast<double>(((const uint64_t *)v)[j]); break;
    case TSFA_I32: d = static_cast<double>(((const int32_t *)v)[j]); break;
    case TSFA_U32: d = static_cast<double>(((const uint32_t *)v)[j]); break;
    case TSFA_I16: d = static_cast<double>(((const int16_t *)v)[j]); break;
    case TSFA_U16: d = static_cast<double>(((const uint16_t *)v)[j]); break;
    case TSFA_I8: d = static_cast<double>(((const int8_t *)v)[j]); break;
    case TSFA_U8: d = static_cast<double>(((const uint8_t *)v)[j]); break;
    case TSFA_BOOL: d = ((const uint8_t *)v)[j] ? 1.0 : 0.0; break;
    default: break;
    }
    return pt_f64_to_bits(d);
}
template <int TYPE>
TSFA_DEV void pr_store(void *out, int64_t i, pk_u64 bits) {
    if (TYPE == TSFA_F32) ((uint32_t *)out)[i] = (uint32_t)bits;
    else ((pk_u64 *)out)[i] = bits;
}

// ---------------------------------------------------------------------------------------------
// 1. the tiles route (sc == 1, n_cols > 1).  Work item w = tile_t sorted positions from w * tile_t, every column tile.
//    `tile`: PD_TILE_WORDS uint32 of LDS, twice that for a 64-bit output (low words, then high words);
//    `rows`: PD_TILE_CELLS / 2 uint32 of LDS (the largest tile_t).
// ---------------------------------------------------------------------------------------------
template <int TYPE>
TSFA_DEV void pr_tiles_body(const PkBlk &b, int64_t first, int64_t stride, const PrArgs &a, uint32_t *tile, uint32_t *rows) {
    const bool wide = TYPE != TSFA_F32;
    uint32_t *const tile_hi = tile + PD_TILE_WORDS;
    for (int64_t w = first; w < a.n_work; w += stride) {   // (w is the same for the whole workgroup)
        const int64_t p0 = w * a.tile_t;
        const int tw = (int)(a.n_rows - p0 < a.tile_t ? a.n_rows - p0 : a.tile_t);
        const int ts = pd_log2(tw);
        pk_sync();  // the previous work item's reads of rows and of the tile are done
        for (int k = b.tid; k < tw; k += b.nt) rows[k] = a.perm[p0 + k];   // the permutation: once per row
        for (int64_t ct = 0; ct < a.tiles_c; ++ct) {
            const int64_t c0 = ct * a.tile_c;
            const int cw = (int)(a.n_cols - c0 < a.tile_c ? a.n_cols - c0 : a.tile_c);
            const int pitch = a.tile_t + pd_tile_pad(cw), cells = tw * cw;
            const int cs = pd_log2(cw);
            pk_sync();  // rows is staged; the previous column tile's reads of the tile are done
            for (int k = b.tid; k < cells; k += b.nt) {
                const int t = cs >= 0 ? k >> cs : k / cw, c = k - t * cw;
                bool nan = false;
                const pk_u64 bits = pr_load<TYPE>(a.values, (int64_t)rows[t] * a.sr + c0 + c, &nan);
                if (nan) pk_or32(&a.nan_flags[c0 + c], 1u);
                tile[c * pitch + t] = (uint32_t)bits;
                if (wide) tile_hi[c * pitch + t] = (uint32_t)(bits >> 32);
            }
            pk_sync();
            for (int k = b.tid; k < cells; k += b.nt) {
                const int c = ts >= 0 ? k >> ts : k / tw, t = k - c * tw;
                pk_u64 bits = tile[c * pitch + t];
                if (wide) bits |= (pk_u64)tile_hi[c * pitch + t] << 32;
                pr_store<TYPE>(a.out, (c0 + c) * a.n_rows + p0 + t, bits);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 2. the gather route: cell e = c * n_rows + p, one lane per cell   (grid-stride)
// ---------------------------------------------------------------------------------------------
template <int TYPE>
TSFA_DEV void pr_gather_body(const PkBlk &b, int64_t first, int64_t stride, const PrArgs &a) {
    for (int64_t e = first + b.tid; e < a.n_work; e += stride) {
        const int64_t c = e / a.n_rows, p = e - c * a.n_rows;
        bool nan = false;
        const pk_u64 bits = pr_load<TYPE>(a.values, (int64_t)a.perm[p] * a.sr + c * a.sc, &nan);
        if (nan) pk_or32(&a.nan_flags[c], 1u);
        pr_store<TYPE>(a.out, e, bits);
    }
}

// ---------------------------------------------------------------------------------------------
// 3. hours since the first stamp of every position's group.  Work item w = positions [w * PK_TILE, (w + 1) * PK_TILE).
//    `starts`: PK_TILE uint32 of LDS; `head`: one int64 of LDS.
// ---------------------------------------------------------------------------------------------
template <int TYPE>
TSFA_DEV void ph_hours_body(const PkBlk &b, int64_t first, int64_t stride, const PhArgs &a, uint32_t *starts, int64_t *head) {
    bool bad = false;
    const pk_u64 *const t = (const pk_u64 *)a.t;
    pk_u64 *const out = (pk_u64 *)a.out;
    for (int64_t w = first; w < a.n_work; w += stride) {   // (w is the same for the whole workgroup)
        const int64_t t0 = w * PK_TILE, t1 = t0 + PK_TILE < a.n_rows ? t0 + PK_TILE : a.n_rows;
        pk_sync();  // the previous work item's reads of starts and head are done
        if (b.tid == 0) {
            int64_t lo = 0, hi = a.n_groups - 1;  // the largest g with offsets[g] <= t0 (offsets[0] = 0)
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (a.offsets[mid] <= t0) lo = mid;
                else hi = mid - 1;
            }
            *head = lo;
        }
        pk_sync();
        const int64_t g0 = *head;
        const int64_t first0 = a.offsets[g0];   // the same address for every lane
        // the groups that start inside the tile are g0 + 1 + k for k = 0 .. (fewer than PK_TILE: every group holds a row)
        int staged = 0;
        for (int k0 = 0; k0 < PK_TILE; k0 += b.nt) {
            const int64_t gu = g0 + 1 + k0;
            if (gu >= a.n_groups || a.offsets[gu] >= t1) break;   // the round's first candidate: the same for every lane
            const int64_t g = gu + b.tid;
            const int64_t o = g < a.n_groups ? a.offsets[g] : t1;
            starts[k0 + b.tid] = o < t1 ? (uint32_t)(o - t0) : 0xffffffffu;
            staged = k0 + b.nt;
        }
        pk_sync();
        const int tw = (int)(t1 - t0);
        for (int k = b.tid; k < tw; k += b.nt) {
            int lo = -1, hi = staged - 1;   // the largest s with starts[s] <= k, or -1
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (starts[mid] <= (uint32_t)k) lo = mid;
                else hi = mid - 1;
            }
            const int64_t fp = lo < 0 ? first0 : t0 + (int64_t)starts[lo];
            const pk_u64 f = t[(int64_t)a.perm[fp] * a.stride];
            const pk_u64 u = t[(int64_t)a.perm[t0 + k] * a.stride];
            out[t0 + k] = pt_hours<TYPE>(u, f, pt_missing(TYPE, f), a.tps, &bad);
        }
    }
    pt_flag(b, a.flags, bad, (unsigned int)TSFA_DENSE_BAD_TIME);
}

// ---------------------------------------------------------------------------------------------
// Host: argument checks, the choice of the route and the work items, shared by the C-ABI and the emulation's driver.
// Return TSFA_OK or the status the entry point reports, with the reason in *why.
// ---------------------------------------------------------------------------------------------
static inline int pr_check(const void *values, int value_type, int64_t n_rows, int64_t n_cols, int64_t sr, int64_t sc,
                           const void *out_packs, const char **why) {
    *why = "";
    if (!values || !out_packs) { *why = "null pointer"; return TSFA_ERR_INVALID; }
    if (pk_itemsize(value_type) == 0) { *why = "unknown element type of the value matrix"; return TSFA_ERR_INVALID; }
    if (n_cols < 1 || n_cols > 0x7fffffffll) { *why = "n_cols must lie in [1, 2 147 483 647]"; return TSFA_ERR_INVALID; }
    if (sr < 0 || sc < 0) { *why = "negative stride"; return TSFA_ERR_INVALID; }
    // every index fits int64 with room, as in pd_check
    const int64_t lim = (int64_t)1 << 62;
    if (n_rows < 1 || n_cols > lim / 8 / n_rows) { *why = "more than 2^59 cells"; return TSFA_ERR_INVALID; }
    if ((sr && n_rows - 1 > lim / 4 / sr) || (sc && n_cols - 1 > lim / 4 / sc)) {
        *why = "a stride reaches beyond 2^60 elements";
        return TSFA_ERR_INVALID;
    }
    return TSFA_OK;
}

static inline int pr_route(int64_t n_cols, int64_t sc) { return (sc == 1 && n_cols > 1) ? PR_ROUTE_TILES : PR_ROUTE_GATHER; }

static inline void pr_plan_work(PrArgs *a, int route) {
    a->tile_c = pd_tile_c(a->n_cols);
    a->tile_t = PD_TILE_CELLS / a->tile_c;
    if (route == PR_ROUTE_TILES) {
        a->tiles_c = (a->n_cols + a->tile_c - 1) / a->tile_c;
        a->n_work = (a->n_rows + a->tile_t - 1) / a->tile_t;
    } else {
        a->tiles_c = 0;
        a->n_work = a->n_cols * a->n_rows;
    }
}

static inline int ph_check(const void *t, int t_type, int64_t ticks_per_second, int64_t n_rows, int64_t stride,
                           const void *hours_out, const void *flags_out, const char **why) {
    *why = "";
    if (!t || !hours_out || !flags_out) { *why = "null pointer"; return TSFA_ERR_INVALID; }
    if (t_type != TSFA_I64 && t_type != TSFA_F64) { *why = "the stamps must be TSFA_I64 (ticks) or TSFA_F64 (seconds)"; return TSFA_ERR_INVALID; }
    if (t_type == TSFA_I64 && ticks_per_second != 1 && ticks_per_second != 1000 && ticks_per_second != 1000000 &&
        ticks_per_second != 1000000000) {
        *why = "ticks_per_second must be 1, 10^3, 10^6 or 10^9";
        return TSFA_ERR_INVALID;
    }
    if (stride < 0) { *why = "negative stride"; return TSFA_ERR_INVALID; }
    if (n_rows < 1 || (stride && n_rows - 1 > ((int64_t)1 << 60) / stride)) { *why = "the stride reaches beyond 2^60 elements"; return TSFA_ERR_INVALID; }
    return TSFA_OK;
}

// one instantiation per element type: CALL(TYPE) is expanded with the constant that equals `type` (checked by pr_check)
#define PR_DISPATCH(type, CALL)                      \
    switch (type) {                                  \
    case TSFA_F32: { CALL(TSFA_F32); break; }        \
    case TSFA_F64: { CALL(TSFA_F64); break; }        \
    case TSFA_I64: { CALL(TSFA_I64); break; }        \
    case TSFA_U64: { CALL(TSFA_U64); break; }        \
    case TSFA_I32: { CALL(TSFA_I32); break; }        \
    case TSFA_U32: { CALL(TSFA_U32); break; }        \
    case TSFA_I16: { CALL(TSFA_I16); break; }        \
    case TSFA_U16: { CALL(TSFA_U16); break; }        \
    case TSFA_I8: { CALL(TSFA_I8); break; }          \
    case TSFA_U8: { CALL(TSFA_U8); break; }          \
    case TSFA_BOOL: { CALL(TSFA_BOOL); break; }      \
    default: break;                                  \
    }

#endif /* TSFA_PACK_ROWS_H */
