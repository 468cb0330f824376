// Valid-row packer: kernel bodies of tsfa_pack_rows_valid and tsfa_pack_set_remap (include/tsfresh_amd.h).
//
// A frame held as columns in HBM -- ids, maybe sort keys, maybe kind codes, a value matrix of logical shape (n_rows, n_cols)
// with any non-negative element strides, maybe stamps -- loses the rows `dropna()` would drop BEFORE the pack set sorts it:
// a row goes when one of its n_cols values is NaN (float32 / float64 values), when its sort key is NaN (float32 / float64
// keys) or when its stamp is NaT (INT64_MIN ticks) or a NaN second.  +-inf is a value and stays.  Only the KEY columns are
// compacted (they are what the sort reads); the values and stamps are never copied: the kept rows' input indices `src` are
// composed into the set's permutation afterwards (prv_remap_body: perm[p] = src[perm[p]]), and tsfa_pack_set_rows / _values /
// _hours gather from the ORIGINAL arrays through it.
//
// A block is PRV_BLOCK = 1024 consecutive rows = PRV_WORDS = 16 validity words of 64 rows; a workgroup of four wavefronts
// takes a block, wavefront v the words [4 v, 4 v + 4).  Three launches, no workgroup waits on another, no atomic at all:
//   mark     bit l of word k of block w is set when row w * 1024 + k * 64 + l exists and is kept: the word is the 64-lane
//            ballot of the lanes' verdicts.  The verdict on the values takes one of two routes:
//              FLAT (stride_col == 1, 1 < n_cols <= PRV_FLAT_COLS: a row-major matrix)  the block's rows x n_cols cells are
//                   walked with lane = CELL, consecutive lanes on consecutive columns of a row and then on the next row --
//                   one coalesced stretch when stride_row == n_cols --, and a NaN cell raises its row's flag in LDS (4 KiB;
//                   plain stores of the same 1, no atomic).  The ballot lanes then read the flags.  A lane per row walking
//                   n_cols elements would touch n_cols cache lines per wavefront load.
//              else lane = ROW, a loop over the columns: unit-stride along the rows of a column-major matrix or of one
//                   column; a gather for anything else.
//            Integer and bool values are not read at all (VT == PRV_NO_VALUES).  The key columns are read in their own type
//            with lane = row.  The wavefronts' kept counts meet in LDS; thread 0 stores the block's count.
//   scan     the block counts become their exclusive scan: pk_scan_body (pack_device.h), the scan of the sort's tile
//            counts, which lives in the translation unit that launches these bodies; kept rows <= n_rows < 2^32 fit its words.
//   compact  wavefront v re-reads its words.  Slot of a kept row = scanned base of the block + kept rows of the block's
//            earlier words + kept rows below the lane in its word (v_mbcnt_lo / v_mbcnt_hi on the word's halves).  Kept rows
//            write ids_out[slot], sort_out[slot], kinds_out[slot] in the columns' own types and src[slot] = row: the kept
//            lanes of a word write consecutive cells, and the order is the input order (the sort is stable and a frame
//            without a sort column relies on it).
//
// Like pack_valid.h this file follows the two-build form of the packers: under g++ -DTSFA_EMUL one thread stands for the
// workgroup, takes all PRV_WORDS words and loops over its 64 lanes (PV_LANES, pv_vote, pv_popc of pack_valid.h).
//
// Bounds: a lane beyond the end of the last block loads the block's last row instead (an address some lane reads anyway;
// its bit is not set), so every load's row is below n_rows; the FLAT walk's cell k < rw * n_cols belongs to row
// k / n_cols < rw; words holds n_blocks * PRV_WORDS entries and every block writes all of its 16; slots are below the total
// of the counts = n_kept <= the capacity of the outputs (n_rows, the caller's); prv_remap_body reads src[perm[p]] with
// perm[p] < n_kept (the set was made on the compacted columns) and writes a value < n_source_rows.
#ifndef TSFA_PACK_ROWS_VALID_H
#define TSFA_PACK_ROWS_VALID_H

#include "pack_rows.h"
#include "pack_valid.h"

#define PRV_BLOCK TSFA_ROWS_VALID_BLOCK      /* rows of one work item (include/tsfresh_amd.h: 1024) */
#define PRV_WORDS (PRV_BLOCK / 64)           /* validity words of a block */
#if TSFA_GPU
#define PRV_WAVES (PK_THREADS / 64)          /* wavefronts of a workgroup of the mark and compact kernels */
#else
#define PRV_WAVES 1
#endif
#define PRV_WPW (PRV_WORDS / PRV_WAVES)      /* consecutive words of one wavefront */
#define PRV_FLAT_COLS (1 << 20)              /* most columns of the FLAT route: a block's cells fit 31 bits */
#define PRV_MAX_GRID 2048                    /* workgroups of a launch; the blocks beyond are taken by striding */
#define PRV_NO_VALUES (-1)                   /* VT of a value matrix that cannot hold NaN */

struct PrvArgs {
    const void *ids, *sort, *kinds;          // key columns, contiguous; sort and kinds may be NULL
    int id_size, sort_size, kind_size;       // bytes per element (0: absent)
    int sort_type;                           // TSFA_F32 / TSFA_F64: the keys are tested; anything else: not read by mark
    const void *values;                      // NULL when VT == PRV_NO_VALUES
    int64_t n_cols, sr, sc;                  // element strides of values
    const void *t;                           // NULL: no stamps
    int t_type;                              // TSFA_I64 | TSFA_F64
    int64_t t_stride;
    int64_t n_rows, n_blocks;
    pk_u64 *words;                           // n_blocks * PRV_WORDS validity words
    uint32_t *counts;                        // n_blocks kept counts, after the scan the first slot of each block
    void *ids_out, *sort_out, *kinds_out;    // compacted key columns
    uint32_t *src;                           // src[slot] = input row
};

template <int VT>
TSFA_DEV bool prv_nan(const void *v, int64_t j) {
    if (VT == TSFA_F32) return (((const uint32_t *)v)[j] & 0x7fffffffu) > 0x7f800000u;
    return (((const pk_u64 *)v)[j] & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

// kept rows of word m below `lane`
TSFA_DEV int prv_rank(pk_u64 m, int lane) {
#if TSFA_GPU
    (void)lane;
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#else
    return pv_popc(m & ((1ull << lane) - 1ull));
#endif
}

// ---------------------------------------------------------------------------------------------
// 1. mark: the validity words and the kept count of every block.  `bad`: PRV_BLOCK uint32 of LDS (FLAT only);
//    `ws`: PRV_WAVES words of LDS.
// ---------------------------------------------------------------------------------------------
template <int VT, bool FLAT>
TSFA_DEV void prv_mark_body(const PkBlk &b, int64_t first, int64_t stride, const PrvArgs &a, uint32_t *bad, unsigned int *ws) {
    const int wave = pv_wave(b);
    const bool sort_f32 = a.sort && a.sort_type == TSFA_F32, sort_f64 = a.sort && a.sort_type == TSFA_F64;
    for (int64_t w = first; w < a.n_blocks; w += stride) {   // (w is the same for the whole workgroup)
        const int64_t r0 = w * PRV_BLOCK;
        const int rw = (int)(a.n_rows - r0 < PRV_BLOCK ? a.n_rows - r0 : PRV_BLOCK);
        if (FLAT) {
            const int nc = (int)a.n_cols, cells = rw * nc, cs = pd_log2(nc);
            pk_sync();  // the previous block's reads of bad are done
            for (int k = b.tid; k < rw; k += b.nt) bad[k] = 0u;
            pk_sync();
            for (int k = b.tid; k < cells; k += b.nt) {
                const int t = cs >= 0 ? k >> cs : k / nc;
                if (prv_nan<VT>(a.values, (r0 + t) * a.sr + (k - t * nc))) bad[t] = 1u;
            }
            pk_sync();
        }
        pk_u64 m[PRV_WPW];
#pragma unroll
        for (int j = 0; j < PRV_WPW; ++j) m[j] = 0;
        PV_LANES(lane, b) {
            bool nan[PRV_WPW];
            int tj[PRV_WPW];
#pragma unroll
            for (int j = 0; j < PRV_WPW; ++j) {
                const int t = (wave * PRV_WPW + j) * 64 + lane;
                tj[j] = t < rw ? t : rw - 1;   // a lane beyond the end tests the block's last row: no load behind a branch
                nan[j] = FLAT ? bad[tj[j]] != 0u : false;
            }
            if (!FLAT && VT != PRV_NO_VALUES) {
                for (int64_t c = 0; c < a.n_cols; ++c) {
#pragma unroll
                    for (int j = 0; j < PRV_WPW; ++j)
                        if (prv_nan<VT>(a.values, (r0 + tj[j]) * a.sr + c * a.sc)) nan[j] = true;
                }
            }
#pragma unroll
            for (int j = 0; j < PRV_WPW; ++j) {
                if (sort_f32 && prv_nan<TSFA_F32>(a.sort, r0 + tj[j])) nan[j] = true;
                if (sort_f64 && prv_nan<TSFA_F64>(a.sort, r0 + tj[j])) nan[j] = true;
                if (a.t && pt_missing(a.t_type, ((const pk_u64 *)a.t)[(r0 + tj[j]) * a.t_stride])) nan[j] = true;
            }
#pragma unroll
            for (int j = 0; j < PRV_WPW; ++j) m[j] |= pv_vote(!nan[j] && (wave * PRV_WPW + j) * 64 + lane < rw, lane);
        }
        unsigned int cnt = 0;
#pragma unroll
        for (int j = 0; j < PRV_WPW; ++j) cnt += (unsigned int)pv_popc(m[j]);
        // lane j < PRV_WPW of the wavefront stores word j (one vector store, PRV_WPW lanes wide)
        PV_LANES(lane, b) {
            if (lane >= PRV_WPW) continue;
            pk_u64 mine = 0;
#pragma unroll
            for (int j = 0; j < PRV_WPW; ++j)
                if (j == lane) mine = m[j];
            a.words[w * PRV_WORDS + wave * PRV_WPW + lane] = mine;
        }
        pk_sync();  // ws of the previous block has been read
        if (pv_lane0(b)) ws[wave] = cnt;
        pk_sync();
        if (b.tid == 0) {
            unsigned int all = 0;
            for (int k = 0; k < PRV_WAVES; ++k) all += ws[k];
            a.counts[w] = all;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 3. compact: the kept rows' keys and input indices go to their slots (counts[] has been scanned).
// ---------------------------------------------------------------------------------------------
TSFA_DEV void prv_compact_body(const PkBlk &b, int64_t first, int64_t stride, const PrvArgs &a) {
    const int wave = pv_wave(b);
    for (int64_t w = first; w < a.n_blocks; w += stride) {
        const int64_t r0 = w * PRV_BLOCK;
        const pk_u64 *const wd = a.words + w * PRV_WORDS;
        int64_t pre = (int64_t)a.counts[w];
        for (int k = 0; k < wave * PRV_WPW; ++k) pre += pv_popc(wd[k]);   // (the same addresses for every lane)
#pragma unroll
        for (int j = 0; j < PRV_WPW; ++j) {
            const pk_u64 m = wd[wave * PRV_WPW + j];
            PV_LANES(lane, b) {
                if (!((m >> lane) & 1ull)) continue;
                const int64_t row = r0 + (wave * PRV_WPW + j) * 64 + lane, slot = pre + prv_rank(m, lane);
                pk_copy_raw(a.ids_out, slot, a.ids, row, a.id_size);
                if (a.sort) pk_copy_raw(a.sort_out, slot, a.sort, row, a.sort_size);
                if (a.kinds) pk_copy_raw(a.kinds_out, slot, a.kinds, row, a.kind_size);
                a.src[slot] = (uint32_t)row;
            }
            pre += pv_popc(m);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 4. compose: a permutation over the compacted rows becomes one over the input rows   (grid-stride)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void prv_remap_body(const PkBlk &b, int64_t first, int64_t stride, uint32_t *perm, const uint32_t *src, int64_t n) {
    for (int64_t p = first + b.tid; p < n; p += stride) perm[p] = src[perm[p]];
}

// ---------------------------------------------------------------------------------------------
// Host: argument checks and the route, shared by the C-ABI and any driver of the bodies.
// Returns TSFA_OK or the status tsfa_pack_rows_valid reports, with the reason in *why.
// ---------------------------------------------------------------------------------------------
static inline bool prv_is_float(int type) { return type == TSFA_F32 || type == TSFA_F64; }

static inline bool prv_flat(int64_t n_cols, int64_t sc) { return sc == 1 && n_cols > 1 && n_cols <= PRV_FLAT_COLS; }

static inline int prv_check(const void *ids, int id_type, const void *sort, int sort_type, const void *kinds, int kind_type,
                            const void *values, int value_type, int64_t n_cols, int64_t sr, int64_t sc, const void *t, int t_type,
                            int64_t t_stride, int64_t n_rows, const void *ids_out, const void *sort_out, const void *kinds_out,
                            const void *src_out, const void *n_kept, const char **why) {
    *why = "";
    if (!ids || !ids_out || !src_out || !n_kept || (sort && !sort_out) || (kinds && !kinds_out)) { *why = "null pointer"; return TSFA_ERR_INVALID; }
    if (n_rows < 1) { *why = "n_rows must be positive"; return TSFA_ERR_INVALID; }
    if (n_rows > 0xffffffffll) { *why = "more than 4 294 967 295 rows (the row indices are 32 bits wide)"; return TSFA_ERR_TOO_LONG; }
    if (!pk_is_key_type(id_type, false)) { *why = "the id column must be of an integer type"; return TSFA_ERR_INVALID; }
    if (sort && !pk_is_key_type(sort_type, true)) { *why = "the sort column must be of an integer type, float32 or float64"; return TSFA_ERR_INVALID; }
    if (kinds && !pk_is_key_type(kind_type, false)) { *why = "the kind column must be of an integer type"; return TSFA_ERR_INVALID; }
    if (values) {
        const void *const some = why;   // (pr_check wants its caller's out_packs; there are none here)
        if (int rc = pr_check(values, value_type, n_rows, n_cols, sr, sc, some, why)) return rc;
    }
    if (t) {
        if (t_type != TSFA_I64 && t_type != TSFA_F64) { *why = "the stamps must be TSFA_I64 (ticks) or TSFA_F64 (seconds)"; return TSFA_ERR_INVALID; }
        if (t_stride < 0) { *why = "negative stride"; return TSFA_ERR_INVALID; }
        if (t_stride && n_rows - 1 > ((int64_t)1 << 60) / t_stride) { *why = "the stride reaches beyond 2^60 elements"; return TSFA_ERR_INVALID; }
    }
    return TSFA_OK;
}

#endif /* TSFA_PACK_ROWS_VALID_H */
