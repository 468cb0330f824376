// Dense packer: kernel bodies of tsfa_pack_dense (include/tsfresh_amd.h).
//
// A batch that already IS an array on the device -- logical shape (n_batch, n_channels, n_time), any non-negative element
// strides, float64 / float32 / float16 / bfloat16 -- becomes the ragged layout tsfa_extract* consumes without a sort:
//     values_out[c * channel_stride_out + offsets[b] + t] = x[b * stride_batch + c * stride_channel + t * stride_time]
// for t < len(b), one int64 offsets array shared by every channel (b * n_time in closed form, or the exclusive scan of the
// clamped lengths), and one flag word.  float16 and bfloat16 become float32 (both conversions are exact), the two wide types
// stay what they are.  Every conversion and every NaN test is integer code on the bit patterns, so the two builds agree.
//
// Like pack_device.h this file is compiled two ways: by hipcc for gfx950 (tsfa_pack_dense.hip wraps every body in a
// __global__ kernel) and by g++ -DTSFA_EMUL with ONE thread per workgroup (tests/emul/emul_pack_dense.cpp drives the same
// bodies work item by work item).  The emulation sees the index arithmetic of the three routes, the tile edges, the clamping
// of the lengths, the scan's carry, the conversions and the flags.  It cannot see what only exists with 64 lanes: the
// wavefront prefix of the scan (one lane's exclusive prefix is always 0), the barriers around the LDS tile and the bank
// behaviour of the tile's pitch.
//
// Routes (pd_route, host):
//   PD_ROUTE_ROWS_UNIT   stride_time == 1: a (batch, channel) row is contiguous; consecutive lanes copy consecutive samples.
//   PD_ROUTE_TRANSPOSE   stride_channel == 1, n_channels > 1 (channels-last): a workgroup reads a [time tile x channel tile]
//                        block with the lanes running along the channels, turns it in an LDS tile, and writes every
//                        channel's run with the lanes running along time.  Both sides of HBM see unit-stride lanes.
//   PD_ROUTE_ROWS        anything else: the rows kernel with the time stride multiplied in (a gather, uncoalesced by nature).
//
// The unit-stride rows route moves 16 bytes of input per lane and step -- 4 float32 (one 16-byte store), 8 halves (two 16-byte
// stores), 4 float64 as 2 x 16 bytes -- for every work item whose source and destination addresses are both aligned to that:
// every row of a dense batch whose n_time is a multiple of 4 (8 for the half types).  Otherwise (ragged offsets, odd views),
// and for the tail of a row, it moves one sample per lane.
//
// The LDS tile of the transpose route holds PD_TILE_CELLS = 2048 samples: tile_c channels x tile_t time steps, tile_c the
// power of two in [2, 32] that holds n_channels (32 beyond), tile_t = 2048 / tile_c (64 .. 1024) -- a recording of 8 channels
// is turned in tiles of 8 x 256, so a workgroup moves 8 samples per thread between two barriers whatever the channel count.
// The tile is tile_c rows (channels) of `pitch` 32-bit words, pitch = tile_t + pad.  Only 32-bit LDS accesses are issued (a
// float64 sample is kept as two words in two planes), so for every access the bank of byte address a is (a / 4) % 32 and
// lanes conflict only inside their 32-lane half (the CDNA4 rule for ds_write_b32 / ds_read_b32: the LDS serves a wavefront's
// 32-bit access in two groups of 32 lanes, 32 banks of 4 bytes each; equal addresses broadcast, every further distinct address on
// a bank costs the group one more cycle).
//   write (lane k of the block: t = k / cw, c = k % cw, cw = channels of this tile): word c * pitch + t.  tile_t is a
//     multiple of 32, so the bank is (c * pad + t) % 32.  pad = ceil(32 / cw) (1 for a full tile of 32 channels) spreads the
//     cw channels of one time step over the bank row: with cw a power of two a 32-lane half holds cw channels x 32 / cw
//     consecutive time steps and c * (32 / cw) + t is a different bank for each: conflict-free (degree 1).  Any other cw (the
//     last channel tile; 3, 5, 6, 7 ... channels in all), and a half that straddles a tile row in the last partial tile, is at
//     most 2-way.  (pitch = tile_t alone would put the cw channels of a time step on ONE bank: cw-way.)
//   read (lane k: c = k / tw, t = k % tw, tw = time steps of this tile): consecutive lanes read consecutive words:
//     conflict-free, 2-way only where a half straddles two rows of a partial tile.
//
// Determinism and progress: no workgroup waits on a word another workgroup writes.  The scan of the lengths is ONE workgroup
// with a 64-bit running carry (pd_scan_lengths_body); the only atomic is the OR into the flag word.
//
// Bounds: the lengths are clamped into [0, n_time] BEFORE the scan, the copy kernels read the lengths back as differences of
// the scanned offsets, so whatever `lengths` holds no sample outside x is read and none outside [0, sum of the clamped
// lengths) <= n_batch * n_time <= channel_stride_out is written.
#ifndef TSFA_PACK_DENSE_H
#define TSFA_PACK_DENSE_H

#include "pack_device.h"

#define PD_THREADS 256                       /* the copy kernels: four wavefronts */
#define PD_ROW_CHUNK 1024                    /* samples of one (batch, channel) row per work item of the rows routes */
#define PD_VEC 4                             /* samples per lane and step of the aligned unit-stride copy; 2 * PD_VEC of a half type */
#define PD_TILE_CELLS 2048                   /* samples of one LDS tile: tile_c channels x tile_t time steps */
#define PD_TILE_C 32                         /* most channels of one LDS tile (tile_c: a power of two, 2 .. 32) */
#define PD_TILE_WORDS (PD_TILE_CELLS + 32 * PD_TILE_C)   /* per plane, pad <= 32 per row; float64 uses two planes: 24 KiB */
#define PD_SCAN_THREADS 1024                 /* the single workgroup of the length scan */
#define PD_MAX_GRID 65536                    /* workgroups of a copy launch; the work items beyond are taken by striding */
#define PD_MAX_LEN 33554431ll                /* tsfa_extract*'s longest series */

enum { PD_ROUTE_ROWS_UNIT = 0, PD_ROUTE_TRANSPOSE = 1, PD_ROUTE_ROWS = 2 };

struct PdArgs {
    const void *x;
    int64_t n_batch, n_channels, n_time;
    int64_t sb, sc, st;          // element strides of x
    const int64_t *offsets;      // n_batch + 1 (written before the copy kernel runs)
    int uniform;                 // no lengths: offsets[b] = b * n_time, not read
    void *out;
    int64_t cso;                 // channel_stride_out
    unsigned int *flags;
    int64_t n_work;              // work items of the route
    int64_t per_row;             // rows routes: chunks per row; transpose: time tiles
    int64_t tiles_c;             // transpose: channel tiles
    int tile_c, tile_t;          // transpose: channels and time steps of a tile (pd_tile_c), tile_c * tile_t = PD_TILE_CELLS
};

// ---- element types ----
PK_HD int pd_in_size(int type) {
    switch (type) {
    case TSFA_F64: return 8;
    case TSFA_F32: return 4;
    case TSFA_F16: case TSFA_BF16: return 2;
    default: return 0;
    }
}
PK_HD int pd_out_type(int type) { return type == TSFA_F64 ? TSFA_F64 : TSFA_F32; }

// binary16 -> binary32, exact: every half value (subnormals included) is a float; a NaN keeps its sign and its payload
// (shifted), +-inf stays +-inf
PK_HD uint32_t pd_f16_to_f32_bits(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 31u, man = h & 0x3ffu;
    if (exp == 31u) return sign | 0x7f800000u | (man << 13);
    if (exp == 0u) {
        if (man == 0u) return sign;
        // subnormal: man * 2^-24.  Shift the leading one up to bit 10; every shift lowers the exponent by one from 2^-14
        exp = 113u;
        while (!(man & 0x400u)) { man <<= 1; --exp; }
        return sign | (exp << 23) | ((man & 0x3ffu) << 13);
    }
    return sign | ((exp + 112u) << 23) | (man << 13);
}
// bfloat16 IS the upper half of a binary32
PK_HD uint32_t pd_bf16_to_f32_bits(uint32_t h) { return h << 16; }

// Element i of x as the bit pattern of its output type (float32 in the low word, or float64); *nan is raised for a NaN.
template <int TYPE>
TSFA_DEV pk_u64 pd_load(const void *x, int64_t i, bool *nan) {
    if (TYPE == TSFA_F64) {
        const pk_u64 u = ((const pk_u64 *)x)[i];
        if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) *nan = true;
        return u;
    }
    uint32_t u;
    if (TYPE == TSFA_F32) u = ((const uint32_t *)x)[i];
    else if (TYPE == TSFA_F16) u = pd_f16_to_f32_bits(((const uint16_t *)x)[i]);
    else u = pd_bf16_to_f32_bits(((const uint16_t *)x)[i]);
    if ((u & 0x7fffffffu) > 0x7f800000u) *nan = true;
    return (pk_u64)u;
}
template <int TYPE>
TSFA_DEV void pd_store(void *out, int64_t i, pk_u64 bits) {
    if (TYPE == TSFA_F64) ((pk_u64 *)out)[i] = bits;
    else ((uint32_t *)out)[i] = (uint32_t)bits;
}

// first sample and length of series b in every channel's stretch of the output
TSFA_DEV void pd_series(const PdArgs &a, int64_t b, int64_t *off, int64_t *len) {
    if (a.uniform) {
        *off = b * a.n_time;
        *len = a.n_time;
    } else {
        *off = a.offsets[b];
        *len = a.offsets[b + 1] - *off;
    }
}

// ---------------------------------------------------------------------------------------------
// 1a. offsets without lengths: offsets[b] = b * n_time for b = 0 .. n_batch   (grid-stride)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void pd_offsets_body(const PkBlk &b, int64_t first, int64_t stride, int64_t n_batch, int64_t n_time, int64_t *offsets) {
    for (int64_t i = first + b.tid; i <= n_batch; i += stride) offsets[i] = i * n_time;
}

// exclusive prefix of v over the lower-numbered threads of the workgroup, and the workgroup total (`ws`: 16 pk_u64 of LDS)
TSFA_DEV pk_u64 pd_blk_excl_sum64(const PkBlk &b, pk_u64 v, pk_u64 *ws, pk_u64 *total) {
#if TSFA_GPU
    const int lane = b.tid & 63, w = b.tid >> 6, nw = (b.nt + 63) >> 6;
    pk_u64 inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const pk_u64 t = __shfl_up(inc, s);
        if (lane >= s) inc += t;
    }
    pk_sync();  // ws of the previous call has been read by everyone
    if (lane == 63 || b.tid == b.nt - 1) ws[w] = inc;
    pk_sync();
    pk_u64 base = 0, all = 0;
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

// a length as the copy kernels may use it: inside [0, n_time]; *bad is raised for one outside [1, n_time]
TSFA_DEV int64_t pd_load_length(const void *lengths, int type, int64_t i, int64_t n_time, bool *bad) {
    const int64_t v = type == TSFA_I32 ? (int64_t)((const int32_t *)lengths)[i] : ((const int64_t *)lengths)[i];
    if (v < 1 || v > n_time) *bad = true;
    return v < 0 ? 0 : (v > n_time ? n_time : v);
}

// ---------------------------------------------------------------------------------------------
// 1b. offsets = exclusive scan of the clamped lengths, by ONE workgroup, 64 bits wide: four consecutive lengths per thread
//     and step, the running total carried from step to step in a register every thread holds.  offsets[n_batch] = total.
// ---------------------------------------------------------------------------------------------
TSFA_DEV void pd_scan_lengths_body(const PkBlk &b, const void *lengths, int type, int64_t n_batch, int64_t n_time,
                                   int64_t *offsets, pk_u64 *ws, unsigned int *flags) {
    pk_u64 carry = 0;
    bool bad = false;
    for (int64_t base = 0; base < n_batch; base += (int64_t)b.nt * 4) {
        const int64_t i0 = base + (int64_t)b.tid * 4;
        pk_u64 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i0 + k < n_batch) ? (pk_u64)pd_load_length(lengths, type, i0 + k, n_time, &bad) : 0ull;
        pk_u64 tot;
        pk_u64 run = carry + pd_blk_excl_sum64(b, v[0] + v[1] + v[2] + v[3], ws, &tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < n_batch) offsets[i0 + k] = (int64_t)run;
            run += v[k];
        }
        carry += tot;
    }
    if (b.tid == 0) offsets[n_batch] = (int64_t)carry;
    if (bad) pk_or32(flags, (unsigned int)TSFA_DENSE_BAD_LENGTH);
}

// ---------------------------------------------------------------------------------------------
// 2. the rows routes.  Work item w = ((batch * n_channels) + channel) * per_row + chunk: PD_ROW_CHUNK samples of one row.
//    UNIT: stride_time == 1 is known at compile time (the loads of a wavefront are one contiguous stretch).
// ---------------------------------------------------------------------------------------------
// What one lane moves in one step of the aligned copy: pd_vec<TYPE>() samples.
struct __attribute__((aligned(16), may_alias)) PdW4 { uint32_t w[4]; };
template <int TYPE>
PK_HD int pd_vec() { return (TYPE == TSFA_F16 || TYPE == TSFA_BF16) ? 2 * PD_VEC : PD_VEC; }

TSFA_DEV bool pd_nan64(uint32_t lo, uint32_t hi) {
    hi &= 0x7fffffffu;
    return hi > 0x7ff00000u || (hi == 0x7ff00000u && lo != 0u);
}

// samples [t, t + pd_vec<TYPE>()) of a unit-stride row, converted; src / dst: element indices of sample t
template <int TYPE>
TSFA_DEV void pd_copy_vec(const PdArgs &a, int64_t src, int64_t dst, bool *nan) {
    if (TYPE == TSFA_F64) {
        const PdW4 *p = (const PdW4 *)((const pk_u64 *)a.x + src);
        PdW4 *q = (PdW4 *)((pk_u64 *)a.out + dst);
        const PdW4 lo = p[0], hi = p[1];
        if (pd_nan64(lo.w[0], lo.w[1]) || pd_nan64(lo.w[2], lo.w[3]) || pd_nan64(hi.w[0], hi.w[1]) || pd_nan64(hi.w[2], hi.w[3])) *nan = true;
        q[0] = lo;
        q[1] = hi;
    } else if (TYPE == TSFA_F32) {
        const PdW4 v = *(const PdW4 *)((const uint32_t *)a.x + src);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((v.w[k] & 0x7fffffffu) > 0x7f800000u) *nan = true;
        *(PdW4 *)((uint32_t *)a.out + dst) = v;
    } else {
        const PdW4 h = *(const PdW4 *)((const uint16_t *)a.x + src);   // 8 halves
        PdW4 *q = (PdW4 *)((uint32_t *)a.out + dst);
        PdW4 v[2];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t bits = (h.w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
            const uint32_t f = TYPE == TSFA_F16 ? pd_f16_to_f32_bits(bits) : pd_bf16_to_f32_bits(bits);
            if ((f & 0x7fffffffu) > 0x7f800000u) *nan = true;
            v[k >> 2].w[k & 3] = f;
        }
        q[0] = v[0];
        q[1] = v[1];
    }
}

template <int TYPE, bool UNIT>
TSFA_DEV void pd_rows_body(const PkBlk &b, int64_t first, int64_t stride, const PdArgs &a) {
    bool nan = false;
    const int isz = TYPE == TSFA_F64 ? 8 : (TYPE == TSFA_F32 ? 4 : 2), osz = TYPE == TSFA_F64 ? 8 : 4;
    for (int64_t w = first; w < a.n_work; w += stride) {
        const int64_t row = w / a.per_row, chunk = w - row * a.per_row;
        const int64_t bb = row / a.n_channels, c = row - bb * a.n_channels;
        int64_t off, len;
        pd_series(a, bb, &off, &len);
        int64_t t0 = chunk * PD_ROW_CHUNK;
        if (t0 >= len) continue;
        const int64_t t1 = t0 + PD_ROW_CHUNK < len ? t0 + PD_ROW_CHUNK : len;
        const int64_t src = bb * a.sb + c * a.sc, dst = c * a.cso + off;
        if (UNIT) {
            // both sides aligned to what a lane moves in one step (the same for the whole work item): the bulk goes in
            // 16-byte accesses, the scalar loop below takes what is left of the chunk
            const pk_u64 sa = (pk_u64)(uintptr_t)a.x + (pk_u64)(src + t0) * isz, da = (pk_u64)(uintptr_t)a.out + (pk_u64)(dst + t0) * osz;
            const int vec = pd_vec<TYPE>();
            if (sa % (vec * isz) == 0 && da % (vec * osz) == 0) {
                const int64_t nq = (t1 - t0) / vec;
                for (int64_t q = b.tid; q < nq; q += b.nt) pd_copy_vec<TYPE>(a, src + t0 + q * vec, dst + t0 + q * vec, &nan);
                t0 += nq * vec;
            }
        }
        for (int64_t t = t0 + b.tid; t < t1; t += b.nt)
            pd_store<TYPE>(a.out, dst + t, pd_load<TYPE>(a.x, src + (UNIT ? t : t * a.st), &nan));
    }
    if (nan) pk_or32(a.flags, (unsigned int)TSFA_PACK_VALUE_NAN);
}

// pad of the LDS tile's pitch for a tile of cw channels (see the head of this file)
PK_HD int pd_tile_pad(int cw) { return cw >= 32 ? 1 : (32 + cw - 1) / cw; }
// channels of a tile for an array of n_channels: the power of two in [2, PD_TILE_C] that holds them, or PD_TILE_C
PK_HD int pd_tile_c(int64_t n_channels) {
    int tc = 2;
    while (tc < PD_TILE_C && tc < n_channels) tc <<= 1;
    return tc;
}
// log2 of a power of two, -1 for anything else: the cell index of a full tile splits by shift and mask
TSFA_DEV int pd_log2(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int s = 0;
    while ((1 << s) < v) ++s;
    return s;
}

// ---------------------------------------------------------------------------------------------
// 3. the transpose route (stride_channel == 1).  Work item w = ((batch * tiles_c) + channel tile) * per_row + time tile.
//    `tile`: PD_TILE_WORDS uint32 of LDS, twice that for float64 (low words, then high words).
// ---------------------------------------------------------------------------------------------
template <int TYPE>
TSFA_DEV void pd_transpose_body(const PkBlk &b, int64_t first, int64_t stride, const PdArgs &a, uint32_t *tile) {
    bool nan = false;
    uint32_t *const tile_hi = tile + PD_TILE_WORDS;
    for (int64_t w = first; w < a.n_work; w += stride) {
        const int64_t r = w / a.per_row, tt = w - r * a.per_row;
        const int64_t bb = r / a.tiles_c, ct = r - bb * a.tiles_c;
        int64_t off, len;
        pd_series(a, bb, &off, &len);
        const int64_t t0 = tt * a.tile_t;
        if (t0 >= len) continue;   // (w is the same for the whole workgroup: no barrier is skipped by a part of it)
        const int64_t c0 = ct * a.tile_c;
        const int tw = (int)(len - t0 < a.tile_t ? len - t0 : a.tile_t);
        const int cw = (int)(a.n_channels - c0 < a.tile_c ? a.n_channels - c0 : a.tile_c);
        const int pitch = a.tile_t + pd_tile_pad(cw), cells = tw * cw;
        const int cs = pd_log2(cw), ts = pd_log2(tw);
        const int64_t src = bb * a.sb + t0 * a.st + c0;
        pk_sync();  // the previous work item's reads of the tile are done
        for (int k = b.tid; k < cells; k += b.nt) {
            const int t = cs >= 0 ? k >> cs : k / cw, c = k - t * cw;
            const pk_u64 bits = pd_load<TYPE>(a.x, src + (int64_t)t * a.st + c, &nan);
            tile[c * pitch + t] = (uint32_t)bits;
            if (TYPE == TSFA_F64) tile_hi[c * pitch + t] = (uint32_t)(bits >> 32);
        }
        pk_sync();
        for (int k = b.tid; k < cells; k += b.nt) {
            const int c = ts >= 0 ? k >> ts : k / tw, t = k - c * tw;
            pk_u64 bits = tile[c * pitch + t];
            if (TYPE == TSFA_F64) bits |= (pk_u64)tile_hi[c * pitch + t] << 32;
            pd_store<TYPE>(a.out, (c0 + c) * a.cso + off + t0 + t, bits);
        }
    }
    if (nan) pk_or32(a.flags, (unsigned int)TSFA_PACK_VALUE_NAN);
}

// ---------------------------------------------------------------------------------------------
// Host: argument checks and the choice of the route, shared by tsfa_pack_dense and the emulation's driver.
// Returns TSFA_OK or the status tsfa_pack_dense reports, with the reason in *why.
// ---------------------------------------------------------------------------------------------
static inline int pd_check(const void *x, int x_type, int64_t n_batch, int64_t n_channels, int64_t n_time, int64_t sb, int64_t sc,
                           int64_t st, const void *lengths, int lengths_type, const void *values_out, int64_t cso,
                           const void *offsets_out, const void *flags_out, const char **why) {
    *why = "";
    if (!x || !values_out || !offsets_out || !flags_out) { *why = "null pointer"; return TSFA_ERR_INVALID; }
    if (pd_in_size(x_type) == 0) { *why = "the element type must be TSFA_F64, TSFA_F32, TSFA_F16 or TSFA_BF16"; return TSFA_ERR_INVALID; }
    if (lengths && lengths_type != TSFA_I32 && lengths_type != TSFA_I64) { *why = "lengths must be TSFA_I32 or TSFA_I64"; return TSFA_ERR_INVALID; }
    if (n_batch < 1 || n_channels < 1 || n_time < 1) { *why = "a dimension is zero or negative"; return TSFA_ERR_INVALID; }
    if (sb < 0 || sc < 0 || st < 0) { *why = "negative stride"; return TSFA_ERR_INVALID; }
    if (n_time > PD_MAX_LEN) { *why = "more than 33 554 431 samples per series"; return TSFA_ERR_TOO_LONG; }
    // every index below fits int64 with room: n_batch * n_channels * n_time and the largest source index stay under 2^62
    const int64_t lim = (int64_t)1 << 62;
    if (n_batch > lim / n_time || n_batch * n_time > lim / n_channels) { *why = "more than 2^62 samples"; return TSFA_ERR_INVALID; }
    if (cso < n_batch * n_time) { *why = "channel_stride_out is below n_batch * n_time"; return TSFA_ERR_INVALID; }
    if (n_channels > 1 && cso > lim / n_channels) { *why = "channel_stride_out * n_channels exceeds 2^62"; return TSFA_ERR_INVALID; }
    if ((sb && n_batch - 1 > lim / 4 / sb) || (sc && n_channels - 1 > lim / 4 / sc) || (st && n_time - 1 > lim / 4 / st)) {
        *why = "a stride reaches beyond 2^60 elements";
        return TSFA_ERR_INVALID;
    }
    return TSFA_OK;
}

static inline int pd_route(int64_t n_channels, int64_t sc, int64_t st) {
    if (st == 1) return PD_ROUTE_ROWS_UNIT;
    if (sc == 1 && n_channels > 1) return PD_ROUTE_TRANSPOSE;
    return PD_ROUTE_ROWS;
}

// the work items of a route (a.n_work, a.per_row, a.tiles_c)
static inline void pd_plan_work(PdArgs *a, int route) {
    a->tile_c = pd_tile_c(a->n_channels);
    a->tile_t = PD_TILE_CELLS / a->tile_c;
    if (route == PD_ROUTE_TRANSPOSE) {
        a->per_row = (a->n_time + a->tile_t - 1) / a->tile_t;
        a->tiles_c = (a->n_channels + a->tile_c - 1) / a->tile_c;
        a->n_work = a->n_batch * a->tiles_c * a->per_row;
    } else {
        a->per_row = (a->n_time + PD_ROW_CHUNK - 1) / PD_ROW_CHUNK;
        a->tiles_c = 0;
        a->n_work = a->n_batch * a->n_channels * a->per_row;
    }
}

#endif /* TSFA_PACK_DENSE_H */
