// Valid-step packer: kernel bodies of tsfa_pack_dense_valid (include/tsfresh_amd.h).
//
// The dense packer (pack_dense.h) for a batch with gaps: the same array on the device -- logical shape (n_batch, n_channels,
// n_time), any non-negative element strides, float64 / float32 / float16 / bfloat16, optional lengths -- becomes the ragged
// layout tsfa_extract* consumes, WITHOUT the steps a wide frame loses to `dropna()`: step t of series b is dropped for every
// channel when any channel's sample x[b, :, t] is NaN, or (with stamps) when its stamp is NaT (INT64_MIN ticks) or a NaN
// second.  +-inf is a value and stays.  For the kept steps t_0 < t_1 < ... of series b
//     values_out[c * channel_stride_out + offsets[b] + k] = x[b, c, t_k]        (converted as tsfa_pack_dense converts)
//     steps_out[offsets[b] + k] = t_k                                           (the original step index)
//     stamps_out[b * n_time + k] = t[b, t_k]                                    (right-padded (n_batch, n_time), with stamps)
// and offsets[] is the exclusive scan of the kept counts, one array shared by the channels.  The hours of the kept stamps are
// NOT computed here: tsfa_pack_times on (stamps_out, the new offsets) gives them with its own arithmetic.
//
// Three launches, no workgroup waits on another, no atomic but the OR into the flag word, so the result is deterministic:
//   count    a work item is PD_ROW_CHUNK steps of one series (w = batch * per_row + chunk), in PV_ROUNDS rounds of 64 steps;
//            a wavefront takes PV_RPW consecutive rounds.  Every lane tests its step of each round in every channel (and its
//            stamp) -- the loads of the rounds are issued together, channel by channel --, the 64-lane ballot of a round is
//            its keep mask, the population count its kept steps.  The wavefronts exchange their totals through LDS; the
//            masks, the kept steps of the work item BEFORE each round (`pre`) and the work item's count go to scratch, each
//            as vector stores by the first lanes of the wavefront.
//   scan     ONE workgroup turns the counts into their exclusive scan in place -- 64 bits wide, four entries per thread and
//            trip, the running total carried from trip to trip (pd_scan_lengths_body is the model) -- and writes
//            offsets[b] where a work item is chunk 0 of series b, and offsets[n_batch] = the total.
//   compact  the same work items and rounds: a lane whose bit is set writes to
//                base of the work item + pre of the round + population count of the mask below its lane
//            every channel's sample, its step index and its stamp.  The kept lanes of a round write consecutive cells.
//            Chunk 0 of a series whose offsets are equal raises TSFA_DENSE_EMPTY_SERIES.
// The samples are read twice (count, compact); the masks make the second pass independent of the channel count: a lane needs
// no register per channel, and nothing is decided twice.  A lane beyond the end of its series loads the series' last step
// of the chunk instead (an address inside x that some lane reads anyway), so that no load stands behind a branch.
//
// One route serves every layout, with the time stride known at compile time when it is 1 (UNIT): consecutive lanes are on
// consecutive steps, so a unit-stride row is read in contiguous stretches of 64 samples per channel; channels-last reads a
// contiguous stretch of 64 * n_channels samples per round, one channel at a time (the first channel's pass brings the lines
// in, the others hit them in the cache); anything else is a gather.
//
// Scratch (the caller's): PV_SCRATCH_WORDS = 25 words of 8 bytes per work item, n_batch * ceil(n_time / PD_ROW_CHUNK) work
// items: the counts / bases first, then PV_ROUNDS masks per work item, then PV_ROUNDS 32-bit `pre` per work item.
//
// Like pack_dense.h this file is compiled two ways: by hipcc for gfx950 (tsfa_pack_valid.hip wraps every body in a __global__
// kernel of PD_THREADS threads) and by g++ -DTSFA_EMUL (tests/emul/emul_pack_valid.cpp) with ONE thread per workgroup that
// stands for one wavefront, takes all PV_ROUNDS rounds and LOOPS over its 64 lanes (PV_LANES): the vote is the OR of the
// lanes' bits, the prefix the population count below the lane, as on the device.  The emulation sees the index arithmetic,
// the chunk and round edges, the clamping of the lengths and of the loads, the scan's carry, the conversions, the NaN / NaT
// tests and the flags.  It cannot see what only exists with several wavefronts: the hardware ballot, the split of the rounds
// over four wavefronts, the barriers around the count's LDS words and the 1024-thread prefix of the scan (one thread's
// exclusive prefix is always 0).
//
// Bounds: a length is clamped into [0, n_time] wherever it is loaded and a load's step into the chunk's part of the series,
// so no sample or stamp outside the arrays is read whatever `lengths` holds; the kept steps of a series are at most its
// clamped length, so every write stays inside [0, n_batch * n_time) <= channel_stride_out of a channel, of steps_out and of
// stamps_out.
#ifndef TSFA_PACK_VALID_H
#define TSFA_PACK_VALID_H

#include "pack_times.h"

#define PV_ROUNDS (PD_ROW_CHUNK / 64)        /* 64-step rounds of one work item */
#if TSFA_GPU
#define PV_WAVES (PD_THREADS / 64)           /* wavefronts of a workgroup of the count and compact kernels */
#else
#define PV_WAVES 1
#endif
#define PV_RPW (PV_ROUNDS / PV_WAVES)        /* consecutive rounds of one wavefront */
#define PV_SCRATCH_WORDS (1 + PV_ROUNDS + PV_ROUNDS / 2)   /* 8-byte scratch words per work item: count / base, masks, pre */

struct PvArgs {
    const void *x;
    int64_t n_batch, n_channels, n_time;
    int64_t sb, sc, st;          // element strides of x
    const void *lengths;         // NULL: every series has n_time steps
    int lengths_type;
    const void *t;               // NULL: no stamps
    int t_type;                  // TSFA_I64 | TSFA_F64
    int64_t tsb, tst;            // element strides of t
    void *out;
    int64_t cso;                 // channel_stride_out
    int64_t *offsets;            // n_batch + 1
    int32_t *steps;              // [0, T)
    pk_u64 *stamps;              // (n_batch, n_time) right-padded, or NULL
    pk_u64 *base;                // scratch: n_work counts, after the scan the first output cell of each work item
    pk_u64 *masks;               // scratch: n_work * PV_ROUNDS keep masks
    uint32_t *pre;               // scratch: n_work * PV_ROUNDS kept steps of the work item before each round
    unsigned int *flags;
    int64_t n_work, per_row;     // work items; chunks per series
};

// ---- the wavefront as the two builds see it ----
#if TSFA_GPU
#define PV_LANES(lane, b) for (int lane = (b).tid & 63, once_ = 1; once_; once_ = 0)
TSFA_DEV pk_u64 pv_vote(bool keep, int lane) { (void)lane; return __ballot(keep ? 1 : 0); }
TSFA_DEV int pv_popc(pk_u64 m) { return __popcll(m); }
TSFA_DEV int pv_wave(const PkBlk &b) { return b.tid >> 6; }
TSFA_DEV bool pv_lane0(const PkBlk &b) { return (b.tid & 63) == 0; }
#else
#define PV_LANES(lane, b) for (int lane = 0; lane < 64; ++lane)
TSFA_DEV pk_u64 pv_vote(bool keep, int lane) { return keep ? 1ull << lane : 0ull; }
TSFA_DEV int pv_popc(pk_u64 m) { return __builtin_popcountll(m); }
TSFA_DEV int pv_wave(const PkBlk &b) { return b.tid; }
TSFA_DEV bool pv_lane0(const PkBlk &b) { (void)b; return true; }
#endif

TSFA_DEV int64_t pv_length(const PvArgs &a, int64_t bb, bool *bad) {
    return a.lengths ? pd_load_length(a.lengths, a.lengths_type, bb, a.n_time, bad) : a.n_time;
}

// ---------------------------------------------------------------------------------------------
// 1. count: the keep masks and `pre` of every round and the kept steps of every work item.  `ws`: PV_WAVES words of LDS.
// ---------------------------------------------------------------------------------------------
template <int TYPE, bool UNIT>
TSFA_DEV void pv_count_body(const PkBlk &b, int64_t first, int64_t stride, const PvArgs &a, unsigned int *ws) {
    bool bad = false;
    const int wave = pv_wave(b);
    for (int64_t w = first; w < a.n_work; w += stride) {
        const int64_t bb = w / a.per_row, chunk = w - bb * a.per_row;
        const int64_t len = pv_length(a, bb, &bad);
        const int64_t t0 = chunk * PD_ROW_CHUNK;
        const int64_t t1 = t0 + PD_ROW_CHUNK < len ? t0 + PD_ROW_CHUNK : len;
        if (t0 >= t1) {   // nothing of the series lies in this chunk (w is the same for the whole workgroup)
            if (b.tid == 0) a.base[w] = 0;
            continue;
        }
        const int64_t tw = t0 + (int64_t)wave * PV_RPW * 64;   // the wavefront's first step
        pk_u64 m[PV_RPW];
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) m[j] = 0;
        PV_LANES(lane, b) {
            bool nan[PV_RPW];
            int64_t tj[PV_RPW];
#pragma unroll
            for (int j = 0; j < PV_RPW; ++j) {
                const int64_t t = tw + j * 64 + lane;
                tj[j] = t < t1 ? t : t1 - 1;   // a lane beyond the end loads the last step: no load behind a branch
                nan[j] = false;
            }
            for (int64_t c = 0; c < a.n_channels; ++c) {
                const int64_t src = bb * a.sb + c * a.sc;
#pragma unroll
                for (int j = 0; j < PV_RPW; ++j) (void)pd_load<TYPE>(a.x, src + (UNIT ? tj[j] : tj[j] * a.st), &nan[j]);
            }
            if (a.t) {
#pragma unroll
                for (int j = 0; j < PV_RPW; ++j)
                    if (pt_missing(a.t_type, ((const pk_u64 *)a.t)[bb * a.tsb + tj[j] * a.tst])) nan[j] = true;
            }
#pragma unroll
            for (int j = 0; j < PV_RPW; ++j) m[j] |= pv_vote(!nan[j] && tw + j * 64 + lane < t1, lane);
        }
        unsigned int cnt = 0;
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) cnt += (unsigned int)pv_popc(m[j]);
        pk_sync();  // ws of the previous work item has been read
        if (pv_lane0(b)) ws[wave] = cnt;
        pk_sync();
        unsigned int before = 0, all = 0;   // kept steps of the wavefronts below this one, and of the work item
#pragma unroll
        for (int k = 0; k < PV_WAVES; ++k) {
            if (k < wave) before += ws[k];
            all += ws[k];
        }
        // lane j < PV_RPW of the wavefront stores round j's mask and pre (vector stores, PV_RPW lanes wide)
        PV_LANES(lane, b) {
            if (lane >= PV_RPW) continue;
            pk_u64 mine = 0;
            unsigned int pre = before;
#pragma unroll
            for (int j = 0; j < PV_RPW; ++j) {
                if (j == lane) mine = m[j];
                if (j < lane) pre += (unsigned int)pv_popc(m[j]);
            }
            const int64_t r = w * PV_ROUNDS + wave * PV_RPW + lane;
            a.masks[r] = mine;
            a.pre[r] = pre;
        }
        if (b.tid == 0) a.base[w] = all;
    }
    if (bad) pk_or32(a.flags, (unsigned int)TSFA_DENSE_BAD_LENGTH);
}

// ---------------------------------------------------------------------------------------------
// 2. scan: base[] becomes its exclusive scan in place, by ONE workgroup, 64 bits wide; offsets[b] = base[b * per_row],
//    offsets[n_batch] = the total.  `ws`: 16 pk_u64 of LDS.
// ---------------------------------------------------------------------------------------------
TSFA_DEV void pv_scan_body(const PkBlk &b, const PvArgs &a, pk_u64 *ws) {
    pk_u64 carry = 0;
    for (int64_t s = 0; s < a.n_work; s += (int64_t)b.nt * 4) {
        const int64_t i0 = s + (int64_t)b.tid * 4;
        pk_u64 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i0 + k < a.n_work) ? a.base[i0 + k] : 0ull;
        pk_u64 tot;
        pk_u64 run = carry + pd_blk_excl_sum64(b, v[0] + v[1] + v[2] + v[3], ws, &tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < a.n_work) {
                a.base[i0 + k] = run;
                const int64_t bb = (i0 + k) / a.per_row;
                if (bb * a.per_row == i0 + k) a.offsets[bb] = (int64_t)run;
            }
            run += v[k];
        }
        carry += tot;
    }
    if (b.tid == 0) a.offsets[a.n_batch] = (int64_t)carry;
}

// ---------------------------------------------------------------------------------------------
// 3. compact: every kept step's samples, step index and stamp go to their cells.
// ---------------------------------------------------------------------------------------------
template <int TYPE, bool UNIT>
TSFA_DEV void pv_compact_body(const PkBlk &b, int64_t first, int64_t stride, const PvArgs &a) {
    bool ignored = false;
    const int wave = pv_wave(b);
    for (int64_t w = first; w < a.n_work; w += stride) {
        const int64_t bb = w / a.per_row, chunk = w - bb * a.per_row;
        const int64_t row0 = a.offsets[bb];
        if (chunk == 0 && b.tid == 0 && a.offsets[bb + 1] == row0) pk_or32(a.flags, (unsigned int)TSFA_DENSE_EMPTY_SERIES);
        const int64_t len = pv_length(a, bb, &ignored);
        const int64_t t0 = chunk * PD_ROW_CHUNK;
        const int64_t t1 = t0 + PD_ROW_CHUNK < len ? t0 + PD_ROW_CHUNK : len;
        if (t0 >= t1) continue;   // (the count pass wrote no mask for this work item)
        const int64_t dst0 = (int64_t)a.base[w];
        const int64_t tw = t0 + (int64_t)wave * PV_RPW * 64, r0 = w * PV_ROUNDS + wave * PV_RPW;
        pk_u64 m[PV_RPW];
        int64_t d0[PV_RPW];
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) {
            m[j] = a.masks[r0 + j];
            d0[j] = dst0 + (int64_t)a.pre[r0 + j];
        }
        PV_LANES(lane, b) {
            bool keep[PV_RPW];
            int64_t tj[PV_RPW], d[PV_RPW];
#pragma unroll
            for (int j = 0; j < PV_RPW; ++j) {
                const int64_t t = tw + j * 64 + lane;
                tj[j] = t < t1 ? t : t1 - 1;   // (as in the count pass; such a lane's bit is not set)
                keep[j] = (m[j] >> lane) & 1ull;
                d[j] = d0[j] + pv_popc(m[j] & ((1ull << lane) - 1ull));
            }
            for (int64_t c = 0; c < a.n_channels; ++c) {
                const int64_t src = bb * a.sb + c * a.sc, dst = c * a.cso;
                pk_u64 v[PV_RPW];
#pragma unroll
                for (int j = 0; j < PV_RPW; ++j) v[j] = pd_load<TYPE>(a.x, src + (UNIT ? tj[j] : tj[j] * a.st), &ignored);
#pragma unroll
                for (int j = 0; j < PV_RPW; ++j)
                    if (keep[j]) pd_store<TYPE>(a.out, dst + d[j], v[j]);
            }
#pragma unroll
            for (int j = 0; j < PV_RPW; ++j)
                if (keep[j]) a.steps[d[j]] = (int32_t)tj[j];
            if (a.t) {
                pk_u64 s[PV_RPW];
#pragma unroll
                for (int j = 0; j < PV_RPW; ++j) s[j] = ((const pk_u64 *)a.t)[bb * a.tsb + tj[j] * a.tst];
#pragma unroll
                for (int j = 0; j < PV_RPW; ++j)
                    if (keep[j]) a.stamps[bb * a.n_time + (d[j] - row0)] = s[j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Host: argument checks and the work items, shared by tsfa_pack_dense_valid and the emulation's driver.
// Returns TSFA_OK or the status tsfa_pack_dense_valid reports, with the reason in *why.
// ---------------------------------------------------------------------------------------------
static inline int64_t pv_per_row(int64_t n_time) { return (n_time + PD_ROW_CHUNK - 1) / PD_ROW_CHUNK; }

static inline int pv_check(const void *x, int x_type, int64_t n_batch, int64_t n_channels, int64_t n_time, int64_t sb, int64_t sc,
                           int64_t st, const void *lengths, int lengths_type, const void *t, int t_type, int64_t tsb, int64_t tst,
                           const void *values_out, int64_t cso, const void *offsets_out, const void *steps_out,
                           const void *stamps_out, const void *scratch, int64_t scratch_bytes, const void *flags_out,
                           const char **why) {
    if (int rc = pd_check(x, x_type, n_batch, n_channels, n_time, sb, sc, st, lengths, lengths_type, values_out, cso, offsets_out,
                          flags_out, why))
        return rc;
    if (!steps_out || !scratch) { *why = "null pointer"; return TSFA_ERR_INVALID; }
    if ((uintptr_t)scratch % 8) { *why = "scratch must be aligned to 8 bytes"; return TSFA_ERR_INVALID; }
    if (t) {
        if (t_type != TSFA_I64 && t_type != TSFA_F64) { *why = "the stamps must be TSFA_I64 (ticks) or TSFA_F64 (seconds)"; return TSFA_ERR_INVALID; }
        if (!stamps_out) { *why = "stamps without stamps_out"; return TSFA_ERR_INVALID; }
        if (tsb < 0 || tst < 0) { *why = "negative stride"; return TSFA_ERR_INVALID; }
        const int64_t lim = (int64_t)1 << 62;
        if ((tsb && n_batch - 1 > lim / 4 / tsb) || (tst && n_time - 1 > lim / 4 / tst)) {
            *why = "a stride reaches beyond 2^60 elements";
            return TSFA_ERR_INVALID;
        }
    }
    // n_batch * n_time < 2^62 (pd_check), so the product below cannot overflow
    if (scratch_bytes < n_batch * pv_per_row(n_time) * PV_SCRATCH_WORDS * 8) {
        *why = "scratch_bytes is below 200 * n_batch * ceil(n_time / 1024)";
        return TSFA_ERR_INVALID;
    }
    return TSFA_OK;
}

// the work items and the three parts of the scratch (a.n_work, a.per_row, a.base, a.masks, a.pre)
static inline void pv_plan_work(PvArgs *a, void *scratch) {
    a->per_row = pv_per_row(a->n_time);
    a->n_work = a->n_batch * a->per_row;
    a->base = (pk_u64 *)scratch;
    a->masks = a->base + a->n_work;
    a->pre = (uint32_t *)(a->masks + a->n_work * PV_ROUNDS);
}

#endif /* TSFA_PACK_VALID_H */
