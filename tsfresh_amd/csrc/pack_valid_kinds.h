// Per-kind valid-step packer: kernel bodies of tsfa_pack_dense_valid_kinds (include/tsfresh_amd.h).
//
// The valid-step packer (pack_valid.h) for a multi-rate batch: the same array, strides, element types, lengths and stamps,
// but every (kind, series) pair keeps ITS OWN steps -- what the LONG frame of the batch holds after `dropna()`, where each
// (id, kind) group has its own length.  Step t of (b, c) is dropped when x[b, c, t] is NaN or (with stamps) when the stamp
// t[b, t] is NaT / a NaN second; the stamp belongs to the step, so such a step goes for every kind.  +-inf stays.  For the
// kept steps t_0 < t_1 < ... of (b, c), with off = offsets[c * (n_batch + 1) + b]
//     values_out[c * channel_stride_out + off + k] = x[b, c, t_k]                  (converted as tsfa_pack_dense converts)
//     steps_out[c * n_batch * n_time + off + k]    = t_k
//     stamps_out[(c * n_batch + b) * n_time + k]   = t[b, t_k]                      (right-padded, with stamps)
// Every kind has its own n_batch + 1 offsets that start at 0: kind c is then a channel of tsfa_pack_dense with its own
// offsets array, and tsfa_pack_times on (stamps_out of c, offsets of c) gives its hours.
//
// Three launches, no workgroup waits on another, no atomic but the OR into the flag word:
//   count    a work item is PD_ROW_CHUNK = 1024 steps of ONE (kind, series) row, kind-major: w = (c * n_batch + b) * per_row
//            + chunk, so a kind's work items, counts and bases are contiguous.  pack_valid.h's rounds: 64 steps per ballot,
//            PV_RPW rounds per wavefront of a PD_THREADS workgroup, the loads of a wavefront's rounds issued together, the
//            time stride a compile-time 1 when it is 1; a lane beyond the end re-loads the last step, so no load stands
//            behind a branch.  A lane reads one channel only, so nothing loops over the kinds.  The masks, the kept
//            samples before each round (`pre`) and the work item's count go to scratch as there.
//   scan     one workgroup PER KIND runs pack_valid.h's scan (pv_scan_body) on the kind's stretch of `base` and writes the
//            kind's offsets.
//   compact  the same work items: a kept sample goes to base + pre + the population count of its round's mask below the
//            lane, its step index and stamp with it: the kept lanes of a round write consecutive cells.  Chunk 0 of a
//            (kind, series) whose offsets are equal raises TSFA_DENSE_EMPTY_SERIES.
// A second route for aligned unit-stride rows -- a lane owning the samples of one 16-byte load, one ballot per sub-step --
// was built and measured: its count pass took the time of this one and its compaction 1.6 times as long for the same
// bytes, so it is not here (profiles/dropna_kinds_timing.md; the route is profiles/lab/pack_valid_kinds_vector_route.patch).
//
// Scratch: pack_valid.h's layout (PV_SCRATCH_WORDS words per work item) for n_channels * n_batch rows.
//
// Bounds: a length is clamped into [0, n_time] wherever it is loaded and a load's step into the chunk's part of the series,
// so no sample or stamp outside the arrays is read whatever `lengths` holds.  The kept steps of a row are at most its
// clamped length, so every write stays inside [0, n_batch * n_time) <= channel_stride_out of its kind, of the kind's
// stretch of steps_out and of the row's stretch of stamps_out.
//
// Device code only: there is no g++ build of these bodies (tests/test_pack_valid_kinds_gpu.py holds them to the rule).
#ifndef TSFA_PACK_VALID_KINDS_H
#define TSFA_PACK_VALID_KINDS_H

#include "pack_valid.h"

// ---- the work item ----
struct PvkItem {
    int64_t c, bb;               // kind, series
    int64_t t0, t1;              // its steps of the series: [t0, t1), t1 <= the clamped length
    int64_t src, trow;           // element index of x[bb, c, 0] and of t[bb, 0]
};
// false: nothing of the series lies in the chunk (the same answer for the whole workgroup)
TSFA_DEV bool pvk_item(const PvArgs &a, int64_t w, bool *bad, PvkItem *it) {
    const int64_t row = w / a.per_row, chunk = w - row * a.per_row;
    it->c = row / a.n_batch;
    it->bb = row - it->c * a.n_batch;
    const int64_t len = pv_length(a, it->bb, bad);
    it->t0 = chunk * PD_ROW_CHUNK;
    it->t1 = it->t0 + PD_ROW_CHUNK < len ? it->t0 + PD_ROW_CHUNK : len;
    it->src = it->bb * a.sb + it->c * a.sc;
    it->trow = it->bb * a.tsb;
    return it->t0 < it->t1;
}
TSFA_DEV pk_u64 pvk_stamp(const PvArgs &a, const PvkItem &it, int64_t t) {   // t clamped into [t0, t1) by the caller
    return ((const pk_u64 *)a.t)[it.trow + t * a.tst];
}

// ---------------------------------------------------------------------------------------------
// 1. count: the keep masks and `pre` of every round and the kept steps of every work item.  `ws`: one word of LDS per
//    wavefront.
// ---------------------------------------------------------------------------------------------
template <int TYPE, bool UNIT>
TSFA_DEV void pvk_count_body(const PkBlk &b, int64_t first, int64_t stride, const PvArgs &a, unsigned int *ws) {
    bool bad = false;
    const int wave = b.tid >> 6, lane = b.tid & 63;
    for (int64_t w = first; w < a.n_work; w += stride) {
        PvkItem it;
        if (!pvk_item(a, w, &bad, &it)) {
            if (b.tid == 0) a.base[w] = 0;
            continue;
        }
        const int64_t tw = it.t0 + (int64_t)wave * PV_RPW * 64 + lane;   // the lane's step of the wavefront's first round
        bool nan[PV_RPW];
        int64_t tj[PV_RPW];
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) {
            const int64_t t = tw + j * 64;
            tj[j] = t < it.t1 ? t : it.t1 - 1;   // a lane beyond the end loads the last step: no load behind a branch
            nan[j] = false;
        }
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) (void)pd_load<TYPE>(a.x, it.src + (UNIT ? tj[j] : tj[j] * a.st), &nan[j]);
        if (a.t) {
#pragma unroll
            for (int j = 0; j < PV_RPW; ++j)
                if (pt_missing(a.t_type, pvk_stamp(a, it, tj[j]))) nan[j] = true;
        }
        pk_u64 m[PV_RPW];
        unsigned int cnt = 0;
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) {
            m[j] = pv_vote(!nan[j] && tw + j * 64 < it.t1, lane);
            cnt += (unsigned int)pv_popc(m[j]);
        }
        pk_sync();  // ws of the previous work item has been read
        if (lane == 0) ws[wave] = cnt;
        pk_sync();
        unsigned int before = 0, all = 0;   // kept steps of the wavefronts below this one, and of the work item
#pragma unroll
        for (int k = 0; k < PV_WAVES; ++k) {
            if (k < wave) before += ws[k];
            all += ws[k];
        }
        if (lane < PV_RPW) {   // lane j stores round j's mask and pre: vector stores, PV_RPW lanes wide
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
// 2. scan of kind c: pv_scan_body on the kind's stretch of `base` and its own offsets.  `ws`: 16 pk_u64 of LDS.
// ---------------------------------------------------------------------------------------------
TSFA_DEV void pvk_scan_body(const PkBlk &b, int64_t c, const PvArgs &a, pk_u64 *ws) {
    PvArgs k = a;
    k.n_work = a.n_batch * a.per_row;
    k.base = a.base + c * k.n_work;
    k.offsets = a.offsets + c * (a.n_batch + 1);
    pv_scan_body(b, k, ws);
}

// ---------------------------------------------------------------------------------------------
// 3. compact: every kept sample, its step index and its stamp go to their cells of the kind.
// ---------------------------------------------------------------------------------------------
template <int TYPE, bool UNIT>
TSFA_DEV void pvk_compact_body(const PkBlk &b, int64_t first, int64_t stride, const PvArgs &a) {
    bool ignored = false;
    const int wave = b.tid >> 6, lane = b.tid & 63;
    for (int64_t w = first; w < a.n_work; w += stride) {
        PvkItem it;
        const bool any = pvk_item(a, w, &ignored, &it);
        const int64_t *offs = a.offsets + it.c * (a.n_batch + 1) + it.bb;
        const int64_t row0 = offs[0];
        if (it.t0 == 0 && b.tid == 0 && offs[1] == row0) pk_or32(a.flags, (unsigned int)TSFA_DENSE_EMPTY_SERIES);
        if (!any) continue;   // (the count pass wrote no mask for this work item)
        const int64_t dst0 = (int64_t)a.base[w], r0 = w * PV_ROUNDS + wave * PV_RPW;
        const int64_t tw = it.t0 + (int64_t)wave * PV_RPW * 64 + lane;
        bool keep[PV_RPW];
        int64_t tj[PV_RPW], d[PV_RPW];
        pk_u64 v[PV_RPW], s[PV_RPW];
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) {
            const pk_u64 m = a.masks[r0 + j];
            const int64_t t = tw + j * 64;
            tj[j] = t < it.t1 ? t : it.t1 - 1;   // (as in the count pass; such a lane's bit is not set)
            keep[j] = (m >> lane) & 1ull;
            d[j] = dst0 + (int64_t)a.pre[r0 + j] + pv_popc(m & ((1ull << lane) - 1ull));
        }
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) v[j] = pd_load<TYPE>(a.x, it.src + (UNIT ? tj[j] : tj[j] * a.st), &ignored);
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) s[j] = a.t ? pvk_stamp(a, it, tj[j]) : 0ull;
#pragma unroll
        for (int j = 0; j < PV_RPW; ++j) {
            if (!keep[j]) continue;
            pd_store<TYPE>(a.out, it.c * a.cso + d[j], v[j]);
            a.steps[it.c * a.n_batch * a.n_time + d[j]] = (int32_t)tj[j];
            if (a.t) a.stamps[(it.c * a.n_batch + it.bb) * a.n_time + (d[j] - row0)] = s[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Host: argument checks and the work items.  Returns TSFA_OK or the status the entry reports, with the reason in *why.
// ---------------------------------------------------------------------------------------------
static inline int pvk_check(const void *x, int x_type, int64_t n_batch, int64_t n_channels, int64_t n_time, int64_t sb, int64_t sc,
                            int64_t st, const void *lengths, int lengths_type, const void *t, int t_type, int64_t tsb, int64_t tst,
                            const void *values_out, int64_t cso, const void *offsets_out, const void *steps_out,
                            const void *stamps_out, const void *scratch, int64_t scratch_bytes, const void *flags_out,
                            const char **why) {
    if (int rc = pv_check(x, x_type, n_batch, n_channels, n_time, sb, sc, st, lengths, lengths_type, t, t_type, tsb, tst, values_out,
                          cso, offsets_out, steps_out, stamps_out, scratch, scratch_bytes, flags_out, why))
        return rc;
    // n_batch * n_channels * n_time < 2^62 (pd_check), so the product below cannot overflow
    if (scratch_bytes < n_channels * n_batch * pv_per_row(n_time) * PV_SCRATCH_WORDS * 8) {
        *why = "scratch_bytes is below 200 * n_channels * n_batch * ceil(n_time / 1024)";
        return TSFA_ERR_INVALID;
    }
    return TSFA_OK;
}

// the work items and the three parts of the scratch: pv_plan_work for n_channels * n_batch rows
static inline void pvk_plan_work(PvArgs *a, void *scratch) {
    const int64_t n_batch = a->n_batch;
    a->n_batch = n_batch * a->n_channels;
    pv_plan_work(a, scratch);
    a->n_batch = n_batch;
}

#endif /* TSFA_PACK_VALID_KINDS_H */
