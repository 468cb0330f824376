// Times packer: kernel bodies of tsfa_pack_times (include/tsfresh_amd.h).
//
// The clock of a batch that already IS an array on the device -- logical shape (n_batch, n_time), any non-negative element
// strides (stride_batch 0: one clock for every series), int64 ticks or float64 seconds -- becomes the per-sample `times` of
// tsfa_extract_timed / tsfa_extract_windows in the ragged layout the dense packer (pack_dense.h) wrote for the samples:
//     hours_out[offsets[b] + i] = hours between stamp (b, i) and stamp (b, 0)        for i < offsets[b + 1] - offsets[b]
// It replaces, for such a batch, the host's pandas arithmetic (feature_extraction/data.py: _hours_since_first).
//
// Arithmetic.  linear_trend_timewise regresses on (index - index[0]).total_seconds() / 3600.0 (the reference's
// feature_calculators.py:2291-2296), and the features are compared bit for bit with the frame route, so the hours are
// evaluated exactly as pandas >= 2 evaluates that expression: TimedeltaArray.total_seconds is `asi8 / periods_per_second`
// (int64 ticks converted to float64, divided by the float64 ticks per second), then `/ 3600.0`:
//     ticks:    (double)(t[b,i] - t[b,0]) / (double)ticks_per_second / 3600.0
//               the subtraction in int64, ONE correctly rounded int64 -> float64 conversion, TWO IEEE divisions
//     seconds:  (t[b,i] - t[b,0]) / 3600.0
// No reciprocal multiply, no division by the product 3600 * ticks_per_second: either rounds differently from the two
// divisions for some differences (a span beyond 2^53 ticks rounds in the conversion already, and the quotient by 10^9 is
// rarely exact).  pandas 1.x multiplied by 1e-9 instead (`asi8 * 1e-9` for nanoseconds) and gives other last bits; this
// file follows pandas >= 2.  The file needs -ffp-contract=off and no fast-math, like the rest of the library.
//
// Missing stamps: a NaT tick (INT64_MIN) or a NaN second, in the sample or in the series' first stamp, gives NaN hours and
// raises TSFA_DENSE_BAD_TIME in the flag word.  A tick difference that overflows int64 wraps (it is computed in uint64):
// stamps more than 2^63 - 1 ticks apart are the caller's problem, as are infinite seconds (inf - inf is a NaN that raises
// no flag).
//
// Like pack_dense.h this file is compiled two ways: by hipcc for gfx950 (tsfa_pack_times.hip wraps the body in a __global__
// kernel) and by g++ -DTSFA_EMUL with ONE thread per workgroup (tests/emul/emul_pack_times.cpp drives the same body work
// item by work item).  The emulation sees the index arithmetic, the chunk edges, the pair path's alignment test, the
// arithmetic and the flag.  It cannot see what only exists with 64 lanes (the wavefront vote before the flag's atomic) nor
// the device's own division and conversion sequences: tests/test_tensor_times_gpu.py compares those bit for bit.
//
// Shape: the rows routes of pack_dense.h.  A work item is PD_ROW_CHUNK stamps of one series, w = batch * per_row + chunk;
// consecutive lanes are on consecutive stamps; UNIT (stride_time == 1) is known at compile time, so a wavefront's loads
// are one contiguous stretch, and where source and destination are both 16-byte aligned a lane moves two stamps per step
// (one 16-byte load, one 16-byte store).  The first stamp of the series is one load at an address every lane of the work
// item shares.  No LDS, no barrier, no atomic but the OR into the flag word -- at most one per wavefront -- and no
// workgroup waits on another.
//
// Bounds: a series' length is the difference of its offsets, clamped into [0, n_time], so whatever `offsets` holds no
// stamp outside t is read; a series of length 0 reads nothing, not even its first stamp.  Writes go to
// [offsets[b], offsets[b] + len(b)) only.
#ifndef TSFA_PACK_TIMES_H
#define TSFA_PACK_TIMES_H

#include "pack_dense.h"

#define PT_NAT ((int64_t)(-9223372036854775807ll - 1))   /* numpy's / pandas' NaT as int64 ticks */
#define PT_NAN_BITS 0x7ff8000000000000ull                /* the quiet NaN numpy writes for a NaT difference */

struct PtArgs {
    const void *t;
    int64_t n_batch, n_time;
    int64_t sb, st;              // element strides of t
    double tps;                  // ticks per second (TSFA_I64), exact in float64
    const int64_t *offsets;      // n_batch + 1, written by tsfa_pack_dense for the same batch
    double *out;
    unsigned int *flags;
    int64_t n_work, per_row;     // work items; chunks per series
};

struct __attribute__((aligned(16), may_alias)) PtU2 { pk_u64 v[2]; };

TSFA_DEV double pt_bits_to_f64(pk_u64 u) {
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}
TSFA_DEV pk_u64 pt_f64_to_bits(double d) {
    pk_u64 u;
    __builtin_memcpy(&u, &d, 8);
    return u;
}
TSFA_DEV bool pt_missing(int type, pk_u64 u) {
    return type == TSFA_I64 ? (int64_t)u == PT_NAT : (u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

// hours between the stamp `u` and the series' first stamp `first` (bit patterns of TYPE), as the bits of a float64
template <int TYPE>
TSFA_DEV pk_u64 pt_hours(pk_u64 u, pk_u64 first, bool first_missing, double tps, bool *bad) {
    if (first_missing || pt_missing(TYPE, u)) {
        *bad = true;
        if (TYPE == TSFA_I64) return PT_NAN_BITS;
    }
    if (TYPE == TSFA_I64) {
        const int64_t d = (int64_t)(u - first);   // wraps on overflow (see the head of this file)
        return pt_f64_to_bits((double)d / tps / 3600.0);
    }
    return pt_f64_to_bits((pt_bits_to_f64(u) - pt_bits_to_f64(first)) / 3600.0);
}

// raise `bit` in the flag word when a lane of the wavefront asks for it: one atomic per wavefront at most
TSFA_DEV void pt_flag(const PkBlk &b, unsigned int *flags, bool bad, unsigned int bit) {
#if TSFA_GPU
    if (__any(bad ? 1 : 0) && (b.tid & 63) == 0) pk_or32(flags, bit);
#else
    (void)b;
    if (bad) pk_or32(flags, bit);
#endif
}

template <int TYPE, bool UNIT>
TSFA_DEV void pt_rows_body(const PkBlk &b, int64_t first_item, int64_t stride, const PtArgs &a) {
    bool bad = false;
    const pk_u64 *const t = (const pk_u64 *)a.t;
    pk_u64 *const out = (pk_u64 *)a.out;
    for (int64_t w = first_item; w < a.n_work; w += stride) {
        const int64_t bb = w / a.per_row, chunk = w - bb * a.per_row;
        const int64_t off = a.offsets[bb];
        int64_t len = a.offsets[bb + 1] - off;
        if (len > a.n_time) len = a.n_time;
        int64_t t0 = chunk * PD_ROW_CHUNK;
        if (t0 >= len) continue;   // (also a length of 0 or below: nothing is read)
        const int64_t t1 = t0 + PD_ROW_CHUNK < len ? t0 + PD_ROW_CHUNK : len;
        const int64_t src = bb * a.sb;
        const pk_u64 first = t[src];   // the same address for every lane of the work item
        const bool first_missing = pt_missing(TYPE, first);
        if (UNIT) {
            // both sides 16-byte aligned (the same for the whole work item): the bulk goes two stamps per lane and step,
            // the loop below takes what is left of the chunk
            const pk_u64 sa = (pk_u64)(uintptr_t)(t + src + t0), da = (pk_u64)(uintptr_t)(out + off + t0);
            if (sa % 16 == 0 && da % 16 == 0) {
                const int64_t nq = (t1 - t0) / 2;
                for (int64_t q = b.tid; q < nq; q += b.nt) {
                    const PtU2 v = *(const PtU2 *)(t + src + t0 + 2 * q);
                    PtU2 h;
                    h.v[0] = pt_hours<TYPE>(v.v[0], first, first_missing, a.tps, &bad);
                    h.v[1] = pt_hours<TYPE>(v.v[1], first, first_missing, a.tps, &bad);
                    *(PtU2 *)(out + off + t0 + 2 * q) = h;
                }
                t0 += nq * 2;
            }
        }
        for (int64_t i = t0 + b.tid; i < t1; i += b.nt)
            out[off + i] = pt_hours<TYPE>(t[src + (UNIT ? i : i * a.st)], first, first_missing, a.tps, &bad);
    }
    pt_flag(b, a.flags, bad, (unsigned int)TSFA_DENSE_BAD_TIME);
}

// ---------------------------------------------------------------------------------------------
// Host: argument checks, shared by tsfa_pack_times and the emulation's driver.
// Returns TSFA_OK or the status tsfa_pack_times reports, with the reason in *why.
// ---------------------------------------------------------------------------------------------
static inline int pt_check(const void *t, int t_type, int64_t ticks_per_second, int64_t n_batch, int64_t n_time, int64_t sb,
                           int64_t st, const void *offsets, const void *hours_out, const void *flags_out, const char **why) {
    *why = "";
    if (!t || !offsets || !hours_out || !flags_out) { *why = "null pointer"; return TSFA_ERR_INVALID; }
    if (t_type != TSFA_I64 && t_type != TSFA_F64) { *why = "the stamps must be TSFA_I64 (ticks) or TSFA_F64 (seconds)"; return TSFA_ERR_INVALID; }
    if (t_type == TSFA_I64 && ticks_per_second != 1 && ticks_per_second != 1000 && ticks_per_second != 1000000 &&
        ticks_per_second != 1000000000) {
        *why = "ticks_per_second must be 1, 10^3, 10^6 or 10^9";
        return TSFA_ERR_INVALID;
    }
    if (n_batch < 1 || n_time < 1) { *why = "a dimension is zero or negative"; return TSFA_ERR_INVALID; }
    if (sb < 0 || st < 0) { *why = "negative stride"; return TSFA_ERR_INVALID; }
    if (n_time > PD_MAX_LEN) { *why = "more than 33 554 431 stamps per series"; return TSFA_ERR_TOO_LONG; }
    // every index below fits int64 with room, as in pd_check
    const int64_t lim = (int64_t)1 << 62;
    if (n_batch > lim / n_time) { *why = "more than 2^62 stamps"; return TSFA_ERR_INVALID; }
    if ((sb && n_batch - 1 > lim / 4 / sb) || (st && n_time - 1 > lim / 4 / st)) {
        *why = "a stride reaches beyond 2^60 elements";
        return TSFA_ERR_INVALID;
    }
    return TSFA_OK;
}

// the work items (a.n_work, a.per_row)
static inline void pt_plan_work(PtArgs *a) {
    a->per_row = (a->n_time + PD_ROW_CHUNK - 1) / PD_ROW_CHUNK;
    a->n_work = a->n_batch * a->per_row;
}

#endif /* TSFA_PACK_TIMES_H */
