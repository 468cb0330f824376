// Window builder: kernel bodies of tsfa_roll_windows (include/tsfresh_amd.h).
//
// The rolled (forecasting) layout of one packed kind, built on the device from the pack's offsets: for every series the
// windows of tsfresh/utilities/dataframe_functions.py:340-358 (_roll_out_time_series) as (start, end) views into the
// pack's ragged value buffer, in (series, ascending timeshift) order -- what the host computes with
// utilities.dataframe_functions.roll_views(lengths + [steps]) minus the phantom's windows.
//
// The valid timeshifts of a series of `len` samples have a closed form (a = |rolling_direction|, mts = max_timeshift or
// steps, both clamped to steps, which changes no window; no window at all when mts < min_timeshift):
//   direction > 0   ts = steps - k a, 1 <= ts <= len, window [max(ts - mts - 1, 0), ts): its length min(ts, mts + 1) must
//                   reach min_timeshift + 1, so  min_timeshift + 1 <= ts <= len  and  ts = steps (mod a):
//                   first = the smallest such ts, count = (len - first) / a + 1, window j has ts = first + j a
//   direction < 0   ts = 1 + k a <= steps, frm = ts - 1 < len, window [frm, min(frm + mts + 1, len)): its length
//                   min(mts + 1, len - frm) must reach min_timeshift + 1, so  k a <= len - min_timeshift - 1:
//                   count = (len - min_timeshift - 1) / a + 1, window j has frm = j a
// so the build is three launches and no n_series x n_shifts intermediate exists:
//   1. rl_count_body   per series: its window count (O(1)) and, by the way, the longest series of the pack
//   2. pk_scan_body    exclusive scan of the counts (the packer's single-workgroup scan)
//   3. rl_fill_body    window w finds its series by bisection over the scanned counts (the last series whose first window is
//                      <= w: series without windows share their successor's value and are skipped) and derives its shift
//                      arithmetically
// A series of len samples has at most len windows, so the counts and their total fit the packer's 32-bit scan (a pack holds
// fewer than 2^32 rows); every index a window carries is int64.
//
// The same windows for a batch that is no pack (tsfa_roll_count / tsfa_roll_fill: raw offsets in, caller-owned buffers out) take
// one of two routes.  Ragged: steps 1-3 above, with the counts scanned in place in the caller's `scanned` buffer.  Uniform (every
// series has n samples, offsets[s] = offsets[0] + s n): the count per series c = rl_count(p, n) is known on the host, so
// n_windows = n_series * c, window w belongs to series w / c with shift index w % c, and one launch of rl_fill_uniform_body is the
// whole build: no counts, no scan, no bisection, nothing read back.  The host side of both (rl_check_extent, rl_uniform_count)
// lives here too, so that the emulation runs the driver's checks and not a copy of them.
//
// Compiled two ways like pack_device.h: by hipcc for gfx950 and by g++ -DTSFA_EMUL with one thread per workgroup
// (tests/emul/emul_roll.cpp, tests/emul/emul_roll_dense.cpp).  The bodies are grid-stride loops without ballots or DPP (one LDS word collects a workgroup's
// maximum length): the emulation sees all of their arithmetic.  No workgroup waits on another; the maximum length is the only
// atomic and does not depend on arrival order.
#ifndef TSFA_ROLL_DEVICE_H
#define TSFA_ROLL_DEVICE_H

#include "pack_device.h"

struct RlParams {
    int64_t amount;    // |rolling_direction| >= 1
    int64_t steps;     // prediction_steps: the longest series of the whole frame (>= every length of this pack)
    int64_t mts;       // max_timeshift or steps, clamped to steps
    int64_t min_ts;    // min_timeshift, clamped to steps + 1
    int32_t positive;  // rolling_direction > 0
};

struct RlStats {
    pk_u64 max_len;        // the longest series of the pack
    unsigned int total;    // total of the count scan: the number of windows
    unsigned int pad;
};

// Host code (the .hip driver and the emulation share it): 0, or the reason tsfa_roll_windows refuses the arguments.
static inline const char *rl_make_params(int32_t rolling_direction, int64_t max_timeshift, int64_t min_timeshift, int64_t steps,
                                         RlParams *p) {
    if (rolling_direction == 0) return "rolling_direction is 0";
    if (max_timeshift < 0) return "max_timeshift is negative (0 = none)";
    if (min_timeshift < 0) return "min_timeshift is negative";
    if (steps < 1) return "steps is below 1";
    p->positive = rolling_direction > 0 ? 1 : 0;
    p->amount = rolling_direction > 0 ? (int64_t)rolling_direction : -(int64_t)rolling_direction;
    p->steps = steps;
    p->mts = (max_timeshift == 0 || max_timeshift > steps) ? steps : max_timeshift;
    p->min_ts = min_timeshift > steps ? steps + 1 : min_timeshift;
    return nullptr;
}

// first valid timeshift (direction > 0) of a series; only meaningful where rl_count > 0
// (PK_HD: the uniform route of tsfa_roll_count / tsfa_roll_fill evaluates the two closed forms on the host as well)
PK_HD int64_t rl_first_shift(const RlParams &p) {
    const int64_t lo = p.min_ts + 1;                       // the smallest admissible ts
    int64_t d = (p.steps - lo) % p.amount;                 // (C++ remainder: negative when lo > steps) -> the residue
    if (d < 0) d += p.amount;
    return lo + d;                                         // the smallest ts >= lo with ts = steps (mod amount)
}

PK_HD int64_t rl_count(const RlParams &p, int64_t len) {
    if (p.mts < p.min_ts) return 0;
    if (p.positive) {
        const int64_t first = rl_first_shift(p);
        return first > len ? 0 : (len - first) / p.amount + 1;
    }
    const int64_t top = len - p.min_ts - 1;                // the largest admissible frm
    return top < 0 ? 0 : top / p.amount + 1;
}

// ---------------------------------------------------------------------------------------------
// 1. counts[s] = windows of series s; st->max_len = the longest series  (grid-stride; `red`: 1 pk_u64 of LDS: the threads'
//    maxima meet there, so one atomic per workgroup reaches the global word, as in pk_minmax_body)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void rl_count_body(const PkBlk &b, int64_t first, int64_t stride, const int64_t *offsets, int64_t n_series,
                            RlParams p, uint32_t *counts, pk_u64 *red, RlStats *st) {
    if (b.tid == 0) *red = 0;
    pk_sync();
    pk_u64 longest = 0;
    for (int64_t s = first + b.tid; s < n_series; s += stride) {
        const int64_t len = offsets[s + 1] - offsets[s];
        if ((pk_u64)len > longest) longest = (pk_u64)len;
        counts[s] = (uint32_t)rl_count(p, len);
    }
    if (longest) pk_max64(red, longest);
    pk_sync();
    if (b.tid == 0 && *red) pk_max64(&st->max_len, *red);
}

// ---------------------------------------------------------------------------------------------
// 3. the windows.  scanned: the exclusive scan of the counts.  (grid-stride over the windows)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void rl_fill_body(const PkBlk &b, int64_t first, int64_t stride, const int64_t *offsets, int64_t n_series,
                           const uint32_t *scanned, int64_t n_windows, RlParams p, int64_t *starts, int64_t *ends,
                           int64_t *series, int64_t *shifts) {
    for (int64_t w = first + b.tid; w < n_windows; w += stride) {
        int64_t lo = 0, hi = n_series - 1;  // the largest s with scanned[s] <= w
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if ((int64_t)scanned[mid] <= w) lo = mid;
            else hi = mid - 1;
        }
        const int64_t j = w - (int64_t)scanned[lo], o = offsets[lo], len = offsets[lo + 1] - o;
        int64_t ts, frm, until;
        if (p.positive) {
            ts = rl_first_shift(p) + j * p.amount;
            until = ts;
            frm = ts - p.mts - 1;
            if (frm < 0) frm = 0;
        } else {
            frm = j * p.amount;
            ts = frm + 1;
            until = frm + p.mts + 1;
            if (until > len) until = len;
        }
        starts[w] = o + frm;
        ends[w] = o + until;
        series[w] = lo;
        shifts[w] = ts;
    }
}

// ---------------------------------------------------------------------------------------------
// 3u. the windows of a batch of n_series series of n samples each, c = rl_count(p, n) > 0 windows per series, n_windows =
//     n_series * c.  offsets: the batch's offsets (only offsets[0], the base, is read) or NULL for base 0.
//     (grid-stride over the windows)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void rl_fill_uniform_body(const PkBlk &b, int64_t first, int64_t stride, const int64_t *offsets, int64_t n, int64_t c,
                                   int64_t n_windows, RlParams p, int64_t *starts, int64_t *ends, int64_t *series,
                                   int64_t *shifts) {
    const int64_t base = offsets ? offsets[0] : 0;
    for (int64_t w = first + b.tid; w < n_windows; w += stride) {
        const int64_t s = w / c, j = w - s * c, o = base + s * n;
        int64_t ts, frm, until;
        if (p.positive) {
            ts = rl_first_shift(p) + j * p.amount;
            until = ts;
            frm = ts - p.mts - 1;
            if (frm < 0) frm = 0;
        } else {
            frm = j * p.amount;
            ts = frm + 1;
            until = frm + p.mts + 1;
            if (until > n) until = n;
        }
        starts[w] = o + frm;
        ends[w] = o + until;
        series[w] = s;
        shifts[w] = ts;
    }
}

// ---------------------------------------------------------------------------------------------
// Host code of tsfa_roll_count / tsfa_roll_fill (the .hip driver and the emulation share it).  The counts and their scan are
// 32 bits wide, which holds because no series has more windows than samples: a batch of 2^32 or more samples is refused.
// ---------------------------------------------------------------------------------------------
#define RL_MAX_SAMPLES 0xffffffffll

// extent = offsets[n_series] - offsets[0] of a ragged batch: a tsfa_status, *why set when it is not TSFA_OK
static inline int rl_check_extent(int64_t extent, const char **why) {
    if (extent < 0) {
        *why = "offsets[n_series] is below offsets[0]";
        return TSFA_ERR_INVALID;
    }
    if (extent > RL_MAX_SAMPLES) {
        *why = "4 294 967 296 or more samples (the window counts are 32 bits wide)";
        return TSFA_ERR_TOO_LONG;
    }
    return TSFA_OK;
}

// The uniform route: n_series series of series_len samples -> *per_series = rl_count(p, series_len) and *n_windows, their
// product (below 2^32, as the samples are).  A tsfa_status, *why set when it is not TSFA_OK.
static inline int rl_uniform_count(const RlParams &p, int64_t n_series, int64_t series_len, int64_t *per_series, int64_t *n_windows,
                                   const char **why) {
    if (n_series < 0 || series_len < 1) {
        *why = "n_series is negative or series_len is below 1";
        return TSFA_ERR_INVALID;
    }
    if (series_len > p.steps) {
        *why = "steps is below series_len";
        return TSFA_ERR_INVALID;
    }
    if (n_series > RL_MAX_SAMPLES / series_len) {   // n_series * series_len >= 2^32, without forming the product
        *why = "4 294 967 296 or more samples (the window counts are 32 bits wide)";
        return TSFA_ERR_TOO_LONG;
    }
    *per_series = rl_count(p, series_len);          // <= series_len: the product below cannot overflow
    *n_windows = n_series * *per_series;
    return TSFA_OK;
}

// ---------------------------------------------------------------------------------------------
// The value of the sort column that names a window (the second half of the (id, shift) window id): the stamp of the window's
// last row for a positive direction, of its first row for a negative one.  Element type unchanged.  (grid-stride)
// ---------------------------------------------------------------------------------------------
TSFA_DEV void rl_shift_values_body(const PkBlk &b, int64_t first, int64_t stride, const void *sort, int itemsize, int64_t n_rows,
                                   const int64_t *starts, const int64_t *ends, int positive, int64_t n_windows, void *out) {
    for (int64_t w = first + b.tid; w < n_windows; w += stride) {
        const int64_t r = positive ? ends[w] - 1 : starts[w];
        if (r >= 0 && r < n_rows) pk_copy_raw(out, w, sort, r, itemsize);  // always true for windows built on this pack
    }
}

#endif /* TSFA_ROLL_DEVICE_H */
