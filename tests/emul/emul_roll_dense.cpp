// TEST INFRASTRUCTURE ONLY: tsfa_roll_count / tsfa_roll_fill (tsfresh_amd/csrc/tsfa_pack_device.hip) without the device -- the
// host checks they share with this file through roll_device.h (rl_make_params, rl_check_extent, rl_uniform_count), in the
// driver's order, and the kernel bodies compiled by g++ -DTSFA_EMUL and driven with ONE thread per workgroup over `grid`
// workgroups: the per-series count, the packer's scan (pk_scan_body), the fill by bisection; or, for a uniform batch, the
// closed-form fill alone.  The product never loads this; it lets tests/test_roll_dense_emul.py compare the builder with
// utilities.dataframe_functions.roll_views on a box without a GPU.
// With -DRL_EMUL_MAIN the file is a stand-alone program that runs both routes over a grid of lengths and roll arguments
// into heap blocks of EXACTLY n_windows cells and compares them with a plain enumeration of the reference's windows: the
// form an AddressSanitizer / UBSan run of the driver logic and the bodies takes.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tsfresh_amd/csrc/roll_device.h"

// The arguments of tsfa_roll_count without the device and the stream; grid: emulated workgroups of the count launch.
// Returns the status tsfa_roll_count would (TSFA_OK, TSFA_ERR_INVALID, TSFA_ERR_TOO_LONG).
extern "C" int tsfa_emul_roll_count(const int64_t *offsets, int64_t n_series, int64_t series_len, int32_t rolling_direction,
                                    int64_t max_timeshift, int64_t min_timeshift, int64_t steps, uint32_t *scanned,
                                    int64_t *n_windows_host, int64_t grid) {
    if (!n_windows_host) return TSFA_ERR_INVALID;
    *n_windows_host = 0;
    RlParams p;
    const char *why = rl_make_params(rolling_direction, max_timeshift, min_timeshift, steps, &p);
    if (why) return TSFA_ERR_INVALID;
    if (!scanned) {
        int64_t per_series = 0;
        return rl_uniform_count(p, n_series, series_len, &per_series, n_windows_host, &why);
    }
    if (!offsets || n_series < 0) return TSFA_ERR_INVALID;
    if (n_series == 0) return TSFA_OK;
    if (int rc = rl_check_extent(offsets[n_series] - offsets[0], &why)) return rc;   // (the two words the driver reads back)
    if (grid < 1) grid = 1;
    const PkBlk b{0, 1};
    RlStats st;
    memset(&st, 0, sizeof(st));
    unsigned int ws[16];
    pk_u64 red;
    for (int64_t blk = 0; blk < grid; ++blk) rl_count_body(b, blk, grid, offsets, n_series, p, scanned, &red, &st);
    pk_scan_body(b, scanned, (size_t)n_series, ws, &st.total);
    if ((int64_t)st.max_len > steps) return TSFA_ERR_INVALID;
    *n_windows_host = (int64_t)st.total;
    return TSFA_OK;
}

// The arguments of tsfa_roll_fill without the device and the stream; grid: emulated workgroups of the fill launch.
extern "C" int tsfa_emul_roll_fill(const int64_t *offsets, int64_t n_series, const uint32_t *scanned, int64_t series_len,
                                   int64_t n_windows, int32_t rolling_direction, int64_t max_timeshift, int64_t min_timeshift,
                                   int64_t steps, int64_t *starts, int64_t *ends, int64_t *series, int64_t *timeshifts,
                                   int64_t grid) {
    RlParams p;
    const char *why = rl_make_params(rolling_direction, max_timeshift, min_timeshift, steps, &p);
    if (why) return TSFA_ERR_INVALID;
    if (n_windows < 0 || n_series < 0) return TSFA_ERR_INVALID;
    int64_t per_series = 0;
    if (!scanned) {
        int64_t expect = 0;
        if (int rc = rl_uniform_count(p, n_series, series_len, &per_series, &expect, &why)) return rc;
        if (n_windows != expect) return TSFA_ERR_INVALID;
    } else if (!offsets || n_windows > RL_MAX_SAMPLES) {
        return TSFA_ERR_INVALID;
    }
    if (n_windows == 0) return TSFA_OK;
    if (n_series < 1 || !starts || !ends || !series || !timeshifts) return TSFA_ERR_INVALID;
    if (grid < 1) grid = 1;
    const PkBlk b{0, 1};
    for (int64_t blk = 0; blk < grid; ++blk) {
        if (scanned) rl_fill_body(b, blk, grid, offsets, n_series, scanned, n_windows, p, starts, ends, series, timeshifts);
        else rl_fill_uniform_body(b, blk, grid, offsets, series_len, per_series, n_windows, p, starts, ends, series, timeshifts);
    }
    return TSFA_OK;
}

#ifdef RL_EMUL_MAIN
#include <stdio.h>

static int64_t g_cases = 0, g_failed = 0;

struct Win {
    int64_t start, end, series, ts;
};

// dataframe_functions.py:340-358 for every shift of every series, (series, ascending timeshift)
static std::vector<Win> reference(const std::vector<int64_t> &len, const std::vector<int64_t> &off, int dir, int64_t max_ts,
                                  int64_t min_ts, int64_t steps) {
    std::vector<Win> out;
    const int64_t a = dir > 0 ? dir : -dir, mts = max_ts ? max_ts : steps;
    for (size_t s = 0; s < len.size(); ++s) {
        const int64_t first = dir > 0 ? ((steps - 1) % a) + 1 : 1;   // the shifts are steps, steps - a, ... > 0, or 1, 1 + a, ... <= steps
        for (int64_t ts = first; ts <= steps; ts += a) {
            int64_t frm, until;
            if (dir > 0) {
                until = ts;
                frm = until - mts - 1 > 0 ? until - mts - 1 : 0;
                if (until > len[s]) continue;
            } else {
                frm = ts - 1;
                until = frm + mts + 1 < len[s] ? frm + mts + 1 : len[s];
                if (frm >= len[s]) continue;
            }
            if (until - frm < min_ts + 1) continue;
            out.push_back(Win{off[s] + frm, off[s] + until, (int64_t)s, ts});
        }
    }
    return out;
}

static void one_case(const std::vector<int64_t> &len, int64_t base, int dir, int64_t max_ts, int64_t min_ts, int64_t steps,
                     bool uniform, int64_t grid) {
    const int64_t ns = (int64_t)len.size();
    std::vector<int64_t> off((size_t)ns + 1);
    off[0] = base;
    for (int64_t s = 0; s < ns; ++s) off[(size_t)s + 1] = off[(size_t)s] + len[(size_t)s];
    const std::vector<Win> want = reference(len, off, dir, max_ts, min_ts, steps);
    std::vector<uint32_t> scanned((size_t)ns);
    int64_t nw = -1;
    int rc = tsfa_emul_roll_count(off.data(), ns, uniform ? len[0] : 0, dir, max_ts, min_ts, steps, uniform ? nullptr : scanned.data(),
                                  &nw, grid);
    ++g_cases;
    bool ok = rc == TSFA_OK && nw == (int64_t)want.size();
    if (ok) {
        // exactly nw cells each: a write beyond the last window is the sanitizer's to find
        std::vector<int64_t> st((size_t)nw), en((size_t)nw), se((size_t)nw), sh((size_t)nw);
        rc = tsfa_emul_roll_fill(off.data(), ns, uniform ? nullptr : scanned.data(), uniform ? len[0] : 0, nw, dir, max_ts, min_ts, steps,
                                 nw ? st.data() : nullptr, nw ? en.data() : nullptr, nw ? se.data() : nullptr,
                                 nw ? sh.data() : nullptr, grid);
        ok = rc == TSFA_OK;
        for (int64_t w = 0; w < nw && ok; ++w)
            ok = st[(size_t)w] == want[(size_t)w].start && en[(size_t)w] == want[(size_t)w].end &&
                 se[(size_t)w] == want[(size_t)w].series && sh[(size_t)w] == want[(size_t)w].ts;
    }
    if (!ok) {
        ++g_failed;
        fprintf(stderr, "FAILED %s series %lld first length %lld direction %d max %lld min %lld steps %lld: rc %d windows %lld / %lld\n",
                uniform ? "uniform" : "ragged", (long long)ns, (long long)len[0], dir, (long long)max_ts, (long long)min_ts,
                (long long)steps, rc, (long long)nw, (long long)want.size());
    }
}

int main() {
    const int64_t L[6] = {1, 2, 3, 5, 8, 13};
    std::vector<std::vector<int64_t>> sets;
    for (int64_t v : L) sets.push_back({v});                                   // one series
    for (int64_t v : L) sets.push_back({v, v, v});                             // uniform
    sets.push_back({1, 2, 3, 5, 8, 13});
    sets.push_back({13, 8, 5, 3, 2, 1});
    sets.push_back({1, 1, 13, 1, 2, 2, 8, 1});
    sets.push_back({5, 5, 1, 13, 13, 3});
    sets.push_back({2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3});
    for (const auto &len : sets) {
        int64_t longest = 0;
        bool same = true;
        for (int64_t v : len) { longest = v > longest ? v : longest; same = same && v == len[0]; }
        for (int dir : {1, -1, 2, -2, 3, -3})
            for (int64_t max_ts : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)4, (int64_t)100})
                for (int64_t min_ts : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)7, (int64_t)20})
                    for (int64_t steps : {longest, longest + 4}) {
                        one_case(len, 0, dir, max_ts, min_ts, steps, false, 3);
                        if (same) one_case(len, 7, dir, max_ts, min_ts, steps, true, 3);
                    }
    }
    // more than 4096 series of 1 .. 3 samples: the scan's carry
    std::vector<int64_t> many(5000);
    for (size_t s = 0; s < many.size(); ++s) many[s] = 1 + (int64_t)((s * 7 + s / 3) % 3);
    for (int dir : {1, -1, 2}) one_case(many, 0, dir, 0, 0, 3, false, 5);
    // the refusals
    int64_t nw = 0;
    const int64_t claims[2] = {0, (int64_t)1 << 32};
    uint32_t cell = 0;
    ++g_cases;
    if (tsfa_emul_roll_count(claims, 1, 0, 1, 0, 0, (int64_t)1 << 32, &cell, &nw, 1) != TSFA_ERR_TOO_LONG ||
        tsfa_emul_roll_count(nullptr, (int64_t)1 << 16, (int64_t)1 << 16, 1, 0, 0, (int64_t)1 << 16, nullptr, &nw, 1) != TSFA_ERR_TOO_LONG ||
        tsfa_emul_roll_count(nullptr, 65535, 65537, 1, 0, 0, 65537, nullptr, &nw, 1) != TSFA_OK || nw != (int64_t)65535 * 65537 ||
        tsfa_emul_roll_count(claims, 1, 0, 0, 0, 0, 5, &cell, &nw, 1) != TSFA_ERR_INVALID) {
        ++g_failed;
        fprintf(stderr, "FAILED the refusals\n");
    }
    printf("%lld cases, %lld failed\n", (long long)g_cases, (long long)g_failed);
    return g_failed ? 1 : 0;
}
#endif
