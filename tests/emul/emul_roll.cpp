// TEST INFRASTRUCTURE ONLY: the window builder's kernel bodies (tsfresh_amd/csrc/roll_device.h) compiled by g++ -DTSFA_EMUL and
// driven with ONE thread per workgroup, in the order tsfa_roll_windows launches them on the GPU: the per-series count, the
// packer's scan (pk_scan_body), the fill.  The product never loads this; it lets tests/test_roll_device_emul.py compare the
// builder with utilities.dataframe_functions.roll_views on a box without a GPU.  The argument checks are the shared
// rl_make_params of the header and the steps check is the driver's.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tsfresh_amd/csrc/roll_device.h"

// offsets: n_series + 1 int64.  out_*: room for offsets[n_series] - offsets[0] windows each (a series never has more windows
// than samples).  sort / out_shift_values: the packed sort column and room for as many elements of its type, or NULL.
// Returns the number of windows, or -1 (TSFA_ERR_INVALID) for arguments tsfa_roll_windows refuses.
extern "C" int64_t tsfa_emul_roll(const int64_t *offsets, int64_t n_series, int32_t rolling_direction, int64_t max_timeshift,
                                  int64_t min_timeshift, int64_t steps, int64_t *out_starts, int64_t *out_ends,
                                  int64_t *out_series, int64_t *out_shifts, const void *sort, int32_t sort_type,
                                  void *out_shift_values) {
    RlParams p;
    if (!offsets || n_series < 0 || rl_make_params(rolling_direction, max_timeshift, min_timeshift, steps, &p)) return TSFA_ERR_INVALID;
    if (n_series == 0) return 0;
    const PkBlk b{0, 1};
    RlStats st;
    memset(&st, 0, sizeof(st));
    std::vector<uint32_t> counts((size_t)n_series);
    unsigned int ws[16];
    pk_u64 red;
    rl_count_body(b, 0, 1, offsets, n_series, p, counts.data(), &red, &st);
    pk_scan_body(b, counts.data(), (size_t)n_series, ws, &st.total);
    if ((int64_t)st.max_len > steps) return TSFA_ERR_INVALID;
    const int64_t nw = (int64_t)st.total;
    rl_fill_body(b, 0, 1, offsets, n_series, counts.data(), nw, p, out_starts, out_ends, out_series, out_shifts);
    if (sort && out_shift_values)
        rl_shift_values_body(b, 0, 1, sort, pk_itemsize(sort_type), offsets[n_series], out_starts, out_ends, p.positive, nw,
                             out_shift_values);
    return nw;
}
