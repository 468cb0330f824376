// TEST INFRASTRUCTURE ONLY -- never loaded by the tsfresh_amd package.
//
// The two ridge-line linkers of number_cwt_peaks (tsfresh_amd/csrc/fam_cwt.h: cwt_link_general, cwt_link_columns) as a
// single-thread g++ program, fed a relative-maximum mask directly and run through the DEVICE'S OWN LDS LAYOUT
// (tsfa_layout.h: CwtPeaksLayout).  The layout is carved for 3 n columns, so the line arrays hold 3 n lines and the general
// linker's capacity never binds (five rows of at most n / 2 maxima are 2.5 n lines).  The buffer starts out as 0x7f bytes, as
// LDS starts out with another series' contents; the driver then clears what number_cwt_peaks_one clears before phase A.
// Returns each linker's entries (end column, end row) and the marks it left in the mask (tests/test_cwt_links_emul.py).
// It does not exercise the workgroup scan or the barriers; the `-m gpu` tests do.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/tsfresh_amd.h"
#include "../../tsfresh_amd/csrc/fam_cwt.h"
#include "../../tsfresh_amd/csrc/tsfa_layout.h"

// mask_in: n columns, bit r = a relative maximum of CWT row r (r < W).  route 1: the column linker (W <= 5), 0: the general
// linker.  ent_col / ent_row: room for ent_cap entries; mask_out: n columns, the mask after the linker (marks: bit W + 1).
// Returns the number of entries, or -1 for arguments the linker does not serve; *overflow: the linker's overflow flag.
extern "C" int tsfa_emul_cwt_links(const unsigned short *mask_in, int n, int W, int derive_w1, int route, int *ent_col,
                                   int *ent_row, int ent_cap, unsigned short *mask_out, int *overflow) {
    if (n < 1 || W < 1 || W > TSFA_CWTP_MAXW - 2 || (route != 0 && W > TSFA_CWT_COLUMN_LINKS_MAXW)) return -1;
    const int cap = 3 * n;
    CwtPeaksLayout L;
    const size_t bytes = L.carve(nullptr, cap, 0);
    std::vector<double> lds(bytes / sizeof(double) + 2);
    memset(lds.data(), 0x7f, lds.size() * sizeof(double));
    L.carve((unsigned char *)lds.data(), cap, 0);
    const Blk b{0, 1, L.p.red, nullptr};
    for (int c = 0; c < n; ++c) { L.p.mask[c] = mask_in[c]; L.p.colmap[c] = 0; L.p.mline[c] = 0; }
    const CwtOwnCols own = cwt_own_columns(b, n);
    const int start_row = cwt_start_row(b, W, L.p, own);
    int ovf = 0;
    const int cnt = route ? cwt_link_columns(b, n, W, start_row, L.p, own, cap, derive_w1 != 0, &ovf)
                          : cwt_link_general(b, n, W, start_row, L.p, own, cap, derive_w1 != 0, &ovf);
    for (int k = 0; k < cnt && k < ent_cap; ++k) {
        ent_col[k] = (int)L.p.lcol[k];
        ent_row[k] = (int)L.p.linf[k];
    }
    for (int c = 0; c < n; ++c) mask_out[c] = L.p.mask[c];
    *overflow = ovf;
    return cnt;
}
