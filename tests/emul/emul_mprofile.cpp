// TEST INFRASTRUCTURE ONLY: the body of k_mprofile (tsfresh_amd/csrc/fam_mprofile.h) compiled by g++ -DTSFA_EMUL and run with
// ONE thread per series, its working set carved by the kernel's own layout (tsfa_layout.h: MpLds) from host memory, its
// columns ordered by the host routine the C-ABI uses (tsfa_prepare_family).  The product never loads this; it lets
// tests/test_mprofile_emul.py compare the kernel's arithmetic with a brute force of the definition on a box without a GPU.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../tsfresh_amd/csrc/fam_mprofile.h"
#include "../../tsfresh_amd/csrc/tsfa_host_tables.h"
#include "../../tsfresh_amd/csrc/tsfa_layout.h"

extern "C" int tsfa_emul_mprofile_restart(void) { return TSFA_MP_RESTART; }
// bytes of the kernel's working set for series of up to n samples of xs_bytes each, and the LDS a workgroup may take
extern "C" long long tsfa_emul_mprofile_lds_bytes(int n, int xs_bytes) { MpLds L; return (long long)L.carve(nullptr, n, xs_bytes); }
extern "C" long long tsfa_emul_mprofile_lds_limit(void) { return TSFA_LDS_LIMIT; }

// params: n_cols pairs (windows, feature code); dtype 0: float32 values, 1: float64; out: [n_series x n_cols].
// Returns 0, or -1 for a column tsfa_validate_spec refuses.
extern "C" int tsfa_emul_mprofile(const double *params, int n_cols, const void *values, int dtype, const int64_t *offsets,
                                  int64_t n_series, double *out) {
    std::vector<TsfaSpec> specs;
    for (int c = 0; c < n_cols; ++c) {
        TsfaSpec s;
        s.calc = TSFA_C_MATRIX_PROFILE;
        s.col = c;
        s.p[0] = params[2 * c];
        s.p[1] = params[2 * c + 1];
        s.p[2] = s.p[3] = 0.0;
        if (!tsfa_validate_spec(s).empty()) return -1;
        specs.push_back(s);
    }
    TsfaFamHints hints;
    tsfa_prepare_family(TSFA_FAM_MPROFILE, specs, hints);
    for (int64_t s = 0; s < n_series; ++s) {
        const int n = (int)(offsets[s + 1] - offsets[s]);
        const int xs_bytes = dtype == 0 ? 4 : 8;
        MpLds L;
        std::vector<unsigned char> mem(L.carve(nullptr, n, xs_bytes) + 16);
        unsigned char *base = mem.data() + ((16 - ((uintptr_t)mem.data() & 15)) & 15);
        L.carve(base, n, xs_bytes);
        const Blk b{0, 1, L.red, L.np};
        double *row = out + s * n_cols;
        if (dtype == 0) {
            memcpy(L.xs, (const float *)values + offsets[s], (size_t)n * 4);
            fam_mprofile_series(b, XsView<float>{(const float *)L.xs}, n, specs.data(), n_cols, row, L.w);
        } else {
            memcpy(L.xs, (const double *)values + offsets[s], (size_t)n * 8);
            fam_mprofile_series(b, XsView<double>{(const double *)L.xs}, n, specs.data(), n_cols, row, L.w);
        }
    }
    return 0;
}
