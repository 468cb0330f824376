// TEST INFRASTRUCTURE ONLY -- never loaded by the tsfresh_amd package.
//
// The SORT family's kernel body (tsfresh_amd/csrc/fam_sort.h) as a single-thread g++ program, run through the DEVICE'S OWN
// LDS LAYOUT of a one-wavefront launch (tsfa_layout.h: SortLds with nt = 64): the resident series in its input precision, two
// reduction slots, the numpy-order scratch inside the Langevin scratch, the table of logarithms at that scratch's end, and --
// mode 2 -- the sorted series as a 16-bit sample order (OrdView) with the permutation_entropy columns left to k_perm's code.
// Everything is carved from one buffer that starts out as 0x7f bytes, as LDS starts out with another series' contents: an
// overlap of two live regions or a read of something unwritten shows as a mismatch with the oracle (tests/test_sort_one_wave.py).
// It does not exercise wavefront shuffles or the wave-local wait; the `-m gpu` tests do.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tsfresh_amd.h"
#include "../../tsfresh_amd/csrc/fam_ar.h"
#include "../../tsfresh_amd/csrc/fam_ar_dd.h"
#include "../../tsfresh_amd/csrc/fam_basic.h"
#include "../../tsfresh_amd/csrc/fam_cwt.h"
#include "../../tsfresh_amd/csrc/fam_entropy.h"
#include "../../tsfresh_amd/csrc/fam_perm.h"
#include "../../tsfresh_amd/csrc/fam_seq.h"
#include "../../tsfresh_amd/csrc/fam_sort.h"
#include "../../tsfresh_amd/csrc/fam_general.h"
#include "../../tsfresh_amd/csrc/fam_spectral.h"
#include "../../tsfresh_amd/csrc/tsfa_host_tables.h"
#include "../../tsfresh_amd/csrc/tsfa_layout.h"

extern "C" int tsfa_emul_sort_calc_id(const char *name) {
    for (int i = 0; i < TSFA_N_CALCS; ++i)
        if (strcmp(tsfa_calc_table[i].name, name) == 0) return i;
    return -1;
}

// bytes of the layout a launch of this shape carves (mode: k_sort's instantiation, 1 or 2)
extern "C" long long tsfa_emul_sort_lds_bytes(int maxn, int xs_bytes, int w_doubles, int mode, int with_np) {
    SortLds L;
    return (long long)L.carve(nullptr, maxn, 64, xs_bytes, w_doubles, mode == 2 ? 1 : 0, with_np);
}

template <class ST>
static void run_series(const ST *x, int n, int maxn, int mode, const std::vector<TsfaSpec> &specs, const TsfaFamHints &h,
                       int n_loop, double *row) {
    const int wd = (h.a >= 320) ? h.a : 1280;   // (tsfa_kernels.hip: launch_all_t)
    SortLds L;
    const size_t bytes = L.carve(nullptr, maxn, 64, (int)sizeof(ST), wd, mode == 2 ? 1 : 0, 1);
    std::vector<double> lds(bytes / sizeof(double) + 2);
    memset(lds.data(), 0x7f, lds.size() * sizeof(double));
    L.carve((unsigned char *)lds.data(), maxn, 64, (int)sizeof(ST), wd, mode == 2 ? 1 : 0, 1);
    const Blk b{0, 1, L.red, L.np};
    ST *xs = (ST *)L.xs;
    for (int i = 0; i < n; ++i) xs[i] = x[i];
    std::vector<unsigned short> order;
    if (mode == 2 && n >= 3) {   // (the order's owner, k_entropy_bits, leaves none for fewer than three samples)
        order.resize(n);
        for (int i = 0; i < n; ++i) order[i] = (unsigned short)i;
        std::stable_sort(order.begin(), order.end(), [&](unsigned short a, unsigned short c) { return x[a] < x[c]; });
    }
    const FrDefer nodefer{nullptr, nullptr, TSFA_PF_HDR + 2 * TSFA_FRIEDRICH_MAX_R, 0, 0};
    const int pe_hint = (mode == 2) ? h.d : 0;
    if (mode == 2)
        fam_sort_series<ST, true>(b, xs, n, specs.data(), (int)specs.size(), row, (ST *)L.srt, L.w, L.iw, h.cq, L.cq, nullptr,
                                  n_loop, L.ctx, wd, nodefer, order.empty() ? nullptr : order.data(), nullptr, pe_hint);
    else
        fam_sort_series<ST, false>(b, xs, n, specs.data(), (int)specs.size(), row, (ST *)L.srt, L.w, L.iw, h.cq, L.cq, nullptr,
                                   n_loop, L.ctx, wd, nodefer, nullptr, nullptr, 0);
    if (pe_hint != 0) {   // k_perm's code: every dimension from one sweep (fam_perm.h)
        std::vector<int> hist(TSFA_PE_HIST_WORDS + 4, 0x5a5a5a5a);
        std::vector<double> ltab(TSFA_PE_LOGS + TSFA_PE_MAXD + 1, 1.0e30);
        fam_perm_series(b, x, n, specs.data(), (int)specs.size(), row, h.d >> 8, hist.data(), ltab.data());
    }
}

// specs: SORT-family columns only.  dtype 0: float32 samples, 1: float64.  mode 1: sorted copy, sorted by the kernel; mode 2: the
// 16-bit order (the launch chooses it only where k_perm serves the plan's permutation_entropy columns: tsfa_api.cpp).
// Every series is a launch of its own when own_launch != 0, else the layout is sized for the call's longest series (<= 2048).
extern "C" int tsfa_emul_sort_extract(const tsfa_feature_spec *specs, int n_specs, const void *values, int dtype,
                                      const int64_t *offsets, int64_t n_series, int mode, int own_launch, double *out,
                                      int64_t ld, char *err, int errlen) {
    std::vector<TsfaSpec> fam;
    for (int i = 0; i < n_specs; ++i) {
        TsfaSpec s;
        s.calc = specs[i].calc;
        s.col = i;
        for (int k = 0; k < 4; ++k) s.p[k] = specs[i].p[k];
        if (s.calc < 0 || s.calc >= TSFA_N_CALCS || tsfa_calc_table[s.calc].family != TSFA_FAM_SORT) {
            snprintf(err, errlen, "spec %d: not a calculator of the SORT family", i);
            return TSFA_ERR_UNSUPPORTED;
        }
        const std::string why = tsfa_validate_spec(s);
        if (!why.empty()) {
            snprintf(err, errlen, "spec %d (%s): %s", i, tsfa_calc_table[s.calc].name, why.c_str());
            return TSFA_ERR_UNSUPPORTED;
        }
        fam.push_back(s);
    }
    TsfaFamHints h;
    tsfa_prepare_family(TSFA_FAM_SORT, fam, h);
    if (mode != 1 && mode != 2) { snprintf(err, errlen, "mode: 1 or 2"); return TSFA_ERR_INVALID; }
    if (mode == 2 && h.d == 0) {
        snprintf(err, errlen, "mode 2 needs a plan whose permutation_entropy columns go to k_perm");
        return TSFA_ERR_INVALID;
    }
    int call_maxn = 1;
    for (int64_t s = 0; s < n_series; ++s) call_maxn = std::max(call_maxn, (int)(offsets[s + 1] - offsets[s]));
    if (call_maxn > 2048) { snprintf(err, errlen, "one wavefront per series serves up to 2048 samples"); return TSFA_ERR_INVALID; }
    for (int64_t s = 0; s < n_series; ++s) {
        const int n = (int)(offsets[s + 1] - offsets[s]);
        double *row = out + s * ld;
        for (int c = 0; c < n_specs; ++c) row[c] = TSFA_NAN;
        if (n < 1) { snprintf(err, errlen, "empty series"); return TSFA_ERR_INVALID; }
        const int maxn = own_launch ? n : call_maxn;
        const int n_loop = (s % 2) ? -1 : h.c;   // both homes of the lane = column epilogue
        if (dtype == 0) run_series<float>((const float *)values + offsets[s], n, maxn, mode, fam, h, n_loop, row);
        else run_series<double>((const double *)values + offsets[s], n, maxn, mode, fam, h, n_loop, row);
    }
    return 0;
}
