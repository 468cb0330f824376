// TEST INFRASTRUCTURE ONLY: the times packer's kernel body (tsfresh_amd/csrc/pack_times.h) compiled by g++ -DTSFA_EMUL and
// driven work item by work item with ONE thread per workgroup, as tsfa_pack_times launches it on the GPU, after the same
// argument checks (pt_check / pt_plan_work of the header).  The product never loads this; it lets
// tests/test_pack_times_emul.py compare the packer with pandas' arithmetic on a box without a GPU.
// With -DPT_EMUL_MAIN the file is a stand-alone program that runs the driver over a grid of shapes, strides, types and
// lengths with heap blocks of exactly the extent the call may touch: the form an AddressSanitizer / UBSan run of the body
// takes.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tsfresh_amd/csrc/pack_times.h"

// samples of one work item
extern "C" int tsfa_emul_pack_times_chunk(void) { return PD_ROW_CHUNK; }

template <int TYPE>
static void run_rows(const PtArgs &a, int64_t grid) {
    const PkBlk b{0, 1};
    for (int64_t blk = 0; blk < grid; ++blk) {
        if (a.st == 1) pt_rows_body<TYPE, true>(b, blk, grid, a);
        else pt_rows_body<TYPE, false>(b, blk, grid, a);
    }
}

// The arguments of tsfa_pack_times without the device and the stream.  grid: emulated workgroups of the launch (work items
// beyond are taken by striding, as on the GPU).  Returns the status tsfa_pack_times would.
extern "C" int tsfa_emul_pack_times(const void *t, int32_t t_type, int64_t ticks_per_second, int64_t n_batch, int64_t n_time,
                                    int64_t stride_batch, int64_t stride_time, const int64_t *offsets, double *hours_out,
                                    int32_t *flags_out, int64_t grid) {
    const char *why;
    if (int rc = pt_check(t, t_type, ticks_per_second, n_batch, n_time, stride_batch, stride_time, offsets, hours_out, flags_out, &why))
        return rc;
    PtArgs a;
    a.t = t; a.n_batch = n_batch; a.n_time = n_time; a.sb = stride_batch; a.st = stride_time;
    a.tps = t_type == TSFA_I64 ? (double)ticks_per_second : 1.0;
    a.offsets = offsets; a.out = hours_out; a.flags = (unsigned int *)flags_out;
    pt_plan_work(&a);
    if (grid < 1) grid = 1;
    if (grid > a.n_work) grid = a.n_work;
    if (t_type == TSFA_I64) run_rows<TSFA_I64>(a, grid);
    else run_rows<TSFA_F64>(a, grid);
    return TSFA_OK;
}

#ifdef PT_EMUL_MAIN
#include <math.h>
#include <stdio.h>

static int64_t g_cases = 0, g_failed = 0;

// layout 0: contiguous (B, n); 1: one clock (stride_batch 0); 2: transposed (stride_time = B); 3: stepped, offset slice
static void one_case(int type, int64_t B, int64_t n, int layout, int ragged, int64_t tps) {
    int64_t sb = n, st = 1, base = 0;
    if (layout == 1) sb = 0;
    if (layout == 2) { sb = 1; st = B; }
    if (layout == 3) { sb = 2 * (3 * n + 2); st = 3; base = 5; }
    const int64_t extent = base + (B - 1) * sb + (n - 1) * st + 1;
    std::vector<int64_t> len((size_t)B), offsets((size_t)B + 1);
    int64_t T = 0;
    for (int64_t b = 0; b < B; ++b) {
        len[(size_t)b] = !ragged ? n : (b == 0 ? 1 : (b == B - 1 ? n : 1 + (b * 7 + 3) % n));
        offsets[(size_t)b] = T;
        T += len[(size_t)b];
    }
    offsets[(size_t)B] = T;
    std::vector<int64_t> ti((size_t)extent);
    std::vector<double> tf((size_t)extent);
    uint64_t seed = (uint64_t)(type * 7919 + B * 31 + n * 3 + layout * 5 + ragged);
    for (int64_t i = 0; i < extent; ++i) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        ti[(size_t)i] = (int64_t)(seed >> 12) - ((int64_t)1 << 50);
        tf[(size_t)i] = (double)(int64_t)(seed >> 40) * 0.001;
    }
    std::vector<double> out((size_t)T);   // EXACTLY T cells
    int32_t flags = 0;
    const void *tp = type == TSFA_I64 ? (const void *)(ti.data() + base) : (const void *)(tf.data() + base);
    const int rc = tsfa_emul_pack_times(tp, type, tps, B, n, sb, st, offsets.data(), out.data(), &flags, 3);
    ++g_cases;
    int ok = rc == TSFA_OK && flags == 0;
    for (int64_t b = 0; b < B && ok; ++b)
        for (int64_t i = 0; i < len[(size_t)b] && ok; ++i) {
            double want;
            if (type == TSFA_I64) want = (double)(ti[(size_t)(base + b * sb + i * st)] - ti[(size_t)(base + b * sb)]) / (double)tps / 3600.0;
            else want = (tf[(size_t)(base + b * sb + i * st)] - tf[(size_t)(base + b * sb)]) / 3600.0;
            ok = memcmp(&want, &out[(size_t)(offsets[(size_t)b] + i)], 8) == 0;
        }
    if (!ok) {
        ++g_failed;
        fprintf(stderr, "FAILED type %d B %lld n %lld layout %d ragged %d rc %d flags %d\n", type, (long long)B, (long long)n, layout,
                ragged, rc, flags);
    }
}

int main() {
    for (int type : {TSFA_I64, TSFA_F64})
        for (int64_t B : {(int64_t)1, (int64_t)3, (int64_t)5})
            for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)7, (int64_t)PD_ROW_CHUNK - 1, (int64_t)PD_ROW_CHUNK, (int64_t)PD_ROW_CHUNK + 1,
                              (int64_t)2 * PD_ROW_CHUNK + 5})
                for (int layout = 0; layout < 4; ++layout)
                    for (int ragged = 0; ragged < 2; ++ragged)
                        for (int64_t tps : {(int64_t)1, (int64_t)1000000000}) one_case(type, B, n, layout, ragged, tps);
    printf("%lld cases, %lld failed\n", (long long)g_cases, (long long)g_failed);
    return g_failed ? 1 : 0;
}
#endif
