// TEST INFRASTRUCTURE ONLY: the dense packer's kernel bodies (tsfresh_amd/csrc/pack_dense.h) compiled by g++ -DTSFA_EMUL and
// driven work item by work item with ONE thread per workgroup, in the order tsfa_pack_dense launches them on the GPU, after the
// same argument checks and the same choice of the route (pd_check / pd_route / pd_plan_work of the header).  The product never
// loads this; it lets tests/test_pack_dense_emul.py compare the packer with numpy indexing on a box without a GPU.
// With -DPD_EMUL_MAIN the file is a stand-alone program that runs the driver over a grid of shapes, layouts, element types and
// lengths with guard regions around both buffers: the form an AddressSanitizer / UBSan run of the bodies takes.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tsfresh_amd/csrc/pack_dense.h"

// 0: time steps of an LDS tile for an array of n_channels, 1: most channels of an LDS tile, 2: samples of a rows-route work
// item, 3: most samples a lane moves in one step of the aligned unit-stride copy (the half types'; half of it otherwise)
extern "C" int tsfa_emul_pack_dense_tile(int which, int64_t n_channels) {
    switch (which) {
    case 0: return PD_TILE_CELLS / pd_tile_c(n_channels);
    case 1: return PD_TILE_C;
    case 2: return PD_ROW_CHUNK;
    default: return pd_vec<TSFA_BF16>();
    }
}

extern "C" uint32_t tsfa_emul_f16_to_f32_bits(uint32_t h) { return pd_f16_to_f32_bits(h & 0xffffu); }
extern "C" uint32_t tsfa_emul_bf16_to_f32_bits(uint32_t h) { return pd_bf16_to_f32_bits(h & 0xffffu); }

template <int TYPE>
static void run_route(int route, const PdArgs &a, int64_t grid, uint32_t *tile) {
    const PkBlk b{0, 1};
    for (int64_t blk = 0; blk < grid; ++blk) {
        if (route == PD_ROUTE_ROWS_UNIT) pd_rows_body<TYPE, true>(b, blk, grid, a);
        else if (route == PD_ROUTE_TRANSPOSE) pd_transpose_body<TYPE>(b, blk, grid, a, tile);
        else pd_rows_body<TYPE, false>(b, blk, grid, a);
    }
}

// The arguments of tsfa_pack_dense without the device and the stream; *route_out (may be NULL): the PD_ROUTE_* taken.
// grid: emulated workgroups of the copy launch (work items beyond are taken by striding, as on the GPU).
// Returns the status tsfa_pack_dense would (TSFA_OK, TSFA_ERR_INVALID, TSFA_ERR_TOO_LONG).
extern "C" int tsfa_emul_pack_dense(const void *x, int32_t x_type, int64_t n_batch, int64_t n_channels, int64_t n_time,
                                    int64_t stride_batch, int64_t stride_channel, int64_t stride_time, const void *lengths,
                                    int32_t lengths_type, void *values_out, int64_t channel_stride_out, int64_t *offsets_out,
                                    int32_t *flags_out, int64_t grid, int32_t *route_out) {
    const char *why;
    if (int rc = pd_check(x, x_type, n_batch, n_channels, n_time, stride_batch, stride_channel, stride_time, lengths, lengths_type,
                          values_out, channel_stride_out, offsets_out, flags_out, &why))
        return rc;
    PdArgs a;
    a.x = x; a.n_batch = n_batch; a.n_channels = n_channels; a.n_time = n_time;
    a.sb = stride_batch; a.sc = stride_channel; a.st = stride_time;
    a.offsets = offsets_out; a.uniform = lengths ? 0 : 1;
    a.out = values_out; a.cso = channel_stride_out; a.flags = (unsigned int *)flags_out;
    const int route = pd_route(n_channels, stride_channel, stride_time);
    pd_plan_work(&a, route);
    if (route_out) *route_out = route;
    if (grid < 1) grid = 1;
    if (grid > a.n_work) grid = a.n_work;
    const PkBlk b{0, 1};
    pk_u64 ws[16];
    if (lengths) pd_scan_lengths_body(b, lengths, lengths_type, n_batch, n_time, offsets_out, ws, (unsigned int *)flags_out);
    else pd_offsets_body(b, 0, 1, n_batch, n_time, offsets_out);
    std::vector<uint32_t> tile(2 * PD_TILE_WORDS);
    switch (x_type) {
    case TSFA_F64: run_route<TSFA_F64>(route, a, grid, tile.data()); break;
    case TSFA_F32: run_route<TSFA_F32>(route, a, grid, tile.data()); break;
    case TSFA_F16: run_route<TSFA_F16>(route, a, grid, tile.data()); break;
    default: run_route<TSFA_BF16>(route, a, grid, tile.data()); break;
    }
    return TSFA_OK;
}

#ifdef PD_EMUL_MAIN
#include <stdio.h>
#include <stdlib.h>

// The buffers are heap blocks of EXACTLY the extent the call may touch (the sanitizer's red zones are the guard), the
// expected output comes from plain index arithmetic, and the cells of a channel beyond T must keep their fill.
static int64_t g_cases = 0, g_failed = 0;

static uint64_t expect_bits(const std::vector<unsigned char> &x, int type, int64_t i) {
    if (type == TSFA_F64) { uint64_t u; memcpy(&u, &x[(size_t)i * 8], 8); return u; }
    if (type == TSFA_F32) { uint32_t u; memcpy(&u, &x[(size_t)i * 4], 4); return u; }
    uint16_t h; memcpy(&h, &x[(size_t)i * 2], 2);
    return type == TSFA_F16 ? pd_f16_to_f32_bits(h) : pd_bf16_to_f32_bits(h);
}

static void one_case(int type, int64_t B, int64_t C, int64_t n, int64_t sb, int64_t sc, int64_t st, int64_t base, int len_mode,
                     int len_type) {
    const int isz = pd_in_size(type), osz = type == TSFA_F64 ? 8 : 4;
    const int64_t extent = base + (B - 1) * sb + (C - 1) * sc + (n - 1) * st + 1;
    std::vector<unsigned char> x((size_t)extent * isz);
    uint32_t seed = (uint32_t)(type * 7919 + B * 31 + C * 17 + n * 3 + st + len_mode);
    for (auto &v : x) { seed = seed * 1664525u + 1013904223u; v = (unsigned char)(seed >> 24); }
    std::vector<int64_t> len64((size_t)B);
    std::vector<int32_t> len32((size_t)B);
    int bad = 0;
    for (int64_t b = 0; b < B; ++b) {
        int64_t L = n;
        if (len_mode == 2) L = b == 0 ? 1 : (b == B - 1 ? n : 1 + (b * 7 + 3) % n);
        if (len_mode == 3) { L = b % 3 == 0 ? 0 : (b % 3 == 1 ? -1 : n + 1); bad = 1; }
        len64[(size_t)b] = L; len32[(size_t)b] = (int32_t)L;
    }
    const void *lengths = len_mode == 0 ? nullptr : (len_type == TSFA_I32 ? (const void *)len32.data() : (const void *)len64.data());
    const int64_t cso = B * n;
    std::vector<unsigned char> out((size_t)(C * cso) * osz, 0xA5);
    std::vector<int64_t> offsets((size_t)B + 1, -7);
    int32_t flags = 0, route = -1;
    const int rc = tsfa_emul_pack_dense(x.data() + base * isz, type, B, C, n, sb, sc, st, lengths, len_type, out.data(), cso,
                                        offsets.data(), &flags, 3, &route);
    ++g_cases;
    int ok = rc == TSFA_OK && ((flags & TSFA_DENSE_BAD_LENGTH) != 0) == (bad != 0);
    int64_t run = 0;
    for (int64_t b = 0; b < B && ok; ++b) {
        int64_t L = lengths ? len64[(size_t)b] : n;
        L = L < 0 ? 0 : (L > n ? n : L);
        ok = offsets[(size_t)b] == run;
        for (int64_t c = 0; c < C && ok; ++c)
            for (int64_t t = 0; t < L && ok; ++t) {
                const uint64_t want = expect_bits(x, type, base + b * sb + c * sc + t * st);
                uint64_t got = 0;
                memcpy(&got, &out[(size_t)(c * cso + run + t) * osz], (size_t)osz);
                ok = got == want;
            }
        run += L;
    }
    ok = ok && offsets[(size_t)B] == run;
    for (int64_t c = 0; c < C && ok; ++c)
        for (size_t k = (size_t)(c * cso + run) * osz; k < (size_t)((c + 1) * cso) * osz && ok; ++k) ok = out[k] == 0xA5;
    if (!ok) {
        ++g_failed;
        fprintf(stderr, "FAILED type %d B %lld C %lld n %lld strides %lld %lld %lld lengths %d/%d route %d rc %d\n", type, (long long)B,
                (long long)C, (long long)n, (long long)sb, (long long)sc, (long long)st, len_mode, len_type, route, rc);
    }
}

static int64_t tt(int64_t C) { return PD_TILE_CELLS / pd_tile_c(C); }

int main() {
    const int types[4] = {TSFA_F64, TSFA_F32, TSFA_F16, TSFA_BF16};
    const int64_t Bs[2] = {1, 3};
    const int64_t Cs[6] = {1, 2, 5, PD_TILE_C - 1, PD_TILE_C, PD_TILE_C + 1};
    for (int type : types)
        for (int64_t B : Bs)
            for (int64_t C : Cs)
                for (int64_t n : {(int64_t)1, (int64_t)PD_VEC - 1, (int64_t)PD_VEC, (int64_t)PD_VEC + 1, (int64_t)2 * PD_VEC, (int64_t)2 * PD_VEC + 1, tt(C) - 1, tt(C), tt(C) + 1, 2 * tt(C) + 3})
                    for (int layout = 0; layout < 4; ++layout)
                        for (int len_mode = 0; len_mode < 4; ++len_mode)
                            for (int len_type : {TSFA_I32, TSFA_I64}) {
                                if (len_mode == 0 && len_type == TSFA_I64) continue;
                                switch (layout) {
                                case 0: one_case(type, B, C, n, C * n, n, 1, 0, len_mode, len_type); break;             // [B, C, n]
                                case 1: one_case(type, B, C, n, n * C, 1, C, 0, len_mode, len_type); break;             // [B, n, C]
                                case 2: one_case(type, B, C, n, 2 * (C + 1) * (3 * n + 2), 3 * n + 2, 3, 5, len_mode, len_type); break;  // stepped, offset slice
                                default: one_case(type, B, C, n, 0, n, 1, 0, len_mode, len_type); break;                // batch expanded with stride 0
                                }
                            }
    // a row longer than one rows-route work item, in both rows routes
    one_case(TSFA_BF16, 2, 1, 2 * PD_ROW_CHUNK + 5, 2 * PD_ROW_CHUNK + 5, 0, 1, 0, 2, TSFA_I64);
    one_case(TSFA_F32, 2, 2, PD_ROW_CHUNK + 1, 4 * (PD_ROW_CHUNK + 1), 2 * (PD_ROW_CHUNK + 1), 2, 0, 0, TSFA_I32);
    printf("%lld cases, %lld failed\n", (long long)g_cases, (long long)g_failed);
    return g_failed ? 1 : 0;
}
#endif
