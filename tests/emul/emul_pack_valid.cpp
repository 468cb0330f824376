// TEST INFRASTRUCTURE ONLY: the valid-step packer's kernel bodies (tsfresh_amd/csrc/pack_valid.h) compiled by g++ -DTSFA_EMUL
// and driven work item by work item with ONE thread per workgroup that stands for one wavefront and loops over its 64 lanes,
// in the order tsfa_pack_dense_valid launches them on the GPU (count, scan, compact), after the same argument checks
// (pv_check / pv_plan_work of the header).  The product never loads this; it lets tests/test_pack_valid_emul.py compare the
// packer with a numpy statement of dropna() on a box without a GPU.
// With -DPV_EMUL_MAIN the file is a stand-alone program that runs the driver over a grid of shapes, layouts, types, validity
// patterns and lengths with heap blocks of exactly the extent the call may touch: the form an AddressSanitizer / UBSan run
// of the bodies takes.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tsfresh_amd/csrc/pack_valid.h"

// 0: steps of one work item; 1: steps of one round (one vote); 2: scratch bytes per work item
extern "C" int tsfa_emul_pack_valid_const(int what) {
    return what == 0 ? PD_ROW_CHUNK : (what == 1 ? 64 : PV_SCRATCH_WORDS * 8);
}

template <int TYPE, bool UNIT>
static void run_typed(const PvArgs &a, int64_t grid) {
    const PkBlk b{0, 1};
    unsigned int ws_count[1];
    pk_u64 ws_scan[16];
    for (int64_t blk = 0; blk < grid; ++blk) pv_count_body<TYPE, UNIT>(b, blk, grid, a, ws_count);
    pv_scan_body(b, a, ws_scan);
    for (int64_t blk = 0; blk < grid; ++blk) pv_compact_body<TYPE, UNIT>(b, blk, grid, a);
}

template <int TYPE>
static void run(const PvArgs &a, int64_t grid) {
    if (a.st == 1) run_typed<TYPE, true>(a, grid);
    else run_typed<TYPE, false>(a, grid);
}

// The arguments of tsfa_pack_dense_valid without the device and the stream.  grid: emulated workgroups of the two strided
// launches (work items beyond are taken by striding, as on the GPU).  Returns the status tsfa_pack_dense_valid would.
extern "C" int tsfa_emul_pack_valid(const void *x, int32_t x_type, int64_t n_batch, int64_t n_channels, int64_t n_time,
                                    int64_t stride_batch, int64_t stride_channel, int64_t stride_time, const void *lengths,
                                    int32_t lengths_type, const void *t, int32_t t_type, int64_t t_stride_batch,
                                    int64_t t_stride_time, void *values_out, int64_t channel_stride_out, int64_t *offsets_out,
                                    int32_t *steps_out, void *stamps_out, void *scratch, int64_t scratch_bytes,
                                    int32_t *flags_out, int64_t grid) {
    const char *why;
    if (int rc = pv_check(x, x_type, n_batch, n_channels, n_time, stride_batch, stride_channel, stride_time, lengths, lengths_type,
                          t, t_type, t_stride_batch, t_stride_time, values_out, channel_stride_out, offsets_out, steps_out,
                          stamps_out, scratch, scratch_bytes, flags_out, &why))
        return rc;
    PvArgs a;
    a.x = x; a.n_batch = n_batch; a.n_channels = n_channels; a.n_time = n_time;
    a.sb = stride_batch; a.sc = stride_channel; a.st = stride_time;
    a.lengths = lengths; a.lengths_type = lengths_type;
    a.t = t; a.t_type = t_type; a.tsb = t_stride_batch; a.tst = t_stride_time;
    a.out = values_out; a.cso = channel_stride_out; a.offsets = offsets_out; a.steps = steps_out;
    a.stamps = (pk_u64 *)stamps_out; a.flags = (unsigned int *)flags_out;
    pv_plan_work(&a, scratch);
    if (grid < 1) grid = 1;
    if (grid > a.n_work) grid = a.n_work;
    switch (x_type) {
    case TSFA_F64: run<TSFA_F64>(a, grid); break;
    case TSFA_F32: run<TSFA_F32>(a, grid); break;
    case TSFA_F16: run<TSFA_F16>(a, grid); break;
    default: run<TSFA_BF16>(a, grid); break;
    }
    return TSFA_OK;
}

#ifdef PV_EMUL_MAIN
#include <stdio.h>

static int64_t g_cases = 0, g_failed = 0;

static int isz_of(int type) { return type == TSFA_F64 ? 8 : (type == TSFA_F32 ? 4 : 2); }

// NaN / a finite value as the bit pattern of `type` (a NaN payload that is not the canonical one for the half types)
static uint64_t nan_bits(int type) {
    return type == TSFA_F64 ? 0x7ff0000000000001ull : (type == TSFA_F32 ? 0xffc00001u : (type == TSFA_F16 ? 0x7c01u : 0xff81u));
}
static uint64_t fin_bits(int type, uint64_t seed) {
    if (type == TSFA_F64) return (0x3ffull << 52) | (seed & 0xfffffffffffffull);
    if (type == TSFA_F32) return 0x3f800000u | (uint32_t)(seed & 0x7fffffu);
    if (type == TSFA_F16) return 0x3c00u | (uint32_t)(seed & 0x3ffu);
    return 0x3f80u | (uint32_t)(seed & 0x7fu);
}
static void put(std::vector<unsigned char> &buf, int type, int64_t i, uint64_t bits) { memcpy(buf.data() + i * isz_of(type), &bits, (size_t)isz_of(type)); }
static uint64_t get(const std::vector<unsigned char> &buf, int type, int64_t i) {
    uint64_t bits = 0;
    memcpy(&bits, buf.data() + i * isz_of(type), (size_t)isz_of(type));
    return bits;
}
static uint64_t out_bits(int type, uint64_t in) {
    if (type == TSFA_F16) return pd_f16_to_f32_bits((uint32_t)in);
    if (type == TSFA_BF16) return pd_bf16_to_f32_bits((uint32_t)in);
    return in;
}

// pattern 0: all kept; 1: every other step; 2: only the first; 3: only the last; 4: a run of 64 dropped steps across a chunk
// edge; 5: NaN only in the last channel, every third step; 6: a NaT stamp every fifth step, values fine
static bool dropped(int pattern, int64_t t, int64_t len, int64_t c, int64_t C, bool *by_stamp) {
    *by_stamp = false;
    switch (pattern) {
    case 0: return false;
    case 1: return (t & 1) && c == t % C;
    case 2: return t > 0 && c == 0;
    case 3: return t < len - 1 && c == C - 1;
    case 4: return t >= PD_ROW_CHUNK - 30 && t < PD_ROW_CHUNK + 34 && c == 0;
    case 5: return t % 3 == 1 && c == C - 1;
    default: *by_stamp = t % 5 == 2; return false;
    }
}

// layout 0: (B, C, n) contiguous; 1: channels-last (B, n, C); 2: stepped and offset in time
static void one_case(int type, int64_t B, int64_t C, int64_t n, int layout, int pattern, int ragged, int stamps) {
    int64_t sb = C * n, sc = n, st = 1, base = 0;
    if (layout == 1) { sb = n * C; sc = 1; st = C; }
    if (layout == 2) { st = 3; sc = 3 * n + 1; sb = C * sc + 2; base = 3; }
    const int64_t extent = base + (B - 1) * sb + (C - 1) * sc + (n - 1) * st + 1;
    std::vector<int64_t> len((size_t)B);
    for (int64_t b = 0; b < B; ++b) len[(size_t)b] = !ragged ? n : (b == 0 ? 1 : (b == B - 1 ? n : 1 + (b * 7 + 3) % n));
    std::vector<unsigned char> xb((size_t)(extent * isz_of(type)));
    std::vector<int64_t> tb((size_t)(B * n));
    std::vector<std::vector<int64_t>> kept((size_t)B);
    uint64_t seed = (uint64_t)(type * 7919 + B * 31 + n * 3 + layout * 5 + pattern * 11 + ragged);
    for (int64_t i = 0; i < extent; ++i) put(xb, type, i, nan_bits(type));   // the cells no series owns, and the padding
    for (int64_t b = 0; b < B; ++b)
        for (int64_t t = 0; t < n; ++t) {
            bool keep = t < len[(size_t)b], by_stamp = false;
            tb[(size_t)(b * n + t)] = 1000 * b + t;
            for (int64_t c = 0; c < C; ++c) {
                seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                const bool drop = t >= len[(size_t)b] || dropped(pattern, t, len[(size_t)b], c, C, &by_stamp);
                put(xb, type, base + b * sb + c * sc + t * st, drop ? nan_bits(type) : fin_bits(type, seed >> 20));
                if (drop) keep = false;
                if (by_stamp && stamps && t < len[(size_t)b]) { tb[(size_t)(b * n + t)] = PT_NAT; keep = false; }
            }
            if (t >= len[(size_t)b]) tb[(size_t)(b * n + t)] = PT_NAT;
            if (keep) kept[(size_t)b].push_back(t);
        }
    int64_t T = 0;
    bool empty = false;
    for (int64_t b = 0; b < B; ++b) { T += (int64_t)kept[(size_t)b].size(); empty = empty || kept[(size_t)b].empty(); }
    const int osz = type == TSFA_F64 ? 8 : 4;
    // EXACTLY the cells the call may touch: C channels of B * n (the last one only to T), T steps, B * n stamps, the scratch
    const int64_t cso = B * n, n_work = B * pv_per_row(n);
    std::vector<unsigned char> out((size_t)(((C - 1) * cso + T) * osz));
    std::vector<int64_t> offsets((size_t)B + 1), stamps_out((size_t)(B * n));
    std::vector<int32_t> steps((size_t)T);
    std::vector<uint64_t> scratch((size_t)(n_work * PV_SCRATCH_WORDS));
    std::vector<int64_t> lens64(len);
    int32_t flags = 0;
    const int rc = tsfa_emul_pack_valid(xb.data() + base * isz_of(type), type, B, C, n, sb, sc, st, ragged ? lens64.data() : nullptr,
                                        TSFA_I64, stamps ? tb.data() : nullptr, TSFA_I64, n, 1, out.data(), cso, offsets.data(),
                                        steps.data(), stamps ? stamps_out.data() : nullptr, scratch.data(),
                                        (int64_t)(scratch.size() * 8), &flags, 3);
    ++g_cases;
    int ok = rc == TSFA_OK && flags == (empty ? TSFA_DENSE_EMPTY_SERIES : 0) && offsets[(size_t)B] == T;
    int64_t at = 0;
    for (int64_t b = 0; b < B && ok; ++b) {
        ok = offsets[(size_t)b] == at;
        for (size_t k = 0; k < kept[(size_t)b].size() && ok; ++k, ++at) {
            const int64_t t = kept[(size_t)b][k];
            ok = steps[(size_t)at] == t && (!stamps || stamps_out[(size_t)(b * n) + k] == 1000 * b + t);
            for (int64_t c = 0; c < C && ok; ++c) {
                uint64_t got = 0;
                memcpy(&got, out.data() + (c * cso + at) * osz, (size_t)osz);
                ok = got == out_bits(type, get(xb, type, base + b * sb + c * sc + t * st));
            }
        }
    }
    if (!ok) {
        ++g_failed;
        fprintf(stderr, "FAILED type %d B %lld C %lld n %lld layout %d pattern %d ragged %d stamps %d rc %d flags %d\n", type,
                (long long)B, (long long)C, (long long)n, layout, pattern, ragged, stamps, rc, flags);
    }
}

int main() {
    for (int type : {TSFA_F64, TSFA_F32, TSFA_F16, TSFA_BF16})
        for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)2049})
            for (int layout = 0; layout < 3; ++layout)
                for (int pattern = 0; pattern < 7; ++pattern)
                    for (int ragged = 0; ragged < 2; ++ragged) {
                        one_case(type, 3, 3, n, layout, pattern, ragged, pattern == 6);
                        if (layout == 1 && (n == 65 || n == 1025)) one_case(type, 2, 33, n, layout, pattern, ragged, 1);
                        if (layout == 0 && n == 63) one_case(type, 7, 1, n, layout, pattern, ragged, 0);   // more than 4 scanned entries
                    }
    printf("%lld cases, %lld failed\n", (long long)g_cases, (long long)g_failed);
    return g_failed ? 1 : 0;
}
#endif
