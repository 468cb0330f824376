// Device packer of the C-ABI (include/tsfresh_amd.h: tsfa_pack_device*): the kernels around the bodies of pack_device.h
// and the host code that strings them together.  See pack_device.h for the scratch formula and the sort's design.
// tsfa_pack_device and tsfa_pack_set_create share their steps 1-3 -- min / max, keys, the planned radix passes between two
// buffer sets -- as PkSorter, which states the invariants the kernels rely on (n_tiles, the size and reuse of counts, one
// buffer set when in order); each entry goes on with its own boundary and gather kernels.  tests/emul/emul_pack_sort.h is the
// sorter's twin on looped kernel bodies.  Staging, argument checks, view filling and copy-out are one helper each.
// The window builder (tsfa_roll_windows, roll_device.h) lives here as well: it reads a pack's buffers and reuses k_pack_scan.
// So does the row packer (tsfa_pack_set_rows, tsfa_pack_set_hours; pack_rows.h): it reads a set's permutation and offsets.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "pack_device.h"
#include "pack_rows.h"
#include "roll_device.h"
#include "tsfa_devmem.h"

struct tsfa_pack {
    int32_t device = 0;
    int64_t n_rows = 0, n_groups = 0;
    int32_t flags = 0, n_passes = 0;
    int32_t id_type = 0, sort_type = 0, out_type = TSFA_F64;
    // device buffers: the pointers are the views the accessors return, hold[k] keeps buffer k alive (pk_share).  A pack made
    // by tsfa_pack_device is the only holder of its four; one handed out by tsfa_pack_set_values looks into buffers it
    // shares with the set and with its sibling packs.  Either way destroying the pack only drops its references.
    void *values = nullptr;      // ragged buffer, n_rows x out_type
    int64_t *offsets = nullptr;  // n_groups + 1
    void *uniq = nullptr;        // n_groups x id_type
    void *sort = nullptr;        // n_rows x sort_type (TSFA_PACK_KEEP_SORT)
    std::shared_ptr<void> hold[4];  // values, offsets, uniq, sort
};

// One frame sorted once by (kind, id, sort): see include/tsfresh_amd.h.  Every device buffer is reference-counted: it goes
// with its last holder, the set or a pack, whichever is destroyed last.
struct tsfa_pack_set {
    int32_t device = 0;
    int64_t n_rows = 0, n_groups = 0;
    int32_t n_kinds = 0, flags = 0, n_passes = 0;
    int32_t id_type = 0, sort_type = 0, kind_type = 0;
    bool has_kinds = false;
    std::shared_ptr<void> perm;     // n_rows x uint32: sorted position -> input row
    std::shared_ptr<void> offsets;  // n_groups + 1 int64 over the whole sorted frame
    std::shared_ptr<void> rebased;  // n_groups + n_kinds int64 (several kinds only): pk_rebase_body's layout
    std::shared_ptr<void> uniq;     // n_groups x id_type; kind k owns [kind_groups[k], kind_groups[k + 1])
    std::shared_ptr<void> sort;     // n_rows x sort_type (TSFA_PACK_KEEP_SORT)
    std::vector<int64_t> kind_rows, kind_groups;  // n_kinds + 1 each (host copies)
    std::vector<unsigned char> kind_vals;         // n_kinds x kind_type (host copy), ascending
};

namespace {

#define PK_GRID_THREADS 256

__global__ void __launch_bounds__(PK_GRID_THREADS) k_pack_minmax(const void *ids, int id_type, const void *sort, int sort_type,
                                                                   int64_t n, PkStats *st) {
    __shared__ pk_u64 red[5];
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pk_minmax_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, ids, id_type, sort, sort_type, n, red, st);
}

__global__ void __launch_bounds__(PK_GRID_THREADS) k_pack_keys(const void *ids, int id_type, const void *sort, int sort_type,
                                                                 int64_t n, pk_u64 min0, pk_u64 min1, int nb0, int nb1, int do_hist,
                                                                 pk_u64 *hi, pk_u64 *lo, uint32_t *idx, PkStats *st) {
    __shared__ unsigned int lh[16 * PK_RADIX];
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pk_keys_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, ids, id_type, sort, sort_type, n, min0, min1,
                 nb0, nb1, do_hist, hi, lo, idx, lh, st);
}

// ---- the three sort kernels of one pass ----
__global__ void __launch_bounds__(PK_THREADS) k_pack_hist(int64_t n_tiles, const pk_u64 *key, int shift, int64_t n, uint32_t *counts) {
    __shared__ unsigned int lh[PK_RADIX];
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    pk_hist_body(b, (int64_t)blockIdx.x, n_tiles, key, shift, n, lh, counts);
}

__global__ void __launch_bounds__(PK_SCAN_THREADS) k_pack_scan(uint32_t *data, size_t m, unsigned int *total_out) {
    __shared__ unsigned int ws[16];
    const PkBlk b{(int)threadIdx.x, PK_SCAN_THREADS};
    pk_scan_body(b, data, m, ws, total_out);
}

__global__ void __launch_bounds__(PK_THREADS) k_pack_scatter(int64_t n_tiles, const pk_u64 *key, int shift, int64_t n,
                                                              const uint32_t *scanned, const pk_u64 *hi_in, const pk_u64 *lo_in,
                                                              const uint32_t *idx_in, pk_u64 *hi_out, pk_u64 *lo_out, uint32_t *idx_out) {
    __shared__ unsigned int wbase[(PK_THREADS / 64) * PK_RADIX];
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    pk_scatter_body(b, (int64_t)blockIdx.x, n_tiles, key, shift, n, scanned, hi_in, lo_in, idx_in, hi_out, lo_out, idx_out, wbase);
}

__global__ void __launch_bounds__(PK_THREADS) k_pack_heads(const pk_u64 *hi, int64_t n, uint32_t *tile_heads) {
    __shared__ unsigned int cnt;
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    pk_heads_count_body(b, (int64_t)blockIdx.x, hi, n, &cnt, tile_heads);
}

__global__ void __launch_bounds__(PK_THREADS) k_pack_groups(const pk_u64 *hi, const uint32_t *idx, int64_t n, const uint32_t *tile_heads,
                                                             int64_t n_groups, const void *ids, int id_size, int64_t *offsets, void *uniq) {
    __shared__ unsigned int ws[16];
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    pk_groups_body(b, (int64_t)blockIdx.x, hi, idx, n, tile_heads, n_groups, ids, id_size, offsets, uniq, ws);
}

__global__ void __launch_bounds__(PK_GRID_THREADS) k_pack_gather(const void *values, int value_type, const uint32_t *idx, int64_t n,
                                                                   void *out, PkStats *st) {
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pk_gather_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, values, value_type, idx, n, out, st);
}

__global__ void __launch_bounds__(PK_GRID_THREADS) k_pack_gather_raw(const void *col, int itemsize, const uint32_t *idx, int64_t n, void *out) {
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pk_gather_raw_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, col, itemsize, idx, n, out);
}

// ---- the pack set's kernels ----
__global__ void __launch_bounds__(PK_GRID_THREADS) k_pack_kind_minmax(const void *kinds, int kind_type, const void *ids, int id_type,
                                                                        const void *sort, int sort_type, int64_t n, PkSetStats *st) {
    __shared__ pk_u64 red[3];
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pk_kind_minmax_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, kinds, kind_type, ids, id_type, sort,
                        sort_type, n, red, st);
}

__global__ void __launch_bounds__(PK_GRID_THREADS) k_pack_kind_hist(const void *kinds, int kind_type, int64_t n, pk_u64 kmin, int nb,
                                                                      PkSetStats *st) {
    __shared__ unsigned int lh[8 * PK_RADIX];
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pk_kind_hist_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, kinds, kind_type, n, kmin, nb, lh, st);
}

__global__ void __launch_bounds__(PK_THREADS) k_pack_hist_kind(int64_t n_tiles, PkKindDigit dg, int64_t n, uint32_t *counts) {
    __shared__ unsigned int lh[PK_RADIX];
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    pk_hist_impl(b, (int64_t)blockIdx.x, n_tiles, dg, n, lh, counts);
}

__global__ void __launch_bounds__(PK_THREADS) k_pack_scatter_kind(int64_t n_tiles, PkKindDigit dg, int64_t n, const uint32_t *scanned,
                                                                   const pk_u64 *hi_in, const pk_u64 *lo_in, const uint32_t *idx_in,
                                                                   pk_u64 *hi_out, pk_u64 *lo_out, uint32_t *idx_out) {
    __shared__ unsigned int wbase[(PK_THREADS / 64) * PK_RADIX];
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    pk_scatter_impl(b, (int64_t)blockIdx.x, n_tiles, dg, n, scanned, hi_in, lo_in, idx_in, hi_out, lo_out, idx_out, wbase);
}

__global__ void __launch_bounds__(PK_THREADS) k_pack_set_heads(const pk_u64 *hi, const uint32_t *idx, const void *kinds, int kind_type,
                                                                int64_t n, uint32_t *tile_heads, uint32_t *tile_kheads) {
    __shared__ unsigned int cnt[2];
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    pk_set_heads_count_body(b, (int64_t)blockIdx.x, hi, idx, kinds, kind_type, n, cnt, tile_heads, tile_kheads);
}

__global__ void __launch_bounds__(PK_THREADS) k_pack_set_groups(const pk_u64 *hi, const uint32_t *idx, const void *kinds, int kind_type,
                                                                 int64_t n, const uint32_t *tile_heads, const uint32_t *tile_kheads,
                                                                 int64_t n_groups, int64_t n_kinds, const void *ids, int id_size,
                                                                 int64_t *offsets, void *uniq, int64_t *kind_rows, int64_t *kind_groups,
                                                                 void *kind_vals) {
    __shared__ unsigned int ws[16];
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    pk_set_groups_body(b, (int64_t)blockIdx.x, hi, idx, kinds, kind_type, n, tile_heads, tile_kheads, n_groups, n_kinds, ids, id_size,
                       offsets, uniq, kind_rows, kind_groups, kind_vals, ws);
}

__global__ void __launch_bounds__(PK_GRID_THREADS) k_pack_rebase(const int64_t *global, const int64_t *kind_rows,
                                                                   const int64_t *kind_groups, int64_t n_kinds, int64_t total,
                                                                   int64_t *out) {
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pk_rebase_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, global, kind_rows, kind_groups, n_kinds, total,
                   out);
}

// ---- the row packer's kernels (pack_rows.h) ----
template <int TYPE>
__global__ void __launch_bounds__(PD_THREADS) k_pack_rows_tiles(PrArgs a) {
    __shared__ uint32_t tile[(TYPE == TSFA_F32 ? 1 : 2) * PD_TILE_WORDS];
    __shared__ uint32_t rows[PD_TILE_CELLS / 2];
    const PkBlk b{(int)threadIdx.x, PD_THREADS};
    pr_tiles_body<TYPE>(b, (int64_t)blockIdx.x, (int64_t)gridDim.x, a, tile, rows);
}

template <int TYPE>
__global__ void __launch_bounds__(PK_GRID_THREADS) k_pack_rows_gather(PrArgs a) {
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pr_gather_body<TYPE>(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, a);
}

template <int TYPE>
__global__ void __launch_bounds__(PK_THREADS) k_pack_set_hours(PhArgs a) {
    __shared__ uint32_t starts[PK_TILE];
    __shared__ int64_t head;
    const PkBlk b{(int)threadIdx.x, PK_THREADS};
    ph_hours_body<TYPE>(b, (int64_t)blockIdx.x, (int64_t)gridDim.x, a, starts, &head);
}

// a device buffer as several holders keep it: freed on its device when the last of them goes
std::shared_ptr<void> pk_share(void *p, int32_t device) {
    return std::shared_ptr<void>(p, [device](void *q) {
        (void)hipSetDevice(device);
        (void)hipFree(q);
    });
}

int pk_grid(int64_t n) {
    const int64_t blocks = (n + PK_GRID_THREADS - 1) / PK_GRID_THREADS;
    return (int)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
}

// A pack that looks into the buffers of `set` and into `out`, the ragged samples of one call: what the views of
// tsfa_pack_set_values and tsfa_pack_set_rows have in common.  The caller sets rows, groups and the four pointers.
tsfa_pack *pk_view(const tsfa_pack_set *set, int out_type, unsigned int nan_flag, const std::shared_ptr<void> &out) {
    tsfa_pack *pk = new tsfa_pack();
    pk->device = set->device;
    pk->flags = set->flags | (nan_flag ? TSFA_PACK_VALUE_NAN : 0);
    pk->n_passes = set->n_passes;
    pk->id_type = set->id_type; pk->sort_type = set->sort_type; pk->out_type = out_type;
    pk->hold[0] = out;
    pk->hold[1] = set->rebased ? set->rebased : set->offsets;  // (several kinds : one)
    pk->hold[2] = set->uniq;
    pk->hold[3] = set->sort;
    return pk;
}

// ---- what several entry points share.  Each helper takes its entry's name as `who` (an argument or a member), and that is
// ---- the function HIP_TRY and HIP_TRY_ALLOC name in the messages here.
#undef TSFA_WHO
#define TSFA_WHO who

// A host column (TSFA_HOST) is staged: `own` takes the device copy and *col is repointed at it.  A device column
// (TSFA_DEVICE) and an absent one (NULL) stay as they are.  what: the column's noun in the out-of-memory message.
int pk_stage(const char *who, int32_t space, DevPtr<void> &own, const void **col, size_t bytes, const char *what) {
    if (space != TSFA_HOST || !*col) return TSFA_OK;
    HIP_TRY_ALLOC(own, bytes, what);
    HIP_TRY(hipMemcpy(own.get(), *col, bytes, hipMemcpyHostToDevice));
    *col = own.get();
    return TSFA_OK;
}

// The argument checks of tsfa_pack_device and tsfa_pack_set_create, in the order both make them.  own: NULL, or what the
// entry refuses its own column with (values / kinds); it is reported where both report it, after the key columns' types.
// dev_who: the name in front of the device check's messages.
int pk_check_frame(const char *who, const void *ids, int32_t id_type, const void *sort, int32_t sort_type, int64_t n_rows,
                   int32_t space, int32_t options, const char *own, const char *dev_who, int32_t device) {
    const auto refuse = [who](int code, const char *why) { return tsfa_fail(code, (std::string(who) + ": " + why).c_str()); };
    if (!ids || n_rows < 1 || (space != TSFA_HOST && space != TSFA_DEVICE) || (options & ~TSFA_PACK_KEEP_SORT))
        return refuse(TSFA_ERR_INVALID, "bad arguments");
    if (!pk_is_key_type(id_type, false)) return refuse(TSFA_ERR_INVALID, "the id column must be of an integer type");
    if (sort && !pk_is_key_type(sort_type, true))
        return refuse(TSFA_ERR_INVALID, "the sort column must be of an integer type, float32 or float64");
    if (own) return refuse(TSFA_ERR_INVALID, own);
    if ((options & TSFA_PACK_KEEP_SORT) && !sort) return refuse(TSFA_ERR_INVALID, "TSFA_PACK_KEEP_SORT without a sort column");
    if (int rc = tsfa_check_device(dev_who, device)) return rc;
    if (n_rows > 0xffffffffll) return refuse(TSFA_ERR_TOO_LONG, "more than 4 294 967 295 rows (the row indices are 32 bits wide)");
    return TSFA_OK;
}

// Steps 1-3 of tsfa_pack_device and tsfa_pack_set_create: the rows' indices sorted by (id, sort) or, with a kind column, by
// (kind, id, sort), on the null stream.  After run() the entry reads hi[cur] / idx[cur] (the sorted id keys and the
// permutation), counts, d_st and st, in_order and n_passes, and goes on with its own step 4; what it does not release()
// goes with the sorter.  tests/emul/emul_pack_sort.h is the same sequence on looped kernel bodies.
struct PkSorter {
    const char *who;                 // the entry point the messages name
    PkStats st;                      // host copy of *d_st, as last read back
    PkSetStats ks;                   // host copy of *d_ks, the caller's kind counters (read back here only with a kind column)
    DevPtr<PkStats> d_st;
    DevPtr<pk_u64> hi[2], lo[2];     // id and sort keys of the rows in the order of idx
    DevPtr<uint32_t> idx[2], counts;
    int64_t n_tiles = 0;
    int cur = 0, n_passes = 0;       // the live set of hi / lo / idx; the passes that ran
    bool in_order = false;

    explicit PkSorter(const char *w) : who(w) { pk_set_stats_init(&ks); }

    // kinds (optional) with d_ks, its initialised counters on the device: without a kind column nothing is launched,
    // allocated or copied on its behalf.  n <= 2^32 - 1 (pk_check_frame).
    int run(const void *ids, int id_type, const void *sort, int sort_type, int64_t n, const void *kinds = nullptr, int kind_type = 0,
            PkSetStats *d_ks = nullptr) {
        // INVARIANT n_tiles = ceil(n / PK_TILE) is the grid of every tile kernel (k_pack_hist*, k_pack_scatter*, the entries'
        // heads and groups kernels): block t owns rows [t * PK_TILE, (t + 1) * PK_TILE) and row t * PK_RADIX .. of counts.
        n_tiles = (n + PK_TILE - 1) / PK_TILE;
        HIP_TRY_ALLOC(d_st, sizeof(PkStats), "the packer's counters");
        pk_stats_init(&st);
        HIP_TRY(hipMemcpy(d_st.get(), &st, sizeof(st), hipMemcpyHostToDevice));

        // 1. min / max of the keys, descents of (id, sort) and of (kind, id, sort)
        k_pack_minmax<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(ids, id_type, sort, sort_type, n, d_st.get());
        if (kinds) k_pack_kind_minmax<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(kinds, kind_type, ids, id_type, sort, sort_type, n, d_ks);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&st, d_st.get(), sizeof(st), hipMemcpyDeviceToHost));
        if (kinds) HIP_TRY(hipMemcpy(&ks, d_ks, sizeof(ks), hipMemcpyDeviceToHost));
        const bool inner_in_order = st.descents == 0;              // (id, sort): only the kind passes are left
        in_order = kinds ? ks.descents == 0 : inner_in_order;      // (kind, id, sort): nothing is sorted

        // 2. id and sort keys, identity permutation, byte histograms.
        // INVARIANT one set of buffers when in order: no pass runs, cur stays 0 and set 1 is never touched (20 of the 40
        // scratch bytes per row).  INVARIANT counts holds n_tiles x PK_RADIX words, a pass's (digit, tile) matrix; step 4
        // of either entry reuses its front for per-tile head counts, n_tiles words (2 n_tiles in the set) <= that size.
        for (int k = 0; k < (in_order ? 1 : 2); ++k) {
            HIP_TRY_ALLOC(hi[k], (size_t)n * 8, "the id keys (sort scratch: 40 bytes per row in all)");
            HIP_TRY_ALLOC(lo[k], (size_t)n * 8, "the sort keys (sort scratch: 40 bytes per row in all)");
            HIP_TRY_ALLOC(idx[k], (size_t)n * 4, "the row indices (sort scratch: 40 bytes per row in all)");
        }
        HIP_TRY_ALLOC(counts, (size_t)n_tiles * PK_RADIX * 4, "the per-tile digit counts");
        const int inner_passes = (in_order || inner_in_order) ? 0 : 1;
        k_pack_keys<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(ids, id_type, sort, sort_type, n, st.kmin[0], sort ? st.kmin[1] : 0ull,
                                                             pk_sig_bytes(st.kmax[0] - st.kmin[0]),
                                                             sort ? pk_sig_bytes(st.kmax[1] - st.kmin[1]) : 0, inner_passes,
                                                             hi[0].get(), lo[0].get(), idx[0].get(), d_st.get());
        if (kinds && !in_order)
            k_pack_kind_hist<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(kinds, kind_type, n, ks.kmin, pk_sig_bytes(ks.kmax - ks.kmin), d_ks);
        HIP_TRY(hipGetLastError());
        if (in_order) return TSFA_OK;

        // 3. the radix passes, least significant digit first: sort bytes, id bytes, kind bytes; constant digits are skipped.
        // A pass sorts set cur into set cur ^ 1.  The plain digit (a key word and a shift) and the kind digit (read
        // through the row index: PkKindDigit) differ only in the two launches around the scan.
        int pass_word[16], pass_byte[16], kind_byte[8];
        HIP_TRY(hipMemcpy(&st, d_st.get(), sizeof(st), hipMemcpyDeviceToHost));
        if (kinds) HIP_TRY(hipMemcpy(&ks, d_ks, sizeof(ks), hipMemcpyDeviceToHost));
        const int np = inner_passes ? pk_plan_passes(&st, n, sort != nullptr, pass_word, pass_byte) : 0;
        const int nkp = kinds ? pk_plan_kind_passes(&ks, n, kind_byte) : 0;
        for (int p = 0; p < np + nkp; ++p) {
            const bool plain = p < np;
            pk_u64 *const h0 = hi[cur].get(), *const l0 = lo[cur].get(), *const h1 = hi[cur ^ 1].get(), *const l1 = lo[cur ^ 1].get();
            uint32_t *const i0 = idx[cur].get(), *const i1 = idx[cur ^ 1].get(), *const cnt = counts.get();
            const pk_u64 *key = (plain && pass_word[p]) ? l0 : h0;
            const int shift = 8 * (plain ? pass_byte[p] : kind_byte[p - np]);
            const PkKindDigit dg{kinds, kind_type, ks.kmin, i0, shift};
            if (plain) k_pack_hist<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(n_tiles, key, shift, n, cnt);
            else k_pack_hist_kind<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(n_tiles, dg, n, cnt);
            k_pack_scan<<<1, PK_SCAN_THREADS, 0, 0>>>(cnt, (size_t)n_tiles * PK_RADIX, nullptr);
            if (plain) k_pack_scatter<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(n_tiles, key, shift, n, cnt, h0, l0, i0, h1, l1, i1);
            else k_pack_scatter_kind<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(n_tiles, dg, n, cnt, h0, l0, i0, h1, l1, i1);
            HIP_TRY(hipGetLastError());
            cur ^= 1;
        }
        n_passes = np + nkp;
        return TSFA_OK;
    }
};

}  // namespace

#undef TSFA_WHO
#define TSFA_WHO "tsfa_pack_device"
extern "C" int tsfa_pack_device(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *values,
                                int32_t value_type, int64_t n_rows, int32_t space, int32_t options, int32_t device,
                                tsfa_pack **out_pack) {
    if (!out_pack) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device: out_pack is NULL");
    *out_pack = nullptr;
    if (!values) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device: bad arguments");
    int rc = pk_check_frame(TSFA_WHO, ids, id_type, sort, sort_type, n_rows, space, options,
                            pk_itemsize(value_type) == 0 ? "unknown element type of the value column" : nullptr, TSFA_WHO, device);
    if (rc) return rc;

    const int64_t n = n_rows;
    const int id_size = pk_itemsize(id_type), sort_size = sort ? pk_itemsize(sort_type) : 0, val_size = pk_itemsize(value_type);
    const int out_type = pk_out_type(value_type);
    std::unique_ptr<tsfa_pack, void (*)(tsfa_pack *)> pk(new tsfa_pack(), tsfa_pack_device_destroy);
    pk->device = device; pk->n_rows = n; pk->id_type = id_type; pk->sort_type = sort ? sort_type : 0; pk->out_type = out_type;

    HIP_TRY(hipSetDevice(device));
    DevPtr<void> d_ids, d_sort, d_vals;  // staged copies (TSFA_HOST only)
    if ((rc = pk_stage(TSFA_WHO, space, d_ids, &ids, (size_t)n * id_size, "the id column"))) return rc;
    if ((rc = pk_stage(TSFA_WHO, space, d_sort, &sort, (size_t)n * sort_size, "the sort column"))) return rc;
    if ((rc = pk_stage(TSFA_WHO, space, d_vals, &values, (size_t)n * val_size, "the value column"))) return rc;
    // 1. - 3. the rows' indices sorted by (id, sort)
    PkSorter s(TSFA_WHO);
    if ((rc = s.run(ids, id_type, sort, sort_type, n))) return rc;
    PkStats &st = s.st;
    PkStats *const d_st = s.d_st.get();
    const int64_t n_tiles = s.n_tiles;
    const pk_u64 *const hi = s.hi[s.cur].get();
    const uint32_t *const idx = s.idx[s.cur].get();
    uint32_t *const counts = s.counts.get();
    if (s.in_order) pk->flags |= TSFA_PACK_IN_ORDER;
    pk->n_passes = s.n_passes;
    // 4. group boundaries (counts is reused for the per-tile head counts)
    k_pack_heads<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(hi, n, counts);
    k_pack_scan<<<1, PK_SCAN_THREADS, 0, 0>>>(counts, (size_t)n_tiles, &d_st->n_groups);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost));
    pk->n_groups = (int64_t)st.n_groups;
    DevPtr<int64_t> d_offsets;
    DevPtr<void> d_uniq, d_out, d_psort;
    HIP_TRY_ALLOC(d_offsets, (size_t)(pk->n_groups + 1) * 8, "the offsets");
    HIP_TRY_ALLOC(d_uniq, (size_t)pk->n_groups * id_size, "the unique ids");
    k_pack_groups<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(hi, idx, n, counts, pk->n_groups, ids, id_size, d_offsets.get(), d_uniq.get());
    HIP_TRY(hipGetLastError());
    // 5. gather
    HIP_TRY_ALLOC(d_out, (size_t)n * pk_itemsize(out_type), "the ragged sample buffer");
    k_pack_gather<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(values, value_type, idx, n, d_out.get(), d_st);
    HIP_TRY(hipGetLastError());
    if (options & TSFA_PACK_KEEP_SORT) {
        HIP_TRY_ALLOC(d_psort, (size_t)n * sort_size, "the packed sort column");
        k_pack_gather_raw<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(sort, sort_size, idx, n, d_psort.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost));  // (synchronises: the staged columns may go)
    if (st.nan_flag) pk->flags |= TSFA_PACK_VALUE_NAN;
    // the pack takes over what outlives the call
    pk->values = d_out.get(); pk->hold[0] = pk_share(d_out.release(), device);
    pk->offsets = d_offsets.get(); pk->hold[1] = pk_share(d_offsets.release(), device);
    pk->uniq = d_uniq.get(); pk->hold[2] = pk_share(d_uniq.release(), device);
    if (d_psort) { pk->sort = d_psort.get(); pk->hold[3] = pk_share(d_psort.release(), device); }
    *out_pack = pk.release();
    return TSFA_OK;
}

extern "C" int64_t tsfa_pack_device_n_rows(const tsfa_pack *pack) { return pack ? pack->n_rows : 0; }
extern "C" int64_t tsfa_pack_device_n_groups(const tsfa_pack *pack) { return pack ? pack->n_groups : 0; }
extern "C" int32_t tsfa_pack_device_flags(const tsfa_pack *pack) { return pack ? pack->flags : 0; }
extern "C" int32_t tsfa_pack_device_n_passes(const tsfa_pack *pack) { return pack ? pack->n_passes : 0; }

extern "C" int tsfa_pack_device_values(const tsfa_pack *pack, const void **values, int32_t *dtype) {
    if (!pack || !values || !dtype) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device_values: null pointer");
    *values = pack->values;
    *dtype = pack->out_type;
    return TSFA_OK;
}

extern "C" const int64_t *tsfa_pack_device_offsets(const tsfa_pack *pack) { return pack ? pack->offsets : nullptr; }
extern "C" const void *tsfa_pack_device_ids(const tsfa_pack *pack) { return pack ? pack->uniq : nullptr; }

// One device buffer of a pack or of a window set (the two handle types) to the host.  A pack refuses a buffer it does not
// hold (no TSFA_PACK_KEEP_SORT); a window set without a window has nothing to copy.
template <class Handle>
static int pk_copy_out(const Handle *h, void *dst, const void *src, size_t bytes, const char *who) {
    constexpr bool is_pack = std::is_same<Handle, tsfa_pack>::value;
    if (!h || !dst) return tsfa_fail(TSFA_ERR_INVALID, (std::string(who) + ": null pointer").c_str());
    if (is_pack && !src) return tsfa_fail(TSFA_ERR_INVALID, (std::string(who) + ": the pack does not hold that buffer").c_str());
    if (!is_pack && !bytes) return TSFA_OK;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? (int)TSFA_OK : tsfa_fail_hip(who, "hipMemcpy", e);
}

extern "C" int tsfa_pack_device_copy_ids(const tsfa_pack *pack, void *ids_host) {
    return pk_copy_out(pack, ids_host, pack ? pack->uniq : nullptr,
                       pack ? (size_t)pack->n_groups * pk_itemsize(pack->id_type) : 0, "tsfa_pack_device_copy_ids");
}

extern "C" int tsfa_pack_device_copy_offsets(const tsfa_pack *pack, int64_t *offsets_host) {
    return pk_copy_out(pack, offsets_host, pack ? pack->offsets : nullptr, pack ? (size_t)(pack->n_groups + 1) * 8 : 0,
                       "tsfa_pack_device_copy_offsets");
}

extern "C" int tsfa_pack_device_copy_sort(const tsfa_pack *pack, void *sort_host) {
    return pk_copy_out(pack, sort_host, pack ? pack->sort : nullptr,
                       pack ? (size_t)pack->n_rows * pk_itemsize(pack->sort_type) : 0, "tsfa_pack_device_copy_sort");
}

extern "C" void tsfa_pack_device_destroy(tsfa_pack *pack) {
    if (!pack) return;
    (void)hipSetDevice(pack->device);
    delete pack;  // drops the references; a buffer goes with its last holder
}

// ---------------------------------------------------------------------------------------------
// Pack set: one sort per frame, one ordinary tsfa_pack per kind and value column
// ---------------------------------------------------------------------------------------------
#undef TSFA_WHO
#define TSFA_WHO "tsfa_pack_set_create"
extern "C" int tsfa_pack_set_create(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *kinds,
                                    int32_t kind_type, int64_t n_rows, int32_t space, int32_t options, int32_t device,
                                    tsfa_pack_set **out_set) {
    if (!out_set) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_set_create: out_set is NULL");
    *out_set = nullptr;
    // (the device check names tsfa_pack_device, as it always has)
    int rc = pk_check_frame(TSFA_WHO, ids, id_type, sort, sort_type, n_rows, space, options,
                            kinds && !pk_is_key_type(kind_type, false) ? "the kind column must be of an integer type" : nullptr,
                            "tsfa_pack_device", device);
    if (rc) return rc;

    const int64_t n = n_rows;
    const int id_size = pk_itemsize(id_type), sort_size = sort ? pk_itemsize(sort_type) : 0, kind_size = kinds ? pk_itemsize(kind_type) : 0;
    std::unique_ptr<tsfa_pack_set, void (*)(tsfa_pack_set *)> set(new tsfa_pack_set(), tsfa_pack_set_destroy);
    set->device = device; set->n_rows = n; set->id_type = id_type; set->sort_type = sort ? sort_type : 0;
    set->kind_type = kinds ? kind_type : 0; set->has_kinds = kinds != nullptr;

    HIP_TRY(hipSetDevice(device));
    DevPtr<void> d_ids, d_sort, d_kinds;  // staged copies (TSFA_HOST only)
    if ((rc = pk_stage(TSFA_WHO, space, d_ids, &ids, (size_t)n * id_size, "the id column"))) return rc;
    if ((rc = pk_stage(TSFA_WHO, space, d_sort, &sort, (size_t)n * sort_size, "the sort column"))) return rc;
    if ((rc = pk_stage(TSFA_WHO, space, d_kinds, &kinds, (size_t)n * kind_size, "the kind column"))) return rc;
    // 1. - 3. the rows' indices sorted by (kind, id, sort).  The kind counters are the entry's: step 4 counts the kinds
    // in them with or without a kind column.
    PkSorter s(TSFA_WHO);
    PkSetStats &ks = s.ks;
    DevPtr<PkSetStats> d_ks_own;
    HIP_TRY_ALLOC(d_ks_own, sizeof(PkSetStats), "the packer's kind counters");
    PkSetStats *const d_ks = d_ks_own.get();
    HIP_TRY(hipMemcpy(d_ks, &ks, sizeof(ks), hipMemcpyHostToDevice));
    if ((rc = s.run(ids, id_type, sort, sort_type, n, kinds, kind_type, d_ks))) return rc;
    PkStats &st = s.st;
    PkStats *const d_st = s.d_st.get();
    const int64_t n_tiles = s.n_tiles;
    const pk_u64 *const hi = s.hi[s.cur].get();
    const uint32_t *const idx = s.idx[s.cur].get();
    uint32_t *const counts = s.counts.get();
    if (s.in_order) set->flags |= TSFA_PACK_IN_ORDER;
    set->n_passes = s.n_passes;
    // 4. group and kind boundaries (counts is reused: [0, n_tiles) head counts, [n_tiles, 2 n_tiles) kind-head counts)
    k_pack_set_heads<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(hi, idx, kinds, kind_type, n, counts, counts + n_tiles);
    k_pack_scan<<<1, PK_SCAN_THREADS, 0, 0>>>(counts, (size_t)n_tiles, &d_st->n_groups);
    k_pack_scan<<<1, PK_SCAN_THREADS, 0, 0>>>(counts + n_tiles, (size_t)n_tiles, &d_ks->n_kinds);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&ks, d_ks, sizeof(ks), hipMemcpyDeviceToHost));
    if (ks.n_kinds > 0x7fffffffu) return tsfa_fail(TSFA_ERR_TOO_LONG, "tsfa_pack_set_create: more than 2 147 483 647 distinct kinds");
    set->n_groups = (int64_t)st.n_groups;
    set->n_kinds = (int32_t)ks.n_kinds;
    DevPtr<int64_t> d_offsets, d_rebased, d_krows, d_kgroups;
    DevPtr<void> d_uniq, d_kvals, d_psort;
    {
        const int64_t nk = set->n_kinds, ng = set->n_groups;
        HIP_TRY_ALLOC(d_offsets, (size_t)(ng + 1) * 8, "the offsets");
        HIP_TRY_ALLOC(d_uniq, (size_t)ng * id_size, "the unique ids");
        HIP_TRY_ALLOC(d_krows, (size_t)(nk + 1) * 8, "the kinds' row ranges");
        HIP_TRY_ALLOC(d_kgroups, (size_t)(nk + 1) * 8, "the kinds' group ranges");
        HIP_TRY_ALLOC(d_kvals, (size_t)nk * kind_size, "the kind values");
        k_pack_set_groups<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(hi, idx, kinds, kind_type, n, counts, counts + n_tiles, ng, nk,
                                                                    ids, id_size, d_offsets.get(), d_uniq.get(), d_krows.get(),
                                                                    d_kgroups.get(), d_kvals.get());
        HIP_TRY(hipGetLastError());
        if (nk > 1) {
            HIP_TRY_ALLOC(d_rebased, (size_t)(ng + nk) * 8, "the offsets of every kind");
            k_pack_rebase<<<pk_grid(ng + nk), PK_GRID_THREADS, 0, 0>>>(d_offsets.get(), d_krows.get(), d_kgroups.get(), nk, ng + nk,
                                                                        d_rebased.get());
            HIP_TRY(hipGetLastError());
        }
        if (options & TSFA_PACK_KEEP_SORT) {
            HIP_TRY_ALLOC(d_psort, (size_t)n * sort_size, "the packed sort column");
            k_pack_gather_raw<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(sort, sort_size, idx, n, d_psort.get());
            HIP_TRY(hipGetLastError());
        }
        set->kind_rows.resize((size_t)nk + 1);
        set->kind_groups.resize((size_t)nk + 1);
        set->kind_vals.resize((size_t)nk * kind_size);
        HIP_TRY(hipMemcpy(set->kind_rows.data(), d_krows.get(), (size_t)(nk + 1) * 8, hipMemcpyDeviceToHost));  // (synchronises)
        HIP_TRY(hipMemcpy(set->kind_groups.data(), d_kgroups.get(), (size_t)(nk + 1) * 8, hipMemcpyDeviceToHost));
        if (kind_size) HIP_TRY(hipMemcpy(set->kind_vals.data(), d_kvals.get(), (size_t)nk * kind_size, hipMemcpyDeviceToHost));
    }
    // the set takes over what outlives the call
    set->perm = pk_share(s.idx[s.cur].release(), device);
    set->offsets = pk_share(d_offsets.release(), device);
    set->uniq = pk_share(d_uniq.release(), device);
    if (d_rebased) set->rebased = pk_share(d_rebased.release(), device);
    if (d_psort) set->sort = pk_share(d_psort.release(), device);
    *out_set = set.release();
    return TSFA_OK;
}

extern "C" int32_t tsfa_pack_set_n_kinds(const tsfa_pack_set *set) { return set ? set->n_kinds : 0; }
extern "C" int32_t tsfa_pack_set_flags(const tsfa_pack_set *set) { return set ? set->flags : 0; }
extern "C" int32_t tsfa_pack_set_n_passes(const tsfa_pack_set *set) { return set ? set->n_passes : 0; }

extern "C" int tsfa_pack_set_copy_kinds(const tsfa_pack_set *set, void *kinds_host) {
    if (!set || !kinds_host) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_set_copy_kinds: null pointer");
    if (!set->has_kinds) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_set_copy_kinds: the set was made without a kind column");
    memcpy(kinds_host, set->kind_vals.data(), set->kind_vals.size());
    return TSFA_OK;
}

#undef TSFA_WHO
#define TSFA_WHO "tsfa_pack_set_values"
extern "C" int tsfa_pack_set_values(tsfa_pack_set *set, const void *values, int32_t value_type, int32_t space, tsfa_pack **out_packs) {
    if (!set || !values || !out_packs || (space != TSFA_HOST && space != TSFA_DEVICE))
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_set_values: bad arguments");
    const int val_size = pk_itemsize(value_type);
    if (val_size == 0) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_set_values: unknown element type of the value column");
    const int64_t n = set->n_rows;
    const int out_type = pk_out_type(value_type), out_size = pk_itemsize(out_type);
    const int id_size = pk_itemsize(set->id_type), sort_size = pk_itemsize(set->sort_type);
    unsigned int nan_flag = 0;
    for (int32_t k = 0; k < set->n_kinds; ++k) out_packs[k] = nullptr;

    HIP_TRY(hipSetDevice(set->device));
    DevPtr<void> d_vals, d_out_own;
    DevPtr<PkStats> d_st_own;
    if (int rc = pk_stage(TSFA_WHO, space, d_vals, &values, (size_t)n * val_size, "the value column")) return rc;
    HIP_TRY_ALLOC(d_st_own, sizeof(PkStats), "the packer's counters");
    PkStats *const d_st = d_st_own.get();
    HIP_TRY(hipMemset(d_st, 0, sizeof(PkStats)));
    HIP_TRY_ALLOC(d_out_own, (size_t)n * out_size, "the ragged sample buffer");
    void *const d_out = d_out_own.get();
    const std::shared_ptr<void> out = pk_share(d_out_own.release(), set->device);
    k_pack_gather<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(values, value_type, (const uint32_t *)set->perm.get(), n, d_out, d_st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&nan_flag, &d_st->nan_flag, sizeof(nan_flag), hipMemcpyDeviceToHost));  // (synchronises: the staged column may go)
    for (int32_t k = 0; k < set->n_kinds; ++k) {
        const int64_t r0 = set->kind_rows[(size_t)k], g0 = set->kind_groups[(size_t)k];
        tsfa_pack *pk = out_packs[k] = pk_view(set, out_type, nan_flag, out);
        pk->n_rows = set->kind_rows[(size_t)k + 1] - r0;
        pk->n_groups = set->kind_groups[(size_t)k + 1] - g0;
        pk->values = (char *)d_out + (size_t)r0 * out_size;
        // one kind: the set's own offsets; several: the kind's stretch of the rebased buffer (pk_rebase_body's layout)
        pk->offsets = (int64_t *)pk->hold[1].get() + (set->rebased ? g0 + k : 0);
        pk->uniq = (char *)set->uniq.get() + (size_t)g0 * id_size;
        if (set->sort) pk->sort = (char *)set->sort.get() + (size_t)r0 * sort_size;
    }
    return TSFA_OK;
}

#undef TSFA_WHO
#define TSFA_WHO "tsfa_pack_set_rows"
extern "C" int tsfa_pack_set_rows(tsfa_pack_set *set, const void *values, int32_t value_type, int64_t n_cols, int64_t stride_row,
                                  int64_t stride_col, tsfa_pack **out_packs) {
    if (!set) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_set_rows: set is NULL");
    if (set->has_kinds) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_set_rows: the set was made with a kind column (a value matrix is a wide frame)");
    const char *why;
    if (int rc = pr_check(values, value_type, set->n_rows, n_cols, stride_row, stride_col, out_packs, &why))
        return tsfa_fail(rc, (std::string("tsfa_pack_set_rows: ") + why).c_str());
    const int64_t n = set->n_rows;
    const int out_type = pk_out_type(value_type), out_size = pk_itemsize(out_type);
    for (int64_t c = 0; c < n_cols; ++c) out_packs[c] = nullptr;

    HIP_TRY(hipSetDevice(set->device));
    DevPtr<void> d_out_own;
    DevPtr<unsigned int> d_flags;
    HIP_TRY_ALLOC(d_flags, (size_t)n_cols * sizeof(unsigned int), "the columns' NaN flags");
    HIP_TRY(hipMemset(d_flags.get(), 0, (size_t)n_cols * sizeof(unsigned int)));
    HIP_TRY_ALLOC(d_out_own, (size_t)n_cols * (size_t)n * out_size, "the ragged sample buffers");
    void *const d_out = d_out_own.get();
    const std::shared_ptr<void> out = pk_share(d_out_own.release(), set->device);

    PrArgs a;
    a.values = values; a.perm = (const uint32_t *)set->perm.get(); a.n_rows = n; a.n_cols = n_cols;
    a.sr = stride_row; a.sc = stride_col; a.out = d_out; a.nan_flags = d_flags.get();
    const int route = pr_route(n_cols, stride_col);
    pr_plan_work(&a, route);
    if (route == PR_ROUTE_TILES) {
        const unsigned grid = (unsigned)(a.n_work < PR_MAX_GRID ? a.n_work : PR_MAX_GRID);
#define PR_LAUNCH(T) k_pack_rows_tiles<T><<<grid, PD_THREADS, 0, 0>>>(a)
        PR_DISPATCH(value_type, PR_LAUNCH)
#undef PR_LAUNCH
    } else {
        const int64_t blocks = (a.n_work + PK_GRID_THREADS - 1) / PK_GRID_THREADS;
        const unsigned grid = (unsigned)(blocks < PR_MAX_GRID ? blocks : PR_MAX_GRID);
#define PR_LAUNCH(T) k_pack_rows_gather<T><<<grid, PK_GRID_THREADS, 0, 0>>>(a)
        PR_DISPATCH(value_type, PR_LAUNCH)
#undef PR_LAUNCH
    }
    HIP_TRY(hipGetLastError());
    std::vector<unsigned int> nan_flags((size_t)n_cols);
    HIP_TRY(hipMemcpy(nan_flags.data(), d_flags.get(), (size_t)n_cols * sizeof(unsigned int), hipMemcpyDeviceToHost));  // (synchronises)
    for (int64_t c = 0; c < n_cols; ++c) {
        tsfa_pack *pk = out_packs[c] = pk_view(set, out_type, nan_flags[(size_t)c], out);  // (no kind column: one kind)
        pk->n_rows = n;
        pk->n_groups = set->n_groups;
        pk->values = (char *)d_out + (size_t)c * (size_t)n * out_size;
        pk->offsets = (int64_t *)set->offsets.get();
        pk->uniq = set->uniq.get();
        pk->sort = set->sort.get();
    }
    return TSFA_OK;
}

#undef TSFA_WHO
#define TSFA_WHO "tsfa_pack_set_hours"
extern "C" int tsfa_pack_set_hours(const tsfa_pack_set *set, const void *t, int32_t t_type, int64_t ticks_per_second, int64_t stride,
                                   double *hours_out, int32_t *flags_out) {
    if (!set) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_set_hours: set is NULL");
    const char *why;
    if (int rc = ph_check(t, t_type, ticks_per_second, set->n_rows, stride, hours_out, flags_out, &why))
        return tsfa_fail(rc, (std::string("tsfa_pack_set_hours: ") + why).c_str());
    PhArgs a;
    a.t = t; a.stride = stride; a.tps = t_type == TSFA_I64 ? (double)ticks_per_second : 1.0;
    a.perm = (const uint32_t *)set->perm.get(); a.offsets = (const int64_t *)set->offsets.get();
    a.n_rows = set->n_rows; a.n_groups = set->n_groups; a.out = hours_out; a.flags = (unsigned int *)flags_out;
    a.n_work = (set->n_rows + PK_TILE - 1) / PK_TILE;
    const unsigned grid = (unsigned)(a.n_work < PH_MAX_GRID ? a.n_work : PH_MAX_GRID);
    HIP_TRY(hipSetDevice(set->device));
    if (t_type == TSFA_I64) k_pack_set_hours<TSFA_I64><<<grid, PK_THREADS, 0, 0>>>(a);
    else k_pack_set_hours<TSFA_F64><<<grid, PK_THREADS, 0, 0>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return TSFA_OK;
}

extern "C" void tsfa_pack_set_destroy(tsfa_pack_set *set) { delete set; }

// ---------------------------------------------------------------------------------------------
// Window builder: the rolled layout of one pack (roll_device.h), built from the pack's offsets on the device
// ---------------------------------------------------------------------------------------------
struct tsfa_windows {
    int32_t device = 0;
    int32_t positive = 0;
    int64_t n_windows = 0;
    DevPtr<int64_t> starts, ends, series, shifts;  // n_windows int64 each; freed on `device` (tsfa_windows_destroy)
};

namespace {

__global__ void __launch_bounds__(PK_GRID_THREADS) k_roll_count(const int64_t *offsets, int64_t n_series, RlParams p, uint32_t *counts,
                                                                  RlStats *st) {
    __shared__ pk_u64 red;
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    rl_count_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, offsets, n_series, p, counts, &red, st);
}

__global__ void __launch_bounds__(PK_GRID_THREADS) k_roll_fill(const int64_t *offsets, int64_t n_series, const uint32_t *scanned,
                                                                 int64_t n_windows, RlParams p, int64_t *starts, int64_t *ends,
                                                                 int64_t *series, int64_t *shifts) {
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    rl_fill_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, offsets, n_series, scanned, n_windows, p, starts,
                 ends, series, shifts);
}

__global__ void __launch_bounds__(PK_GRID_THREADS) k_roll_fill_uniform(const int64_t *offsets, int64_t n, int64_t c, int64_t n_windows,
                                                                         RlParams p, int64_t *starts, int64_t *ends, int64_t *series,
                                                                         int64_t *shifts) {
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    rl_fill_uniform_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, offsets, n, c, n_windows, p, starts, ends,
                         series, shifts);
}

__global__ void __launch_bounds__(PK_GRID_THREADS) k_roll_shift_values(const void *sort, int itemsize, int64_t n_rows,
                                                                         const int64_t *starts, const int64_t *ends, int positive,
                                                                         int64_t n_windows, void *out) {
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    rl_shift_values_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, sort, itemsize, n_rows, starts, ends,
                         positive, n_windows, out);
}

}  // namespace

#undef TSFA_WHO
#define TSFA_WHO "tsfa_roll_windows"
extern "C" int tsfa_roll_windows(const tsfa_pack *pack, int32_t rolling_direction, int64_t max_timeshift, int64_t min_timeshift,
                                 int64_t steps, tsfa_windows **out_windows) {
    if (!out_windows) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_roll_windows: out_windows is NULL");
    *out_windows = nullptr;
    // before the handle is looked at: without a device no pack can exist (ordinal 0: that there is one; the pack names its own)
    if (int rc = tsfa_check_device(TSFA_WHO, 0)) return rc;
    if (!pack) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_roll_windows: pack is NULL");
    RlParams p;
    if (const char *why = rl_make_params(rolling_direction, max_timeshift, min_timeshift, steps, &p))
        return tsfa_fail(TSFA_ERR_INVALID, (std::string("tsfa_roll_windows: ") + why).c_str());
    const int64_t ns = pack->n_groups;
    RlStats st;
    std::unique_ptr<tsfa_windows, void (*)(tsfa_windows *)> win(new tsfa_windows(), tsfa_windows_destroy);
    win->device = pack->device;
    win->positive = p.positive;
    memset(&st, 0, sizeof(st));

    HIP_TRY(hipSetDevice(pack->device));
    DevPtr<uint32_t> counts;
    DevPtr<RlStats> d_st;
    if (ns > 0) {
        HIP_TRY_ALLOC(counts, (size_t)ns * 4, "the window counts");
        HIP_TRY_ALLOC(d_st, sizeof(RlStats), "the window builder's counters");
        HIP_TRY(hipMemcpy(d_st.get(), &st, sizeof(st), hipMemcpyHostToDevice));
        k_roll_count<<<pk_grid(ns), PK_GRID_THREADS, 0, 0>>>(pack->offsets, ns, p, counts.get(), d_st.get());
        k_pack_scan<<<1, PK_SCAN_THREADS, 0, 0>>>(counts.get(), (size_t)ns, &d_st.get()->total);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&st, d_st.get(), sizeof(st), hipMemcpyDeviceToHost));
        if ((int64_t)st.max_len > steps)
            return tsfa_fail(TSFA_ERR_INVALID, ("tsfa_roll_windows: steps = " + std::to_string(steps) + " is below the pack's longest series (" +
                                                std::to_string(st.max_len) + " samples)").c_str());
        win->n_windows = (int64_t)st.total;
    }
    if (win->n_windows > 0) {
        const int64_t nw = win->n_windows;
        HIP_TRY_ALLOC(win->starts, (size_t)nw * 8, "the window starts");
        HIP_TRY_ALLOC(win->ends, (size_t)nw * 8, "the window ends");
        HIP_TRY_ALLOC(win->series, (size_t)nw * 8, "the windows' series indices");
        HIP_TRY_ALLOC(win->shifts, (size_t)nw * 8, "the windows' timeshifts");
        k_roll_fill<<<pk_grid(nw), PK_GRID_THREADS, 0, 0>>>(pack->offsets, ns, counts.get(), nw, p, win->starts.get(), win->ends.get(),
                                                              win->series.get(), win->shifts.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    *out_windows = win.release();
    return TSFA_OK;
}

extern "C" int64_t tsfa_windows_n_windows(const tsfa_windows *windows) { return windows ? windows->n_windows : 0; }
extern "C" const int64_t *tsfa_windows_starts(const tsfa_windows *windows) { return windows ? windows->starts.get() : nullptr; }
extern "C" const int64_t *tsfa_windows_ends(const tsfa_windows *windows) { return windows ? windows->ends.get() : nullptr; }

extern "C" int tsfa_windows_copy_series(const tsfa_windows *windows, int64_t *series_host) {
    return pk_copy_out(windows, series_host, windows ? windows->series.get() : nullptr, windows ? (size_t)windows->n_windows * 8 : 0,
                       "tsfa_windows_copy_series");
}

extern "C" int tsfa_windows_copy_timeshifts(const tsfa_windows *windows, int64_t *timeshifts_host) {
    return pk_copy_out(windows, timeshifts_host, windows ? windows->shifts.get() : nullptr, windows ? (size_t)windows->n_windows * 8 : 0,
                       "tsfa_windows_copy_timeshifts");
}

extern "C" int tsfa_windows_copy_starts(const tsfa_windows *windows, int64_t *starts_host) {
    return pk_copy_out(windows, starts_host, windows ? windows->starts.get() : nullptr, windows ? (size_t)windows->n_windows * 8 : 0,
                       "tsfa_windows_copy_starts");
}

extern "C" int tsfa_windows_copy_ends(const tsfa_windows *windows, int64_t *ends_host) {
    return pk_copy_out(windows, ends_host, windows ? windows->ends.get() : nullptr, windows ? (size_t)windows->n_windows * 8 : 0,
                       "tsfa_windows_copy_ends");
}

// ---------------------------------------------------------------------------------------------
// The same windows for a batch that is no pack: raw offsets in, caller-owned buffers out (see roll_device.h for the two routes)
// ---------------------------------------------------------------------------------------------
#undef TSFA_WHO
#define TSFA_WHO "tsfa_roll_count"
extern "C" int tsfa_roll_count(const int64_t *offsets, int64_t n_series, int64_t series_len, int32_t rolling_direction,
                               int64_t max_timeshift, int64_t min_timeshift, int64_t steps, uint32_t *scanned,
                               int64_t *n_windows_host, int32_t device, void *stream) {
    int rc = tsfa_check_device(TSFA_WHO, device);  // before the arguments: without a device no device pointer can exist
    if (rc) return rc;
    if (!n_windows_host) return tsfa_fail(TSFA_ERR_INVALID, TSFA_WHO ": n_windows_host is NULL");
    *n_windows_host = 0;
    RlParams p;
    const char *why = rl_make_params(rolling_direction, max_timeshift, min_timeshift, steps, &p);
    if (why) return tsfa_fail(TSFA_ERR_INVALID, (std::string(TSFA_WHO ": ") + why).c_str());
    if (!scanned) {  // the uniform route: the closed form on the host, nothing is launched
        int64_t per_series = 0;
        if ((rc = rl_uniform_count(p, n_series, series_len, &per_series, n_windows_host, &why)))
            return tsfa_fail(rc, (std::string(TSFA_WHO ": ") + why).c_str());
        return TSFA_OK;
    }
    if (!offsets || n_series < 0) return tsfa_fail(TSFA_ERR_INVALID, TSFA_WHO ": offsets is NULL or n_series is negative");
    if (n_series == 0) return TSFA_OK;
    hipStream_t st = (hipStream_t)stream;  // NULL: the null stream
    int64_t edge[2] = {0, 0};
    RlStats hst;
    memset(&hst, 0, sizeof(hst));

    HIP_TRY(hipSetDevice(device));
    // the extent the offsets claim, before anything is launched on them
    HIP_TRY(hipMemcpyAsync(&edge[0], offsets, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&edge[1], offsets + n_series, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = rl_check_extent(edge[1] - edge[0], &why))) return tsfa_fail(rc, (std::string(TSFA_WHO ": ") + why).c_str());
    DevPtr<RlStats> d_st;
    HIP_TRY_ALLOC(d_st, sizeof(RlStats), "the window builder's counters");
    HIP_TRY(hipMemsetAsync(d_st.get(), 0, sizeof(RlStats), st));
    k_roll_count<<<pk_grid(n_series), PK_GRID_THREADS, 0, st>>>(offsets, n_series, p, scanned, d_st.get());
    k_pack_scan<<<1, PK_SCAN_THREADS, 0, st>>>(scanned, (size_t)n_series, &d_st.get()->total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&hst, d_st.get(), sizeof(hst), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the total is the call's result: this route waits for the stream whoever owns it
    if ((int64_t)hst.max_len > steps)
        return tsfa_fail(TSFA_ERR_INVALID, (TSFA_WHO ": steps = " + std::to_string(steps) + " is below the batch's longest series (" +
                                            std::to_string(hst.max_len) + " samples)").c_str());
    *n_windows_host = (int64_t)hst.total;
    return TSFA_OK;
}

#undef TSFA_WHO
#define TSFA_WHO "tsfa_roll_fill"
extern "C" int tsfa_roll_fill(const int64_t *offsets, int64_t n_series, const uint32_t *scanned, int64_t series_len,
                              int64_t n_windows, int32_t rolling_direction, int64_t max_timeshift, int64_t min_timeshift,
                              int64_t steps, int64_t *starts, int64_t *ends, int64_t *series, int64_t *timeshifts, int32_t device,
                              void *stream) {
    int rc = tsfa_check_device(TSFA_WHO, device);  // before the arguments: without a device no device pointer can exist
    if (rc) return rc;
    RlParams p;
    const char *why = rl_make_params(rolling_direction, max_timeshift, min_timeshift, steps, &p);
    if (why) return tsfa_fail(TSFA_ERR_INVALID, (std::string(TSFA_WHO ": ") + why).c_str());
    if (n_windows < 0 || n_series < 0) return tsfa_fail(TSFA_ERR_INVALID, TSFA_WHO ": n_windows or n_series is negative");
    int64_t per_series = 0;
    if (!scanned) {
        int64_t expect = 0;
        if ((rc = rl_uniform_count(p, n_series, series_len, &per_series, &expect, &why)))
            return tsfa_fail(rc, (std::string(TSFA_WHO ": ") + why).c_str());
        if (n_windows != expect)
            return tsfa_fail(TSFA_ERR_INVALID, (TSFA_WHO ": n_windows = " + std::to_string(n_windows) + ", but " + std::to_string(n_series) +
                                                " series of " + std::to_string(series_len) + " samples have " + std::to_string(expect) +
                                                " windows").c_str());
    } else if (!offsets || n_windows > RL_MAX_SAMPLES) {
        return tsfa_fail(TSFA_ERR_INVALID, TSFA_WHO ": offsets is NULL, or n_windows is beyond what tsfa_roll_count returns");
    }
    if (n_windows == 0) return TSFA_OK;
    if (n_series < 1 || !starts || !ends || !series || !timeshifts)
        return tsfa_fail(TSFA_ERR_INVALID, TSFA_WHO ": windows without a series, or an output pointer is NULL");
    hipStream_t st = (hipStream_t)stream;  // NULL: the null stream
    HIP_TRY(hipSetDevice(device));
    if (scanned)
        k_roll_fill<<<pk_grid(n_windows), PK_GRID_THREADS, 0, st>>>(offsets, n_series, scanned, n_windows, p, starts, ends, series, timeshifts);
    else
        k_roll_fill_uniform<<<pk_grid(n_windows), PK_GRID_THREADS, 0, st>>>(offsets, series_len, per_series, n_windows, p, starts, ends,
                                                                             series, timeshifts);
    HIP_TRY(hipGetLastError());
    if (!stream) HIP_TRY(hipStreamSynchronize(st));
    return TSFA_OK;
}

#undef TSFA_WHO
#define TSFA_WHO "tsfa_roll_shift_values"
extern "C" int tsfa_roll_shift_values(const tsfa_windows *windows, const tsfa_pack *pack, void *out_host) {
    if (!windows || !pack || !out_host) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_roll_shift_values: null pointer");
    if (!pack->sort)
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_roll_shift_values: the pack was made without TSFA_PACK_KEEP_SORT: it holds no sort column");
    if (pack->device != windows->device)
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_roll_shift_values: the windows and the pack live on different devices");
    const int64_t nw = windows->n_windows;
    if (nw == 0) return TSFA_OK;
    const int itemsize = pk_itemsize(pack->sort_type);
    HIP_TRY(hipSetDevice(pack->device));
    DevPtr<void> d_out;
    HIP_TRY_ALLOC(d_out, (size_t)nw * itemsize, "the windows' shift values");
    k_roll_shift_values<<<pk_grid(nw), PK_GRID_THREADS, 0, 0>>>(pack->sort, itemsize, pack->n_rows, windows->starts.get(),
                                                                  windows->ends.get(), windows->positive, nw, d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_host, d_out.get(), (size_t)nw * itemsize, hipMemcpyDeviceToHost));
    return TSFA_OK;
}

extern "C" void tsfa_windows_destroy(tsfa_windows *windows) {
    if (!windows) return;
    (void)hipSetDevice(windows->device);
    delete windows;
}
