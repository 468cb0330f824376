// Device packer of the C-ABI (include/tsfresh_amd.h: tsfa_pack_device*): the kernels around the bodies of pack_device.h
// and the host code that strings them together.  See pack_device.h for the scratch formula and the sort's design.
#include <hip/hip_runtime.h>

#include <string>

#include "pack_device.h"

int tsfa_fail(int code, const char *msg);

struct tsfa_pack {
    int32_t device = 0;
    int64_t n_rows = 0, n_groups = 0;
    int32_t flags = 0, n_passes = 0;
    int32_t id_type = 0, sort_type = 0, out_type = TSFA_F64;
    // owned device buffers: ALL of them are freed by tsfa_pack_device_destroy
    void *values = nullptr;      // ragged buffer, n_rows x out_type
    int64_t *offsets = nullptr;  // n_groups + 1
    void *uniq = nullptr;        // n_groups x id_type
    void *sort = nullptr;        // n_rows x sort_type (TSFA_PACK_KEEP_SORT)
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

int pk_fail_hip(const char *what, hipError_t e) {
    return tsfa_fail(TSFA_ERR_HIP, (std::string("tsfa_pack_device: ") + what + ": " + hipGetErrorString(e)).c_str());
}

#define PK_HIP(expr)                                        \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) {                             \
            rc = pk_fail_hip(#expr, e_);                    \
            goto done;                                      \
        }                                                   \
    } while (0)

// hipMalloc that names the byte count when it fails
#define PK_ALLOC(ptr, bytes, what)                                                                                        \
    do {                                                                                                                  \
        const size_t nb_ = (size_t)(bytes);                                                                               \
        hipError_t e_ = hipMalloc((void **)&(ptr), nb_ ? nb_ : 1);                                                        \
        if (e_ != hipSuccess) {                                                                                           \
            (ptr) = nullptr;                                                                                              \
            rc = tsfa_fail(TSFA_ERR_HIP, (std::string("tsfa_pack_device: cannot allocate ") + std::to_string(nb_) +       \
                                          " bytes of device memory for " + (what) + ": " + hipGetErrorString(e_)).c_str()); \
            goto done;                                                                                                    \
        }                                                                                                                 \
    } while (0)

int pk_check_device(int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return tsfa_fail(TSFA_ERR_NO_DEVICE, "tsfa_pack_device: no HIP device visible: tsfresh_amd has no CPU fallback");
    if (device < 0 || device >= ndev) return tsfa_fail(TSFA_ERR_NO_DEVICE, "tsfa_pack_device: no such HIP device");
    return TSFA_OK;
}

int pk_grid(int64_t n) {
    const int64_t blocks = (n + PK_GRID_THREADS - 1) / PK_GRID_THREADS;
    return (int)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
}

}  // namespace

extern "C" int tsfa_pack_device(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *values,
                                int32_t value_type, int64_t n_rows, int32_t space, int32_t options, int32_t device,
                                tsfa_pack **out_pack) {
    if (!out_pack) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device: out_pack is NULL");
    *out_pack = nullptr;
    if (!ids || !values || n_rows < 1 || (space != TSFA_HOST && space != TSFA_DEVICE) || (options & ~TSFA_PACK_KEEP_SORT))
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device: bad arguments");
    if (!pk_is_key_type(id_type, false)) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device: the id column must be of an integer type");
    if (sort && !pk_is_key_type(sort_type, true))
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device: the sort column must be of an integer type, float32 or float64");
    if (pk_itemsize(value_type) == 0) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device: unknown element type of the value column");
    if ((options & TSFA_PACK_KEEP_SORT) && !sort)
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_pack_device: TSFA_PACK_KEEP_SORT without a sort column");
    int rc = pk_check_device(device);
    if (rc) return rc;
    if (n_rows > 0xffffffffll)
        return tsfa_fail(TSFA_ERR_TOO_LONG, "tsfa_pack_device: more than 4 294 967 295 rows (the row indices are 32 bits wide)");

    const int64_t n = n_rows, n_tiles = (n + PK_TILE - 1) / PK_TILE;
    const int id_size = pk_itemsize(id_type), sort_size = sort ? pk_itemsize(sort_type) : 0, val_size = pk_itemsize(value_type);
    const int out_type = pk_out_type(value_type);
    void *d_ids = nullptr, *d_sort = nullptr, *d_vals = nullptr;  // staged copies (TSFA_HOST only)
    pk_u64 *hi[2] = {nullptr, nullptr}, *lo[2] = {nullptr, nullptr};
    uint32_t *idx[2] = {nullptr, nullptr}, *counts = nullptr;
    PkStats *d_st = nullptr;
    PkStats st;
    tsfa_pack *pk = new tsfa_pack();
    int cur = 0;
    pk->device = device; pk->n_rows = n; pk->id_type = id_type; pk->sort_type = sort ? sort_type : 0; pk->out_type = out_type;

    PK_HIP(hipSetDevice(device));
    if (space == TSFA_HOST) {
        PK_ALLOC(d_ids, (size_t)n * id_size, "the id column");
        PK_HIP(hipMemcpy(d_ids, ids, (size_t)n * id_size, hipMemcpyHostToDevice));
        if (sort) {
            PK_ALLOC(d_sort, (size_t)n * sort_size, "the sort column");
            PK_HIP(hipMemcpy(d_sort, sort, (size_t)n * sort_size, hipMemcpyHostToDevice));
        }
        PK_ALLOC(d_vals, (size_t)n * val_size, "the value column");
        PK_HIP(hipMemcpy(d_vals, values, (size_t)n * val_size, hipMemcpyHostToDevice));
        ids = d_ids; sort = d_sort; values = d_vals;
    }
    PK_ALLOC(d_st, sizeof(PkStats), "the packer's counters");
    pk_stats_init(&st);
    PK_HIP(hipMemcpy(d_st, &st, sizeof(st), hipMemcpyHostToDevice));

    // 1. min / max of both keys, descents
    k_pack_minmax<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(ids, id_type, sort, sort_type, n, d_st);
    PK_HIP(hipGetLastError());
    PK_HIP(hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost));
    {
        const bool in_order = st.descents == 0;
        if (in_order) pk->flags |= TSFA_PACK_IN_ORDER;
        // 2. keys, identity permutation, byte histograms.  An ordered frame needs one set of buffers only.
        for (int k = 0; k < (in_order ? 1 : 2); ++k) {
            PK_ALLOC(hi[k], (size_t)n * 8, "the id keys (sort scratch: 40 bytes per row in all)");
            PK_ALLOC(lo[k], (size_t)n * 8, "the sort keys (sort scratch: 40 bytes per row in all)");
            PK_ALLOC(idx[k], (size_t)n * 4, "the row indices (sort scratch: 40 bytes per row in all)");
        }
        PK_ALLOC(counts, (size_t)n_tiles * PK_RADIX * 4, "the per-tile digit counts");
        k_pack_keys<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(ids, id_type, sort, sort_type, n, st.kmin[0], sort ? st.kmin[1] : 0ull,
                                                             pk_sig_bytes(st.kmax[0] - st.kmin[0]),
                                                             sort ? pk_sig_bytes(st.kmax[1] - st.kmin[1]) : 0, in_order ? 0 : 1, hi[0],
                                                             lo[0], idx[0], d_st);
        PK_HIP(hipGetLastError());
        if (!in_order) {
            // 3. the radix passes, least significant digit first; constant digits are skipped
            int pass_word[16], pass_byte[16];
            PK_HIP(hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost));
            const int np = pk_plan_passes(&st, n, sort != nullptr, pass_word, pass_byte);
            for (int p = 0; p < np; ++p) {
                const pk_u64 *key = pass_word[p] ? lo[cur] : hi[cur];
                const int shift = 8 * pass_byte[p];
                k_pack_hist<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(n_tiles, key, shift, n, counts);
                k_pack_scan<<<1, PK_SCAN_THREADS, 0, 0>>>(counts, (size_t)n_tiles * PK_RADIX, nullptr);
                k_pack_scatter<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(n_tiles, key, shift, n, counts, hi[cur], lo[cur], idx[cur],
                                                                         hi[cur ^ 1], lo[cur ^ 1], idx[cur ^ 1]);
                PK_HIP(hipGetLastError());
                cur ^= 1;
            }
            pk->n_passes = np;
        }
    }
    // 4. group boundaries (counts is reused for the per-tile head counts)
    k_pack_heads<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(hi[cur], n, counts);
    k_pack_scan<<<1, PK_SCAN_THREADS, 0, 0>>>(counts, (size_t)n_tiles, &d_st->n_groups);
    PK_HIP(hipGetLastError());
    PK_HIP(hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost));
    pk->n_groups = (int64_t)st.n_groups;
    PK_ALLOC(pk->offsets, (size_t)(pk->n_groups + 1) * 8, "the offsets");
    PK_ALLOC(pk->uniq, (size_t)pk->n_groups * id_size, "the unique ids");
    k_pack_groups<<<(unsigned)n_tiles, PK_THREADS, 0, 0>>>(hi[cur], idx[cur], n, counts, pk->n_groups, ids, id_size, pk->offsets, pk->uniq);
    PK_HIP(hipGetLastError());
    // 5. gather
    PK_ALLOC(pk->values, (size_t)n * pk_itemsize(out_type), "the ragged sample buffer");
    k_pack_gather<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(values, value_type, idx[cur], n, pk->values, d_st);
    PK_HIP(hipGetLastError());
    if (options & TSFA_PACK_KEEP_SORT) {
        PK_ALLOC(pk->sort, (size_t)n * sort_size, "the packed sort column");
        k_pack_gather_raw<<<pk_grid(n), PK_GRID_THREADS, 0, 0>>>(sort, sort_size, idx[cur], n, pk->sort);
        PK_HIP(hipGetLastError());
    }
    PK_HIP(hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost));  // (synchronises: the staged columns may go)
    if (st.nan_flag) pk->flags |= TSFA_PACK_VALUE_NAN;
done:
    for (int k = 0; k < 2; ++k) {
        (void)hipFree(hi[k]); (void)hipFree(lo[k]); (void)hipFree(idx[k]);
    }
    (void)hipFree(counts); (void)hipFree(d_st);
    (void)hipFree(d_ids); (void)hipFree(d_sort); (void)hipFree(d_vals);
    if (rc) {
        tsfa_pack_device_destroy(pk);
        return rc;
    }
    *out_pack = pk;
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

static int pk_copy_out(const tsfa_pack *pack, void *dst, const void *src, size_t bytes, const char *who) {
    if (!pack || !dst) return tsfa_fail(TSFA_ERR_INVALID, (std::string(who) + ": null pointer").c_str());
    if (!src) return tsfa_fail(TSFA_ERR_INVALID, (std::string(who) + ": the pack does not hold that buffer").c_str());
    hipError_t e = hipSetDevice(pack->device);
    if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? (int)TSFA_OK : pk_fail_hip(who, e);
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
    if (pack->values || pack->offsets || pack->uniq || pack->sort) {
        (void)hipSetDevice(pack->device);
        (void)hipFree(pack->values);
        (void)hipFree(pack->offsets);
        (void)hipFree(pack->uniq);
        (void)hipFree(pack->sort);
    }
    delete pack;
}
