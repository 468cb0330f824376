// Dense packer of the C-ABI (include/tsfresh_amd.h: tsfa_pack_dense): the kernels around the bodies of pack_dense.h and the
// host code that picks the route.  See pack_dense.h for the layout, the three routes and the LDS tile.
#include <hip/hip_runtime.h>

#include <string>

#include "pack_dense.h"
#include "tsfa_devmem.h"

#undef TSFA_WHO
#define TSFA_WHO "tsfa_pack_dense"

namespace {

#define PD_GRID_THREADS 256

__global__ void __launch_bounds__(PD_GRID_THREADS) k_dense_offsets(int64_t n_batch, int64_t n_time, int64_t *offsets) {
    const PkBlk b{(int)threadIdx.x, (int)blockDim.x};
    pd_offsets_body(b, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, n_batch, n_time, offsets);
}

__global__ void __launch_bounds__(PD_SCAN_THREADS) k_dense_scan(const void *lengths, int type, int64_t n_batch, int64_t n_time,
                                                                 int64_t *offsets, unsigned int *flags) {
    __shared__ pk_u64 ws[16];
    const PkBlk b{(int)threadIdx.x, PD_SCAN_THREADS};
    pd_scan_lengths_body(b, lengths, type, n_batch, n_time, offsets, ws, flags);
}

template <int TYPE, bool UNIT>
__global__ void __launch_bounds__(PD_THREADS) k_dense_rows(PdArgs a) {
    const PkBlk b{(int)threadIdx.x, PD_THREADS};
    pd_rows_body<TYPE, UNIT>(b, (int64_t)blockIdx.x, (int64_t)gridDim.x, a);
}

template <int TYPE>
__global__ void __launch_bounds__(PD_THREADS) k_dense_transpose(PdArgs a) {
    __shared__ uint32_t tile[(TYPE == TSFA_F64 ? 2 : 1) * PD_TILE_WORDS];
    const PkBlk b{(int)threadIdx.x, PD_THREADS};
    pd_transpose_body<TYPE>(b, (int64_t)blockIdx.x, (int64_t)gridDim.x, a, tile);
}

template <int TYPE>
void pd_launch(int route, const PdArgs &a, unsigned grid, hipStream_t st) {
    if (route == PD_ROUTE_ROWS_UNIT) k_dense_rows<TYPE, true><<<grid, PD_THREADS, 0, st>>>(a);
    else if (route == PD_ROUTE_TRANSPOSE) k_dense_transpose<TYPE><<<grid, PD_THREADS, 0, st>>>(a);
    else k_dense_rows<TYPE, false><<<grid, PD_THREADS, 0, st>>>(a);
}

}  // namespace

extern "C" int tsfa_pack_dense(const void *x, int32_t x_type, int64_t n_batch, int64_t n_channels, int64_t n_time,
                               int64_t stride_batch, int64_t stride_channel, int64_t stride_time, const void *lengths,
                               int32_t lengths_type, void *values_out, int64_t channel_stride_out, int64_t *offsets_out,
                               int32_t *flags_out, int32_t device, void *stream) {
    // before the arguments are looked at: without a device no device pointer can exist
    if (int rc = tsfa_check_device(TSFA_WHO, device)) return rc;
    const char *why;
    if (int rc = pd_check(x, x_type, n_batch, n_channels, n_time, stride_batch, stride_channel, stride_time, lengths, lengths_type,
                          values_out, channel_stride_out, offsets_out, flags_out, &why))
        return tsfa_fail(rc, (std::string("tsfa_pack_dense: ") + why).c_str());

    PdArgs a;
    a.x = x; a.n_batch = n_batch; a.n_channels = n_channels; a.n_time = n_time;
    a.sb = stride_batch; a.sc = stride_channel; a.st = stride_time;
    a.offsets = offsets_out; a.uniform = lengths ? 0 : 1;
    a.out = values_out; a.cso = channel_stride_out; a.flags = (unsigned int *)flags_out;
    const int route = pd_route(n_channels, stride_channel, stride_time);
    pd_plan_work(&a, route);
    const unsigned grid = (unsigned)(a.n_work < PD_MAX_GRID ? a.n_work : PD_MAX_GRID);
    hipStream_t st = (hipStream_t)stream;   // NULL: the null stream

    HIP_TRY(hipSetDevice(device));
    if (lengths) {
        k_dense_scan<<<1, PD_SCAN_THREADS, 0, st>>>(lengths, lengths_type, n_batch, n_time, offsets_out, (unsigned int *)flags_out);
    } else {
        const int64_t blocks = (n_batch + 1 + PD_GRID_THREADS - 1) / PD_GRID_THREADS;
        k_dense_offsets<<<(unsigned)(blocks > 2048 ? 2048 : blocks), PD_GRID_THREADS, 0, st>>>(n_batch, n_time, offsets_out);
    }
    HIP_TRY(hipGetLastError());
    switch (x_type) {
    case TSFA_F64: pd_launch<TSFA_F64>(route, a, grid, st); break;
    case TSFA_F32: pd_launch<TSFA_F32>(route, a, grid, st); break;
    case TSFA_F16: pd_launch<TSFA_F16>(route, a, grid, st); break;
    default: pd_launch<TSFA_BF16>(route, a, grid, st); break;
    }
    HIP_TRY(hipGetLastError());
    if (!stream) HIP_TRY(hipStreamSynchronize(st));
    return TSFA_OK;
}
