// Valid-step packer of the C-ABI (include/tsfresh_amd.h: tsfa_pack_dense_valid): the kernels around the bodies of
// pack_valid.h and the host code that launches them.  See pack_valid.h for the semantics, the three passes and the scratch.
#include <hip/hip_runtime.h>

#include <string>

#include "pack_valid.h"
#include "tsfa_devmem.h"

#undef TSFA_WHO
#define TSFA_WHO "tsfa_pack_dense_valid"

namespace {

template <int TYPE, bool UNIT>
__global__ void __launch_bounds__(PD_THREADS) k_valid_count(PvArgs a) {
    __shared__ unsigned int ws[PD_THREADS / 64];
    const PkBlk b{(int)threadIdx.x, PD_THREADS};
    pv_count_body<TYPE, UNIT>(b, (int64_t)blockIdx.x, (int64_t)gridDim.x, a, ws);
}

__global__ void __launch_bounds__(PD_SCAN_THREADS) k_valid_scan(PvArgs a) {
    __shared__ pk_u64 ws[16];
    const PkBlk b{(int)threadIdx.x, PD_SCAN_THREADS};
    pv_scan_body(b, a, ws);
}

template <int TYPE, bool UNIT>
__global__ void __launch_bounds__(PD_THREADS) k_valid_compact(PvArgs a) {
    const PkBlk b{(int)threadIdx.x, PD_THREADS};
    pv_compact_body<TYPE, UNIT>(b, (int64_t)blockIdx.x, (int64_t)gridDim.x, a);
}

template <int TYPE, bool UNIT>
void pv_launch_typed(const PvArgs &a, unsigned grid, hipStream_t st) {
    k_valid_count<TYPE, UNIT><<<grid, PD_THREADS, 0, st>>>(a);
    k_valid_scan<<<1, PD_SCAN_THREADS, 0, st>>>(a);
    k_valid_compact<TYPE, UNIT><<<grid, PD_THREADS, 0, st>>>(a);
}

template <int TYPE>
void pv_launch(const PvArgs &a, unsigned grid, hipStream_t st) {
    if (a.st == 1) pv_launch_typed<TYPE, true>(a, grid, st);
    else pv_launch_typed<TYPE, false>(a, grid, st);
}

}  // namespace

extern "C" int tsfa_pack_dense_valid(const void *x, int32_t x_type, int64_t n_batch, int64_t n_channels, int64_t n_time,
                                     int64_t stride_batch, int64_t stride_channel, int64_t stride_time, const void *lengths,
                                     int32_t lengths_type, const void *t, int32_t t_type, int64_t t_stride_batch,
                                     int64_t t_stride_time, void *values_out, int64_t channel_stride_out, int64_t *offsets_out,
                                     int32_t *steps_out, void *stamps_out, void *scratch, int64_t scratch_bytes,
                                     int32_t *flags_out, int32_t device, void *stream) {
    // before the arguments are looked at: without a device no device pointer can exist
    if (int rc = tsfa_check_device(TSFA_WHO, device)) return rc;
    const char *why;
    if (int rc = pv_check(x, x_type, n_batch, n_channels, n_time, stride_batch, stride_channel, stride_time, lengths, lengths_type,
                          t, t_type, t_stride_batch, t_stride_time, values_out, channel_stride_out, offsets_out, steps_out,
                          stamps_out, scratch, scratch_bytes, flags_out, &why))
        return tsfa_fail(rc, (std::string("tsfa_pack_dense_valid: ") + why).c_str());

    PvArgs a;
    a.x = x; a.n_batch = n_batch; a.n_channels = n_channels; a.n_time = n_time;
    a.sb = stride_batch; a.sc = stride_channel; a.st = stride_time;
    a.lengths = lengths; a.lengths_type = lengths_type;
    a.t = t; a.t_type = t_type; a.tsb = t_stride_batch; a.tst = t_stride_time;
    a.out = values_out; a.cso = channel_stride_out; a.offsets = offsets_out; a.steps = steps_out;
    a.stamps = (pk_u64 *)stamps_out; a.flags = (unsigned int *)flags_out;
    pv_plan_work(&a, scratch);
    const unsigned grid = (unsigned)(a.n_work < PD_MAX_GRID ? a.n_work : PD_MAX_GRID);
    hipStream_t st = (hipStream_t)stream;   // NULL: the null stream

    HIP_TRY(hipSetDevice(device));
    switch (x_type) {
    case TSFA_F64: pv_launch<TSFA_F64>(a, grid, st); break;
    case TSFA_F32: pv_launch<TSFA_F32>(a, grid, st); break;
    case TSFA_F16: pv_launch<TSFA_F16>(a, grid, st); break;
    default: pv_launch<TSFA_BF16>(a, grid, st); break;
    }
    HIP_TRY(hipGetLastError());
    if (!stream) HIP_TRY(hipStreamSynchronize(st));
    return TSFA_OK;
}
