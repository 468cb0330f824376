// Times packer of the C-ABI (include/tsfresh_amd.h: tsfa_pack_times): the kernel around the body of pack_times.h and the host
// code that launches it.  See pack_times.h for the arithmetic, the layout and the bounds.
#include <hip/hip_runtime.h>

#include <string>

#include "pack_times.h"
#include "tsfa_devmem.h"

#undef TSFA_WHO
#define TSFA_WHO "tsfa_pack_times"

namespace {

template <int TYPE, bool UNIT>
__global__ void __launch_bounds__(PD_THREADS) k_pack_times(PtArgs a) {
    const PkBlk b{(int)threadIdx.x, PD_THREADS};
    pt_rows_body<TYPE, UNIT>(b, (int64_t)blockIdx.x, (int64_t)gridDim.x, a);
}

template <int TYPE>
void pt_launch(const PtArgs &a, unsigned grid, hipStream_t st) {
    if (a.st == 1) k_pack_times<TYPE, true><<<grid, PD_THREADS, 0, st>>>(a);
    else k_pack_times<TYPE, false><<<grid, PD_THREADS, 0, st>>>(a);
}

}  // namespace

extern "C" int tsfa_pack_times(const void *t, int32_t t_type, int64_t ticks_per_second, int64_t n_batch, int64_t n_time,
                               int64_t stride_batch, int64_t stride_time, const int64_t *offsets, double *hours_out,
                               int32_t *flags_out, int32_t device, void *stream) {
    // before the arguments are looked at: without a device no device pointer can exist
    if (int rc = tsfa_check_device(TSFA_WHO, device)) return rc;
    const char *why;
    if (int rc = pt_check(t, t_type, ticks_per_second, n_batch, n_time, stride_batch, stride_time, offsets, hours_out, flags_out, &why))
        return tsfa_fail(rc, (std::string("tsfa_pack_times: ") + why).c_str());

    PtArgs a;
    a.t = t; a.n_batch = n_batch; a.n_time = n_time; a.sb = stride_batch; a.st = stride_time;
    a.tps = t_type == TSFA_I64 ? (double)ticks_per_second : 1.0;
    a.offsets = offsets; a.out = hours_out; a.flags = (unsigned int *)flags_out;
    pt_plan_work(&a);
    const unsigned grid = (unsigned)(a.n_work < PD_MAX_GRID ? a.n_work : PD_MAX_GRID);
    hipStream_t st = (hipStream_t)stream;   // NULL: the null stream

    HIP_TRY(hipSetDevice(device));
    if (t_type == TSFA_I64) pt_launch<TSFA_I64>(a, grid, st);
    else pt_launch<TSFA_F64>(a, grid, st);
    HIP_TRY(hipGetLastError());
    if (!stream) HIP_TRY(hipStreamSynchronize(st));
    return TSFA_OK;
}
