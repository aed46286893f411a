// hz_fr_raw_ops, form 0: the kernels of fr_raw_ops.h built with HZ_FR_INLINE, as every kernel of the step has it; and the entry point.
#define HZ_FR_INLINE 1
#define HZ_FR_RAW_FORM 0
#include <hip/hip_runtime.h>
#include "fr_raw_ops.h"
#include "hostutil.h"

namespace hz {
hipError_t fr_raw_launch_form1(int op, size_t n, const uint32_t* d_in, uint32_t* d_out, hipStream_t s);   // fr_raw_outline.hip
}

using namespace hz;

extern "C" hz_status hz_fr_raw_ops(int32_t device, int32_t op, int32_t form, size_t n, const uint32_t* operands, int32_t n_operands, uint32_t* out) {
    if (fr_raw_operands(op) < 0 || n_operands != fr_raw_operands(op) || (form != 0 && form != 1) || (n && (!operands || !out)))
        return set_err(HZ_ERR_ARG, "hz_fr_raw_ops: bad argument (op %d, form %d, %d operands)", op, form, n_operands);
    if (n > (size_t)1 << 26) return set_err(HZ_ERR_ARG, "hz_fr_raw_ops: %zu elements (a self test: at most 2^26)", n);
    if (n == 0) return HZ_OK;
    if (hz_device_count() <= 0) return set_err(HZ_ERR_NODEVICE, "no usable gfx950 device");
    HZ_HIP(hipSetDevice(device));
    const size_t in_bytes = (size_t)n_operands * n * 9 * sizeof(uint32_t), out_bytes = n * 9 * sizeof(uint32_t);
    DevBuf d_in, d_out;
    HZ_HIP(d_in.alloc(in_bytes));
    HZ_HIP(d_out.alloc(out_bytes));
    HZ_HIP(hipMemcpy(d_in.p, operands, in_bytes, hipMemcpyHostToDevice));
    HZ_HIP((form ? fr_raw_launch_form1 : fr_raw_launch_form0)(op, n, (const uint32_t*)d_in.p, (uint32_t*)d_out.p, 0));
    HZ_HIP(hipDeviceSynchronize());
    HZ_HIP(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
    return HZ_OK;
}
