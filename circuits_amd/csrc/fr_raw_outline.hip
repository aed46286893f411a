// hz_fr_raw_ops, form 1: the kernels of fr_raw_ops.h built WITHOUT HZ_FR_INLINE -- fr_mul, fr_sqr, fr_to_canon and fr_inv are the
// out-of-line bodies that the gadget mains and the fee / withdraw / SHA kernels call.
#define HZ_FR_RAW_FORM 1
#include <hip/hip_runtime.h>
#include "fr_raw_ops.h"
