// inst_scan_valu.hip -- every instantiation of the VALU scan kernel the host launches (launch_scan_t in host_launch.h), compiled in a
// translation unit of its own: an edit of the kernel recompiles this object only.  The shapes: kernel_shapes.h.
#include "common.h"
#include "kernels_scan_valu.h"
#include "kernel_shapes.h"

#define RQ_INST(W, CPL)                                                                                                              \
    template __global__ void scan_kernel<W, CPL, false>(SCAN_PARAMS);                                                                \
    template __global__ void scan_kernel<W, CPL, true>(SCAN_PARAMS);                                                                 \
    template __global__ void scan_kernel<W, CPL, false, true>(SCAN_PARAMS);                                                          \
    template __global__ void scan_kernel<W, CPL, true, true>(SCAN_PARAMS);
RQ_SCAN_VALU_SHAPES(RQ_INST)
#undef RQ_INST
