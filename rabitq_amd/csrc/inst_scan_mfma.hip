// inst_scan_mfma.hip -- every instantiation of the matrix-core scan kernel the host launches (launch_scan_mfma_* in host_launch.h),
// compiled in a translation unit of its own: an edit of the kernel recompiles this object only.  The shapes: kernel_shapes.h.
#include "common.h"
#include "kernels_scan_mfma.h"
#include "kernel_shapes.h"

#define RQ_MFMA_PARAMS                                                                                                               \
    const uint32_t *, const float4 *, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *, SurvRec *, RunRec *,   \
        unsigned long long *, unsigned long long *, const uint4 *, const float4 *, const float4 *, const ScanArgs
#define RQ_INST(W, NT)                                                                                                               \
    template __global__ void scan_mfma_kernel<W, NT, false, false>(RQ_MFMA_PARAMS);                                                  \
    template __global__ void scan_mfma_kernel<W, NT, true, false>(RQ_MFMA_PARAMS);                                                   \
    template __global__ void scan_mfma_kernel<W, NT, false, false, true>(RQ_MFMA_PARAMS);                                            \
    template __global__ void scan_mfma_kernel<W, NT, true, false, true>(RQ_MFMA_PARAMS);
RQ_SCAN_MFMA_SHAPES(RQ_INST)
#undef RQ_INST
// the additive-gate instantiations (dim 64 / 128, uniform survivor buffers)
#define RQ_INST(W, NT) template __global__ void scan_mfma_kernel<W, NT, false, true>(RQ_MFMA_PARAMS);
RQ_SCAN_MFMA_ADD_SHAPES(RQ_INST)
#undef RQ_INST
