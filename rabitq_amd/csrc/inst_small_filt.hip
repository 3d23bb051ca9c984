// inst_small_filt.hip -- the filtered instantiations of sb_query_kernel (kernels_small.h: six widths x three ranker modes), compiled
// in a translation unit of their own so that the host unit builds as fast as it did without them.  The host side reaches them through
// the two functions at the end (declared in host_launch.h).  Every kernel of the headers gets internal linkage here (the host unit
// owns the external definitions), and only the instantiations below are launched from this unit.
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#include "kernels_small.h"
#include "kernel_shapes.h"

template <int W>
static void launch_w(int mode, uint32_t nq, size_t dyn, hipStream_t st, const SbArgs &sa) {
    if (mode == 2) sb_query_kernel<W, 2, true><<<nq, 1024, dyn, st>>>(sa);
    else if (mode == 1) sb_query_kernel<W, 1, true><<<nq, 1024, dyn, st>>>(sa);
    else sb_query_kernel<W, 0, true><<<nq, 1024, dyn, st>>>(sa);
}
void launch_sb_query_filtered(uint32_t W, int mode, uint32_t nq, size_t dyn, hipStream_t st, const SbArgs &sa) {
#define RQ_SBQ(WW) case WW: launch_w<WW>(mode, nq, dyn, st, sa); break;
    switch (W) {
        RQ_SMALL_BATCH_WIDTHS(RQ_SBQ)
        default: break;  // (not reached: plan_pass takes the path for the widths of the same list only)
    }
#undef RQ_SBQ
}

template <int W>
static hipError_t attr_w(int bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(sb_query_kernel<W, 0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(sb_query_kernel<W, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(sb_query_kernel<W, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return e;
}
hipError_t sb_query_filtered_set_attributes(int bytes) {
    hipError_t e = hipSuccess;
#define RQ_SBQ(WW) if (e == hipSuccess) e = attr_w<WW>(bytes);
    RQ_SMALL_BATCH_WIDTHS(RQ_SBQ)
#undef RQ_SBQ
    return e;
}
