// inst_keyed_tiered.hip -- the dimension-sliced keyed scan (kernels_keyed_tiered.h) and its launch, in a translation unit of its own,
// beside inst_keyed.hip: nothing another unit launches is compiled differently.  Every kernel of the headers gets internal linkage
// here; the host side reaches this unit through the launch functions below, and the kernels the entry shares with the keyed and the
// exact search (prep, clear, the scan that reads no row, exact distances, bounds, selection) through inst_keyed.hip's,
// inst_exact_tiered.hip's and inst_exact.hip's.
#include <algorithm>
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#define RQ_KEYED_KERNELS
#define RQ_KEYED_TIERED_KERNELS
#include "kernels_keyed_tiered.h"

// the forms: (plane, S)
template <bool PLANE, int S>
static hipError_t sliced_attribute() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(keyed_scan_sliced_kernel<PLANE, S>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_KEYED_LDS_MAX);
}
hipError_t keyed_sliced_set_attributes() {
    const hipError_t e[4] = {sliced_attribute<false, 64>(), sliced_attribute<false, 128>(), sliced_attribute<true, 64>(), sliced_attribute<true, 128>()};
    for (hipError_t x : e)
        if (x != hipSuccess) return x;
    return hipSuccess;
}
template <bool PLANE>
static void sliced_plane(const KeyedArgs &a, uint32_t nitems, hipStream_t st) {
    const uint32_t S = keyed_sliced_slice(a.dim);  // (the caller has checked that the dimension has a matrix pass)
    if (S == 128) keyed_scan_sliced_kernel<PLANE, 128><<<nitems, 256, keyed_sliced_lds(a.dim, 128).total, st>>>(a);
    else if (S == 64) keyed_scan_sliced_kernel<PLANE, 64><<<nitems, 256, keyed_sliced_lds(a.dim, 64).total, st>>>(a);
}
void launch_keyed_scan_sliced(const KeyedArgs &a, uint32_t nitems, bool plane, hipStream_t st) {
    if (nitems == 0) return;
    if (plane) sliced_plane<true>(a, nitems, st);
    else sliced_plane<false>(a, nitems, st);
}
