// inst_keyed.hip -- the kernels of the postings and of the keyed exact search (kernels_keyed.h) and their launches, in a translation
// unit of their own, beside inst_exact.hip and inst_maxsim.hip: the host unit's build time stays what it was.  Every kernel of the
// headers gets internal linkage here (the host unit owns the external definitions of the shared ones); the host side reaches this
// unit through the launch functions below.
#include <algorithm>
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#define RQ_KEYED_KERNELS
#include "kernels_keyed.h"

template <int MODE>
static hipError_t scan_attribute() {  // PRE = true may take more than the 64 KB a launch gets as it is
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(keyed_scan_kernel<MODE, true, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_KEYED_LDS_MAX);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(keyed_scan_kernel<MODE, true, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_KEYED_LDS_MAX);
}
hipError_t keyed_set_attributes() {
    const hipError_t e[3] = {scan_attribute<FETCH_F32>(), scan_attribute<FETCH_HALF>(), scan_attribute<FETCH_BYTE>()};
    for (hipError_t x : e)
        if (x != hipSuccess) return x;
    return hipSuccess;
}

void launch_post_pass(const PostArgs &a, bool wide, bool scatter, hipStream_t st) {
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((a.n + 255) / 256, 8192));
    if (wide && scatter) post_pass_kernel<true, true><<<grid, 256, 0, st>>>(a);
    else if (wide) post_pass_kernel<true, false><<<grid, 256, 0, st>>>(a);
    else if (scatter) post_pass_kernel<false, true><<<grid, 256, 0, st>>>(a);
    else post_pass_kernel<false, false><<<grid, 256, 0, st>>>(a);
}
void launch_post_compact(const PostArgs &a, uint4 *pairs, uint32_t cap, uint32_t *out_n, hipStream_t st) {
    post_compact_kernel<<<4096, 256, 0, st>>>(a, pairs, cap, out_n);
}
void launch_post_cursor(const uint2 *slot_start, uint32_t nv, uint32_t *count, hipStream_t st) {
    if (nv) post_cursor_kernel<<<(nv + 255) / 256, 256, 0, st>>>(slot_start, nv, count);
}

void launch_keyed_clear(unsigned int *cnt, uint32_t n, hipStream_t st) {
    if (n) keyed_clear_kernel<<<(n + 255) / 256, 256, 0, st>>>(cnt, n);
}
void launch_keyed_prep(const KeyedArgs &a, hipStream_t st) {
    if (a.tiles) keyed_prep_kernel<<<a.tiles * 8u, 256, 0, st>>>(a);
}
template <int MODE>
static void scan_mode(const KeyedArgs &a, uint32_t nitems, bool pre, uint32_t slabs, hipStream_t st) {
    if (pre && slabs == 2) keyed_scan_kernel<MODE, true, 2><<<nitems, 256, keyed_lds(a.dim, true, 2).total, st>>>(a);
    else if (pre) keyed_scan_kernel<MODE, true, 1><<<nitems, 256, keyed_lds(a.dim, true, 1).total, st>>>(a);
    else keyed_scan_kernel<MODE, false, 1><<<nitems, 256, keyed_lds(a.dim, false, 1).total, st>>>(a);
}
// row_kind: ROW_KIND_* of the index (rows.h), one instantiation per kind, as launch_maxsim_score picks the gather's mode; slabs: 2 =
// the double-buffered form (the caller has checked keyed_slabs)
void launch_keyed_scan(const KeyedArgs &a, uint32_t nitems, int row_kind, bool pre, uint32_t slabs, hipStream_t st) {
    if (nitems == 0) return;
    if (row_kind == ROW_KIND_BYTE) scan_mode<FETCH_BYTE>(a, nitems, pre, slabs, st);
    else if (row_kind == ROW_KIND_HALF) scan_mode<FETCH_HALF>(a, nitems, pre, slabs, st);
    else scan_mode<FETCH_F32>(a, nitems, pre, slabs, st);
}
