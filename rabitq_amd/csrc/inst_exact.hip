// inst_exact.hip -- the kernels of the exact search (kernels_exact.h) and their launches, in a translation unit of their own, beside
// inst_scan_*.hip: an edit of the scan recompiles this object only.  Every kernel of the headers gets internal linkage here (the host
// unit owns the external definitions of the shared ones); the host side reaches this unit through the launch functions below.
#include <algorithm>
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#define RQ_EXACT_KERNELS
#include "kernels_exact.h"

hipError_t exact_set_attributes() {
    // RT = 1 (the wide dimensions) may take the whole LDS of a CU; the other forms stay within what a launch may ask for as it is
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(exact_scan_kernel<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_EXACT_LDS_MAX);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(exact_scan_kernel<1, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_EXACT_LDS_MAX);
}

void launch_exact_prep(const ExactArgs &a, hipStream_t st) {
    exact_prep_kernel<<<(a.nq32 + 3) / 4, 256, 0, st>>>(a);
}
void launch_exact_thr(const float *seed_dist, const uint32_t *seed_n, uint32_t nq, uint32_t topk, float *thr, unsigned int *unfilled, hipStream_t st) {
    exact_thr_kernel<<<(nq + 255) / 256, 256, 0, st>>>(seed_dist, seed_n, nq, topk, thr, unfilled);
}
template <int RT>
static void scan_rt(const ExactArgs &a, bool prefilter, hipStream_t st) {
    const uint32_t blocks = (uint32_t)(((uint64_t)a.rows + 32 * RT - 1) / (32 * RT));
    if (prefilter) exact_scan_kernel<RT, true><<<blocks, 256, exact_scan_lds_bytes(RT, a.dim), st>>>(a);
    else exact_scan_kernel<RT, false><<<blocks, 256, (size_t)RT * 32 * 12, st>>>(a);
}
void launch_exact_scan(const ExactArgs &a, bool prefilter, hipStream_t st) {
    const uint32_t rt = prefilter ? exact_scan_subtiles(a.dim) : 4u;
    if (rt == 4) scan_rt<4>(a, prefilter, st);
    else if (rt == 2) scan_rt<2>(a, prefilter, st);
    else scan_rt<1>(a, prefilter, st);
}
void launch_exact_dist(const ExactArgs &a, hipStream_t st) {
    const uint32_t per_q = std::min<uint32_t>(std::max<uint32_t>((a.cap + 127) / 128, 1u), 64u);
    exact_dist_kernel<<<dim3(a.nq, per_q), 256, (size_t)a.dim * 4, st>>>(a);
}
void launch_exact_select(const ExactArgs &a, hipStream_t st) {
    exact_select_kernel<<<a.nq, 256, 0, st>>>(a);
}

// ---- the range form (the scan's RANGE instantiations, the arena's exact distances, the scatter into segments) ----
void launch_exact_range_thr(const float *radius, uint32_t nq, float *thr, hipStream_t st) {
    exact_range_thr_kernel<<<(nq + 255) / 256, 256, 0, st>>>(radius, nq, thr);
}
template <int RT>
static void range_scan_rt(const ExactArgs &a, bool prefilter, hipStream_t st) {
    const uint32_t blocks = (uint32_t)(((uint64_t)a.rows + 32 * RT - 1) / (32 * RT));
    if (prefilter) exact_scan_kernel<RT, true, true><<<blocks, 256, exact_scan_lds_bytes(RT, a.dim), st>>>(a);
    else exact_scan_kernel<RT, false, true><<<blocks, 256, (size_t)RT * 32 * 12, st>>>(a);
}
void launch_exact_range_scan(const ExactArgs &a, bool prefilter, hipStream_t st) {
    const uint32_t rt = prefilter ? exact_scan_subtiles(a.dim) : 4u;
    if (rt == 4) range_scan_rt<4>(a, prefilter, st);
    else if (rt == 2) range_scan_rt<2>(a, prefilter, st);
    else range_scan_rt<1>(a, prefilter, st);
}
void launch_exact_range_dist(const ExactArgs &a, uint32_t *hits, uint32_t records, hipStream_t st) {
    if (records == 0) return;
    exact_range_dist_kernel<<<std::min<uint32_t>((uint32_t)(((uint64_t)records + 127) / 128), 1u << 20), 256, 0, st>>>(a, hits, records);
}
void launch_exact_range_scatter(const ExactArgs &a, const ExactSegments &sg, uint32_t records, hipStream_t st) {
    if (records == 0) return;
    exact_range_scatter_kernel<<<std::min<uint32_t>((uint32_t)(((uint64_t)records + 255) / 256), 1u << 20), 256, 0, st>>>(a.rec, a.keys, records, sg);
}
