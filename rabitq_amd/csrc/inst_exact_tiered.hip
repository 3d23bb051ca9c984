// inst_exact_tiered.hip -- the kernels of the exact search on split-row and tiered indexes (kernels_exact_tiered.h) and their launches,
// in a translation unit of their own, beside inst_exact.hip: nothing another unit launches is compiled differently.  Every kernel of
// the headers gets internal linkage here; the host side reaches this unit through the launch functions below, and the kernels it
// shares with the plain exact search (prep, bounds, selection, the scan without a pre-filter, the range tail) through inst_exact.hip's.
#include <algorithm>
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#define RQ_EXACT_KERNELS
#define RQ_EXACT_TIERED_KERNELS
#include "kernels_exact_tiered.h"

hipError_t exact_tiered_set_attributes() {
    // RT = 1 (the wide dimensions) may take the whole LDS of a CU, as exact_scan_kernel<1> does
    const void *wide[4] = {reinterpret_cast<const void *>(exact_scan_plane_kernel<1, true, false>), reinterpret_cast<const void *>(exact_scan_plane_kernel<1, true, true>),
                           reinterpret_cast<const void *>(exact_scan_plane_kernel<1, false, false>), reinterpret_cast<const void *>(exact_scan_plane_kernel<1, false, true>)};
    for (const void *f : wide) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_EXACT_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void launch_tier_tile_list(const TierView &tv, uint32_t tile_rows, uint32_t tiles, uint32_t *tile_list, hipStream_t st) {
    if (tiles) tier_tile_list_kernel<<<(tiles + 255) / 256, 256, 0, st>>>(tv, tile_rows, tiles, tile_list);
}
template <int RT, bool PLANE>
static void scan_tier_rt(const TierScanArgs &ta, bool range, hipStream_t st) {
    const uint32_t blocks = (uint32_t)(((uint64_t)ta.tv.rows + 32 * RT - 1) / (32 * RT));
    if (blocks == 0) return;
    if (range) exact_scan_plane_kernel<RT, PLANE, true><<<blocks, 256, exact_scan_lds_bytes(RT, ta.a.dim), st>>>(ta);
    else exact_scan_plane_kernel<RT, PLANE, false><<<blocks, 256, exact_scan_lds_bytes(RT, ta.a.dim), st>>>(ta);
}
template <bool PLANE>
static void scan_tier(const TierScanArgs &ta, bool range, hipStream_t st) {
    const uint32_t rt = exact_scan_subtiles(ta.a.dim);  // (the caller has checked that a tile fits)
    if (rt == 4) scan_tier_rt<4, PLANE>(ta, range, st);
    else if (rt == 2) scan_tier_rt<2, PLANE>(ta, range, st);
    else scan_tier_rt<1, PLANE>(ta, range, st);
}
void launch_exact_scan_tier(const TierScanArgs &ta, bool plane, bool range, hipStream_t st) {
    if (plane) scan_tier<true>(ta, range, st);
    else scan_tier<false>(ta, range, st);
}
void launch_exact_dist_tiered(const ExactArgs &a, hipStream_t st) {
    const uint32_t per_q = std::min<uint32_t>(std::max<uint32_t>((a.cap + 127) / 128, 1u), 64u);
    exact_dist_tiered_kernel<<<dim3(a.nq, per_q), 256, (size_t)a.dim * 4, st>>>(a);
}
void launch_exact_range_dist_tiered(const ExactArgs &a, uint32_t *hits, uint32_t records, hipStream_t st) {
    if (records == 0) return;
    exact_range_dist_tiered_kernel<<<std::min<uint32_t>((uint32_t)(((uint64_t)records + 127) / 128), 1u << 20), 256, 0, st>>>(a, hits, records);
}
