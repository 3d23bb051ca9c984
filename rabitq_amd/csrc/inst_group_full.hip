// inst_group_full.hip -- the kernels of the complete exact grouped search (kernels_group_full.h) and their launches, in a translation
// unit of their own, beside inst_exact.hip and inst_keyed.hip: no existing unit is recompiled differently.  Every kernel of the headers
// gets internal linkage here (the host unit owns the external definitions of the shared ones); the host side reaches this unit through
// the launch functions below.
#include <algorithm>
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#define RQ_GROUP_FULL_KERNELS
#include "kernels_group_full.h"

static uint32_t grid_of(uint64_t items, uint32_t per_block) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, 1u << 20));
}

void launch_group_full_inverse(const uint32_t *post, const uint32_t *starts, uint32_t nv, uint64_t rows, uint32_t *inverse, uint64_t n, hipStream_t st) {
    if (n == 0) return;
    group_full_fill_kernel<<<grid_of(n, 256), 256, 0, st>>>(inverse, n);
    if (rows && nv) group_full_inverse_kernel<<<grid_of(rows, 256), 256, 0, st>>>(post, starts, nv, rows, inverse, n);
}
// (the two LDS shapes: 16 KB up to topk 256, 48 KB beyond)
void launch_group_full_bound(const ExactArgs &sample, const uint32_t *inverse, uint32_t topk, float *thr, hipStream_t st) {
    if (sample.nq == 0) return;
    if (topk <= RQ_GF_TOPK_SMALL) group_full_bound_kernel<RQ_GF_TOPK_SMALL, 3><<<sample.nq, 256, 0, st>>>(sample, inverse, topk, thr);
    else group_full_bound_kernel<2048, 4><<<sample.nq, 256, 0, st>>>(sample, inverse, topk, thr);
}
void launch_group_full_dist(const ExactArgs &a, const uint32_t *inverse, uint32_t *segs, uint32_t *hits, uint32_t records, hipStream_t st) {
    if (records == 0) return;
    group_full_dist_kernel<<<grid_of(records, 128), 256, 0, st>>>(a, inverse, segs, hits, records);
}
void launch_group_full_scatter(const ExactArgs &a, const uint32_t *segs, const ExactSegments &sg, uint32_t *out_segs, uint32_t records, hipStream_t st) {
    if (records == 0) return;
    group_full_scatter_kernel<<<grid_of(records, 256), 256, 0, st>>>(a.rec, a.keys, segs, records, sg, out_segs);
}
void launch_group_full_select(const GroupFullSelectArgs &a, uint32_t nq, hipStream_t st) {
    if (nq == 0) return;
    if (a.topk <= RQ_GF_TOPK_SMALL) group_full_select_kernel<RQ_GF_TOPK_SMALL, 3><<<nq, 256, 0, st>>>(a);
    else group_full_select_kernel<2048, 4><<<nq, 256, 0, st>>>(a);
}
void launch_group_full_expand(const float *q, uint32_t len, uint32_t topk, uint64_t cells, float *out, hipStream_t st) {
    if (cells) group_full_expand_kernel<<<grid_of(cells, 256), 256, 0, st>>>(q, len, topk, cells, out);
}
