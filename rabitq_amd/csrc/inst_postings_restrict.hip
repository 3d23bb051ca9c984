// inst_postings_restrict.hip -- the kernels of restricted postings (kernels_postings_restrict.h) and their launches, in a translation
// unit of their own, beside inst_keyed.hip: that unit and the host unit build as before.  Every kernel of the header gets internal
// linkage here; the host side reaches this unit through the launch functions below.
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#define RQ_POSTINGS_RESTRICT_KERNELS
#include "kernels_postings_restrict.h"

void launch_restrict_admit(const PostRestrictArgs &a, hipStream_t st) { restrict_admit_kernel<<<restrict_chunks(a.n), 256, 0, st>>>(a); }
void launch_restrict_scan(uint32_t *counts, uint32_t chunks, uint32_t *total, hipStream_t st) {
    restrict_scan_kernel<<<1, 1024, 0, st>>>(counts, chunks, total);
}
void launch_restrict_take(const PostRestrictArgs &a, hipStream_t st) { restrict_take_kernel<<<restrict_chunks(a.n), 256, 0, st>>>(a); }
void launch_restrict_segments(const PostRestrictArgs &a, hipStream_t st) { restrict_segments_kernel<<<restrict_chunks(a.nv), 256, 0, st>>>(a); }
void launch_restrict_segments_take(const PostRestrictArgs &a, hipStream_t st) {
    restrict_segments_take_kernel<<<restrict_chunks(a.nv), 256, 0, st>>>(a);
}
