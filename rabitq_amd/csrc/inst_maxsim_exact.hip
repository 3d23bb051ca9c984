// inst_maxsim_exact.hip -- the kernels of exact multi-vector search (kernels_maxsim_exact.h) and their launches, in a translation
// unit of their own, as inst_maxsim.hip is: that unit and the host unit build as before.  Every kernel of the headers gets internal
// linkage here; the host side reaches this unit through the launch functions below.  The scoring kernel is inst_maxsim.hip's.
#include <algorithm>
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#define RQ_MAXSIM_KERNELS  // (the tile routines of kernels_maxsim.h; none of its kernels is launched from here)
#define RQ_MAXSIM_EXACT_KERNELS
#include "kernels_maxsim_exact.h"

template <int MODE>
static hipError_t bound_attributes() {  // the two forms of maxsim_bound_kernel a row kind has
    const void *f[2] = {reinterpret_cast<const void *>(maxsim_bound_kernel<MODE, 1>), reinterpret_cast<const void *>(maxsim_bound_kernel<MODE, 2>)};
    for (const void *x : f) {
        const hipError_t e = hipFuncSetAttribute(x, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_MAXSIM_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t maxsim_exact_set_attributes() {  // every form may take more than the 64 KB a launch gets as it is
    const hipError_t k[3] = {bound_attributes<FETCH_F32>(), bound_attributes<FETCH_HALF>(), bound_attributes<FETCH_BYTE>()};
    for (hipError_t x : k)
        if (x != hipSuccess) return x;
    return hipSuccess;
}

void launch_maxsim_bound_prep(const MaxsimBoundArgs &a, hipStream_t st) {
    const uint64_t rows = (uint64_t)a.nq * ((a.T + 31u) & ~31u);
    maxsim_bound_prep_kernel<<<(uint32_t)((rows + 3) / 4), 256, 0, st>>>(a);
}
template <int MODE>
static void bound_mode(const MaxsimBoundArgs &a, uint32_t slabs, dim3 grid, size_t lds, hipStream_t st) {
    if (slabs == 2) maxsim_bound_kernel<MODE, 2><<<grid, 256, lds, st>>>(a);
    else maxsim_bound_kernel<MODE, 1><<<grid, 256, lds, st>>>(a);
}
// row_kind: ROW_KIND_* of the index (rows.h), one instantiation per kind, as launch_maxsim_score_keyed picks the gather's mode
void launch_maxsim_bound(const MaxsimBoundArgs &a, int row_kind, uint32_t slabs, uint32_t units, size_t lds, hipStream_t st) {
    const dim3 grid(units, (a.nq + a.Bc - 1) / a.Bc);
    if (row_kind == ROW_KIND_BYTE) bound_mode<FETCH_BYTE>(a, slabs, grid, lds, st);
    else if (row_kind == ROW_KIND_HALF) bound_mode<FETCH_HALF>(a, slabs, grid, lds, st);
    else bound_mode<FETCH_F32>(a, slabs, grid, lds, st);
}
void launch_maxsim_bound_threshold(const MaxsimBoundArgs &a, hipStream_t st) { maxsim_bound_threshold_kernel<<<a.nq, 256, 0, st>>>(a); }
void launch_maxsim_bound_compact(const MaxsimBoundArgs &a, hipStream_t st) { maxsim_bound_compact_kernel<<<a.nq, 256, 0, st>>>(a); }
void launch_maxsim_exact_round(const MaxsimBoundArgs &a, uint32_t first, uint32_t slots, uint32_t *cand, uint32_t *cand_n, hipStream_t st) {
    maxsim_exact_round_kernel<<<dim3((slots + 255) / 256, a.nq), 256, 0, st>>>(a, first, slots, cand, cand_n);
}
void launch_maxsim_exact_merge(const MaxsimKeyedArgs &k, unsigned long long *run, uint32_t *run_n, bool first, bool last, hipStream_t st) {
    maxsim_exact_merge_kernel<<<k.m.nq, 256, 0, st>>>(k, run, run_n, first ? 1u : 0u, last ? 1u : 0u);
}
