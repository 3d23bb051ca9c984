// inst_maxsim.hip -- the kernels of multi-vector search (kernels_maxsim.h) and their launches, in a translation unit of their own,
// beside inst_exact.hip: the host unit's build time stays what it was.  Every kernel of the headers gets internal linkage here (the
// host unit owns the external definitions of the shared ones); the host side reaches this unit through the launch functions below.
#include <algorithm>
#include "common.h"
#undef __global__
#define __global__ static __attribute__((global))
#define RQ_MAXSIM_KERNELS
#include "kernels_maxsim.h"

template <int MODE, bool PRE>
static hipError_t score_attribute() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(maxsim_score_kernel<MODE, PRE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_MAXSIM_LDS_MAX);
}
template <int MODE>
static hipError_t keyed_attributes() {  // the three forms of maxsim_score_keyed_kernel a row kind has
    const void *f[3] = {reinterpret_cast<const void *>(maxsim_score_keyed_kernel<MODE, true, 1>), reinterpret_cast<const void *>(maxsim_score_keyed_kernel<MODE, false, 1>),
                        reinterpret_cast<const void *>(maxsim_score_keyed_kernel<MODE, true, 2>)};
    for (const void *x : f) {
        const hipError_t e = hipFuncSetAttribute(x, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQ_MAXSIM_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t maxsim_set_attributes() {  // every form may take more than the 64 KB a launch gets as it is
    const hipError_t e[6] = {score_attribute<FETCH_F32, true>(),  score_attribute<FETCH_F32, false>(),  score_attribute<FETCH_HALF, true>(),
                             score_attribute<FETCH_HALF, false>(), score_attribute<FETCH_BYTE, true>(), score_attribute<FETCH_BYTE, false>()};
    for (hipError_t x : e)
        if (x != hipSuccess) return x;
    const hipError_t k[3] = {keyed_attributes<FETCH_F32>(), keyed_attributes<FETCH_HALF>(), keyed_attributes<FETCH_BYTE>()};
    for (hipError_t x : k)
        if (x != hipSuccess) return x;
    return hipSuccess;
}

template <int MODE>
static void score_mode(const MaxsimArgs &a, bool pre, size_t lds, hipStream_t st) {
    const uint32_t grid = a.nq * a.chunks;
    if (pre) maxsim_score_kernel<MODE, true><<<grid, 256, lds, st>>>(a);
    else maxsim_score_kernel<MODE, false><<<grid, 256, lds, st>>>(a);
}
// row_kind: ROW_KIND_* of the index (rows.h), one instantiation per kind, as launch_diverse_select picks the gather's mode
void launch_maxsim_score(const MaxsimArgs &a, int row_kind, bool pre, size_t lds, hipStream_t st) {
    if (row_kind == ROW_KIND_BYTE) score_mode<FETCH_BYTE>(a, pre, lds, st);
    else if (row_kind == ROW_KIND_HALF) score_mode<FETCH_HALF>(a, pre, lds, st);
    else score_mode<FETCH_F32>(a, pre, lds, st);
}
void launch_maxsim_candidates(const MaxsimArgs &a, hipStream_t st) { maxsim_candidates_kernel<<<a.nq, 256, 0, st>>>(a); }
void launch_maxsim_select(const MaxsimArgs &a, hipStream_t st) { maxsim_select_kernel<<<a.nq, 256, 0, st>>>(a); }

// ---- documents named by a column ----
template <int MODE>
static void score_keyed_mode(const MaxsimKeyedArgs &k, bool pre, uint32_t slabs, size_t lds, hipStream_t st) {
    const uint32_t grid = k.m.nq * k.m.chunks;
    if (!pre) maxsim_score_keyed_kernel<MODE, false, 1><<<grid, 256, lds, st>>>(k);
    else if (slabs == 2) maxsim_score_keyed_kernel<MODE, true, 2><<<grid, 256, lds, st>>>(k);
    else maxsim_score_keyed_kernel<MODE, true, 1><<<grid, 256, lds, st>>>(k);
}
void launch_maxsim_score_keyed(const MaxsimKeyedArgs &k, int row_kind, bool pre, uint32_t slabs, size_t lds, hipStream_t st) {
    if (row_kind == ROW_KIND_BYTE) score_keyed_mode<FETCH_BYTE>(k, pre, slabs, lds, st);
    else if (row_kind == ROW_KIND_HALF) score_keyed_mode<FETCH_HALF>(k, pre, slabs, lds, st);
    else score_keyed_mode<FETCH_F32>(k, pre, slabs, lds, st);
}
void launch_keyed_lookup(const unsigned long long *keys, uint64_t m, const MaxsimKeyedArgs &k, uint32_t *seg, hipStream_t st) {
    keyed_lookup_kernel<<<(uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((m + 255) / 256, 4096)), 256, 0, st>>>(keys, m, k, seg);
}
void launch_maxsim_candidates_keyed(const MaxsimKeyedArgs &k, hipStream_t st) { maxsim_candidates_keyed_kernel<<<k.m.nq, 256, 0, st>>>(k); }
void launch_maxsim_select_keyed(const MaxsimKeyedArgs &k, hipStream_t st) { maxsim_select_keyed_kernel<<<k.m.nq, 256, 0, st>>>(k); }
