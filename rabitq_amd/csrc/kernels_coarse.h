// kernels_coarse.h -- the coarse ranking of RaBitQ::query (src/rabitq.rs:283-297): every query's distance to every centroid, the
// `nprobe` smallest (distance, list id) pairs in ascending order.
//
//   coarse_dist_sreg_kernel / coarse_dist_kernel   all k distances in the reference's operation order
//   select_probe_kernel                            block-per-query radix select over a row of distances
//   select_probe_wave_kernel                       wave-per-query selection, the row in registers (nprobe <= 64, k <= 8192)
//   coarse_approx_kernel                           bf16 matrix-core approximation of the row (the pre-filter)
//   select_refine_wave_kernel / _tiled_kernel      candidates within the pre-filter's margin, exact distances of those, selection
//
// The wave-level pieces (row loader, bisections, ballot append, shuffle sort, row writer, exact-order row, margin, centroid-tile
// streamer) exist once, below; kernels_small.h (select_slice_wave) and kernels_build.h (assign_approx_kernel) use them too.
#pragma once
#ifndef RQ_COLLECT_UNROLL
#define RQ_COLLECT_UNROLL 8  // 16 tiles per step: coarse 1.07 -> 1.03 ms per step (4: the round-4 form; 16 no better)
#endif
#include "common.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// Coarse distances (src/rabitq.rs:285-293): dist[q][j] = l2_squared_distance(centroid_j, y_q) in
// the exact order of src/simd.rs:14-73 (diff rounded, then fused square-accumulate per AVX lane).
// lane <-> centroid j over the TRANSPOSED rotated centroids cent_t[dim][k] (coalesced; this is also
// the reference's on-disk centroids.fvecs layout), QT queries per thread held in LDS (broadcast).
// ------------------------------------------------------------------------------------------------
// Large batches: the same distances with the QUERY side in scalar registers.  A lane still owns one list; the block's
// QT queries are read through the scalar unit (their rows are wave-uniform), 16 dimensions of one query per
// s_load_dwordx16, and enter the packed ops as SGPR pairs: two neighbouring dimensions (= two neighbouring AVX
// lanes of src/simd.rs:14-73, each with its own accumulator and per-component rounding) per v_pk_add_f32 /
// v_pk_fma_f32.  No LDS: the LDS-broadcast form above spends as many LDS cycles as VALU cycles per element and
// stalls at half the packed-f32 rate.  QT queries per centroid element loaded (8: 86 VGPRs, five waves per SIMD; 16 was
// measured slower, three waves per SIMD do not cover the scalar loads).
template <int QT>
__global__ __launch_bounds__(256) void coarse_dist_sreg_kernel(const float *__restrict__ cent_t,
                                                               const float *__restrict__ y, float *__restrict__ dist,
                                                               uint32_t k, uint32_t dim, uint32_t nq, uint32_t kstride) {
    const uint32_t q0 = blockIdx.x * QT;
    const uint32_t j = blockIdx.y * 256 + threadIdx.x;
    const bool live = j < k;
    const float *cp = cent_t + (live ? j : 0);
    f32x2 acc[QT][4];  // [query][pair of AVX lanes]
#pragma unroll
    for (int v = 0; v < QT; ++v)
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[v][l] = f32x2{0.0f, 0.0f};
    static_assert(QT % 4 == 0, "queries are fetched four at a time");
    for (uint32_t c = 0; c < dim; c += 16) {  // dim is a multiple of 64
        float ce[16];
#pragma unroll
        for (int l = 0; l < 16; ++l) ce[l] = cp[(uint64_t)(c + l) * kstride];  // 16 loads in flight
#pragma unroll
        for (int v0 = 0; v0 < QT; v0 += 4) {
            float yv[4][16];  // four queries x 16 dimensions: four s_load_dwordx16 issued together
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const uint32_t q = q0 + v0 + v < nq ? q0 + v0 + v : nq - 1;  // uniform; rows past the batch are computed and dropped
                const float *yq = y + (uint64_t)q * dim + c;
#pragma unroll
                for (int l = 0; l < 16; ++l) yv[v][l] = yq[l];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)  // the two 8-dimension steps of the chunk, in order (one accumulator chain per AVX lane)
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        const f32x2 c2 = {ce[8 * h + 2 * l], ce[8 * h + 2 * l + 1]};
                        const f32x2 y2 = {yv[v][8 * h + 2 * l], yv[v][8 * h + 2 * l + 1]};
                        const f32x2 d2 = c2 - y2;
                        acc[v0 + v][l] = __builtin_elementwise_fma(d2, d2, acc[v0 + v][l]);
                    }
        }
    }
    if (live) {
#pragma unroll
        for (int v = 0; v < QT; ++v) {
            float a[8];
#pragma unroll
            for (int l = 0; l < 4; ++l) a[2 * l] = acc[v][l].x, a[2 * l + 1] = acc[v][l].y;
            if (q0 + v < nq) dist[(uint64_t)(q0 + v) * k + j] = reduce8_regs(a);
        }
    }
}

template <int QT>
__global__ __launch_bounds__(256) void coarse_dist_kernel(const float *__restrict__ cent_t,
                                                          const float *__restrict__ y,
                                                          float *__restrict__ dist, uint32_t k,
                                                          uint32_t dim, uint32_t nq, uint32_t kstride) {
    // cent_t points at the first list of the range; k = number of lists ranked, kstride = row stride
    extern __shared__ __attribute__((aligned(16))) float ys[];  // [dim][QT]: one ds_read_b128 = 4 queries at one dimension
    const uint32_t q0 = blockIdx.x * QT;
    const uint32_t j = blockIdx.y * 256 + threadIdx.x;
    for (uint32_t i = threadIdx.x; i < QT * dim; i += 256) {
        uint32_t v = i / dim, e = i - v * dim;  // coalesced reads of y, transposed into LDS
        ys[e * QT + v] = (q0 + v < nq) ? y[(uint64_t)(q0 + v) * dim + e] : 0.0f;
    }
    __syncthreads();
    static_assert(QT % 4 == 0, "queries are processed in packed pairs, read four at a time");
    f32x2 acc[QT / 2][8];  // [query pair][AVX lane]: v_pk_add_f32 + v_pk_fma_f32, per-component rounding
#pragma unroll
    for (int v = 0; v < QT / 2; ++v)
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[v][l] = f32x2{0.0f, 0.0f};
    const bool live = j < k;
    const float *cp = cent_t + (live ? j : 0);
    for (uint32_t c = 0; c < dim; c += 8) {
        float ce[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) ce[l] = cp[(uint64_t)(c + l) * kstride];  // 8 loads in flight
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const f32x2 ce2 = {ce[l], ce[l]};
#pragma unroll
            for (int v4 = 0; v4 < QT / 4; ++v4) {
                const float4 yq = *reinterpret_cast<const float4 *>(&ys[(c + l) * QT + 4 * v4]);
                const f32x2 y01 = {yq.x, yq.y}, y23 = {yq.z, yq.w};
                const f32x2 d01 = ce2 - y01, d23 = ce2 - y23;
                acc[2 * v4][l] = __builtin_elementwise_fma(d01, d01, acc[2 * v4][l]);
                acc[2 * v4 + 1][l] = __builtin_elementwise_fma(d23, d23, acc[2 * v4 + 1][l]);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int v = 0; v < QT / 2; ++v) {
            float a0[8], a1[8];
#pragma unroll
            for (int l = 0; l < 8; ++l) a0[l] = acc[v][l].x, a1[l] = acc[v][l].y;
            if (q0 + 2 * v < nq) dist[(uint64_t)(q0 + 2 * v) * k + j] = reduce8_regs(a0);
            if (q0 + 2 * v + 1 < nq) dist[(uint64_t)(q0 + 2 * v + 1) * k + j] = reduce8_regs(a1);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Wave-level pieces of the probe selection.  One wave works on one row (or slice of a row) of distances; keys are the monotone
// u32 image of the distance (ord32_biased), 0xFFFFFFFF = "no list" (above every real key; a NaN distance with all-ones payload is
// not supported); a winner is the u64 (key << 32 | list id), unique, so any ascending sort gives one order.
// ------------------------------------------------------------------------------------------------
// register i of lane l holds list 256 (i / 4) + 4 l + (i % 4): a row is read 16 bytes per lane, 1 KiB per wave instruction
__device__ __forceinline__ uint32_t row_list_of(int i, uint32_t lane) { return 256u * (uint32_t)(i >> 2) + 4u * lane + (uint32_t)(i & 3); }

// four consecutive distances d[j0 .. j0 + 4) of a row of n (0 past the end).  vec4: d is 16-byte aligned and n % 4 == 0 (the
// callers pass (k & 3) == 0 of the whole row; slices start at a multiple of 4).  A 16-byte load is issued only where all four
// elements are inside the row and the address is 16-byte aligned; j0 % 4 == 0 and n % 4 == 0 make that every j0 < n.
__device__ __forceinline__ float4 row_load4(const float *__restrict__ d, uint32_t j0, uint32_t n, bool vec4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec4 && j0 + 3 < n) {
        v = *reinterpret_cast<const float4 *>(d + j0);
    } else if (!vec4) {
        if (j0 < n) v.x = d[j0];
        if (j0 + 1 < n) v.y = d[j0 + 1];
        if (j0 + 2 < n) v.z = d[j0 + 2];
        if (j0 + 3 < n) v.w = d[j0 + 3];
    }
    return v;
}

// the row d[0 .. n) as keys in registers (n <= 64 KPL), and the smallest / largest real key, uniform (in scalar registers: the
// bisections run on the scalar unit)
template <int KPL>
__device__ __forceinline__ void row_keys(const float *__restrict__ d, uint32_t n, bool vec4, uint32_t (&key)[KPL], uint32_t &kmin,
                                         uint32_t &kmax) {
    const uint32_t lane = threadIdx.x & 63;
    kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int i4 = 0; i4 < KPL; i4 += 4) {
        const uint32_t j0 = row_list_of(i4, lane);
        const float4 v = row_load4(d, j0, n, vec4);
        const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i4 + e;
            key[i] = 0xFFFFFFFFu;
            if (j0 + e < n) {
                key[i] = ord32_biased(ve[e]);
                kmin = key[i] < kmin ? key[i] : kmin;
                kmax = key[i] > kmax ? key[i] : kmax;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t a = __shfl_xor(kmin, o, 64), c = __shfl_xor(kmax, o, 64);
        kmin = a < kmin ? a : kmin;
        kmax = c > kmax ? c : kmax;
    }
    kmin = __builtin_amdgcn_readfirstlane(kmin), kmax = __builtin_amdgcn_readfirstlane(kmax);
}

// wave-wide count of keys <= t: one compare per register, the lane counts come out of the scalar unit (ballot + s_bcnt1), no
// cross-lane shuffles.  ("no list" slots count exactly when t == 0xFFFFFFFF.)
template <int N>
__device__ __forceinline__ uint32_t count_le(const uint32_t (&key)[N], uint32_t t) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) c += (uint32_t)__popcll(__ballot(key[i] <= t));
    return c;
}

// The `want`-th smallest (key, list id) of a row in registers (1 <= want <= n): T = the smallest threshold with
// count(key <= T) >= want, by bisection on the key, stopping as soon as a threshold selects exactly `want` (typically ~20 steps);
// ties at T are broken by list id (a second bisection, rare): among keys == T only lists <= J are taken (J = 0xFFFFFFFF: all).
template <int KPL>
__device__ __forceinline__ void bisect_exact(const uint32_t (&key)[KPL], uint32_t n, uint32_t want, uint32_t kmin, uint32_t kmax,
                                             uint32_t &T, uint32_t &J) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t lo = kmin, hi = kmax;
    T = kmax, J = 0xFFFFFFFFu;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t c = count_le(key, mid);
        if (c == want) {
            T = mid;
            return;
        }
        if (c > want) hi = mid;
        else lo = mid + 1;
    }
    T = lo;
    const uint32_t c_le = count_le(key, T);
    if (c_le > want) {  // ties at the threshold: the smallest list ids win
        const uint32_t c_lt = T ? count_le(key, T - 1) : 0u;
        const uint32_t need = want - c_lt;  // >= 1
        uint32_t jl = 0, jh = n - 1;
        while (jl < jh) {
            const uint32_t jm = jl + ((jh - jl) >> 1);
            uint32_t c = 0;
#pragma unroll
            for (int i = 0; i < KPL; ++i) c += (key[i] == T && row_list_of(i, lane) <= jm) ? 1u : 0u;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
            c = __builtin_amdgcn_readfirstlane(c);
            if (c >= need) jh = jm;
            else jl = jm + 1;
        }
        J = jl;
    }
}

// ANY T with count(<= T) >= nprobe bounds the nprobe-th smallest key from above, which is all the candidate rule of the
// pre-filter needs: the bisection over [lo, hi] (count(<= hi) >= nprobe) stops as soon as the count lands in
// [nprobe, nprobe + 12] (7-9 steps instead of the ~25 an exact threshold takes; the price is up to 12 more candidates).
template <typename CountFn>
__device__ __forceinline__ uint32_t bisect_loose(uint32_t lo, uint32_t hi, uint32_t nprobe, CountFn count) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t c = count(mid);
        if (c >= nprobe) {
            hi = mid;
            if (c <= nprobe + 12) break;
        } else {
            lo = mid + 1;
        }
    }
    return hi;
}

// ballot append: the lanes with `take` store at consecutive slots from `base`, in lane order; returns the new base.  Nothing is
// stored by a step that would pass `limit` slots, while base still advances (the caller sees base > limit).
template <typename StoreFn>
__device__ __forceinline__ uint32_t wave_compact(bool take, uint32_t base, uint32_t limit, StoreFn store) {
    const uint64_t m = __ballot(take);
    if (m) {  // wave-uniform
        const uint32_t cnt = (uint32_t)__popcll(m);
        if (take && base + cnt <= limit) store(base + (uint32_t)__popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull)));
        base += cnt;
    }
    return base;
}

// bitonic sort of 64 NS keys across the wave, ascending: element index i = lane + 64 s (s = the lane's slot); at a step
// (size, stride) element i keeps the minimum of (i, i ^ stride) iff ((i & stride) == 0) == ((i & size) == 0)  (the last size
// ascends everywhere).  Strides below 64 are shuffles, the others pair slots of the same lane.
template <int NS>
__device__ __forceinline__ void wave_sort_u64(unsigned long long (&vs)[NS]) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int size = 2; size <= 64 * NS; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            if (stride >= 64) {  // the partner is another slot of the same lane
                const int ss = stride / 64;
#pragma unroll
                for (int sl = 0; sl < NS; ++sl) {
                    if (sl & ss) continue;
                    const bool asc = size >= 64 * NS || ((64 * sl) & size) == 0;
                    const unsigned long long a0 = vs[sl], b0 = vs[sl | ss];
                    const unsigned long long mn = a0 < b0 ? a0 : b0, mxv = a0 < b0 ? b0 : a0;
                    vs[sl] = asc ? mn : mxv, vs[sl | ss] = asc ? mxv : mn;
                }
            } else {
                const bool lower = (lane & stride) == 0;
#pragma unroll
                for (int sl = 0; sl < NS; ++sl) {
                    const unsigned long long o = __shfl_xor(vs[sl], stride, 64);
                    const bool asc = size < 64 ? (lane & size) == 0 : (size >= 64 * NS || ((64 * sl) & size) == 0);
                    const unsigned long long mn = o < vs[sl] ? o : vs[sl], mxv = o < vs[sl] ? vs[sl] : o;
                    vs[sl] = lower == asc ? mn : mxv;
                }
            }
        }
}

// One row of the result: thread t of nt writes winner i = t, t + nt, ... (key_at(i) = the i-th smallest key) as
// (list id + id_offset, distance); the rest of the out_stride slots are "no list" (fewer lists than requested).
template <typename KeyFn>
__device__ __forceinline__ void write_probe_row(uint32_t *__restrict__ out_cluster, float *__restrict__ out_dist, uint32_t b,
                                                uint32_t out_stride, uint32_t nprobe, uint32_t id_offset, uint32_t t, uint32_t nt,
                                                KeyFn key_at) {
    __builtin_assume(nt != 64u || nprobe <= 64u);  // a wave writes at most one winner per lane (the wave selections' nprobe <= 64)
    for (uint32_t i = t; i < nprobe; i += nt) {
        const unsigned long long key = key_at(i);
        out_cluster[(uint64_t)b * out_stride + i] = (uint32_t)key + id_offset;
        out_dist[(uint64_t)b * out_stride + i] = ord32_unbias((uint32_t)(key >> 32));
    }
    for (uint32_t i = nprobe + t; i < out_stride; i += nt) {
        out_cluster[(uint64_t)b * out_stride + i] = 0xFFFFFFFFu;
        out_dist[(uint64_t)b * out_stride + i] = __builtin_inff();
    }
}

// The `want` (1 <= want <= min(n, 64)) smallest (key, list id + id_offset) of the row d[0 .. n), n <= 64 KPL, one wave: lane l
// returns the l-th smallest (~0 from lane `want` on).  The row lives in registers, the winners are compacted by ballot into `win`
// (64 u64 of LDS owned by the calling wave) and sorted across the lanes.  No LDS atomics, no block barriers.
template <int KPL>
__device__ __forceinline__ unsigned long long select_row_wave(const float *__restrict__ d, uint32_t n, uint32_t want, bool vec4,
                                                              uint32_t id_offset, unsigned long long *win) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t key[KPL], kmin, kmax, T, J;
    row_keys<KPL>(d, n, vec4, key, kmin, kmax);
    bisect_exact<KPL>(key, n, want, kmin, kmax, T, J);
    uint32_t base = 0;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const uint32_t j = row_list_of(i, lane);
        const bool take = key[i] < T || (key[i] == T && j <= J && j < n);
        base = wave_compact(take, base, 0xFFFFFFFFu, [&](uint32_t at) { win[at] = ((unsigned long long)key[i] << 32) | (j + id_offset); });
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    unsigned long long v[1] = {lane < want ? win[lane] : ~0ull};
    wave_sort_u64<1>(v);
    return v[0];
}

// ------------------------------------------------------------------------------------------------
// Probe selection (src/rabitq.rs:294-297): the `nprobe` smallest (distance, cluster id) pairs in
// ascending order.  total_cmp order == Ord32 order; the composite u64 (biased Ord32 << 32 | id) is
// unique, so an 8-bit-per-pass radix select finds the nprobe-th key exactly, then the selected keys
// are bitonic-sorted in LDS.  Exactly-equal distances are ordered by cluster id (the reference's
// select_nth_unstable leaves that order unspecified).  One 256-thread block per query.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_probe_kernel(const float *__restrict__ dist, uint32_t k,
                                                           uint32_t nprobe,
                                                           uint32_t *__restrict__ out_cluster,
                                                           float *__restrict__ out_dist, uint32_t id_offset,
                                                           uint32_t out_stride, const uint32_t *__restrict__ only_rows = nullptr /* per row: 0 = skip */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint64_t *keys = reinterpret_cast<uint64_t *>(smem_raw);  // nprobe entries
    if (only_rows && only_rows[blockIdx.x] == 0u) return;
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_sel, s_want, s_done, s_cnt;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const float *d = dist + (uint64_t)b * k;

    uint64_t prefix = 0, mask = 0, T = ~0ull;
    uint32_t want = nprobe;  // rank (1-based) of the wanted key inside the current prefix group
    bool done = false;
    for (int pass = 7; pass >= 0 && !done; --pass) {
        const int shift = pass * 8;
        hist[tid] = 0;
        __syncthreads();
        for (uint32_t j = tid; j < k; j += 256) {
            uint64_t key = ((uint64_t)ord32_biased(d[j]) << 32) | j;
            if ((key & mask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {  // wave 0: locate the bin holding rank `want`
            uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            const uint32_t s = h0 + h1 + h2 + h3, incl = wave_incl_scan(s);
            uint32_t excl = incl - s;
            if (excl < want && want <= incl) {
                uint32_t r = want - excl, sel, cntbin;
                if (r <= h0) { sel = 0; cntbin = h0; }
                else if (r <= h0 + h1) { sel = 1; r -= h0; cntbin = h1; }
                else if (r <= h0 + h1 + h2) { sel = 2; r -= h0 + h1; cntbin = h2; }
                else { sel = 3; r -= h0 + h1 + h2; cntbin = h3; }
                s_sel = 4 * tid + sel;
                s_want = r;
                s_done = (cntbin == r) ? 1u : 0u;  // the whole bin is taken: lower bits don't matter
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s_sel << shift;
        mask |= 0xFFull << shift;
        want = s_want;
        if (s_done) {
            T = prefix | ~mask;
            done = true;
        }
        __syncthreads();
    }
    if (!done) T = prefix;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (uint32_t j = tid; j < k; j += 256) {
        uint64_t key = ((uint64_t)ord32_biased(d[j]) << 32) | j;
        if (key <= T) {
            uint32_t p = atomicAdd(&s_cnt, 1u);
            if (p < nprobe) keys[p] = key;
        }
    }
    __syncthreads();
    bitonic_sort_block(keys, nprobe, [](uint64_t v) { return v; });
    write_probe_row(out_cluster, out_dist, b, out_stride, nprobe, id_offset, tid, 256u, [&](uint32_t i) { return keys[i]; });
}

// The same selection with ONE WAVE per query, for nprobe <= 64 and k <= 64*KPL (select_row_wave over the whole row).
// `win`: 64 u64 of LDS owned by the calling wave.
template <int KPL>
__device__ __forceinline__ void select_probe_wave(const float *__restrict__ dist, uint32_t k, uint32_t nprobe,
                                                  uint32_t *__restrict__ out_cluster, float *__restrict__ out_dist,
                                                  uint32_t id_offset, uint32_t out_stride, uint32_t b,
                                                  unsigned long long *win) {
    const unsigned long long v = select_row_wave<KPL>(dist + (uint64_t)b * k, k, nprobe, (k & 3u) == 0u, 0u, win);
    write_probe_row(out_cluster, out_dist, b, out_stride, nprobe, id_offset, threadIdx.x & 63, 64u, [&](uint32_t) { return v; });
}
template <int KPL>
__global__ __launch_bounds__(256) void select_probe_wave_kernel(const float *__restrict__ dist, uint32_t k,
                                                                uint32_t nprobe, uint32_t *__restrict__ out_cluster,
                                                                float *__restrict__ out_dist, uint32_t id_offset,
                                                                uint32_t out_stride, uint32_t nq) {
    __shared__ unsigned long long win[4][64];
    const uint32_t wave = threadIdx.x >> 6, b = blockIdx.x * 4 + wave;
    if (b >= nq) return;
    select_probe_wave<KPL>(dist, k, nprobe, out_cluster, out_dist, id_offset, out_stride, b, win[wave]);
}

// ------------------------------------------------------------------------------------------------
// The matrix-core pre-filter (nearest list of the build: assign_approx_kernel, kernels_build.h; coarse ranking: coarse_approx_kernel
// below).  Every (vector x, centroid c) distance is first APPROXIMATED as (|c|^2 + |x|^2) - 2 <c~, x~> with the inner products from
// v_mfma_f32_32x32x16_bf16 (operands rounded to bf16, f32 accumulation: 16x the f32 MFMA rate), which is within
//     m_x = (2^-8 + (2 dim + 64) 2^-24) 1.05 (Cmax + |x|)^2
// of the reference's f32 value e_j (src/simd.rs:14-73).  bf16 keeps 8 significant bits: round-to-nearest is 2^-8 relative per
// operand, so |<x,c> - <x~,c~>| <= (2^-7 + 2^-16) |x||c|, the term -2<x,c> of the distance is off by at most
// (2^-6 + 2^-15) |x||c| <= (2^-8 + 2^-17) (|x|+|c|)^2   (|x||c| <= (|x|+|c|)^2 / 4): the first term of m_x, with its 2^-17
// tail inside the factor 1.05 -- that factor is LOAD-BEARING (it is the only slack over the bf16 bound: do not tighten it).
// The f32 accumulation of the 128-term products, the two norms (a dim-long f32 fma chain each) and the reference's own chain
// ((dim/8 + 5) 2^-24 relative) are all inside the second term; Cmax = the largest centroid norm.  So the exact minimiser j*
// (and every exact tie) has
//     a_{j*} <= e_{j*} + m <= e_j + m <= a_j + 2 m   for every j,   in particular   a_{j*} <= a_min + 2 m,
// and in the same way the nprobe smallest-a lists all have e <= a + m, so the nprobe-th smallest exact distance is <= tau + m
// (tau = any upper bound of the nprobe-th smallest a) and every list at or below it has a <= e + m <= tau + 2 m.
// prefilter_bound: `from` + 2 m_x, plus the rounding of the comparison itself (norm2 = |x|^2 from an f32 sum in any order: its
// rounding is inside the factors).  inf / NaN in, inf / NaN out.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float prefilter_bound(float from, float cmax, float norm2, uint32_t dim) {
    const float rad = cmax + sqrtf(norm2) * 1.000001f;
    const float mx = (0.00390625f + (float)(2 * dim + 64) * 5.9604645e-8f) * 1.05f * (rad * rad);
    const float thr = from + 2.0f * mx;
    return thr + fabsf(thr) * 1.0e-6f;  // the comparison's own rounding
}

// Centroid tiles of the pre-filter: 32 lists x DIM bf16 (pre-rounded once per build) streamed through two LDS images of
// TILEB + 128 bytes each (row stride ROWB = DIM * 2 + 16 bytes, then the 32 squared norms), by all 256 threads of the block:
// stage = global -> registers (issued before the MFMAs of the current tile), land = registers -> the other image (after them).
// Rows past the last list are zeros with the norm `pad_norm`.
typedef __bf16 asg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float asg_f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ uint32_t asg_bf16_pair(float lo, float hi) {  // two f32 -> packed bf16 (round to nearest even)
    uint32_t a = __builtin_bit_cast(uint32_t, lo), b = __builtin_bit_cast(uint32_t, hi);
    a += 0x7FFFu + ((a >> 16) & 1u);
    b += 0x7FFFu + ((b >> 16) & 1u);
    return (a >> 16) | (b & 0xFFFF0000u);
}
template <int W>
struct CentTile {
    static constexpr int DIM = 64 * W;
    static constexpr uint32_t ROWB = DIM * 2 + 16, TILEB = 32 * ROWB;
    static constexpr uint32_t PIECES = 32 * DIM * 2 / 16, NREG = (PIECES + 255) / 256;  // 16-byte pieces of a tile; per thread
    uint4 regs[NREG];
    float cn;
    __device__ __forceinline__ void stage(const uint16_t *__restrict__ cent_bf, const float *__restrict__ cnorm, uint32_t k, uint32_t tile,
                                          float pad_norm) {
        const uint32_t t = threadIdx.x;
#pragma unroll
        for (uint32_t i = 0; i < NREG; ++i) {
            const uint32_t pc = t + 256 * i, row = pc / (DIM / 8), within = pc - row * (DIM / 8);
            const uint32_t j = 32 * tile + row;
            regs[i] = make_uint4(0u, 0u, 0u, 0u);
            if (pc < PIECES && j < k) regs[i] = *reinterpret_cast<const uint4 *>(cent_bf + (uint64_t)j * DIM + 8 * within);
        }
        cn = pad_norm;
        if (t < 32 && 32 * tile + t < k) cn = cnorm[32 * tile + t];
    }
    __device__ __forceinline__ void land(unsigned char *lds, uint32_t buf) const {
        const uint32_t t = threadIdx.x;
        unsigned char *img = image(lds, buf);
#pragma unroll
        for (uint32_t i = 0; i < NREG; ++i) {
            const uint32_t pc = t + 256 * i, row = pc / (DIM / 8), within = pc - row * (DIM / 8);
            if (pc < PIECES) *reinterpret_cast<uint4 *>(img + row * ROWB + 16 * within) = regs[i];
        }
        if (t < 32) reinterpret_cast<float *>(img + TILEB)[t] = cn;
    }
    static __device__ __forceinline__ unsigned char *image(unsigned char *lds, uint32_t buf) { return lds + buf * (TILEB + 128); }
};

// ------------------------------------------------------------------------------------------------
// Probe selection behind the pre-filter: `dist` holds APPROXIMATE values a'_j = |c_j|^2 - 2 <c~_j, y~> (coarse_approx_kernel), each
// within m_y of e_j - |y|^2 (e_j = the reference's exact-order f32 distance).  One wave per query:
//   1. tau = an upper bound of the nprobe-th smallest a' of the row (bisect_loose);
//   2. candidates = the lists with a' <= tau + 2 m_y: the true nprobe nearest -- and every exact tie with the nprobe-th -- are among
//      them (prefilter_bound has the argument); typically nprobe + a few dozen;
//   3. their EXACT distances in the reference's lane order (src/simd.rs:14-73: 8 GPU lanes = the 8 AVX lanes of one list, folded by
//      reduce8_lanes), 8 lists per wave step;
//   4. the nprobe smallest (distance, list id) keys of the candidates, ascending: exactly what select_probe_wave returns from a row of
//      exact distances.
// A row with more than RQ_COARSE_CAND candidates (near-equidistant centroids) or a margin that is not finite (NaN / inf input) is
// ranked the plain way instead: the wave recomputes ALL k distances in exact order into the row (coarse_exact_row) and the exact
// selection runs on it.
// ------------------------------------------------------------------------------------------------
#define RQ_COARSE_CAND 256u
// exact-order distance (src/simd.rs:14-73) of four lists per 8-lane group to the query row yr: lane al of a group carries AVX
// lane al; all 8 lanes of the group return the folded sum.  dim is a multiple of 64: eight AVX steps at a time, all the loads
// of a chunk in flight before the first is used (one load per step, as a plain loop compiles to, made the caller a chain of
// 256 dependent L2 round trips per query).
__device__ __forceinline__ void coarse_exact_dist4(const float *__restrict__ centroids, const float *__restrict__ yr, uint32_t dim,
                                                   uint32_t al, const uint32_t (&jj)[4], float (&ee)[4]) {
    const float *cp[4];
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < 4; ++q) cp[q] = centroids + (uint64_t)jj[q] * dim + al;
    for (uint32_t e0 = 0; e0 < dim; e0 += 64) {
        float vv[4][8], yv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            yv[i] = yr[e0 + 8 * i + al];
#pragma unroll
            for (int q = 0; q < 4; ++q) vv[q][i] = cp[q][e0 + 8 * i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float df = vv[q][i] - yv[i];
                acc[q] = fmaf(df, df, acc[q]);
            }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) ee[q] = reduce8_lanes(acc[q]);
}

// the plain way, for a row the pre-filter cannot handle: all k distances of the row d in exact order, by one wave (32 lists per
// step).  The caller orders these stores before whatever reads the row back.
__device__ __forceinline__ void coarse_exact_row(const float *__restrict__ centroids, const float *__restrict__ yr, uint32_t dim, uint32_t k,
                                                 float *__restrict__ d) {
    const uint32_t lane = threadIdx.x & 63, grp = lane >> 3, al = lane & 7;  // 8 lanes per list: AVX lane al of list slot grp
    for (uint32_t j0 = 0; j0 < k; j0 += 32) {
        uint32_t jj[4];
        float ee[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) jj[q] = j0 + 8 * q + grp < k ? j0 + 8 * q + grp : 0u;
        coarse_exact_dist4(centroids, yr, dim, al, jj, ee);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (j0 + 8 * q + grp < k && al == 0) d[j0 + 8 * q + grp] = ee[q];
    }
}

// The candidate lists wn[0 .. c2) (list ids; c2 <= RQ_COARSE_CAND, >= nprobe) of query row b: exact keys in the reference's lane
// order, sort of the RQ_COARSE_CAND slots across the wave, the nprobe smallest written out in ascending order.
__device__ __forceinline__ void coarse_refine_tail(unsigned long long *wn, uint32_t c2, const float *__restrict__ centroids,
                                                   const float *__restrict__ yr, uint32_t dim, uint32_t nprobe, uint32_t b,
                                                   uint32_t *__restrict__ out_cluster, float *__restrict__ out_dist, uint32_t out_stride) {
    const uint32_t lane = threadIdx.x & 63, grp = lane >> 3, al = lane & 7;
    // exact keys, 32 candidates per step
    for (uint32_t c0 = 0; c0 < c2; c0 += 32) {
        uint32_t jj[4];
        float ee[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) jj[q] = c0 + 8 * q + grp < c2 ? (uint32_t)wn[c0 + 8 * q + grp] : 0u;
        coarse_exact_dist4(centroids, yr, dim, al, jj, ee);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (c0 + 8 * q + grp < c2 && al == 0) wn[c0 + 8 * q + grp] = ((unsigned long long)ord32_biased(ee[q]) << 32) | jj[q];
    }
    for (uint32_t i = c2 + lane; i < RQ_COARSE_CAND; i += 64) wn[i] = ~0ull;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    constexpr int NS = RQ_COARSE_CAND / 64;
    unsigned long long vs[NS];
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) vs[sl] = wn[lane + 64 * sl];
    wave_sort_u64<NS>(vs);
    const unsigned long long v0 = vs[0];  // of lane l = the l-th smallest key
    write_probe_row(out_cluster, out_dist, b, out_stride, nprobe, 0u, lane, 64u, [&](uint32_t) { return v0; });
}

// the biased key of prefilter_bound(tau) for the query row yr (0xFFFFFFFF: not finite)
__device__ __forceinline__ uint32_t coarse_margin_key(const float *__restrict__ yr, uint32_t dim, float cmax, float tau) {
    const uint32_t lane = threadIdx.x & 63;
    float yn = 0.0f;  // |y|^2
    for (uint32_t e = lane; e < dim; e += 64) yn = fmaf(yr[e], yr[e], yn);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) yn += __shfl_xor(yn, o, 64);
    const float thr2 = prefilter_bound(tau, cmax, yn, dim);
    const bool fin = fabsf(thr2) < 3.0e38f && fabsf(tau) < 3.0e38f;  // false for NaN / inf
    return fin ? ord32_biased(thr2) : 0xFFFFFFFFu;
}

template <int KPL>
__global__ __launch_bounds__(256) void select_refine_wave_kernel(float *__restrict__ dist, const float *__restrict__ y,
                                                                 const float *__restrict__ centroids, float cmax, uint32_t k, uint32_t dim,
                                                                 uint32_t nprobe, uint32_t *__restrict__ out_cluster,
                                                                 float *__restrict__ out_dist, uint32_t out_stride, uint32_t nq,
                                                                 unsigned long long *__restrict__ fallback_rows /* counter, may be null */) {
    __shared__ unsigned long long win[4][RQ_COARSE_CAND];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.x * 4 + wave;
    if (b >= nq) return;
    unsigned long long *wn = win[wave];
    float *d = dist + (uint64_t)b * k;
    const float *yr = y + (uint64_t)b * dim;
    uint32_t key[KPL], kmin, kmax;
    row_keys<KPL>(d, k, (k & 3u) == 0u, key, kmin, kmax);
    const uint32_t hi = bisect_loose(kmin, kmax, nprobe, [&](uint32_t t) { return count_le(key, t); });
    const uint32_t T2 = coarse_margin_key(yr, dim, cmax, ord32_unbias(hi));
    const bool fin = T2 != 0xFFFFFFFFu;
    const uint32_t c2 = fin ? count_le(key, T2) : 0xFFFFFFFFu;
    if (!(c2 <= RQ_COARSE_CAND) || c2 < nprobe) {  // (wave-uniform) the plain way, then the exact selection
        coarse_exact_row(centroids, yr, dim, k, d);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's own stores: read back below by other lanes of the wave
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (fallback_rows && lane == 0) atomicAdd(fallback_rows, 1ull);
        select_probe_wave<KPL>(dist, k, nprobe, out_cluster, out_dist, 0u, out_stride, b, wn);
        return;
    }
    // candidate ids into LDS (low half of the slots), in register order
    uint32_t base = 0;
#pragma unroll
    for (int i = 0; i < KPL; ++i)
        base = wave_compact(key[i] <= T2, base, 0xFFFFFFFFu, [&](uint32_t at) { wn[at] = row_list_of(i, lane); });
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    coarse_refine_tail(wn, c2, centroids, yr, dim, nprobe, b, out_cluster, out_dist, out_stride);
}

// The same for MORE lists than a wave can hold in registers (k > 8192: the probe ranking of a multi-GPU deployment is over the
// lists of ALL shards -- 32 768 at eight GPUs).  One sweep over the row of approximate distances leaves the minimum of every
// TILE of 32 consecutive lists (k / 32 keys: 16 per lane at k = 32 768).  The nprobe-th smallest tile minimum bounds the row's
// nprobe-th smallest a' from above (those nprobe minima are nprobe different lists), and tightly: the nearest lists of a query
// rarely share a tile.  Only the tiles whose minimum is within the margin are read again for the candidates (a few dozen
// 128-byte pieces instead of the row).  A row that cannot be handled (more than RQ_COARSE_CAND candidates, a margin that is not
// finite) gets all its distances in exact order and its flag set: select_probe_kernel then selects those rows (redo_flag).
// dynamic LDS: 4 x 64 TPL dwords (tile keys, then the flagged tiles, per wave)
// (waves per SIMD stated: up to 16 tile keys per lane the kernel sits at the 96-register step between five waves and four, and the
// allocator lands on either side of it from one spelling of the same code to the next)
template <int TPL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TPL <= 16 ? 5 : 4))) void select_refine_tiled_kernel(float *__restrict__ dist, const float *__restrict__ y,
                                                                  const float *__restrict__ centroids, float cmax, uint32_t k, uint32_t dim,
                                                                  uint32_t nprobe, uint32_t *__restrict__ out_cluster,
                                                                  float *__restrict__ out_dist, uint32_t out_stride, uint32_t nq,
                                                                  uint32_t *__restrict__ redo_flag,
                                                                  unsigned long long *__restrict__ fallback_rows /* counter, may be null */) {
    __shared__ unsigned long long win[4][RQ_COARSE_CAND];
    extern __shared__ __attribute__((aligned(16))) uint32_t tile_lds[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.x * 4 + wave;
    if (b >= nq) return;
    unsigned long long *wn = win[wave];
    uint32_t *tkeys = tile_lds + wave * (64 * TPL);
    float *d = dist + (uint64_t)b * k;
    const float *yr = y + (uint64_t)b * dim;
    const uint32_t grp = lane >> 3, al = lane & 7;
    const uint32_t ntile = (k + 31) / 32;  // <= 64 TPL (host)
    const bool vec4 = (k & 3u) == 0u;
    // sweep: 32 tiles (1024 lists) per step -- four 16-byte loads in flight per lane --, 4 lists per lane and load, the 8 lanes of
    // a group fold one tile
    for (uint32_t t0 = 0; t0 < ntile; t0 += 32) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = row_load4(d, (t0 + 8 * u) * 32 + lane * 4, k, vec4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t j0 = (t0 + 8 * u) * 32 + lane * 4;
            const float ve[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t key = j0 + e < k ? ord32_biased(ve[e]) : 0xFFFFFFFFu;
                mn = key < mn ? key : mn;
            }
#pragma unroll
            for (int o = 4; o >= 1; o >>= 1) {
                const uint32_t a = __shfl_xor(mn, o, 8);
                mn = a < mn ? a : mn;
            }
            if (al == 0 && t0 + 8 * u + grp < 64 * TPL) tkeys[t0 + 8 * u + grp] = mn;  // (tiles past the last one come out as "no list")
        }
    }
    for (uint32_t i = ((ntile + 31) & ~31u) + lane; i < 64 * TPL; i += 64) tkeys[i] = 0xFFFFFFFFu;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    uint32_t tk[TPL];  // tile lane + 64 i
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int i = 0; i < TPL; ++i) {
        tk[i] = tkeys[lane + 64 * i];
        if (lane + 64 * i < ntile) {
            kmin = tk[i] < kmin ? tk[i] : kmin;
            kmax = tk[i] > kmax ? tk[i] : kmax;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t a = __shfl_xor(kmin, o, 64), c = __shfl_xor(kmax, o, 64);
        kmin = a < kmin ? a : kmin;
        kmax = c > kmax ? c : kmax;
    }
    kmin = __builtin_amdgcn_readfirstlane(kmin), kmax = __builtin_amdgcn_readfirstlane(kmax);
    // tiles past the last one are masked by index, not by their "no list" key: a threshold of 0xFFFFFFFF must not count them
    auto tile_live = [&](int i, uint32_t t) { return tk[i] <= t && lane + 64 * i < ntile; };
    const uint32_t hi = bisect_loose(kmin, kmax, nprobe, [&](uint32_t t) {  // (ntile >= nprobe: the count at kmax = ntile >= nprobe)
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < TPL; ++i) c += (uint32_t)__popcll(__ballot(tile_live(i, t)));
        return c;
    });
    // every lane has its tile keys in registers by now: the LDS copy becomes the list of flagged tiles
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    // the lists with a' <= T (key << 32 | list id into the candidate slots): only tiles whose minimum is <= T are read again.
    // false: more than RQ_COARSE_CAND of them
    uint32_t base = 0;
    auto collect = [&](uint32_t T) -> bool {
        uint32_t nf = 0;
#pragma unroll
        for (int i = 0; i < TPL; ++i) nf = wave_compact(tile_live(i, T), nf, 0xFFFFFFFFu, [&](uint32_t at) { tkeys[at] = lane + 64 * i; });
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        base = 0;
        constexpr int CU_ = RQ_COLLECT_UNROLL;
        // 2 CU_ flagged tiles per step (one per half-wave, CU_ loads in flight per lane: one at a time the loop was a chain of ~50
        // dependent L2 round trips per query)
        for (uint32_t s0 = 0; base <= RQ_COARSE_CAND && s0 < nf; s0 += 2 * CU_) {
            uint32_t jv[CU_];
            float dv[CU_];
#pragma unroll
            for (int u = 0; u < CU_; ++u) {
                const uint32_t ti = s0 + 2 * u + (lane >> 5);
                jv[u] = ti < nf ? tkeys[ti] * 32 + (lane & 31) : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int u = 0; u < CU_; ++u) dv[u] = jv[u] < k ? d[jv[u]] : 0.0f;
#pragma unroll
            for (int u = 0; u < CU_; ++u) {
                const uint32_t key = ord32_biased(dv[u]);
                base = wave_compact(jv[u] < k && key <= T, base, RQ_COARSE_CAND, [&](uint32_t at) { wn[at] = ((unsigned long long)key << 32) | jv[u]; });
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        return base <= RQ_COARSE_CAND;  // (a step past the limit stores nothing and still advances base)
    };
    // first with the bound the tile minima give (tight when the nearest lists sit in different tiles)
    uint32_t T2 = ntile >= nprobe ? coarse_margin_key(yr, dim, cmax, ord32_unbias(hi)) : 0xFFFFFFFFu;
    bool ok = T2 != 0xFFFFFFFFu;
    if (ok && !collect(T2)) {
        // too many lists within the margin of that bound (wide margins: high dimensions): the row's nprobe-th smallest a' itself --
        // every list at or below the tile bound `hi` is collected (there are at least nprobe), bisection over those keys as the
        // single-wave kernel does over the row -- and the margin from there
        ok = collect(hi);
        if (ok) {
            uint32_t kk[RQ_COARSE_CAND / 64];
#pragma unroll
            for (int i = 0; i < (int)(RQ_COARSE_CAND / 64); ++i) kk[i] = lane + 64 * i < base ? (uint32_t)(wn[lane + 64 * i] >> 32) : 0xFFFFFFFFu;
            const uint32_t h2 = bisect_loose(kmin, hi, nprobe, [&](uint32_t t) { return count_le(kk, t); });
            T2 = coarse_margin_key(yr, dim, cmax, ord32_unbias(h2));
            ok = T2 != 0xFFFFFFFFu && collect(T2);
        }
    }
    if (!ok || base < nprobe) {  // (wave-uniform) the plain way; the block-per-query selection takes the row
        coarse_exact_row(centroids, yr, dim, k, d);
        if (lane == 0) {
            redo_flag[b] = 1u;
            if (fallback_rows) atomicAdd(fallback_rows, 1ull);
        }
        return;
    }
    if (lane == 0) redo_flag[b] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    coarse_refine_tail(wn, base, centroids, yr, dim, nprobe, b, out_cluster, out_dist, out_stride);
}

// ------------------------------------------------------------------------------------------------
// Coarse ranking through the pre-filter (src/rabitq.rs:283-297: all k exact-order distances, select the nprobe smallest, sort
// them).  coarse_approx_kernel writes, for every query, a'_j = |c_j|^2 - 2 <c~_j, y~> (the approximation of prefilter_bound minus the
// query's own |y|^2, a constant of the row) for every list; select_refine_wave_kernel / select_refine_tiled_kernel take it from there.
// Roles are swapped against assign_approx_kernel (queries = A rows, lists = B columns), so that a wave's stores are 128-byte
// runs of one query's row.
// ------------------------------------------------------------------------------------------------
template <int W, int NT>
__global__ __launch_bounds__(256, (W <= 4 ? 2 : 1)) void coarse_approx_kernel(const float *__restrict__ y /* nq x dim, rotated queries */,
                                                              const uint16_t *__restrict__ cent_bf /* k x dim bf16 */,
                                                              const float *__restrict__ cnorm, uint32_t nq, uint32_t k,
                                                              float *__restrict__ dist /* nq x k */,
                                                              const uint16_t *__restrict__ y_bf /* nq x dim bf16 (to_bf16_kernel of y), or null */) {
    constexpr int DIM = 64 * W, NM = DIM / 16;
    constexpr uint32_t ROWB = CentTile<W>::ROWB, TILEB = CentTile<W>::TILEB;
    extern __shared__ __attribute__((aligned(16))) unsigned char asg_lds[];  // the two images of CentTile<W>
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, kh = lane >> 5;
    const uint32_t v0 = (blockIdx.x * 4 + wave) * (32 * NT);
    asg_bf16x8 afrag[NT][NM];  // k-elements 16 m + 8 kh .. + 7 of query v0 + 32 tile + col
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        const uint32_t v = v0 + 32 * tl + col;
        const uint64_t vr = v < nq ? v : (nq - 1);
        if constexpr (NM > 32) {
            // dim > 512: the fragments come pre-rounded (to_bf16_kernel over the query rows, the rounding of asg_bf16_pair), one 16-byte
            // load per slab straight into its place.  Converted here, the f32 loads of all dim / 16 slabs were in flight beside the
            // fragments (384 + 192 registers at dim 768): 142 registers went to scratch memory in round 4 -- the only kernel of the
            // query path that needed any, and a dispatch that needs more scratch than the queue holds is set up and torn down around
            // the launch by the runtime (the 20 ms that appeared BETWEEN launches behind this kernel)
            const uint16_t *xb = y_bf + vr * DIM + 8 * kh;
#pragma unroll
            for (int m = 0; m < NM; ++m) afrag[tl][m] = __builtin_bit_cast(asg_bf16x8, *reinterpret_cast<const uint4 *>(xb + 16 * m));
        } else {
        const float *xp = y + vr * DIM + 8 * kh;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const float4 a = *reinterpret_cast<const float4 *>(xp + 16 * m), b = *reinterpret_cast<const float4 *>(xp + 16 * m + 4);
            const uint4 pk = make_uint4(asg_bf16_pair(a.x, a.y), asg_bf16_pair(a.z, a.w), asg_bf16_pair(b.x, b.y), asg_bf16_pair(b.z, b.w));
            afrag[tl][m] = __builtin_bit_cast(asg_bf16x8, pk);
        }
        }
    }
    const uint32_t ntile = (k + 31) / 32;
    CentTile<W> next;
    next.stage(cent_bf, cnorm, k, 0, 0.0f);
    next.land(asg_lds, 0);
    for (uint32_t tile = 0; tile < ntile; ++tile) {
        __syncthreads();  // tile `tile` is in LDS; the other buffer is free
        if (tile + 1 < ntile) next.stage(cent_bf, cnorm, k, tile + 1, 0.0f);
        const unsigned char *img = CentTile<W>::image(asg_lds, tile & 1u);
        const float cn = reinterpret_cast<const float *>(img + TILEB)[col];  // |c|^2 of this lane's list
        asg_f32x16 acc[NT];
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) acc[tl] = asg_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const asg_bf16x8 cf = *reinterpret_cast<const asg_bf16x8 *>(img + col * ROWB + (16 * m + 8 * kh) * 2);
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag[tl][m], cf, acc[tl], 0, 0, 0);
        }
        const uint32_t j = 32 * tile + col;
        if (j < k) {
#pragma unroll
            for (int tl = 0; tl < NT; ++tl)
#pragma unroll
                for (int r = 0; r < 16; ++r) {  // register r of lane half kh = query row (r & 3) + 8 (r >> 2) + 4 kh of the tile
                    const uint32_t v = v0 + 32 * tl + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
                    if (v < nq) dist[(uint64_t)v * k + j] = fmaf(-2.0f, acc[tl][r], cn);
                }
        }
        if (tile + 1 < ntile) next.land(asg_lds, (tile + 1) & 1u);
    }
}

// ------------------------------------------------------------------------------------------------
// The pre-filter without the nq x k matrix (4096 <= k <= 8192, dim <= 256): coarse_candidates_kernel runs the matrix-core pass TWICE
// and stores only what the refinement needs, refine_candidates_kernel is the tail of select_refine_tiled_kernel.
// Orientation of assign_approx_kernel (lists = MFMA rows, queries = columns): a lane owns ONE query (column `col`, shared by the two
// half-waves) and its 16 accumulator registers are 16 of a tile's 32 lists, so everything per query is lane-private.
//   sweep 1: a'_j = |c_j|^2 - 2 <c~_j, y~> as in coarse_approx_kernel; the minimum of every 32-list tile, as a key, into LDS
//            ([tile][query]: the 32 lanes of a half-wave read 32 consecutive words);
//   between: per lane, tau = any bound with at least nprobe tile keys at or below it (the rule of bisect_loose; the half-waves count
//            the even and the odd tiles), T2 = prefilter_bound(tau, ...): the threshold select_refine_tiled_kernel's first collect uses;
//   sweep 2: the same MFMAs again (the same instruction sequence on the same operands: the values are sweep 1's, bit for bit); every
//            list with a' <= T2 is appended -- its id, 16 bits -- to the query's RQ_COARSE_CAND slots in LDS (over the tile keys, dead
//            by then: 32 queries x 256 x 2 bytes are the keys of 128 tiles, and k >= 4096).  The count keeps advancing past
//            RQ_COARSE_CAND, the stores stop.
//   after:   the slots of every row that fits go to the first RQ_COARSE_CAND words of the query's row of `dist` (nobody else's).
// cand_cnt[q] = the count, 0xFFFFFFFF where the margin is not finite.  Comparisons are on the f32 values (a superset of what the key
// comparison selects: -0 <= +0); NaN never compares true, and a NaN / inf row has no finite margin in the first place.
// Rows past the last list are zeros with the norm RQ_COARSE_PAD_NORM: finite (no inf - inf), above every finite T2 (|T2| < 3.0e38
// is what "finite" means below) and, should it ever be a tile's minimum, a tau that is not "finite" either; the last tile's are
// masked by index as well.
// dynamic LDS: the two images of CentTile<W>, then 4 waves x NT x ntile x 32 tile keys (coarse_candidates_lds_bytes, host_launch.h).
// ------------------------------------------------------------------------------------------------
#define RQ_COARSE_PAD_NORM 3.0e38f
// the bisection stops at any bound that selects nprobe .. nprobe + RQ_FUSED_WINDOW tile keys: narrower than bisect_loose's 12, because
// a step costs this kernel ntile / 2 LDS reads per lane (a few per cent of a sweep) while every spare candidate is a store here and an
// exact distance in refine_candidates_kernel, and a row past the slots has no second collect to fall back on
#define RQ_FUSED_WINDOW 4u
template <int W, int NT>
__global__ __launch_bounds__(256) void coarse_candidates_kernel(const float *__restrict__ y /* nq x dim, rotated queries */,
                                                                const uint16_t *__restrict__ cent_bf /* k x dim bf16 */,
                                                                const float *__restrict__ cnorm, float cmax, uint32_t nq, uint32_t k,
                                                                uint32_t nprobe, float *__restrict__ dist /* nq x k: candidate slots */,
                                                                uint32_t *__restrict__ cand_cnt /* nq */) {
    constexpr int DIM = 64 * W, NM = DIM / 16;
    constexpr uint32_t ROWB = CentTile<W>::ROWB, TILEB = CentTile<W>::TILEB;
    extern __shared__ __attribute__((aligned(16))) unsigned char asg_lds[];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, kh = lane >> 5;
    const uint32_t ntile = (k + 31) / 32;  // >= nprobe (host)
    uint32_t *tkeys = reinterpret_cast<uint32_t *>(asg_lds + 2 * (TILEB + 128)) + wave * (NT * 32) * ntile;  // [tl][tile][col]
    const uint32_t v0 = (blockIdx.x * 4 + wave) * (32 * NT);
    asg_bf16x8 bfrag[NT][NM];  // k-elements 16 m + 8 kh .. + 7 of query v0 + 32 tl + col
    float yn[NT];              // |y|^2
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        const uint32_t v = v0 + 32 * tl + col;
        const float *xp = y + (uint64_t)(v < nq ? v : (nq - 1)) * DIM + 8 * kh;
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const float4 a = *reinterpret_cast<const float4 *>(xp + 16 * m), b = *reinterpret_cast<const float4 *>(xp + 16 * m + 4);
            s0 = fmaf(a.x, a.x, s0), s1 = fmaf(a.y, a.y, s1), s0 = fmaf(a.z, a.z, s0), s1 = fmaf(a.w, a.w, s1);
            s0 = fmaf(b.x, b.x, s0), s1 = fmaf(b.y, b.y, s1), s0 = fmaf(b.z, b.z, s0), s1 = fmaf(b.w, b.w, s1);
            const uint4 pk = make_uint4(asg_bf16_pair(a.x, a.y), asg_bf16_pair(a.z, a.w), asg_bf16_pair(b.x, b.y), asg_bf16_pair(b.z, b.w));
            bfrag[tl][m] = __builtin_bit_cast(asg_bf16x8, pk);
        }
        const float s = s0 + s1;
        yn[tl] = s + __shfl_xor(s, 32, 64);  // both halves of the row
    }
    float thr[NT];        // T2 (sweep 2)
    bool fin[NT];         // the margin is finite
    uint32_t kmin[NT], kmax[NT], cnt[NT];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) thr[tl] = 0.0f, fin[tl] = false, kmin[tl] = 0xFFFFFFFFu, kmax[tl] = 0u, cnt[tl] = 0u;
    for (int pass = 0; pass < 2; ++pass) {
        CentTile<W> next;
        __syncthreads();  // the previous sweep's last tile has been consumed
        next.stage(cent_bf, cnorm, k, 0, RQ_COARSE_PAD_NORM);
        next.land(asg_lds, 0);
        for (uint32_t tile = 0; tile < ntile; ++tile) {
            __syncthreads();  // tile `tile` is in LDS; the other buffer is free
            if (tile + 1 < ntile) next.stage(cent_bf, cnorm, k, tile + 1, RQ_COARSE_PAD_NORM);
            const unsigned char *img = CentTile<W>::image(asg_lds, tile & 1u);
            const float *cnp = reinterpret_cast<const float *>(img + TILEB);
            asg_f32x16 acc[NT];
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) acc[tl] = asg_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const asg_bf16x8 af = *reinterpret_cast<const asg_bf16x8 *>(img + col * ROWB + (16 * m + 8 * kh) * 2);
#pragma unroll
                for (int tl = 0; tl < NT; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfrag[tl][m], acc[tl], 0, 0, 0);
            }
            float cnr[16];  // |c|^2 of this lane's 16 lists: list = 32 tile + (r & 3) + 8 (r >> 2) + 4 kh
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 c4 = *reinterpret_cast<const float4 *>(cnp + 8 * g + 4 * kh);
                cnr[4 * g] = c4.x, cnr[4 * g + 1] = c4.y, cnr[4 * g + 2] = c4.z, cnr[4 * g + 3] = c4.w;
            }
            const bool ragged = 32 * tile + 32 > k;  // (uniform) the last tile, with rows past the last list
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) {
                if (pass == 0) {
                    float mn = __builtin_inff();
#pragma unroll
                    for (int r = 0; r < 16; ++r) mn = fminf(mn, fmaf(-2.0f, acc[tl][r], cnr[r]));
                    mn = fminf(mn, __shfl_xor(mn, 32, 64));  // the other 16 lists of the tile
                    const uint32_t key = ord32_biased(mn);
                    kmin[tl] = key < kmin[tl] ? key : kmin[tl];
                    kmax[tl] = key > kmax[tl] ? key : kmax[tl];
                    if (kh == 0) tkeys[(tl * ntile + tile) * 32 + col] = key;
                } else {
                    uint32_t mine = 0;
#pragma unroll
                    for (int r = 0; r < 16; ++r) mine |= fmaf(-2.0f, acc[tl][r], cnr[r]) <= thr[tl] ? (1u << r) : 0u;
                    if (ragged) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (32 * tile + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh >= k) mine &= ~(1u << r);
                    }
                    if (!fin[tl]) mine = 0;
                    const uint32_t other = (uint32_t)__shfl_xor((int)mine, 32, 64);
                    const uint32_t c_mine = (uint32_t)__popc(mine), c_other = (uint32_t)__popc(other);
                    uint32_t at = cnt[tl] + (kh ? c_other : 0u);  // the lower half-wave's lists first
                    cnt[tl] += c_mine + c_other;
                    // staged in LDS, over the tile keys (dead by now): a store to global memory here would have every tile's
                    // `land` wait for it, since loads and stores share one counter
                    uint16_t *cand = reinterpret_cast<uint16_t *>(tkeys + tl * ntile * 32) + col * RQ_COARSE_CAND;
                    while (mine) {
                        const uint32_t r = (uint32_t)__builtin_ctz(mine);
                        mine &= mine - 1u;
                        if (at < RQ_COARSE_CAND) cand[at] = (uint16_t)(32 * tile + (r & 3u) + 8u * (r >> 2) + 4u * kh);
                        ++at;
                    }
                }
            }
            if (tile + 1 < ntile) next.land(asg_lds, (tile + 1) & 1u);
        }
        if (pass == 0) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // this wave's tile keys: read back by both of its half-waves
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) {
                // bisect_loose per lane: the two half-waves of a query hold the same lo / hi and count the tiles of their parity
                const uint32_t *tk = tkeys + tl * ntile * 32 + col;
                uint32_t lo = kmin[tl], hi = kmax[tl];
                bool open = lo < hi;
                while (__ballot(open)) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    uint32_t c = 0;
#pragma unroll 16
                    for (uint32_t i = kh; i < ntile; i += 2) c += tk[i * 32] <= mid ? 1u : 0u;  // (16 reads in flight)
                    c += (uint32_t)__shfl_xor((int)c, 32, 64);
                    if (open) {
                        if (c >= nprobe) {
                            hi = mid;
                            if (c <= nprobe + RQ_FUSED_WINDOW) open = false;
                        } else {
                            lo = mid + 1;
                        }
                        open = open && lo < hi;
                    }
                }
                const float tau = ord32_unbias(hi);
                const float t2 = prefilter_bound(tau, cmax, yn[tl], DIM);
                fin[tl] = fabsf(t2) < 3.0e38f && fabsf(tau) < 3.0e38f;  // false for NaN / inf
                thr[tl] = t2;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the staged ids: written by the query's two lanes, read by the whole wave
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        const uint32_t v = v0 + 32 * tl + col;
        const uint32_t cval = fin[tl] ? cnt[tl] : 0xFFFFFFFFu;
        if (kh == 0 && v < nq) cand_cnt[v] = cval;
        // the ids of the rows that go on to the refinement, 256 bytes per wave store
        const uint16_t *cand = reinterpret_cast<const uint16_t *>(tkeys + tl * ntile * 32);
        for (uint32_t qi = 0; qi < 32; ++qi) {
            const uint32_t c = (uint32_t)__shfl((int)cval, (int)qi, 64), vq = v0 + 32 * tl + qi;  // (uniform)
            if (vq >= nq || c > RQ_COARSE_CAND) continue;
            uint32_t *slots = reinterpret_cast<uint32_t *>(dist + (uint64_t)vq * k);
            for (uint32_t s = lane; s < c; s += 64) slots[s] = cand[qi * RQ_COARSE_CAND + s];
        }
    }
}

// One wave per query behind coarse_candidates_kernel: the candidate ids from the row's slots, coarse_refine_tail.  A row with more
// than RQ_COARSE_CAND candidates, fewer than nprobe (none: the margin is never negative) or no finite margin is ranked the plain
// way, as select_refine_tiled_kernel's last branch does: all its distances in exact order, its flag set for select_probe_kernel.
// cnt_flag: in, the row's candidate count; out, its redo flag.
__global__ __launch_bounds__(256) void refine_candidates_kernel(float *__restrict__ dist, const float *__restrict__ y,
                                                                const float *__restrict__ centroids, uint32_t k, uint32_t dim, uint32_t nprobe,
                                                                uint32_t *__restrict__ out_cluster, float *__restrict__ out_dist,
                                                                uint32_t out_stride, uint32_t nq, uint32_t *__restrict__ cnt_flag,
                                                                unsigned long long *__restrict__ fallback_rows /* counter, may be null */) {
    __shared__ unsigned long long win[4][RQ_COARSE_CAND];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.x * 4 + wave;
    if (b >= nq) return;
    unsigned long long *wn = win[wave];
    float *d = dist + (uint64_t)b * k;
    const float *yr = y + (uint64_t)b * dim;
    const uint32_t c2 = __builtin_amdgcn_readfirstlane(cnt_flag[b]);
    if (c2 > RQ_COARSE_CAND || c2 < nprobe) {  // (wave-uniform) the plain way; the block-per-query selection takes the row
        coarse_exact_row(centroids, yr, dim, k, d);
        if (lane == 0) {
            cnt_flag[b] = 1u;
            if (fallback_rows) atomicAdd(fallback_rows, 1ull);
        }
        return;
    }
    const uint32_t *slots = reinterpret_cast<const uint32_t *>(d);
    for (uint32_t i = lane; i < c2; i += 64) wn[i] = slots[i];
    if (lane == 0) cnt_flag[b] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    coarse_refine_tail(wn, c2, centroids, yr, dim, nprobe, b, out_cluster, out_dist, out_stride);
}

// ------------------------------------------------------------------------------------------------
// Adaptive probing (rq_probe_rule_t): a query's probe row d_0 <= d_1 <= ... <= d_{m-1} is cut behind the longest prefix whose
// entries all satisfy d_j <= t, t = ratio * d_0 (one f32 multiplication; ratio = +inf: t = +inf, also where d_0 = 0); a NaN
// compares false.  n = min(cap, max(min_probe, prefix)) clamped to [1, m], cap = the query's entry of `caps` clamped to [1, m] (no
// array: m).  Slots n .. m-1 become (0xFFFFFFFF, +inf) = "no list", which every kernel behind the coarse ranking skips before any
// per-pair work; n goes to row_n and, if given, to out_n.
// One wave per query, 64 slots of the row per step: a ballot of the test, the first clear bit ends the prefix.
// ------------------------------------------------------------------------------------------------
struct ProbeRule {
    float ratio = 0.0f;
    uint32_t min_probe = 0;             // 0: no rule (every other field is ignored)
    const uint32_t *caps = nullptr;     // device, one entry per query of the pass; or null
    uint32_t *out_nprobe = nullptr;     // device, one entry per query of the pass; or null
    bool on() const { return min_probe != 0; }
};
__global__ __launch_bounds__(256) void probe_cut_kernel(uint32_t *__restrict__ probe_cluster, float *__restrict__ probe_dist, uint32_t m,
                                                        uint32_t nq, float ratio, uint32_t min_probe, const uint32_t *__restrict__ caps,
                                                        uint32_t *__restrict__ row_n, uint32_t *__restrict__ out_n) {
    const uint32_t lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nq || m == 0) return;  // (wave-uniform)
    uint32_t *pc = probe_cluster + (uint64_t)b * m;
    float *pd = probe_dist + (uint64_t)b * m;
    const float inf = __builtin_inff();
    const float t = ratio == inf ? inf : ratio * pd[0];
    uint32_t p = 0;
    for (uint32_t s0 = 0; s0 < m; s0 += 64) {
        const uint32_t s = s0 + lane, width = m - s0 < 64u ? m - s0 : 64u;
        const bool ok = s < m && pd[s] <= t;
        const unsigned long long have = width == 64u ? ~0ull : (1ull << width) - 1ull;
        const unsigned long long clear = ~__ballot(ok) & have;
        if (clear) {
            p += (uint32_t)__ffsll(clear) - 1u;
            break;
        }
        p += width;
    }
    uint32_t cap = m;
    if (caps) {
        const uint32_t c = caps[b];
        cap = c < 1u ? 1u : (c > m ? m : c);
    }
    uint32_t n = p > min_probe ? p : min_probe;
    n = n < cap ? n : cap;
    n = n < 1u ? 1u : (n > m ? m : n);
    for (uint32_t s = n + lane; s < m; s += 64) pc[s] = 0xFFFFFFFFu, pd[s] = inf;
    if (lane == 0) {
        row_n[b] = n;
        if (out_n) out_n[b] = n;
    }
}
