// kernels_range.h -- the tail of a range pass (rq_range_search*): everything behind the single scan stage and the exact
// distances.  A range query keeps EVERY candidate with rough < r_b and accurate < r_b (src/rerank.rs:83-92 with the threshold
// held at r_b and no bound on the number kept), so its answer is a set: no run directory, no replay, no heap.  What is left is
// making a variable-length result: hit counts, offsets (u64), keys written straight to their query's segment, a segmented
// sort binned by segment length, and the split of the sorted keys into the result's distance / id arrays.
//
// The exact distances themselves are the top-k path's kernels (kernels_rerank.h: accurate_kernel / accurate_filtered8_kernel /
// accurate_filtered_kernel / accurate_split_kernel, launched with the radii as thresholds): they write SurvRec::accurate in
// place -- +inf where a shadow row proves accurate >= r_b -- so the distance bits are the plain query's by construction.
#pragma once

// key of a hit: (Ord32 image of the exact distance, unsigned-sortable) << 32 | original id.  Ids are unique per query, so are
// the keys; ~0 never occurs (its distance word is a NaN's image, and a NaN fails accurate < r_b) and pads the sorts.
#define RQ_RANGE_PAD (~0ull)
#define RQ_RANGE_WAVE_MAX 64u      // segments sorted by one wave in registers
#define RQ_RANGE_SMALL_MAX 2048u   // ... by a 256-thread block in 16 KiB of LDS
#define RQ_RANGE_TILE 16384u       // ... by a 1024-thread block in 128 KiB of LDS; longer segments: tiles of this size + merge passes

__device__ __forceinline__ bool range_hit(const SurvRec &r, float radius) { return r.rough < radius && r.accurate < radius; }

// Hit counts.  One wave per query (four per block).  Also the per-query counters of the pass (metrics_sum_kernel folds them):
// need = survivors of the scan (exact even where the buffer overflowed), ovf, precise = nsurv = survivors of a query that did
// not overflow (an overflowed query counts in its re-run).
__global__ __launch_bounds__(256) void range_count_kernel(const SurvRec *__restrict__ surv, const unsigned long long *__restrict__ surv_cnt,
                                                          uint32_t cap, const float *__restrict__ radius, uint32_t nq,
                                                          uint32_t *__restrict__ hits, uint32_t *__restrict__ need, uint32_t *__restrict__ ovf,
                                                          uint32_t *__restrict__ precise, uint32_t *__restrict__ nsurv) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= nq) return;
    const uint32_t cnt = (uint32_t)surv_cnt[b];
    const bool over = cnt > cap;
    const uint32_t n = over ? 0u : cnt;
    const float r = radius[b];
    const SurvRec *recs = surv + (uint64_t)b * cap;
    uint32_t h = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        h += (uint32_t)__popcll(__ballot(i < n && range_hit(recs[i], r)));
    }
    if (lane == 0) hits[b] = h, need[b] = cnt, ovf[b] = over ? 1u : 0u, precise[b] = n, nsurv[b] = n;
}

// Exclusive prefix sum of n counts into n + 1 u64 offsets (lims[0] = 0, lims[n] = the total).  One block of 1024 threads, any n
// (n is a call's query count: 64 rounds for a full pass of 65 536 queries, microseconds; a call of many millions of queries
// would make this a serial tail of milliseconds beside passes that take seconds -- a multi-block scan is not worth it here).
template <typename T>
__global__ __launch_bounds__(1024) void range_scan_kernel(const T *__restrict__ cnt, uint32_t n, unsigned long long *__restrict__ lims) {
    const unsigned long long total = block_scan_chunked<unsigned long long, uint64_t>(  // (64-bit index: n may be within 1024 of 2^32)
        (uint64_t)n, [&](uint64_t i) { return cnt[i]; }, [&](uint64_t i, unsigned long long at, unsigned long long) { lims[i] = at; });
    if (threadIdx.x == 0) lims[n] = total;
}

// The hits' keys, written straight to the query's segment [lims[b], lims[b + 1]) in survivor order (ballot ranks: no atomics).
__global__ __launch_bounds__(256) void range_emit_kernel(const SurvRec *__restrict__ surv, const unsigned long long *__restrict__ surv_cnt,
                                                         uint32_t cap, const float *__restrict__ radius, uint32_t nq,
                                                         const uint32_t *__restrict__ map_ids, const unsigned long long *__restrict__ lims,
                                                         unsigned long long *__restrict__ keys) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= nq) return;
    const uint32_t cnt = (uint32_t)surv_cnt[b];
    if (cnt > cap) return;  // overflowed: answered by its re-run
    unsigned long long at = lims[b];
    const unsigned long long end = lims[b + 1];
    if (at == end) return;
    const float r = radius[b];
    const SurvRec *recs = surv + (uint64_t)b * cap;
    for (uint32_t i0 = 0; i0 < cnt; i0 += 64) {
        const uint32_t i = i0 + lane;
        SurvRec rec;
        bool hit = false;
        if (i < cnt) {
            rec = recs[i];
            hit = range_hit(rec, r);
        }
        const unsigned long long m = __ballot(hit);
        if (hit) {
            const unsigned long long o = at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (o < end) keys[o] = ((unsigned long long)ord32_biased(rec.accurate) << 32) | map_ids[rec.pos];
        }
        at += (uint32_t)__popcll(m);
    }
}

// A call of several runs (passes, overflow re-runs): run-local query j is query q0 + (rows ? rows[j] : j) of the call.
// Lengths of the runs' segments into the call's per-query counts (every query is answered by exactly one run; the others hold 0).
__global__ void range_piece_counts_kernel(const unsigned long long *__restrict__ plims, const uint32_t *__restrict__ rows, uint32_t q0,
                                          uint32_t m, unsigned long long *__restrict__ counts) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const unsigned long long len = plims[j + 1] - plims[j];
    if (len) counts[q0 + (rows ? rows[j] : j)] += len;
}
// ... and the runs' keys to their places in the call's key array (one wave per query)
__global__ __launch_bounds__(256) void range_piece_scatter_kernel(const unsigned long long *__restrict__ pkeys, const unsigned long long *__restrict__ plims,
                                                                  const uint32_t *__restrict__ rows, uint32_t q0, uint32_t m,
                                                                  const unsigned long long *__restrict__ lims, unsigned long long *__restrict__ keys) {
    const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= m) return;
    const unsigned long long lo = plims[j], len = plims[j + 1] - lo;
    if (!len) return;
    const unsigned long long dst = lims[q0 + (rows ? rows[j] : j)];
    for (unsigned long long e = lane; e < len; e += 64) keys[dst + e] = pkeys[lo + e];
}

// Segments by length: lists of the queries whose segment needs a block of its own -- [0, nq) up to RQ_RANGE_SMALL_MAX keys,
// [nq, 2 nq) up to RQ_RANGE_TILE, [2 nq, 3 nq) beyond -- counters: the three lists' lengths and the longest segment (clipped to u32
// launches by the host).  Segments of at most 64 keys need no list: range_sort_wave_kernel visits every query.
__global__ void range_bin_kernel(const unsigned long long *__restrict__ lims, uint32_t nq, uint32_t *__restrict__ lists,
                                 unsigned long long *__restrict__ counters /* [4], zeroed */) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nq) return;
    const unsigned long long n = lims[b + 1] - lims[b];
    if (n <= RQ_RANGE_WAVE_MAX) return;
    const uint32_t bin = n <= RQ_RANGE_SMALL_MAX ? 0u : (n <= RQ_RANGE_TILE ? 1u : 2u);
    lists[(uint64_t)bin * nq + (uint32_t)atomicAdd(&counters[bin], 1ull)] = b;
    if (bin == 2) atomicMax(&counters[3], n);
}

// Segments of 2 .. 64 keys: one wave each, one key per lane, bitonic network over the lanes.
__global__ __launch_bounds__(256) void range_sort_wave_kernel(unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ lims,
                                                              uint32_t nq) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= nq) return;
    const unsigned long long lo = lims[b], n = lims[b + 1] - lo;
    if (n < 2 || n > RQ_RANGE_WAVE_MAX) return;
    unsigned long long v = lane < n ? keys[lo + lane] : RQ_RANGE_PAD;
    for (uint32_t k = 2; k <= 64; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const unsigned long long o = __shfl_xor(v, (int)j, 64);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            v = keep_min ? (o < v ? o : v) : (o > v ? o : v);
        }
    if (lane < n) keys[lo + lane] = v;
}

// n <= KEYS keys at src, sorted through LDS (padded to a power of two), written to dst.  Whole block.
template <uint32_t THREADS>
__device__ __forceinline__ void range_sort_lds(unsigned long long *s, const unsigned long long *src, unsigned long long *dst, uint32_t n) {
    uint32_t p = 2;
    while (p < n) p <<= 1;
    for (uint32_t i = threadIdx.x; i < p; i += THREADS) s[i] = i < n ? src[i] : RQ_RANGE_PAD;
    __syncthreads();
    for (uint32_t k = 2; k <= p; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < p / 2; t += THREADS) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = s[i], c = s[l];
                if ((a > c) == ((i & k) == 0)) s[i] = c, s[l] = a;
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) dst[i] = s[i];
}
// One block per listed segment (dynamic LDS: KEYS * 8 bytes).
template <uint32_t THREADS, uint32_t KEYS>
__global__ __launch_bounds__(THREADS) void range_sort_block_kernel(unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ lims,
                                                                   const uint32_t *__restrict__ list, uint32_t nlist) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long range_lds[];
    if (blockIdx.x >= nlist) return;
    const uint32_t b = list[blockIdx.x];
    const unsigned long long lo = lims[b], n = lims[b + 1] - lo;
    if (n < 2 || n > KEYS) return;
    range_sort_lds<THREADS>(range_lds, keys + lo, keys + lo, (uint32_t)n);
}
// Segments beyond RQ_RANGE_TILE keys.  First their tiles of RQ_RANGE_TILE keys, each sorted in LDS (grid: tiles of the longest
// segment x listed segments) ...
__global__ __launch_bounds__(1024) void range_sort_tile_kernel(unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ lims,
                                                               const uint32_t *__restrict__ list, uint32_t nlist) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long range_lds[];
    if (blockIdx.y >= nlist) return;
    const uint32_t b = list[blockIdx.y];
    const unsigned long long lo = lims[b], n = lims[b + 1] - lo, first = (unsigned long long)blockIdx.x * RQ_RANGE_TILE;
    if (first >= n) return;
    const uint32_t m = (uint32_t)(n - first < RQ_RANGE_TILE ? n - first : RQ_RANGE_TILE);
    range_sort_lds<1024>(range_lds, keys + lo + first, keys + lo + first, m);
}
// ... then merge passes in global memory: sorted runs of `width` keys are merged pairwise from src into dst (same offsets), every
// key placed by its rank -- its index in its own run + the keys of the partner run below it (keys are unique: one bisection).
// A run without a partner is copied.  One thread per key; grid: keys of the longest segment / 256 x listed segments.
__global__ __launch_bounds__(256) void range_merge_kernel(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst,
                                                          const unsigned long long *__restrict__ lims, const uint32_t *__restrict__ list,
                                                          uint32_t nlist, unsigned long long width) {
    if (blockIdx.y >= nlist) return;
    const uint32_t b = list[blockIdx.y];
    const unsigned long long lo = lims[b], n = lims[b + 1] - lo;
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const unsigned long long run = e / width, pair_lo = (run >> 1) * 2 * width;
    const unsigned long long mid = pair_lo + width < n ? pair_lo + width : n, hi = pair_lo + 2 * width < n ? pair_lo + 2 * width : n;
    const unsigned long long key = src[lo + e];
    // the partner run: [mid, hi) for a key of the first run, [pair_lo, mid) for one of the second
    const bool second = (run & 1ull) != 0;
    unsigned long long l = second ? pair_lo : mid, h = second ? mid : hi;
    const unsigned long long part_lo = l;
    while (l < h) {  // first partner key above `key`
        const unsigned long long c = l + ((h - l) >> 1);
        if (src[lo + c] < key) l = c + 1;
        else h = c;
    }
    const unsigned long long own = e - (second ? mid : pair_lo);
    dst[lo + pair_lo + own + (l - part_lo)] = key;
}

// The sorted keys into the result's arrays.
__global__ void range_split_kernel(const unsigned long long *__restrict__ keys, unsigned long long total, float *__restrict__ dist,
                                   uint32_t *__restrict__ id) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        dist[i] = ord32_unbias((uint32_t)(key >> 32));
        id[i] = (uint32_t)key;
    }
}
