// kernels_postings_restrict.h -- the intersection of a postings object with a filter, as postings of its own
// (host_postings_restrict.h), wave64.  Nothing here writes an array of the index, of the postings or of the filter.
//
// The work is split over fixed chunks of RQ_PR_CHUNK = 2048 consecutive postings (segments differ in length by orders of magnitude:
// no pass is split over them).  A block of four waves owns a chunk; in round r wave w takes the chunk's word 4 r + w, 64 postings.
//   ADMIT    restrict_admit_kernel: per round one coalesced 64-lane load of positions (the eight loads of a wave are issued before
//            anything waits for them), every lane gathers its word of the filter's position bitmap, ONE ballot is one 64-bit word of
//            the admit bitmap over posting order (lanes past the end: 0); the popcounts go through LDS to the chunk's count.
//   SCAN     restrict_scan_kernel: the exclusive prefix of the chunk counts in place, and their total, by one looping block
//            (block_scan_chunked: 49k counts at 100M postings).
//   TAKE     restrict_take_kernel: the chunk's 32 admit words and their popcounts give every word's global rank (chunk prefix +
//            the earlier words of the chunk), written as rank64[w]; an admitted lane stores its position at that rank + the
//            ballot's bits below it -- posting order is preserved.  rank(i) = rank64[i >> 6] + popc(admit[i >> 6] & below(i & 63)).
//   SEGMENTS restrict_segments_kernel: one thread per segment of the source, 2048 segments a block in the same geometry: the new
//            bounds rank(starts[s]) and rank(starts[s + 1]); the segment is kept where they differ, and the kept flags are a bitmap
//            + chunk counts as above (the same routine).  After a second SCAN, restrict_segments_take_kernel stores the kept
//            segments' new starts and values at their ranks, and the last start = the admitted total.
// Vector loads and plain stores only; no atomic anywhere: the same inputs give the same arrays on every run.
#pragma once
#include "common.h"

#define RQ_PR_CHUNK 2048u  // items (postings, segments) of a block
#define RQ_PR_WORDS 32u    // 64-bit words of a chunk's bitmap

struct PostRestrictArgs {
    const uint32_t *post;               // the source postings: n positions
    const uint32_t *allow;              // the filter's position bitmap
    const uint32_t *starts;             // the source segments' starts: nv + 1
    const unsigned long long *values;   // the source values: nv
    uint32_t n, nv;
    unsigned long long *admit;          // RQ_PR_WORDS words per chunk of postings: bit i & 63 of word i >> 6 = posting i is admitted
    uint32_t *chunk;                    // per chunk of postings: its admitted count, after SCAN its exclusive prefix
    uint32_t *rank64;                   // per admit word: the admitted postings before it
    uint32_t *pos_out;                  // n: the admitted positions in posting order
    unsigned long long *keep;           // RQ_PR_WORDS words per chunk of segments: the kept flags
    uint32_t *seg_chunk;                // per chunk of segments: as `chunk`
    uint32_t *seg_lo;                   // nv: every source segment's new start
    uint32_t *starts_out;               // nv + 1
    unsigned long long *values_out;     // nv
    uint32_t *totals;                   // {admitted postings, kept segments}
};
static inline uint32_t restrict_chunks(uint32_t items) { return (uint32_t)(((uint64_t)items + RQ_PR_CHUNK - 1) / RQ_PR_CHUNK); }

// the launches (inst_postings_restrict.hip); every one of them expects n > 0 and nv > 0
void launch_restrict_admit(const PostRestrictArgs &a, hipStream_t st);
void launch_restrict_scan(uint32_t *counts, uint32_t chunks, uint32_t *total, hipStream_t st);
void launch_restrict_take(const PostRestrictArgs &a, hipStream_t st);
void launch_restrict_segments(const PostRestrictArgs &a, hipStream_t st);
void launch_restrict_segments_take(const PostRestrictArgs &a, hipStream_t st);

#ifdef RQ_POSTINGS_RESTRICT_KERNELS
// item `round` of this lane: word 4 round + wave of the block's chunk
__device__ __forceinline__ uint64_t pr_item(uint32_t round) {
    return (uint64_t)blockIdx.x * RQ_PR_CHUNK + (round * 4u + (threadIdx.x >> 6)) * 64u + (threadIdx.x & 63u);
}
// The block's flags (bit r of `mine`: this lane's item of round r is on) as the chunk's RQ_PR_WORDS bitmap words and its count.
__device__ __forceinline__ void pr_mark(uint32_t mine, unsigned long long *__restrict__ bits, uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_pop[RQ_PR_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const unsigned long long bal = __ballot((mine >> r) & 1u);
        if (lane == 0) bits[(uint64_t)blockIdx.x * RQ_PR_WORDS + r * 4u + wave] = bal, s_pop[r * 4u + wave] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (wave == 0) {
        uint32_t c = lane < RQ_PR_WORDS ? s_pop[lane] : 0u;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) counts[blockIdx.x] = c;
    }
}
// The flagged items of the block's chunk, each with its global rank (prefix[chunk] + the chunk's earlier words + the word's bits
// below the lane): put(item, rank).  rank64, where given, receives every word's own rank.
template <typename PutFn>
__device__ __forceinline__ void pr_place(const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ prefix, uint32_t *__restrict__ rank64, PutFn put) {
    __shared__ uint32_t s_base[RQ_PR_WORDS];
    __shared__ unsigned long long s_bits[RQ_PR_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (wave == 0) {
        const uint64_t w = (uint64_t)blockIdx.x * RQ_PR_WORDS + lane;
        const unsigned long long word = lane < RQ_PR_WORDS ? bits[w] : 0ull;
        const uint32_t c = (uint32_t)__popcll(word), before = prefix[blockIdx.x] + (wave_incl_scan(c) - c);
        if (lane < RQ_PR_WORDS) {
            s_bits[lane] = word, s_base[lane] = before;
            if (rank64) rank64[w] = before;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const unsigned long long word = s_bits[r * 4u + wave];
        if ((word >> lane) & 1ull) put(pr_item(r), s_base[r * 4u + wave] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull)));
    }
}

__global__ __launch_bounds__(256) void restrict_admit_kernel(const PostRestrictArgs a) {
    uint32_t p[8], mine = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) p[r] = pr_item(r) < a.n ? a.post[pr_item(r)] : 0xFFFFFFFFu;  // (no position is 2^32 - 1: n fits a u32)
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const uint32_t word = p[r] != 0xFFFFFFFFu ? a.allow[p[r] >> 5] : 0u;
        mine |= ((word >> (p[r] & 31u)) & 1u) << r;
    }
    pr_mark(mine, a.admit, a.chunk);
}

// counts[0 .. chunks) become their exclusive prefix sums; *total their sum.  One block of 1024 threads.
__global__ __launch_bounds__(1024) void restrict_scan_kernel(uint32_t *__restrict__ counts, uint32_t chunks, uint32_t *__restrict__ total) {
    const uint32_t all = block_scan_chunked<uint32_t, uint32_t>(
        chunks, [&](uint32_t i) { return counts[i]; }, [&](uint32_t i, uint32_t excl, uint32_t) { counts[i] = excl; });
    if (threadIdx.x == 0) *total = all;
}

__global__ __launch_bounds__(256) void restrict_take_kernel(const PostRestrictArgs a) {
    pr_place(a.admit, a.chunk, a.rank64, [&](uint64_t i, uint32_t at) {
        if (i < a.n && at < a.n) a.pos_out[at] = a.post[i];  // (both hold by construction: a flag past the end is never set)
    });
}

// admitted postings before posting i (i <= n)
__device__ __forceinline__ uint32_t pr_rank(const PostRestrictArgs &a, uint32_t i) {
    if (i >= a.n) return a.totals[0];
    return a.rank64[i >> 6] + (uint32_t)__popcll(a.admit[i >> 6] & ((1ull << (i & 63u)) - 1ull));
}
__global__ __launch_bounds__(256) void restrict_segments_kernel(const PostRestrictArgs a) {
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const uint64_t s = pr_item(r);
        if (s >= a.nv) continue;
        const uint32_t lo = pr_rank(a, a.starts[s]), hi = pr_rank(a, a.starts[s + 1]);
        a.seg_lo[s] = lo;
        mine |= (hi != lo ? 1u : 0u) << r;
    }
    pr_mark(mine, a.keep, a.seg_chunk);
}
__global__ __launch_bounds__(256) void restrict_segments_take_kernel(const PostRestrictArgs a) {
    pr_place(a.keep, a.seg_chunk, nullptr, [&](uint64_t s, uint32_t at) {
        if (s < a.nv && at < a.nv) a.starts_out[at] = a.seg_lo[s], a.values_out[at] = a.values[s];
    });
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.totals[1] <= a.nv) a.starts_out[a.totals[1]] = a.totals[0];
}
#endif  // RQ_POSTINGS_RESTRICT_KERNELS
