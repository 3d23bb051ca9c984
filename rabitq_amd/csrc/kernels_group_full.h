// kernels_group_full.h -- the complete form of the exact grouped search (rq_exact_search_grouped_full*, host_group_full.h; DESIGN
// §4.27), wave64: per query the topk DISTINCT groups with the smallest minimum distance out of an unbounded number of rows, a group
// being a segment of a postings object (kernels_keyed.h).  Nothing here writes an array of the index.
//
// The pieces, in the order the host runs them:
//   group_full_inverse_kernel  position -> segment, once per postings object: a thread per posting, the segment by bisection over the
//                              segment starts.  Segments ascend with the values, so everything below compares u32 segments and never
//                              column bytes.
//   group_full_bound_kernel    T_q from the bound's sample (the exact search's own sample launches leave a position and a key per
//                              sampled row): the distance at which the topk-th distinct segment first occurs in the sample, f32::MAX
//                              when the sample shows fewer.  Every sampled group's true minimum is at most its sampled one, so at
//                              least topk groups have a minimum <= T_q: like §4.12's bound it changes the work, never the answer.
//   group_full_dist_kernel     exact_range_dist_kernel with a payload: a pair of lanes per arena record, e from exact_l2_row, the key
//                              ord32_biased(e) << 32 | id, the payload seg = inverse[pos]; a hit has e <= T_q (not <: the topk-th
//                              group's minimum may equal T_q), e < f32::MAX and a segment.  Hits are counted per query.
//   group_full_scatter_kernel  the hits' (key, seg) into per-query segments of exactly the hits (after the prefix sum of the counts).
//   group_full_select_kernel   the distinct-minimum selection (below) and the outputs.
//
// DISTINCT-MINIMUM SELECTION (group_full_distinct_min): one block of 256 threads per query over its m hits, m unbounded.  The block
// keeps the RUNNING SET -- at most topk pairs (segment, minimum key), ascending by key -- at the front of one LDS buffer and consumes
// the hits in chunks of 256 PF.  A hit is dropped at once when the set is full and its key is above the set's topk-th minimum
// (topk groups already have a smaller minimum: the hit neither enters the answer nor lowers a minimum in it); the others are appended
// behind the set, their places from ballots and a four-word prefix (no atomic).  When another chunk might not fit, the buffer is
// reduced: sorted by (segment, key), the first member of every run kept (every other key becomes ~0), sorted by key, cut at topk.
// The next chunk's loads are issued before the reduction's sorts and wait in registers.
// Keys are unique -- one per id -- so (segment, key) and key are total orders: after every reduction the set is exactly the topk
// smallest group minima of the hits consumed so far, whatever the chunking and whatever order the hits arrived in; the scatter's
// order (the one place an atomic picks a place) therefore never reaches an output.  Vector loads and stores only.
// LDS: (TOPKCAP + 256 PF) x 16 bytes + 32: 16 KB at topk <= 256 (many blocks per CU), 48 KB up to 2048.
//
// This header has two parts: the launch interface, which the host unit sees, and the kernels, compiled only by inst_group_full.hip
// (RQ_GROUP_FULL_KERNELS).
#pragma once
#include "common.h"
#include "kernels_exact.h"  // ExactArgs: the arena, the sample's slots (the launch interface only)

#define RQ_GF_NO_SEG 0xFFFFFFFFu   // inverse[pos]: the position is in no segment (not live when the postings were made)
#define RQ_GF_TOPK_SMALL 256u      // topk up to here: the 16 KB instantiation

struct GroupFullSelectArgs {
    const unsigned long long *keys;    // the hits' keys in per-query segments [lims[q], lims[q + 1])
    const uint32_t *segs;              // ... and their postings segments
    const unsigned long long *lims;    // nq + 1
    const unsigned long long *values;  // the postings' values (u64 images), by segment
    uint32_t topk, gsize;
    float *out_dist;                   // nq x topk x gsize
    uint32_t *out_id;
    unsigned long long *out_key;       // nq x topk
    uint32_t *out_group_n;
    uint32_t *out_n;                   // nq
    uint32_t *out_fetched;             // nq, nullable: the hits the selection saw
    uint32_t *chosen;                  // nq x topk: the chosen segments, RQ_GF_NO_SEG behind out_n (read back when gsize > 1)
};

// the launches (inst_group_full.hip)
void launch_group_full_inverse(const uint32_t *post, const uint32_t *starts, uint32_t nv, uint64_t rows, uint32_t *inverse, uint64_t n, hipStream_t st);
void launch_group_full_bound(const ExactArgs &sample, const uint32_t *inverse, uint32_t topk, float *thr, hipStream_t st);
void launch_group_full_dist(const ExactArgs &a, const uint32_t *inverse, uint32_t *segs, uint32_t *hits, uint32_t records, hipStream_t st);
void launch_group_full_scatter(const ExactArgs &a, const uint32_t *segs, const ExactSegments &sg, uint32_t *out_segs, uint32_t records, hipStream_t st);
void launch_group_full_select(const GroupFullSelectArgs &a, uint32_t nq, hipStream_t st);
void launch_group_full_expand(const float *q, uint32_t len, uint32_t topk, uint64_t cells, float *out, hipStream_t st);  // out[pq] = q[pq / topk]

#ifdef RQ_GROUP_FULL_KERNELS
#include "kernels_rerank.h"

struct GroupFullItem {
    unsigned long long key;  // ord32_biased(e) << 32 | id; ~0: not a group's minimum (the reduction's own mark)
    uint32_t seg, pad;
};
struct GroupFullBySeg {
    uint32_t seg;
    unsigned long long key;
    __device__ __forceinline__ bool operator<(const GroupFullBySeg &o) const { return seg != o.seg ? seg < o.seg : key < o.key; }
};

__global__ __launch_bounds__(256) void group_full_fill_kernel(uint32_t *__restrict__ inverse, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) inverse[i] = RQ_GF_NO_SEG;
}
// posting i belongs to the largest segment s with starts[s] <= i (starts[0] = 0, starts[nv] = rows)
__global__ __launch_bounds__(256) void group_full_inverse_kernel(const uint32_t *__restrict__ post, const uint32_t *__restrict__ starts, uint32_t nv,
                                                                 uint64_t rows, uint32_t *__restrict__ inverse, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += (uint64_t)gridDim.x * 256) {
        uint32_t lo = 0, hi = nv;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (starts[mid] <= i) lo = mid;
            else hi = mid;
        }
        const uint32_t p = post[i];
        if (p < n) inverse[p] = lo;
    }
}

// See the header comment.  buf: TOPKCAP + 256 PF items; wcnt: 8 words; load(i, key, seg) reads hit i < m (a key of ~0 or a segment of
// RQ_GF_NO_SEG is no hit).  Every thread of the block calls; returns the number of groups r <= topk, block-uniform, with
// buf[0 .. r) the groups ascending by their minimum key.
template <uint32_t TOPKCAP, uint32_t PF, typename LoadFn>
__device__ __forceinline__ uint32_t group_full_distinct_min(GroupFullItem *buf, uint32_t *wcnt, uint32_t m, uint32_t topk, LoadFn load) {
    constexpr uint32_t CH = 256 * PF, CAP = TOPKCAP + CH, PER = CAP / 256;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long nk[PF];
    uint32_t ns[PF];
    const auto fetch = [&](uint32_t c0) {
#pragma unroll
        for (uint32_t j = 0; j < PF; ++j) {
            const uint64_t i = (uint64_t)c0 + j * 256 + t;
            nk[j] = ~0ull, ns[j] = RQ_GF_NO_SEG;
            if (i < m) load((uint32_t)i, nk[j], ns[j]);
        }
    };
    fetch(0);
    uint32_t r = 0, fill = 0, round = 0;
    unsigned long long cutoff = ~0ull;
    for (uint64_t c0 = 0; c0 < m; c0 += CH) {
        unsigned long long ck[PF];
        uint32_t cs[PF];
#pragma unroll
        for (uint32_t j = 0; j < PF; ++j) ck[j] = nk[j], cs[j] = ns[j];
        const bool last = c0 + CH >= m;
        if (!last) fetch((uint32_t)(c0 + CH));  // in flight under the appends and the sorts below
#pragma unroll
        for (uint32_t j = 0; j < PF; ++j, ++round) {
            const bool keep = cs[j] != RQ_GF_NO_SEG && ck[j] != ~0ull && ck[j] <= cutoff;
            const unsigned long long mask = __ballot(keep);
            uint32_t *wc = wcnt + 4 * (round & 1u);  // (two sets: a wave may be a round ahead of the slowest reader)
            if (lane == 0) wc[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t at = fill, all = 0;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {
                if (w < wave) at += wc[w];
                all += wc[w];
            }
            if (keep) buf[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = GroupFullItem{ck[j], cs[j], 0u};
            fill += all;  // (<= CAP: a chunk starts at fill <= TOPKCAP or after a test of fill + CH <= CAP)
        }
        if (!last && fill + CH <= CAP) continue;  // (uniform) the next chunk fits behind this one
        __syncthreads();
        bitonic_sort_block(buf, fill, [](const GroupFullItem &e) { return GroupFullBySeg{e.seg, e.key}; });
        bool head[PER];
        uint32_t heads = 0;
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            const uint32_t i = t + e * 256;
            head[e] = i < fill && (i == 0 || buf[i - 1].seg != buf[i].seg);
            heads += (uint32_t)__syncthreads_count(head[e] ? 1 : 0);  // (the last one is also the barrier between these reads and the marks)
        }
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            const uint32_t i = t + e * 256;
            if (i < fill && !head[e]) buf[i].key = ~0ull;
        }
        __syncthreads();
        bitonic_sort_block(buf, fill, [](const GroupFullItem &e) { return e.key; });
        r = heads < topk ? heads : topk;
        fill = r;
        cutoff = r == topk ? buf[topk - 1].key : ~0ull;
    }
    __syncthreads();
    return r;
}

// T_q of the sample's rows: slot i of query q holds a position (cand) and its key (keys; ~0: e is NaN or f32::MAX).  A bound of zero
// would close the scan for the query (it emits nothing for a bound that is not above zero): the smallest positive f32 bounds as well.
template <uint32_t TOPKCAP, uint32_t PF>
__global__ __launch_bounds__(256) void group_full_bound_kernel(const ExactArgs a, const uint32_t *__restrict__ inverse, uint32_t topk,
                                                               float *__restrict__ thr) {
    __shared__ GroupFullItem buf[TOPKCAP + 256 * PF];
    __shared__ uint32_t wcnt[8];
    const uint32_t q = blockIdx.x;
    const uint32_t m = a.cnt[q] < a.cap ? a.cnt[q] : a.cap;
    const uint64_t base = (uint64_t)q * a.cap;
    const uint32_t r = group_full_distinct_min<TOPKCAP, PF>(buf, wcnt, m, topk, [&](uint32_t i, unsigned long long &key, uint32_t &seg) {
        key = a.keys[base + i], seg = inverse[a.cand[base + i]];
    });
    if (threadIdx.x == 0) {
        float T = 3.4028234663852886e38f;
        if (r == topk) T = fmaxf(ord32_unbias((uint32_t)(buf[topk - 1].key >> 32)), 1.17549435e-38f);
        thr[q] = T;
    }
}

__global__ __launch_bounds__(256) void group_full_dist_kernel(const ExactArgs a, const uint32_t *__restrict__ inverse, uint32_t *__restrict__ segs,
                                                              uint32_t *__restrict__ hit_cnt, uint32_t m) {
    const uint32_t dim = a.dim, hf = threadIdx.x & 1, lane = threadIdx.x & 63;
    const uint32_t rounds = (uint32_t)(((uint64_t)m + 127) / 128);
    for (uint32_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const uint64_t i = (uint64_t)rd * 128 + (threadIdx.x >> 1);
        const bool have = i < m;  // (the same for the two lanes of a pair)
        const uint2 rec = have ? a.rec[i] : make_uint2(0xFFFFFFFFu, 0u);
        bool hit = false;
        if (have) {
            const uint32_t seg = inverse[rec.y];
            const float e = exact_l2_row(a.base.row_at(rec.y, dim), a.qpad + (uint64_t)rec.x * dim, dim, hf);
            if (hf == 0) {
                hit = e <= a.thr[rec.x] && e < 3.4028234663852886e38f && seg != RQ_GF_NO_SEG;
                a.keys[i] = hit ? ((unsigned long long)ord32_biased(e) << 32) | a.map_ids[rec.y] : ~0ull;
                segs[i] = seg;
            }
        }
        const unsigned long long hits = __ballot(hit);
        const uint32_t q0 = __shfl(rec.x, 0, 64);
        if (__all(!have || rec.x == q0)) {
            if (lane == 0 && hits) atomicAdd(&hit_cnt[q0], (uint32_t)__popcll(hits));
        } else if (hit) {
            atomicAdd(&hit_cnt[rec.x], 1u);
        }
    }
}

// The hits into their query's segment [lims[q], lims[q + 1]): the place from the segment's cursor -- whatever the atomics give; the
// selection does not depend on it.
__global__ __launch_bounds__(256) void group_full_scatter_kernel(const uint2 *__restrict__ rec, const unsigned long long *__restrict__ keys,
                                                                 const uint32_t *__restrict__ segs, uint32_t m, const ExactSegments sg,
                                                                 uint32_t *__restrict__ out_segs) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const unsigned long long key = keys[i];
        if (key == ~0ull) continue;
        const uint32_t q = rec[i].x;
        const unsigned long long o = sg.lims[q] + atomicAdd(&sg.cursor[q], 1u);
        if (o < sg.lims[q + 1]) sg.out[o] = key, out_segs[o] = segs[i];
    }
}

// The selection and every output slot of query blockIdx.x.  Row 0 of a group is its minimum; with gsize > 1 the rows of the chosen
// groups follow from the keyed search, which writes the same row 0 again.
template <uint32_t TOPKCAP, uint32_t PF>
__global__ __launch_bounds__(256) void group_full_select_kernel(const GroupFullSelectArgs a) {
    __shared__ GroupFullItem buf[TOPKCAP + 256 * PF];
    __shared__ uint32_t wcnt[8];
    const uint64_t q = blockIdx.x, lo = a.lims[q];
    const uint32_t m = (uint32_t)(a.lims[q + 1] - lo), topk = a.topk, gsize = a.gsize, t = threadIdx.x;
    const uint32_t r = group_full_distinct_min<TOPKCAP, PF>(buf, wcnt, m, topk, [&](uint32_t i, unsigned long long &key, uint32_t &seg) {
        key = a.keys[lo + i], seg = a.segs[lo + i];
    });
    for (uint32_t o = t; o < topk; o += 256) {
        const bool have = o < r;
        a.out_key[q * topk + o] = have ? a.values[buf[o].seg] : 0ull;
        a.out_group_n[q * topk + o] = have ? 1u : 0u;
        a.chosen[q * topk + o] = have ? buf[o].seg : RQ_GF_NO_SEG;
    }
    const uint32_t slots = topk * gsize;
    for (uint32_t s = t; s < slots; s += 256) {
        const uint32_t o = s / gsize;
        const bool have = o < r && s == o * gsize;
        a.out_id[q * slots + s] = have ? (uint32_t)buf[o].key : 0xFFFFFFFFu;
        a.out_dist[q * slots + s] = have ? ord32_unbias((uint32_t)(buf[o].key >> 32)) : __builtin_nanf("");
    }
    if (t == 0) {
        a.out_n[q] = r;
        if (a.out_fetched) a.out_fetched[q] = m;
    }
}

// plan-query pq of the keyed search (query pq / topk against its ord-th group): its raw query row
__global__ __launch_bounds__(256) void group_full_expand_kernel(const float *__restrict__ q, uint32_t len, uint32_t topk, uint64_t cells,
                                                                float *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (uint64_t)gridDim.x * 256) {
        const uint64_t pq = i / len;
        out[i] = q[(pq / topk) * len + (i - pq * len)];
    }
}
#endif  // RQ_GROUP_FULL_KERNELS
