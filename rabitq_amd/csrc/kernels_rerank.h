// kernels_rerank.h -- the exact re-rank stage of RaBitQ::query (src/rerank.rs:85-91): the exact f32 distance of a survivor, the
// shadow rows that prove most survivors out of the result without fetching their f32 row, and the kernels that run both.
// Included by kernels_query.h, whose stage_finish_kernel (and kernels_small.h's finish) call accurate_rows as their phase (A).
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------
// Rerank distances (src/rerank.rs:85-90 -> src/simd.rs:14-73): accurate = ||base[pos] - q||^2 in
// the ORIGINAL space, exact AVX2 order.  8 GPU lanes play the 8 AVX lanes of one candidate (lane l
// runs the fused chain over elements 8c + l), so a wave reranks 8 survivors at a time and each
// 32-byte sector of the 4*dim-byte row is consumed by exactly one load.  In the query pipeline this
// is phase (A) of stage_finish_kernel.
// ------------------------------------------------------------------------------------------------
// flat variant for the per-stage test entry rq_rerank: positions given directly
__global__ __launch_bounds__(256) void accurate_flat_kernel(const uint32_t *__restrict__ pos, uint32_t m,
                                                            const BaseView base,
                                                            const float *__restrict__ q, uint32_t dim,
                                                            float *__restrict__ out) {
    const uint32_t l = threadIdx.x & 7;
    uint32_t i = blockIdx.x * 32 + (threadIdx.x >> 3);
    if (i >= m) return;
    const RowRef x = base.row(pos[i], dim);
    float acc = 0.0f;
    for (uint32_t c = 0; c < dim; c += 8) {
        float d = rq_row_get(x, dim, c + l) - q[c + l];
        acc = fmaf(d, d, acc);
    }
    acc = reduce8_lanes(acc);
    if (l == 0) out[i] = acc;
}

// ------------------------------------------------------------------------------------------------
// The exact f32 L2 of one row against the query held in LDS, by a PAIR of lanes (src/rerank.rs:85-90; lane order of
// src/simd.rs:14-73).  Lane half hf carries AVX lanes 4hf..4hf+3 (elements 8c + 4hf + 0..3, one 16-byte load per chunk); the
// fold ((a0+a4)+(a1+a5)) + ((a2+a6)+(a3+a7)) needs one exchange between the two lanes.  A row is fetched 8 chunks (64
// dimensions, 8 x 16 bytes per lane) at a time so that every lane keeps 8 loads in flight (this is a random 512-byte-row
// gather: latency-bound unless enough bytes are outstanding).  Every caller goes through the ONE accumulate step and the ONE
// fold below: all paths stay bit-identical to the reference.
// ------------------------------------------------------------------------------------------------
// 64 dimensions of a row, already in registers (xv[u] = elements 8u + 4hf + 0..3 of the chunk), against q = q_lds + chunk + 4*hf
__device__ __forceinline__ void exact_l2_acc64(const float4 (&xv)[8], const float *q, float &a0, float &a1, float &a2, float &a3) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float4 qv = *reinterpret_cast<const float4 *>(q + 8 * u);
        const float d0 = xv[u].x - qv.x, d1 = xv[u].y - qv.y, d2 = xv[u].z - qv.z, d3 = xv[u].w - qv.w;
        a0 = fmaf(d0, d0, a0), a1 = fmaf(d1, d1, a1), a2 = fmaf(d2, d2, a2), a3 = fmaf(d3, d3, a3);
    }
}
// c_i = a_i + a_{i+4}: the partner lane holds the other half (commutative, so both lanes agree)
__device__ __forceinline__ float exact_l2_fold(float a0, float a1, float a2, float a3) {
    const float c0 = a0 + __shfl_xor(a0, 1, 2), c1 = a1 + __shfl_xor(a1, 1, 2);
    const float c2 = a2 + __shfl_xor(a2, 1, 2), c3 = a3 + __shfl_xor(a3, 1, 2);
    return (c0 + c1) + (c2 + c3);
}
// a plain row; x already offset by 4*hf
__device__ __forceinline__ float exact_l2_pair(const float *__restrict__ x, const float *q_lds, uint32_t dim, uint32_t hf) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (uint32_t c = 0; c < dim; c += 64) {  // dim is a multiple of 64
        float4 xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = *reinterpret_cast<const float4 *>(x + c + 8 * u);
        exact_l2_acc64(xv, q_lds + c + 4 * hf, a0, a1, a2, a3);
    }
    return exact_l2_fold(a0, a1, a2, a3);
}
// a SPLIT row (common.h: two 16-bit planes): the words are restored exactly, the arithmetic is exact_l2_pair's
__device__ __forceinline__ float exact_l2_pair_split(const float *__restrict__ row, const float *q_lds, uint32_t dim, uint32_t hf) {
    const uint16_t *hp = reinterpret_cast<const uint16_t *>(row) + 4 * hf, *lp = hp + dim;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (uint32_t c = 0; c < dim; c += 64) {
        uint2 hv[8], lv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) hv[u] = *reinterpret_cast<const uint2 *>(hp + c + 8 * u);
#pragma unroll
        for (int u = 0; u < 8; ++u) lv[u] = *reinterpret_cast<const uint2 *>(lp + c + 8 * u);
        float4 xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            xv[u].x = __builtin_bit_cast(float, (hv[u].x << 16) + (uint32_t)(int32_t)(int16_t)lv[u].x);
            xv[u].y = __builtin_bit_cast(float, (hv[u].x & 0xFFFF0000u) + (uint32_t)((int32_t)lv[u].x >> 16));
            xv[u].z = __builtin_bit_cast(float, (hv[u].y << 16) + (uint32_t)(int32_t)(int16_t)lv[u].y);
            xv[u].w = __builtin_bit_cast(float, (hv[u].y & 0xFFFF0000u) + (uint32_t)((int32_t)lv[u].y >> 16));
        }
        exact_l2_acc64(xv, q_lds + c + 4 * hf, a0, a1, a2, a3);
    }
    return exact_l2_fold(a0, a1, a2, a3);
}
// a HALF-PRECISION row (common.h: 2-byte elements as the caller gave them): lane half hf's elements 8u + 4hf + 0..3 of a chunk are
// 8 bytes, widened exactly (f16: v_cvt_f32_f16, subnormals kept; bf16: bits << 16), and the arithmetic is exact_l2_pair's --
// exact_l2_acc64 per 64 dimensions in chunk order, every fused chain inside its lane, then exact_l2_fold.  A round takes 128
// dimensions (16 x 8 bytes per lane: the 128 bytes in flight of exact_l2_pair's round) and the odd 64 of dim = 64 (2m + 1) last.
// x = the row + 4*hf elements.
template <bool BF16>
__device__ __forceinline__ void half_widen64(const uint2 *hv, float4 (&xv)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if constexpr (BF16) {
            xv[u].x = __builtin_bit_cast(float, hv[u].x << 16), xv[u].y = __builtin_bit_cast(float, hv[u].x & 0xFFFF0000u);
            xv[u].z = __builtin_bit_cast(float, hv[u].y << 16), xv[u].w = __builtin_bit_cast(float, hv[u].y & 0xFFFF0000u);
        } else {
            typedef _Float16 rq_half2 __attribute__((ext_vector_type(2)));
            const rq_half2 a = __builtin_bit_cast(rq_half2, hv[u].x), b = __builtin_bit_cast(rq_half2, hv[u].y);
            xv[u].x = (float)a[0], xv[u].y = (float)a[1], xv[u].z = (float)b[0], xv[u].w = (float)b[1];
        }
    }
}
template <bool BF16>
__device__ __forceinline__ float exact_l2_pair_half(const uint16_t *__restrict__ x, const float *q_lds, uint32_t dim, uint32_t hf) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    uint32_t c = 0;
    for (; c + 128 <= dim; c += 128) {
        uint2 hv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) hv[u] = *reinterpret_cast<const uint2 *>(x + c + 8 * u);
        float4 xv[8];
        half_widen64<BF16>(hv, xv);
        exact_l2_acc64(xv, q_lds + c + 4 * hf, a0, a1, a2, a3);
        half_widen64<BF16>(hv + 8, xv);
        exact_l2_acc64(xv, q_lds + c + 64 + 4 * hf, a0, a1, a2, a3);
    }
    if (c < dim) {  // dim is a multiple of 64: one half round is left
        uint2 hv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) hv[u] = *reinterpret_cast<const uint2 *>(x + c + 8 * u);
        float4 xv[8];
        half_widen64<BF16>(hv, xv);
        exact_l2_acc64(xv, q_lds + c + 4 * hf, a0, a1, a2, a3);
    }
    return exact_l2_fold(a0, a1, a2, a3);
}
// a BYTE row (common.h: one-byte elements as the caller gave them): lane half hf's elements 8u + 4hf + 0..3 of a chunk are ONE
// dword, widened exactly in registers (u8: the four byte-to-f32 conversions; i8: a sign-extending extract and the integer
// conversion), and the arithmetic is exact_l2_pair's -- exact_l2_acc64 per 64 dimensions in chunk order, every fused chain inside
// its lane, then exact_l2_fold.  A round takes 256 dimensions (the 128 bytes per lane in flight of exact_l2_pair's round), then
// one tail of 128 and one of 64 dimensions as dim requires.  How the dwords reach the lane is RQ_BYTE_PAIR_LOADS:
//   false  a dword load per chunk (32 per round), nothing crosses lanes before the fold;
//   true   an 8-byte load per TWO chunks (16 per round): lane hf fetches chunk 2j + hf whole and the pair swaps the halves it
//          fetched for each other (one exchange of raw bytes per two chunks; the accumulators still never leave their lane).
// Measured on 100M x 128 / 40M x 768 u8 rows, 65 536 queries: 6.17 / 17.79 ms of rerank with dword loads, 3.05 / 6.61 ms with pair
// loads -- a wave's dword load touches 32 rows for 8 bytes each, and the gather is bound by those requests.
constexpr bool RQ_BYTE_PAIR_LOADS = true;
template <bool SIGNED>
__device__ __forceinline__ void byte_widen64(const uint32_t *bv, float4 (&xv)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const uint32_t w = bv[u];
        if constexpr (SIGNED) {
            const int32_t s = (int32_t)w;
            xv[u].x = (float)((s << 24) >> 24), xv[u].y = (float)((s << 16) >> 24);
            xv[u].z = (float)((s << 8) >> 24), xv[u].w = (float)(s >> 24);
        } else {
            xv[u].x = (float)(w & 0xFFu), xv[u].y = (float)((w >> 8) & 0xFFu);
            xv[u].z = (float)((w >> 16) & 0xFFu), xv[u].w = (float)(w >> 24);
        }
    }
}
// CHUNKS x 64 dimensions of the row from byte `row` on (no lane offset in it): every load first, then widen and accumulate chunk
// by chunk; q = the query from the same dimension on, + 4*hf
template <bool SIGNED, int CHUNKS>
__device__ __forceinline__ void exact_l2_byte_round(const uint8_t *__restrict__ row, uint32_t hf, const float *q, float &a0, float &a1, float &a2,
                                                    float &a3) {
    uint32_t bv[8 * CHUNKS];  // bv[u] = elements 8u + 4hf + 0..3
    if constexpr (RQ_BYTE_PAIR_LOADS) {
        uint2 v[4 * CHUNKS];  // v[j] = chunk 2j + hf: .x its elements 0..3, .y its elements 4..7
#pragma unroll
        for (int j = 0; j < 4 * CHUNKS; ++j) v[j] = *reinterpret_cast<const uint2 *>(row + 16 * j + 8 * hf);
#pragma unroll
        for (int j = 0; j < 4 * CHUNKS; ++j) {
            // lane 0 needs elements 0..3 of both chunks (its own .x and lane 1's), lane 1 elements 4..7 (lane 0's .y and its own)
            const uint32_t recv = (uint32_t)__shfl_xor((int)(hf ? v[j].x : v[j].y), 1, 2);
            bv[2 * j] = hf ? recv : v[j].x;
            bv[2 * j + 1] = hf ? v[j].y : recv;
        }
    } else {
#pragma unroll
        for (int u = 0; u < 8 * CHUNKS; ++u) bv[u] = *reinterpret_cast<const uint32_t *>(row + 8 * u + 4 * hf);
    }
#pragma unroll
    for (int h = 0; h < CHUNKS; ++h) {
        float4 xv[8];
        byte_widen64<SIGNED>(bv + 8 * h, xv);
        exact_l2_acc64(xv, q + 64 * h, a0, a1, a2, a3);
    }
}
// ROUND: the chunks of the full round (4: 256 dimensions; 1: the 64-dimension form for kernels short of registers)
template <bool SIGNED, int ROUND = 4>
__device__ __forceinline__ float exact_l2_pair_byte(const uint8_t *__restrict__ row, const float *q_lds, uint32_t dim, uint32_t hf) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float *q = q_lds + 4 * hf;
    uint32_t c = 0;
    for (; c + 64 * ROUND <= dim; c += 64 * ROUND) exact_l2_byte_round<SIGNED, ROUND>(row + c, hf, q + c, a0, a1, a2, a3);
    if constexpr (ROUND >= 4) {
        if (c + 128 <= dim) {
            exact_l2_byte_round<SIGNED, 2>(row + c, hf, q + c, a0, a1, a2, a3);
            c += 128;
        }
    }
    if constexpr (ROUND >= 2) {
        if (c < dim) exact_l2_byte_round<SIGNED, 1>(row + c, hf, q + c, a0, a1, a2, a3);  // dim is a multiple of 64
    }
    return exact_l2_fold(a0, a1, a2, a3);
}
// an f32 row, plain or split
__device__ __forceinline__ float exact_l2_row_f32(const RowRef rr, const float *q_lds, uint32_t dim, uint32_t hf) {
    // (a pair of lanes shares its survivor: the branch does not split the pair)
    return rr.split ? exact_l2_pair_split(rr.p, q_lds, dim, hf) : exact_l2_pair(rr.p + 4 * hf, q_lds, dim, hf);
}
// a half-precision row of either type
__device__ __forceinline__ float exact_l2_row_half(const RowRef rr, const float *q_lds, uint32_t dim, uint32_t hf) {
    const uint16_t *x = reinterpret_cast<const uint16_t *>(rr.p) + 4 * hf;
    return rr.fmt == RQ_ROWS_BF16 ? exact_l2_pair_half<true>(x, q_lds, dim, hf) : exact_l2_pair_half<false>(x, q_lds, dim, hf);
}
// a byte row of either type
template <int ROUND = 4>
__device__ __forceinline__ float exact_l2_row_byte(const RowRef rr, const float *q_lds, uint32_t dim, uint32_t hf) {
    const uint8_t *x = reinterpret_cast<const uint8_t *>(rr.p);
    return rr.fmt == RQ_ROWS_I8 ? exact_l2_pair_byte<true, ROUND>(x, q_lds, dim, hf) : exact_l2_pair_byte<false, ROUND>(x, q_lds, dim, hf);
}
// a row of any format: the dispatch on RowRef's run-time fields (BYTE_ROUND: exact_l2_pair_byte's ROUND)
template <int BYTE_ROUND = 4>
__device__ __forceinline__ float exact_l2_row(const RowRef rr, const float *q_lds, uint32_t dim, uint32_t hf) {
    if (RowSpec{rr.fmt}.bytes()) return exact_l2_row_byte<BYTE_ROUND>(rr, q_lds, dim, hf);
    return rr.fmt ? exact_l2_row_half(rr, q_lds, dim, hf) : exact_l2_row_f32(rr, q_lds, dim, hf);
}

// The row of a survivor: at its position in an untiered plain index (nothing else is read); else the survivor's slot names its
// list, the list's tier record places the row (HBM or host link).  (Half-precision and byte rows: BaseView::row_at.)
__device__ __forceinline__ RowRef rerank_row(const BaseView &base, const SurvRec &r, const uint32_t *__restrict__ probe_row /* the query's probed lists, by slot */,
                                             uint32_t dim) {
    if (base.host == nullptr && !base.split) return RowRef{base.dev + (uint64_t)r.pos * dim, false, 0u};
    return base.row_of_slot(r.pos, probe_row, r.slot, dim);
}

// Exact f32 L2 of survivors recs[first], recs[first + step], ... against the query held in LDS.  KIND: the row kind of the kernels
// an index is given -- ROW_KIND_HALF / ROW_KIND_BYTE: every row at its position, 2*dim / dim bytes apart, nothing but the row is
// read.  The launch picks the instantiation from the index's row type, so the f32 kernels' loop -- whose two rounds of loads the
// compiler issues together -- is compiled exactly as it was without the other formats in it; which of the two types of its kind a
// row holds stays a run-time field.  (ROW_KIND_*: rows.h.)
template <int KIND = ROW_KIND_F32>
__device__ __forceinline__ void accurate_rows(SurvRec *__restrict__ recs, uint32_t n, const BaseView &base,
                                              const float *q_lds, uint32_t dim, uint32_t first, uint32_t step,
                                              const uint32_t *__restrict__ probe_row) {
    const uint32_t hf = threadIdx.x & 1;
    for (uint32_t i = first; i < n; i += step) {
        float r;
        if constexpr (KIND == ROW_KIND_BYTE) r = exact_l2_row_byte(RowRef{base.dev + (uint64_t)recs[i].pos * (dim >> 2), false, base.fmt}, q_lds, dim, hf);
        else if constexpr (KIND == ROW_KIND_HALF) r = exact_l2_row_half(base.row_at(recs[i].pos, dim), q_lds, dim, hf);
        else r = exact_l2_row_f32(rerank_row(base, recs[i], probe_row, dim), q_lds, dim, hf);
        if (hf == 0) recs[i].accurate = r;
    }
}

// ------------------------------------------------------------------------------------------------
// Rerank pre-filter: an fp16 shadow of the raw vectors (derived state, half the bytes of a row).
//
// The re-ranker's exact distance only matters when it can pass `accurate < threshold` (src/rerank.rs:91): a
// survivor whose exact distance PROVABLY is >= the threshold its stage started with (the threshold only falls)
// is rejected by the reference whatever the exact value is.  For such a survivor the 4*dim-byte row is never
// fetched: the 2*dim-byte shadow row x~ gives
//     ||x - q||  >=  ||x~ - q|| - ||x - x~||,      ||x - x~|| <= 2^-11 ||x|| + sqrt(dim) 2^-25
// (fp16 round-to-nearest: relative 2^-11 per normal element, absolute 2^-25 per subnormal one; an element beyond
// the fp16 range becomes inf and disables the test), and the reference's f32 evaluation of ||x - q||^2
// (src/simd.rs:14-73: dim/8 fused multiply-adds per AVX lane + 3 adds, non-negative terms) is at least
// (1 - (dim/8 + 5) 2^-24) of the real value.  Every quantity below is rounded against the test (factors
// 1 -/+ eps with eps = (dim/4 + 64) 2^-24), so the bound can only be lower than the exact f32 result: a rejected
// survivor gets accurate = +inf, which fails `accurate < threshold` exactly as its exact value would.  Everything
// else goes through the exact path unchanged; results are bit-identical with and without the shadow.
// ------------------------------------------------------------------------------------------------
typedef _Float16 rq_half8 __attribute__((ext_vector_type(8)));

// 8 consecutive elements per thread; total = n * dim (a multiple of 64)
__global__ __launch_bounds__(256) void half_rows_kernel(const float *__restrict__ base, uint64_t total,
                                                        _Float16 *__restrict__ out) {
    for (uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < total; i += (uint64_t)gridDim.x * 2048) {
        const float4 a = *reinterpret_cast<const float4 *>(base + i), b = *reinterpret_cast<const float4 *>(base + i + 4);
        rq_half8 h;
        h[0] = (_Float16)a.x, h[1] = (_Float16)a.y, h[2] = (_Float16)a.z, h[3] = (_Float16)a.w;
        h[4] = (_Float16)b.x, h[5] = (_Float16)b.y, h[6] = (_Float16)b.z, h[7] = (_Float16)b.w;
        *reinterpret_cast<rq_half8 *>(out + i) = h;
    }
}

#define RQ_ACC8_LDS_PROBES 1024u  // probe lists whose maps / tier records the re-rankers stage in LDS (16 B each)

// The pre-filter kernels' common body; the shadow kind is a policy P:
//   P::V                      survivors per lane pair and round (the queue holds 128 V new ones on top of 127 waiting)
//   stage(behind, b)          what the block keeps in LDS behind the query (every thread calls it, ahead of the first barrier)
//   bound(cur, q, hf, up, dt, err)  per survivor of the pair: dt = ||x~ - q||^2 of its shadow row x~ (both lanes hold it), err >= ||x - x~||
//                             (inf: never rejected)
//   exact(rec, q, hf)         the exact distance of a queued survivor
//   P::RING                   the shadow rows travel through an LDS ring, one round ahead of the test (ShadowQ8Ring below): the
//                             records are then kept TWO rounds ahead, ring_issue(records of the next round, slot) starts the copies
//                             of the next round's rows before this round is tested, ring_wait(whether copies were just issued)
//                             retires this round's, and bound() reads slot ring_slot
// grid (gx, nq), block 256 = 128 V survivors per round, two lanes each.  Round: shadow-row test of 128 V survivors; the ones it
// cannot reject queue up in LDS and are re-ranked exactly 128 at a time, so both phases keep every lane busy.
// The kernel is a chain of dependent gathers (survivor record -> its list's map or tier record and its shadow row -> the f32 row of
// the few that stay), i.e. bound by how many of them are in flight: the first round's records are requested before anything else,
// every later round's while the current one is being worked on, and what stage() keeps is read from LDS (one dependent round
// trip less per round).
template <class P>
__device__ __forceinline__ void rerank_prefiltered(P &pol, SurvRec *__restrict__ surv, const unsigned long long *__restrict__ surv_cnt,
                                                   const QSeg &seg, const float *__restrict__ qpad, uint32_t dim,
                                                   const uint32_t *__restrict__ order, const float *__restrict__ thr_start,
                                                   uint32_t *__restrict__ nshadow) {
    constexpr int V = P::V;
    extern __shared__ __attribute__((aligned(16))) float acc_q[];  // dim floats (the padded query), then stage()'s
    __shared__ uint32_t queue[256 * V];
    __shared__ uint32_t qn;
    const uint32_t b = order ? order[blockIdx.y] : blockIdx.y;  // consecutive blocks: queries of the same nearest list
    const uint32_t n = (uint32_t)surv_cnt[b];
    if (n > seg.capof(b) || n == 0) return;  // overflowed: this query is re-run with a larger buffer
    SurvRec *recs = surv + seg.at(b);
    const uint32_t hf = threadIdx.x & 1, pair = threadIdx.x >> 1;
    const uint32_t i_first = blockIdx.x * (128 * V), stride = gridDim.x * (128 * V);
    SurvRec nxt[V], nxt2[V];
#pragma unroll
    for (int v = 0; v < V; ++v) nxt[v] = recs[i_first + 128 * v + pair < n ? i_first + 128 * v + pair : 0u];
    if constexpr (P::RING) {
#pragma unroll
        for (int v = 0; v < V; ++v) nxt2[v] = recs[i_first + stride + 128 * v + pair < n ? i_first + stride + 128 * v + pair : 0u];
    }
    for (uint32_t c = threadIdx.x * 4; c < dim; c += 1024)
        *reinterpret_cast<float4 *>(acc_q + c) = *reinterpret_cast<const float4 *>(qpad + (uint64_t)b * dim + c);
    pol.stage(acc_q + dim, b);
    if (threadIdx.x == 0) qn = 0;
    __syncthreads();
    const float thr = thr_start ? thr_start[b] : __builtin_inff();
    const bool test = thr > 1e-30f && thr < 3.0e38f;  // a finite, normal threshold (false for NaN / inf: everything is exact)
    const float eps = (float)(dim / 4 + 64) * 5.9604645e-8f, down = 1.0f - eps, up = 1.0f + eps;
    auto exact_of = [&](uint32_t j) {
        const float r = pol.exact(recs[j], acc_q, hf);
        if (hf == 0) recs[j].accurate = r;
    };
    uint32_t rejected = 0;
    if constexpr (P::RING) {
        pol.ring_slot = 0;
        if (test && i_first < n) pol.ring_issue(nxt, 0u);  // (block-uniform)
    }
    for (uint32_t i0 = i_first; i0 < n; i0 += stride) {
        uint32_t iv[V];
        bool exact[V];
        SurvRec cur[V];
        if constexpr (P::RING) {
            // the next round's rows are requested before this round's are waited for: they fly while this round is tested.  The
            // records of the round after that are requested behind them (ring_wait counts the copies only).
#pragma unroll
            for (int v = 0; v < V; ++v) {
                iv[v] = i0 + 128 * v + pair, exact[v] = iv[v] < n, cur[v] = nxt[v], nxt[v] = nxt2[v];
                // the records are pinned down HERE, before the next copies are issued (they were requested a round ago, behind this
                // round's copies): the compiler's own wait for them would otherwise come where their fields are first used, behind
                // ring_issue, and drain the copies just issued with it.  Requests return in order, so this wait also retires
                // this round's copies; ring_wait states that condition by itself instead of leaning on where the compiler waits.
                asm volatile("" ::"v"(nxt[v].pos), "v"(nxt[v].slot));
            }
            if (test) {
                const bool more = i0 + stride < n;  // block-uniform
                if (more) pol.ring_issue(nxt, pol.ring_slot ^ 1u);
                pol.ring_wait(more);
            }
#pragma unroll
            for (int v = 0; v < V; ++v) nxt2[v] = recs[iv[v] + 2 * stride < n ? iv[v] + 2 * stride : 0u];
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) {  // this round's records, and the next round's requested (clamped: the last prefetch re-reads record 0)
                iv[v] = i0 + 128 * v + pair, exact[v] = iv[v] < n, cur[v] = nxt[v];
                nxt[v] = recs[iv[v] + stride < n ? iv[v] + stride : 0u];
            }
        }
        if (test && exact[0]) {  // (a pair past the end has nothing to test; its survivor 0 is the lowest)
            float dt[V], err[V];
            pol.bound(cur, acc_q, hf, up, dt, err);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float t = sqrtf(dt[v] * down) * down - err[v] * up;
                if (exact[v] && t > 0.0f && (t * t) * (down * down) > thr) {  // false for NaN
                    exact[v] = false;
                    if (hf == 0) recs[iv[v]].accurate = __builtin_inff();
                    ++rejected;
                }
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (exact[v] && hf == 0) queue[atomicAdd(&qn, 1u)] = iv[v];  // at most 127 waiting + 128 V new
        __syncthreads();
        uint32_t waiting = qn;  // the same value in every thread: nobody touches qn before the next barrier
        __syncthreads();
        if (waiting >= 128) {  // block-uniform
            do {  // (V = 1: at most 255 were waiting, one pass; written so, the loop costs that kernel no registers)
                exact_of(queue[waiting - 128 + pair]);
                waiting -= 128;
            } while (V > 1 && waiting >= 128);
            // nothing is pushed while the passes run, so one barrier after the last orders every read of the queue's entries
            // above `waiting` (and thread 0's qn) ahead of the next round's pushes, which reuse them
            if (threadIdx.x == 0) qn = waiting;
            __syncthreads();
        }
        if constexpr (P::RING) pol.ring_slot ^= 1u;
    }
    if (pair < qn) exact_of(queue[pair]);
    uint32_t rj = hf == 0 ? rejected : 0u;  // per-query counter (one address per query: no hot spot)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) rj += __shfl_xor(rj, o, 64);
    if ((threadIdx.x & 63) == 0 && rj) atomicAdd(&nshadow[b], rj);
}

// Shadow rows of 16-bit elements (fp16 rows, or the first plane of a split row): dt = ||x~ - q||^2 and nx = ||x~||^2 by a pair of
// lanes, x = the row + 8*hf elements; widen(16 bytes of the row, xe) gives their 8 elements as f32.
template <class Widen>
__device__ __forceinline__ void shadow16_bound(const uint16_t *__restrict__ x, const float *q_lds, uint32_t dim, uint32_t hf, Widen widen,
                                               float &dt, float &nx) {
    float d0 = 0.0f, d1 = 0.0f, n0 = 0.0f, n1 = 0.0f;
    for (uint32_t c = 0; c < dim; c += 128) {  // 256 bytes of the row: 8 x 16 bytes per lane in flight
        uint4 xv[8];
        const bool full = dim - c >= 128;  // dim is a multiple of 64: the last chunk may be a half one
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (u < 4 || full) xv[u] = *reinterpret_cast<const uint4 *>(x + c + 16 * u);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (!(u < 4 || full)) continue;
            const float4 qa = *reinterpret_cast<const float4 *>(q_lds + c + 16 * u + 8 * hf);
            const float4 qb = *reinterpret_cast<const float4 *>(q_lds + c + 16 * u + 8 * hf + 4);
            float xe[8];
            widen(xv[u], xe);
            const float e0 = xe[0] - qa.x, e1 = xe[1] - qa.y, e2 = xe[2] - qa.z, e3 = xe[3] - qa.w;
            const float e4 = xe[4] - qb.x, e5 = xe[5] - qb.y, e6 = xe[6] - qb.z, e7 = xe[7] - qb.w;
            d0 = fmaf(e0, e0, d0), d1 = fmaf(e1, e1, d1), d0 = fmaf(e2, e2, d0), d1 = fmaf(e3, e3, d1);
            d0 = fmaf(e4, e4, d0), d1 = fmaf(e5, e5, d1), d0 = fmaf(e6, e6, d0), d1 = fmaf(e7, e7, d1);
            n0 = fmaf(xe[0], xe[0], n0), n1 = fmaf(xe[1], xe[1], n1), n0 = fmaf(xe[2], xe[2], n0), n1 = fmaf(xe[3], xe[3], n1);
            n0 = fmaf(xe[4], xe[4], n0), n1 = fmaf(xe[5], xe[5], n1), n0 = fmaf(xe[6], xe[6], n0), n1 = fmaf(xe[7], xe[7], n1);
        }
    }
    dt = d0 + d1, nx = n0 + n1;
    dt += __shfl_xor(dt, 1, 2), nx += __shfl_xor(nx, 1, 2);
}

struct ShadowHalf {  // fp16 rows beside the f32 ones (untiered, plain)
    static constexpr bool RING = false;
    static constexpr int V = 1;
    const float *base;
    const _Float16 *base_h;
    uint32_t dim;
    __device__ __forceinline__ void stage(float *, uint32_t) const {}
    __device__ __forceinline__ void bound(const SurvRec (&cur)[1], const float *q_lds, uint32_t hf, float up, float (&dt)[1], float (&err)[1]) const {
        float nx;
        shadow16_bound(reinterpret_cast<const uint16_t *>(base_h + (uint64_t)cur[0].pos * dim) + 8 * hf, q_lds, dim, hf,
                       [](const uint4 w, float (&xe)[8]) {
                           const rq_half8 h = __builtin_bit_cast(rq_half8, w);
#pragma unroll
                           for (int e = 0; e < 8; ++e) xe[e] = (float)h[e];
                       },
                       dt[0], nx);
        const float abs_err = sqrtf((float)dim) * 3.0e-8f;  // sqrt(dim) * 2^-25, rounded up
        err[0] = (sqrtf(nx) * up) * 4.8877e-4f + abs_err;  // >= 2^-11 (1 + 2^-10) ||x~|| + sqrt(dim) 2^-25 >= ||x - x~||
#ifdef RQ_EXP_SHADOW_SLACK  // developer experiment (scripts/exp/shadow_slack.sh, rerank_shadow = 1): what a coarser shadow would still reject
        err[0] += RQ_EXP_SHADOW_SLACK;
#endif
    }
    __device__ __forceinline__ float exact(const SurvRec &r, const float *q_lds, uint32_t hf) const {
        return exact_l2_pair(base + (uint64_t)r.pos * dim + 4 * hf, q_lds, dim, hf);
    }
};
__global__ __launch_bounds__(256) void accurate_filtered_kernel(SurvRec *__restrict__ surv,
                                                                const unsigned long long *__restrict__ surv_cnt,
                                                                const QSeg seg, const float *__restrict__ base,
                                                                const _Float16 *__restrict__ base_h,
                                                                const float *__restrict__ qpad, uint32_t dim,
                                                                const uint32_t *__restrict__ order,
                                                                const float *__restrict__ thr_start,
                                                                uint32_t *__restrict__ nshadow) {
    ShadowHalf pol{base, base_h, dim};
    rerank_prefiltered(pol, surv, surv_cnt, seg, qpad, dim, order, thr_start, nshadow);
}

// ------------------------------------------------------------------------------------------------
// Rerank over SPLIT rows (common.h: indexes whose raw vectors leave no room for shadow rows -- tiered ones, and untiered ones that
// fill most of the HBM): the
// first plane of a split row IS one: x^ = the row rounded to bf16, ||x - x^|| <= 2^-8 / (1 - 2^-8) ||x^|| (+ 2^-134 per subnormal
// element).  Same test as accurate_filtered_kernel's with that error term; a survivor it cannot reject has its second plane fetched
// and the words restored exactly, so results are bit-identical to the plain layout's.  Host-tier rows are split rows too (half
// the bytes over the host link for the ones the test rejects).  2*dim bytes per survivor instead of 4*dim for the ones the test rejects.
// ------------------------------------------------------------------------------------------------
struct ShadowPlane {
    static constexpr bool RING = false;
    static constexpr int V = 1;
    const BaseView &base;       // (the kernel's argument itself: its fields stay scalar operands)
    const uint32_t *probe_row;  // the query's probed lists, by slot
    uint32_t nprobe, dim;
    const ListTier *ltl;        // their tier records in LDS, when they fit (launch: LDS for them only then; an untiered index has none)
    __device__ __forceinline__ void stage(float *behind, uint32_t b) {
        probe_row += (uint64_t)b * nprobe;
        if (base.host == nullptr || nprobe > RQ_ACC8_LDS_PROBES) return;
        ListTier *l = reinterpret_cast<ListTier *>(behind);
        for (uint32_t sl = threadIdx.x; sl < nprobe; sl += 256)  // (a padded probe slot -- id 0xFFFFFFFF, "no list" -- has no survivors and no record)
            l[sl] = probe_row[sl] < base.k ? base.lt[probe_row[sl]] : ListTier{0u, 0u, 0u, 0u};
        ltl = l;
    }
    __device__ __forceinline__ RowRef row_of(const SurvRec &r) const {
        if (!base.host) return RowRef{base.dev + (uint64_t)r.pos * dim, base.split != 0};
        return base.row_in_list(r.pos, ltl ? ltl[r.slot] : base.lt[probe_row[r.slot]], dim);
    }
    __device__ __forceinline__ void bound(const SurvRec (&cur)[1], const float *q_lds, uint32_t hf, float up, float (&dt)[1], float (&err)[1]) const {
        const RowRef rr = row_of(cur[0]);
        dt[0] = 0.0f, err[0] = __builtin_inff();
        if (!rr.split) return;  // a plain row has no first plane: exact
        float nx;
        shadow16_bound(reinterpret_cast<const uint16_t *>(rr.p) + 8 * hf, q_lds, dim, hf,
                       [](const uint4 w, float (&xe)[8]) {
                           xe[0] = __builtin_bit_cast(float, w.x << 16), xe[1] = __builtin_bit_cast(float, w.x & 0xFFFF0000u);
                           xe[2] = __builtin_bit_cast(float, w.y << 16), xe[3] = __builtin_bit_cast(float, w.y & 0xFFFF0000u);
                           xe[4] = __builtin_bit_cast(float, w.z << 16), xe[5] = __builtin_bit_cast(float, w.z & 0xFFFF0000u);
                           xe[6] = __builtin_bit_cast(float, w.w << 16), xe[7] = __builtin_bit_cast(float, w.w & 0xFFFF0000u);
                       },
                       dt[0], nx);
        // >= 2^-8 / (1 - 2^-8) ||x^|| + sqrt(dim) 2^-134 >= ||x - x^||  (3.9216e-3 > 2^-8 / (1 - 2^-8) = 3.92157e-3; an
        // x^ with an infinite element makes err infinite and t NaN or -inf: no rejection)
        err[0] = (sqrtf(nx) * up) * 3.9216e-3f + 1.0e-37f;
    }
    __device__ __forceinline__ float exact(const SurvRec &r, const float *q_lds, uint32_t hf) const { return exact_l2_row_f32(row_of(r), q_lds, dim, hf); }
};
__global__ __launch_bounds__(256) void accurate_split_kernel(SurvRec *__restrict__ surv,
                                                             const unsigned long long *__restrict__ surv_cnt,
                                                             const QSeg seg, const BaseView base,
                                                             const float *__restrict__ qpad, uint32_t dim,
                                                             const uint32_t *__restrict__ order,
                                                             const float *__restrict__ thr_start,
                                                             const uint32_t *__restrict__ probe_cluster, uint32_t nprobe,
                                                             uint32_t *__restrict__ nshadow) {
    ShadowPlane pol{base, probe_cluster, nprobe, dim, nullptr};
    rerank_prefiltered(pol, surv, surv_cnt, seg, qpad, dim, order, thr_start, nshadow);
}

// ------------------------------------------------------------------------------------------------
// The 8-bit shadow (round 4): one BYTE per dimension instead of the fp16 shadow's two.
//
// Every list c has an affine map of its own, x^_i = lo_c + s_c * code_i with lo_c = the smallest and lo_c + 255 s_c = the largest
// coordinate of any of its rows (q8_range_kernel), so no coordinate clips and |x_i - x^_i| <= s_c / 2 up to rounding.  The bound
// the pre-filter needs, ||x - x^|| over the rows of the list, is not derived but MEASURED while the codes are written
// (q8_encode_kernel: the largest row norm of x - fmaf(s_c, code, lo_c) over the list, x^ evaluated exactly as the re-ranker evaluates
// it -- round 5; for dimensions whose rows do not map onto a power-of-two thread group: the largest |x_i - x^_i| times sqrt(dim)).
// The test itself is accurate_filtered_kernel's: d^ = ||x^ - q|| in f32, t = d^ (1 - eps) - err, and a survivor is
// dropped only if t^2 (1 - eps) still exceeds the stage's threshold -- the f32 row is then never read (128 instead of 256 shadow
// bytes per survivor at dim 128; measured on the benchmark mixture: 86 % of the survivors rejected against the fp16 shadow's 92 %).
// A list with a non-finite coordinate gets err = inf: nothing of it is ever rejected.
// ------------------------------------------------------------------------------------------------
// whether q8_encode_kernel measures row norms of the error (list_q8[c].w) for this dimension: its dim / 16 threads per row must be
// a power-of-two group inside one wave
__host__ __device__ __forceinline__ bool q8_row_norms(uint32_t dim) {
    const uint32_t tpr = dim / 16;
    return tpr >= 1 && tpr <= 64 && (tpr & (tpr - 1)) == 0;
}
// one block per list: lo, s (and the error accumulator cleared)
__global__ __launch_bounds__(256) void q8_range_kernel(const float *__restrict__ base, const uint32_t *__restrict__ offsets, uint32_t dim,
                                                       float4 *__restrict__ list_q8) {
    __shared__ float smn[4], smx[4];
    __shared__ uint32_t sbad[4];
    const uint32_t c = blockIdx.x;
    const uint64_t e0 = (uint64_t)offsets[c] * dim, e1 = (uint64_t)offsets[c + 1] * dim;
    float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
    uint32_t bad = 0;
    for (uint64_t e = e0 + threadIdx.x * 4ull; e < e1; e += 1024) {  // dim is a multiple of 64: rows are whole float4s
        const float4 v = *reinterpret_cast<const float4 *>(base + e);
        const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!(fabsf(ve[i]) < 3.0e38f)) bad = 1;  // NaN / inf / huge
            mn = ve[i] < mn ? ve[i] : mn;
            mx = ve[i] > mx ? ve[i] : mx;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
        mn = a < mn ? a : mn, mx = b > mx ? b : mx;
        bad |= __shfl_xor(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) smn[threadIdx.x >> 6] = mn, smx[threadIdx.x >> 6] = mx, sbad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) mn = smn[w] < mn ? smn[w] : mn, mx = smx[w] > mx ? smx[w] : mx, bad |= sbad[w];
        float lo = mn, sc = (mx - mn) * (1.0f / 255.0f);
        if (e1 == e0) lo = 0.0f, sc = 1.0f;
        if (!(sc > 0.0f)) sc = 1.0f;                       // all coordinates equal (or an empty list): code 0 everywhere
        if (!(sc < 3.0e38f) || !(fabsf(lo) < 3.0e38f)) bad = 1;
        // .z: the largest |x_i - x^_i| of the list as the bits of a non-negative float (atomicMax by q8_encode_kernel); inf: never reject
        list_q8[c] = make_float4(bad ? 0.0f : lo, bad ? 1.0f : sc, bad ? __builtin_inff() : 0.0f, bad ? __builtin_inff() : 0.0f);  // .w: the largest row norm of the error, likewise
    }
}
// grid (ceil(longest list / 256), k): 256 rows of one list per block; dim / 16 threads per row, 16 codes (one 16-byte store) each
__global__ __launch_bounds__(256) void q8_encode_kernel(const float *__restrict__ base, const uint32_t *__restrict__ offsets, uint32_t dim,
                                                        float4 *__restrict__ list_q8, uint8_t *__restrict__ out) {
    __shared__ float smax[4], snorm[4];
    const uint32_t c = blockIdx.y, r0 = offsets[c] + blockIdx.x * 256u, r1 = offsets[c + 1];
    if (r0 >= r1) return;
    const float4 par = list_q8[c];
    const float lo = par.x, sc = par.y, inv = 1.0f / sc;
    const uint32_t tpr = dim / 16, rows_per_pass = 256 / tpr;  // dim <= 4096
    const uint32_t rr = threadIdx.x / tpr, g = threadIdx.x - rr * tpr;
    const bool row_norms = q8_row_norms(dim);  // the tpr threads of a row are an aligned power-of-two group of one wave
    float emax = 0.0f, nmax = 0.0f;
    for (uint32_t r = r0 + rr; r < r1 && r < r0 + 256u && rr < rows_per_pass; r += rows_per_pass) {
        float e2 = 0.0f;
        const float *x = base + (uint64_t)r * dim + 16 * g;
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 v = *reinterpret_cast<const float4 *>(x + 4 * u);
            const float ve[4] = {v.x, v.y, v.z, v.w};
            w[u] = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float t = rintf((ve[i] - lo) * inv);
                t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);  // (NaN: a list with one has err = inf already)
                const uint32_t code = (uint32_t)t;
                const float e = fabsf(ve[i] - fmaf(sc, (float)code, lo));  // exactly the re-ranker's x^
                emax = (e > emax || !(e < 3.0e38f)) ? (e < 3.0e38f ? e : __builtin_inff()) : emax;
                e2 = fmaf(e, e, e2);
                w[u] |= code << (8 * i);
            }
        }
        *reinterpret_cast<uint4 *>(out + (uint64_t)r * dim + 16 * g) = make_uint4(w[0], w[1], w[2], w[3]);
        if (row_norms) {  // ||x - x^||^2 of the row: the group's partial sums folded (every thread of the group is in this iteration)
            for (uint32_t o = tpr >> 1; o >= 1; o >>= 1) e2 += __shfl_xor(e2, (int)o, 64);
            nmax = (e2 > nmax || !(e2 < 3.0e38f)) ? (e2 < 3.0e38f ? e2 : __builtin_inff()) : nmax;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float a = __shfl_xor(emax, o, 64), b = __shfl_xor(nmax, o, 64);
        emax = a > emax ? a : emax, nmax = b > nmax ? b : nmax;
    }
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = emax, snorm[threadIdx.x >> 6] = nmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w2 = 1; w2 < 4; ++w2) emax = smax[w2] > emax ? smax[w2] : emax, nmax = snorm[w2] > nmax ? snorm[w2] : nmax;
        atomicMax(reinterpret_cast<unsigned int *>(&list_q8[c].z), __builtin_bit_cast(unsigned int, emax));  // non-negative floats order as their bits
        // .w: the largest ||x - x^|| over the list's rows, rounded up past the f32 evaluation above (dim fused multiply-adds + a sqrt)
        const float nrm = sqrtf(nmax) * (1.0f + (float)(dim + 8) * 6.0e-8f);
        if (row_norms) atomicMax(reinterpret_cast<unsigned int *>(&list_q8[c].w), __builtin_bit_cast(unsigned int, nrm));
    }
}

// The test quantities of the V survivors of a lane pair from their 8-bit rows: piece(v, g) = the 16 codes of group g (dimensions
// 16 g .. 16 g + 15) of survivor v's row, par[v] = its list's map.  Lane half hf takes the groups 2u + hf; the pieces of every survivor
// are requested before any is used.  ONE copy of the arithmetic: whatever route the bytes take, the decisions are the same.
template <int V, class Piece>
__device__ __forceinline__ void q8_bound(const float4 (&par)[V], Piece piece, const float *q_lds, uint32_t dim, uint32_t hf, float up,
                                         float (&dt)[V], float (&err)[V]) {
    const uint32_t ngrp = dim / 16;
    float d0[V], d1[V];
#pragma unroll
    for (int v = 0; v < V; ++v) d0[v] = 0.0f, d1[v] = 0.0f;
    for (uint32_t g0 = hf; g0 < ngrp; g0 += 8) {  // four 16-byte pieces of each row in flight per lane
        uint4 cv[V][4];
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (g0 + 2 * u < ngrp) cv[v][u] = piece(v, g0 + 2 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!(g0 + 2 * u < ngrp)) continue;
            const float *q = q_lds + 16 * (g0 + 2 * u);
#pragma unroll
            for (int wi = 0; wi < 4; ++wi) {
                const float4 qa = *reinterpret_cast<const float4 *>(q + 4 * wi);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const uint32_t wv = wi == 0 ? cv[v][u].x : (wi == 1 ? cv[v][u].y : (wi == 2 ? cv[v][u].z : cv[v][u].w));
                    const float e0 = fmaf(par[v].y, (float)(wv & 255u), par[v].x) - qa.x;
                    const float e1 = fmaf(par[v].y, (float)((wv >> 8) & 255u), par[v].x) - qa.y;
                    const float e2 = fmaf(par[v].y, (float)((wv >> 16) & 255u), par[v].x) - qa.z;
                    const float e3 = fmaf(par[v].y, (float)(wv >> 24), par[v].x) - qa.w;
                    d0[v] = fmaf(e0, e0, d0[v]), d1[v] = fmaf(e1, e1, d1[v]), d0[v] = fmaf(e2, e2, d0[v]), d1[v] = fmaf(e3, e3, d1[v]);
                }
            }
            // (the query pieces of the later groups are read when their turn comes: hoisted, the sixteen 16-byte LDS reads of
            // a round held 64 registers and cost the kernel a wave per SIMD)
            asm volatile("" ::: "memory");
        }
    }
    const float sqd = sqrtf((float)dim) * 1.001f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        dt[v] = d0[v] + d1[v];
        dt[v] += __shfl_xor(dt[v], 1, 2);
        // >= ||x - x^||: the largest row norm of the error measured over the list (dimensions q8_encode_kernel measures it for),
        // else sqrt(dim) max |x_i - x^_i|   (inf: a list that is never rejected)
        err[v] = q8_row_norms(dim) ? par[v].w * up : (par[v].z * up) * sqd;
    }
}

// accurate_filtered_kernel with the 8-bit shadow: two survivors per lane pair (lane half hf takes the 16-dimension groups 2u + hf of
// a row; both survivors' pieces are requested before either is used: a 128-byte row is four 16-byte loads per lane, too few in
// flight to keep the memory busy one row at a time)
struct ShadowQ8 {
    static constexpr int V = 2;
    static constexpr bool RING = false;
    const float *base;
    const uint8_t *base_q8;
    const float4 *list_q8;      // per list: lo, s, max |x_i - x^_i|, max ||x - x^||
    const uint32_t *probe_row;  // the query's probed lists, by slot
    uint32_t nprobe, nlists, dim;
    const float4 *lpar;         // the probed lists' maps in LDS, when they fit (launch: LDS for them only then)
    __device__ __forceinline__ void stage(float *behind, uint32_t b) {
        probe_row += (uint64_t)b * nprobe;
        if (nprobe > RQ_ACC8_LDS_PROBES) return;
        float4 *l = reinterpret_cast<float4 *>(behind);
        for (uint32_t sl = threadIdx.x; sl < nprobe; sl += 256)  // (a padded probe slot -- id 0xFFFFFFFF, "no list" -- has no survivors and no map)
            l[sl] = probe_row[sl] < nlists ? list_q8[probe_row[sl]] : make_float4(0.0f, 1.0f, __builtin_inff(), __builtin_inff());
        lpar = l;
    }
    __device__ __forceinline__ void bound(const SurvRec (&cur)[2], const float *q_lds, uint32_t hf, float up, float (&dt)[2], float (&err)[2]) const {
        float4 par[2];
        const uint8_t *x[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            par[v] = lpar ? lpar[cur[v].slot] : list_q8[probe_row[cur[v].slot]];
            x[v] = base_q8 + (uint64_t)cur[v].pos * dim;
        }
        q8_bound<2>(par, [&](int v, uint32_t g) { return *reinterpret_cast<const uint4 *>(x[v] + 16 * g); }, q_lds, dim, hf, up, dt, err);
    }
    __device__ __forceinline__ float exact(const SurvRec &r, const float *q_lds, uint32_t hf) const {
        return exact_l2_pair(base + (uint64_t)r.pos * dim + 4 * hf, q_lds, dim, hf);
    }
};
#ifndef RQ_ACC8_WAVES
#define RQ_ACC8_WAVES 4  // waves per SIMD the register budget is cut for (round 4: 132 registers, three waves; four: rerank 4.76 -> 4.35 ms per step)
#endif
__global__ __launch_bounds__(256, RQ_ACC8_WAVES) void accurate_filtered8_kernel(SurvRec *__restrict__ surv,
                                                                 const unsigned long long *__restrict__ surv_cnt,
                                                                 const QSeg seg, const float *__restrict__ base,
                                                                 const uint8_t *__restrict__ base_q8, const float4 *__restrict__ list_q8,
                                                                 const float *__restrict__ qpad, uint32_t dim,
                                                                 const uint32_t *__restrict__ order,
                                                                 const float *__restrict__ thr_start,
                                                                 const uint32_t *__restrict__ probe_cluster, uint32_t nprobe,
                                                                 uint32_t *__restrict__ nshadow, uint32_t nlists) {
    ShadowQ8 pol{base, base_q8, list_q8, probe_cluster, nprobe, nlists, dim, nullptr};
    rerank_prefiltered(pol, surv, surv_cnt, seg, qpad, dim, order, thr_start, nshadow);
}

// ------------------------------------------------------------------------------------------------
// The 8-bit shadow rows through an LDS ring (dimensions 64 .. 256).  In accurate_filtered8_kernel a round's loads and its arithmetic
// are serialised inside every wave (request 8 pieces per lane, wait, ~400 VALU instructions per 64 survivors, barriers), and a wave load touches 32
// rows for 32 bytes each.  Here a wave copies the rows of ITS OWN 32 lane pairs into LDS with global_load_lds_dwordx4 (glds16): NPC =
// dim / 16 consecutive lanes fetch one row, so a request covers whole rows, one instruction lands 1 KiB, and no register holds the
// bytes on the way.  Each wave owns two slots of 32 V rows; the copies of round r + 1 are issued before round r is tested and stay in
// flight under it.  The slots are private to the wave, so what orders a read behind the copies is the wave's own counted
// s_waitcnt vmcnt (ring_wait: the copies just issued are the youngest requests, everything older has landed) and nothing else: no
// barrier is added, and a slot is refilled a round after the values read from it were consumed.
// Row r of a wave's slot lies at 16 NPC r; its 16-byte piece g lies at position q8_ring_piece(r, g): the lane groups of ds_read_b128
// (16 lanes = 8 lane pairs, which read the same piece index of 8 different rows) would otherwise meet on the same banks 2 (dim 64),
// 4 (128) or 8 (256) times over; the copying lane picks the piece it fetches, so the exchange costs nothing.  (dim 192: 12 pieces do
// not exchange by xor; left as it is, two-way.)
// The arithmetic is q8_bound, the one accurate_filtered8_kernel runs: decisions, counters and outputs are the same bit for bit.
// ------------------------------------------------------------------------------------------------
template <int NPC>
__device__ __forceinline__ uint32_t q8_ring_piece(uint32_t r, uint32_t g) {
    if constexpr (NPC == 4) return g ^ (2u * ((r >> 2) & 1u));
    if constexpr (NPC == 8) return g ^ (2u * ((r >> 1) & 3u));
    if constexpr (NPC == 16) return g ^ (2u * (r & 7u));
    return g;
}
__host__ __device__ constexpr uint32_t q8_ring_bytes(uint32_t v, uint32_t dim) { return 2u * 4u * 32u * v * dim; }  // two slots, four waves, 32 v rows each
template <int VV, int NPC>
struct ShadowQ8Ring : ShadowQ8 {
    static constexpr int V = VV;
    static constexpr bool RING = true;
    static constexpr uint32_t DIM = 16u * NPC, WAVE_BYTES = 32u * VV * DIM, SLOT_BYTES = 4u * WAVE_BYTES, NI = VV * NPC / 2;  // NI: copies per wave and round
    uint32_t rows;         // this lane pair's first row in slot 0, in bytes from the start of the dynamic LDS
    uint32_t wave_lds;     // LDS byte address of this wave's part of slot 0 (wave-uniform)
    uint32_t ring_slot;    // the slot the current round reads
    __device__ __forceinline__ void stage(float *behind, uint32_t b) {
        ShadowQ8::stage(behind, b);  // (the launch rule keeps nprobe <= RQ_ACC8_LDS_PROBES: the maps are in LDS)
        const uint32_t ring = 4u * DIM + 16u * nprobe, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        wave_lds = lds_addr(dyn()) + ring + wave * WAVE_BYTES;
        rows = ring + wave * WAVE_BYTES + ((threadIdx.x & 63u) >> 1) * DIM;
    }
    // The block's dynamic LDS, named here so that every read below is an LDS read to the compiler: through the generic pointers of
    // ShadowQ8 (lpar) it emits FLAT loads, which count on vmcnt too -- waiting for one would drain the copies in flight.
    __device__ __forceinline__ static const uint8_t *dyn() {
        extern __shared__ __attribute__((aligned(16))) uint8_t rq_ring_lds[];
        return rq_ring_lds;
    }
    // the rows of the records nx (lane pair p holds the records of rows p and, V = 2, 32 + p) -> slot
    __device__ __forceinline__ void ring_issue(const SurvRec (&nx)[VV], uint32_t slot) const {
        const uint32_t lane = threadIdx.x & 63u, dst = wave_lds + slot * SLOT_BYTES;
#pragma unroll
        for (uint32_t j = 0; j < NI; ++j) {
            const uint32_t v = j / (NPC / 2), at = 64u * (j % (NPC / 2)) + lane, r = at / NPC, p = at % NPC;  // position p of row r (of survivor v)
            const uint32_t pos = (uint32_t)__shfl((int)nx[v < VV ? v : 0].pos, (int)(2u * r), 64);
            glds16(base_q8 + (uint64_t)pos * DIM + 16u * q8_ring_piece<NPC>(r, p), dst + 1024u * j);
        }
    }
    // everything but the NI copies just issued has landed (requests return in order); none issued: everything has
    __device__ __forceinline__ void ring_wait(bool issued) const {
        if (issued) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __device__ __forceinline__ void bound(const SurvRec (&cur)[VV], const float *q_lds, uint32_t hf, float up, float (&dt)[VV], float (&err)[VV]) const {
        float4 par[VV];
#pragma unroll
        for (int v = 0; v < VV; ++v) par[v] = reinterpret_cast<const float4 *>(dyn() + 4u * DIM)[cur[v].slot];
        const uint8_t *x = dyn() + rows + ring_slot * SLOT_BYTES;
        const uint32_t r = (threadIdx.x & 63u) >> 1;
        q8_bound<VV>(par, [&](int v, uint32_t g) { return *reinterpret_cast<const uint4 *>(x + v * (32u * DIM) + 16u * q8_ring_piece<NPC>(r, g)); },
                     q_lds, DIM, hf, up, dt, err);
    }
};
// Geometry, by measurement on the headline workload (profiles/rerank_ring_ab_runs.txt): one survivor per lane pair and round -- 16 dim
// bytes of ring per wave, four blocks per CU at dim 128 as in accurate_filtered8_kernel -- beat the parent; two per pair (two blocks
// per CU) lost to it.  The register budget follows the blocks the ring's LDS leaves room for.
#ifndef RQ_RING_V
#define RQ_RING_V 1
#endif
__host__ __device__ constexpr int q8_ring_waves(int npc) { return npc <= 8 ? 4 : 2; }
template <int VV, int NPC>
__global__ __launch_bounds__(256, q8_ring_waves(NPC)) void accurate_ring8_kernel(SurvRec *__restrict__ surv, const unsigned long long *__restrict__ surv_cnt,
                                                             const QSeg seg, const float *__restrict__ base,
                                                             const uint8_t *__restrict__ base_q8, const float4 *__restrict__ list_q8,
                                                             const float *__restrict__ qpad, const uint32_t *__restrict__ order,
                                                             const float *__restrict__ thr_start,
                                                             const uint32_t *__restrict__ probe_cluster, uint32_t nprobe,
                                                             uint32_t *__restrict__ nshadow, uint32_t nlists) {
    ShadowQ8Ring<VV, NPC> pol;
    pol.base = base, pol.base_q8 = base_q8, pol.list_q8 = list_q8, pol.probe_row = probe_cluster, pol.nprobe = nprobe, pol.nlists = nlists;
    pol.dim = 16u * NPC, pol.lpar = nullptr;
    rerank_prefiltered(pol, surv, surv_cnt, seg, qpad, 16u * NPC, order, thr_start, nshadow);
}

// ---- the same three phases as separate launches: better for large batches, where all queries'
// survivors are reranked with full-chip parallelism before the (latency-bound) replay --------------
// grid (gx, nq); block 256
// KIND: the row kind of the index (accurate_rows<KIND>); the launch picks the instantiation (host_query.h: with_row_kind)
template <int KIND>
__global__ __launch_bounds__(256) void accurate_kernel(SurvRec *__restrict__ surv,
                                                       const unsigned long long *__restrict__ surv_cnt,
                                                       const QSeg seg, const BaseView base,
                                                       const float *__restrict__ qpad, uint32_t dim,
                                                       const uint32_t *__restrict__ order,
                                                       const uint32_t *__restrict__ probe_cluster, uint32_t nprobe) {
    // TWO lanes per candidate: lane half hf carries AVX lanes 4hf..4hf+3 (elements 8c + 4hf + 0..3, one
    // 16-byte load per chunk), so a row is fetched with float4 loads; the fold
    // ((a0+a4)+(a1+a5)) + ((a2+a6)+(a3+a7)) needs one exchange between the two lanes.
    extern __shared__ __attribute__((aligned(16))) float acc_q[];  // dynamic LDS: dim floats (the padded query)
    const uint32_t b = order ? order[blockIdx.y] : blockIdx.y;  // consecutive blocks: queries of the same nearest list
    const uint32_t n = (uint32_t)surv_cnt[b];
    if (n > seg.capof(b) || n == 0) return;  // overflowed: this query is re-run with a larger buffer
    for (uint32_t c = threadIdx.x * 4; c < dim; c += 1024)
        *reinterpret_cast<float4 *>(acc_q + c) = *reinterpret_cast<const float4 *>(qpad + (uint64_t)b * dim + c);
    __syncthreads();
    accurate_rows<KIND>(surv + seg.at(b), n, base, acc_q, dim, blockIdx.x * 128 + (threadIdx.x >> 1), gridDim.x * 128,
                        probe_cluster + (uint64_t)b * nprobe);
}

