// kernels_query.h -- gfx950 kernels of RaBitQ::query (src/rabitq.rs:268-367) around the scan: what prepares a stage and
// what moves its survivors.  The stages themselves live in headers of their own, included here in pipeline order:
//   kernels_coarse.h   the coarse ranking (src/rabitq.rs:283-297)
//   kernels_scan_*.h   the scan (translation units of their own; kernels_scan_common.h: the record layout shared with them)
//   kernels_rerank.h   exact distances of the survivors (src/rerank.rs:85-90)
//   kernels_replay.h   the survivors' visiting order, the replay of the reference's rankers, the result writers
// In this file: query padding and the VALU rotation, the shard merge, the per-(query, list) quantisation (prep_*), the
// candidate stream's prefix sums (pair_prefix_*), the filter bitmaps, a stage's work lists (group_*, stage_fill_*,
// stage_tail_kernel), the generic-width and dense scans; behind the includes: the rerank order of a large batch (order_*), the
// survivor arena (seg_exact / arena_scatter / seg_scan), the dense directory's clear and the scan's step counters (stat_fold).
//
// Mapping (MI355X-first, not a translation of the reference's per-vector SIMD loop): candidates live one per lane in VGPRs,
// queries stream through the scalar unit -- every per-query operand is wave-uniform and reaches the VALU as an SGPR operand --
// and a list is read from HBM once per launch for every query of the batch that probes it.  The scan emits only the survivors
// of the per-query re-rank threshold; exact f32 distances are computed for those alone; an ordered replay of the reference's
// heap logic over (rough, accurate) pairs reproduces its result id for id.
#pragma once
#include "common.h"
#include "kernels_scan_common.h"
#include "kernels_coarse.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// zero-pad queries to the padded dimension (src/rabitq.rs:277-280)
// ------------------------------------------------------------------------------------------------
__global__ void pad_rows_kernel(const float *__restrict__ in, float *__restrict__ out, uint64_t n,
                                uint32_t len, uint32_t dim) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * dim) return;
    uint64_t r = i / dim;
    uint32_t c = (uint32_t)(i - r * dim);
    out[i] = c < len ? in[r * len + c] : 0.0f;
}

// ------------------------------------------------------------------------------------------------
// Rotation, VALU form: out[r][j] = vector_dot_product(x[r], P[:, j]) in the exact AVX2 order
// (src/utils.rs:237-258 -> src/simd.rs:257-314): 8 accumulators acc[l] = fma(x[8c+l], P[8c+l][j],
// acc[l]) over chunks c, then the fixed fold.  block (64,4): lane <-> column j (coalesced P reads),
// x[r][*] is a wave-uniform broadcast.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rotate_valu_kernel(const float *__restrict__ x,
                                                          const float *__restrict__ P,
                                                          float *__restrict__ out, uint64_t n,
                                                          uint32_t dim) {
    uint64_t r = (uint64_t)blockIdx.x * 4 + threadIdx.y;
    uint32_t j = blockIdx.y * 64 + threadIdx.x;
    if (r >= n) return;
    const float *xr = x + r * dim;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t c = 0; c < dim; c += 8) {
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[l] = fmaf(xr[c + l], P[(uint64_t)(c + l) * dim + j], acc[l]);
    }
    out[r * dim + j] = reduce8_regs(acc);
}

// ------------------------------------------------------------------------------------------------
// Shard merge (multi-GPU fan-out): per query, the m_out smallest of the `world` x `width` u64 keys the ranks
// contributed (all-gathered as in[world][nq][width], rows in any order), ascending.  Used for the probe lists
// (key = distance bits << 32 | list id) and for the per-shard top-k (key = Ord32 image << 32 | global id).
// One block per query, LDS bitonic sort; dynamic LDS: pow2_ceil(world * width) * 8 bytes.
// ------------------------------------------------------------------------------------------------
// rank_stride: keys between the blocks of consecutive ranks (nq * width, or more when a rank's block carries trailing words).
__global__ __launch_bounds__(256) void merge_smallest_u64_kernel(const unsigned long long *__restrict__ in, uint32_t world,
                                                                 uint32_t nq, uint32_t width, uint32_t m_out,
                                                                 unsigned long long *__restrict__ out, uint64_t rank_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char merge_smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(merge_smem);
    const uint32_t b = blockIdx.x, m = world * width;
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
        const uint32_t w = i / width, e = i - w * width;
        keys[i] = in[(uint64_t)w * rank_stride + (uint64_t)b * width + e];
    }
    __syncthreads();
    bitonic_sort_block(keys, m, [](unsigned long long v) { return v; });
    for (uint32_t i = threadIdx.x; i < m_out; i += blockDim.x) out[(uint64_t)b * m_out + i] = i < m ? keys[i] : ~0ull;
}

// ------------------------------------------------------------------------------------------------
// Per-(query, probed list) query quantisation (src/rabitq.rs:304-317):
//   residual = y - c (src/simd.rs:138), (lo, hi) (:143-157), delta = (hi - lo) * (1/15),
//   q = cvtps_epi32((res - lo) * (1/delta)) (:215, sub then mul, RNE, no bias), sum of q,
//   4 bit planes, bit b of word w <-> dimension 64w + b (:103).
// One wave per pair; lane holds dimensions {lane, 64+lane, ...}; a plane word is one __ballot.
// `pair_cluster[p]` is the list paired with rotated query row `pair_row[p]` (or p / nprobe).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_kernel(const float *__restrict__ y,
                                                   const float *__restrict__ centroids,
                                                   const uint32_t *__restrict__ offsets,
                                                   const uint32_t *__restrict__ pair_cluster,
                                                   const float *__restrict__ pair_ycd, uint32_t npairs,
                                                   uint32_t pairs_per_row, uint32_t dim,
                                                   PairScalars *__restrict__ scal,
                                                   uint64_t *__restrict__ planes,
                                                   uint32_t *__restrict__ qnib,
                                                   uint32_t *__restrict__ qf6,
                                                   uint32_t *__restrict__ out_sum_u32, uint32_t nlists,
                                                   uint32_t skip_empty) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npairs) return;
    const uint32_t row = p / pairs_per_row;
    const uint32_t c = pair_cluster[p];
    const uint32_t len_c = c < nlists ? offsets[c + 1] - offsets[c] : 0u;
    if (len_c == 0 && skip_empty) {  // nothing to scan for this pair (e.g. a list another shard owns)
        if (lane == 0) {
            PairScalars s;
            s.lower = 0.0f, s.delta = 0.0f, s.sumq = 0.0f, s.ycd = pair_ycd[p], s.ycd_sqrt = 0.0f;
            s.row = row, s.list_begin = 0, s.list_len = 0, s.stream_begin = 0, s.pad = 0;
            scal[p] = s;
            if (out_sum_u32) out_sum_u32[p] = 0;
        }
        return;
    }
    const float *yr = y + (uint64_t)row * dim;
    const float *cr = centroids + (uint64_t)c * dim;
    const uint32_t W = dim >> 6;
    float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
    for (uint32_t w = 0; w < W; ++w) {
        float r = yr[64 * w + lane] - cr[64 * w + lane];
        mn = r < mn ? r : mn;
        mx = r > mx ? r : mx;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        float a = __shfl_xor(mn, o, 64), bb = __shfl_xor(mx, o, 64);
        mn = a < mn ? a : mn;
        mx = bb > mx ? bb : mx;
    }
    const float scalar = 1.0f / 15.0f;          // consts.rs:10
    const float delta = (mx - mn) * scalar;     // rabitq.rs:307
    const float one_over_delta = 1.0f / delta;  // :308 f32::recip
    uint32_t sum = 0;
    uint64_t *pl = planes + (uint64_t)p * 4 * W;
    for (uint32_t w = 0; w < W; ++w) {
        float r = yr[64 * w + lane] - cr[64 * w + lane];
        int32_t q = cvtps_epi32((r - mn) * one_over_delta);
        sum += (uint32_t)q;
        if (planes) {
#pragma unroll
            for (int bit = 0; bit < 4; ++bit) {
                uint64_t word = __ballot((q >> bit) & 1);
                if (lane == 0) pl[bit * W + w] = word;
            }
        }
        if (qf6) {  // matrix-core operand: q/2 as fp6 e2m3 (every integer 0..15 is exact), 6-bit fields packed as a
                    // little-endian bit stream; lane half h = lane>>5 of word w <-> the 6 dwords [h][w][0..6)
            const uint32_t v = (uint32_t)q & 15u;
            const uint32_t c6 = v < 4 ? 4 * v : (v < 8 ? 8 + 2 * v : 16 + v);
            const uint32_t i16 = lane & 15, bitpos = 6 * i16, d0 = bitpos >> 5, off = bitpos & 31;
            const uint64_t wide = (uint64_t)c6 << off;
            const uint32_t lo32 = (uint32_t)wide, hi32 = (uint32_t)(wide >> 32);
            uint32_t w0 = d0 == 0 ? lo32 : 0u;
            uint32_t w1 = d0 == 0 ? hi32 : (d0 == 1 ? lo32 : 0u);
            uint32_t w2 = d0 == 1 ? hi32 : (d0 == 2 ? lo32 : 0u);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                w0 |= __shfl_xor(w0, o, 16);
                w1 |= __shfl_xor(w1, o, 16);
                w2 |= __shfl_xor(w2, o, 16);
            }
            if (i16 < 3)
                qf6[(uint64_t)p * 12 * W + (lane >> 5) * 6 * W + 6 * w + 3 * ((lane >> 4) & 1) + i16] =
                    i16 == 0 ? w0 : (i16 == 1 ? w1 : w2);
        }
        if (qnib) {  // the same 4-bit codes packed 8 per dword (dword m <-> dims 8m..8m+7, nibble i <-> dim 8m+i):
                     // the operand form of v_dot8_u32_u4 used by the fused scan kernel
            uint32_t nib = ((uint32_t)q & 15u) << (4 * (lane & 7));
            nib |= __shfl_xor(nib, 1, 8);
            nib |= __shfl_xor(nib, 2, 8);
            nib |= __shfl_xor(nib, 4, 8);
            if ((lane & 7) == 0) qnib[(uint64_t)p * 8 * W + 8 * w + (lane >> 3)] = nib;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) {
        PairScalars s;
        float ycd = pair_ycd[p];
        s.lower = mn;
        s.delta = delta;
        s.sumq = (float)sum;  // rabitq.rs:322 `scalar_sum as f32`
        s.ycd = ycd;
        s.ycd_sqrt = sqrtf(ycd);  // :346
        s.row = row;
        s.list_begin = offsets[c];
        s.list_len = offsets[c + 1] - offsets[c];
        s.stream_begin = 0;  // filled by pair_prefix_kernel
        s.pad = 0;
        scal[p] = s;
        if (out_sum_u32) out_sum_u32[p] = sum;
    }
}

// The same quantisation for dim in {64, 128, 256, 512, 768, 1024} with LP lanes per pair (several pairs per wave
// up to dim 128, R rounds of 256 dimensions from dim 512): every lane
// owns 4 consecutive dimensions (one 16-byte load of y and of the centroid), the reductions take log2(LP)
// shuffle steps, and the operand images come out of one neighbour exchange each: a lane's four 4-bit codes
// are half a qnib dword, its four fp6 fields 24 bits of the 6-dword image of its 32-dimension block.
// Writes the fused scan's operands only (no bit planes); arithmetic identical to prep_kernel.
// The pairs p0, p0 + 64/LP, ... (PP of them) of one lane group; p0 already includes the group's index lane / LP.
// does list [begin, begin+len) of the candidate stream intersect the stage [s_lo, s_hi) ?
__device__ __forceinline__ bool stream_in_stage(uint32_t begin, uint32_t len, uint32_t s_lo, uint32_t s_hi) {
    const uint64_t b = begin, e = b + len;
    return len != 0 && b < s_hi && e > s_lo;
}
#define RQ_RANK_ITEMS 32768u  // work items per block of group_rank_kernel
// The twelve tail dwords of a stage record that do not depend on the query's threshold (t[RQ_REC_THR] is left alone).
__device__ __forceinline__ void stage_tail_static(const PairScalars &ps, bool in, uint32_t slot, uint32_t s_lo, uint32_t s_hi,
                                                  uint32_t *__restrict__ t) {
    uint32_t lo = 0, hi = 0;
    if (in) {
        lo = s_lo > ps.stream_begin ? s_lo - ps.stream_begin : 0u;
        hi = s_hi - ps.stream_begin;  // in-stage => stream_begin < s_hi
        hi = hi < ps.list_len ? hi : ps.list_len;
    }
    t[RQ_REC_LOWER] = __builtin_bit_cast(uint32_t, ps.lower);
    t[RQ_REC_DELTA] = __builtin_bit_cast(uint32_t, ps.delta);
    t[RQ_REC_SUMQ] = __builtin_bit_cast(uint32_t, ps.sumq);
    t[RQ_REC_YCD] = __builtin_bit_cast(uint32_t, ps.ycd);
    t[RQ_REC_YCD_SQRT] = __builtin_bit_cast(uint32_t, ps.ycd_sqrt);
    t[RQ_REC_LO] = lo;
    t[RQ_REC_HI] = hi;
    t[RQ_REC_ROW] = ps.row;
    t[RQ_REC_SLOT] = slot;
    t[RQ_REC_LIST_BEGIN] = ps.list_begin;
    t[RQ_REC_LIST_LEN] = ps.list_len;
}
// Placement of the pass's final (matrix-core) stage, decided BEFORE the quantisation (run_pass, option prep_placement): stream
// positions from the list lengths (pair_prefix_lens_kernel), places inside the lists' groups from group_rank_kernel /
// group_scan_kernel.  The quantisation then writes a pair's fp6 operand row and the threshold-free part of its tail straight
// into the stage's tile image (the place stage_fill_item computes: grp_start[c] + blk_base[block][c] + rank), and
// stage_tail_kernel adds the threshold's part once the early stages have run.  Work item = pair (every slot can be in the stage).
struct PrepPlace {
    const uint32_t *stream_begin;                 // per pair
    const uint32_t *rank, *blk_base, *grp_start;  // rank ~0u: the pair is not in the stage
    uint32_t *img;                                // the final stage's tile images
    uint32_t s_lo, s_hi, tile_images;             // tile_images: 1 = bf16 threshold form, 2 = additive form
};
template <int LP, int R, int PP, bool PLACE = false>
__device__ __forceinline__ void prep_small_pairs(const float *__restrict__ y, const float *__restrict__ centroids,
                                                 const uint32_t *__restrict__ offsets,
                                                 const uint32_t *__restrict__ pair_cluster,
                                                 const float *__restrict__ pair_ycd, uint32_t npairs,
                                                 uint32_t pairs_per_row, PairScalars *__restrict__ scal,
                                                 uint32_t *__restrict__ qnib, uint32_t *__restrict__ qf6,
                                                 uint32_t nlists, uint32_t skip_empty, uint32_t p0,
                                                 const uint32_t *__restrict__ live_list = nullptr /* compacted pair ids (pair_split_kernel): p0 indexes it */,
                                                 uint32_t qn_slots = 0xFFFFFFFFu /* the 4-bit operand is written for probe slots below this only */,
                                                 const PrepPlace &pl = PrepPlace{} /* PLACE: qf6 is not used */) {
    // dim = 4 * LP * R: LP lanes per pair, each owning 4 consecutive dimensions in each of R rounds of 4*LP
    // dimensions (R > 1 only with LP = 64: dim 512, 768, 1024).  Every lane group handles PP pairs: the kernel is a
    // chain of dependent gathers (probe list -> centroid row, list bounds), so the loads of all PP pairs are issued
    // before any of them is consumed.
    static_assert(R >= 1 && (LP == 16 || LP == 32 || LP == 64), "lane groups of 16 / 32 / 64; a round = 4 LP dimensions (the packing's neighbour exchanges stay inside a round)");
    constexpr uint32_t DIM = 4 * LP * R, W = DIM / 64, PPW = 64 / LP;
    const uint32_t lane = threadIdx.x & 63, sub = lane % LP;
    uint32_t cl[PP], lb[PP], ll[PP];
    float ycd_in[PP];
    bool live[PP];
    uint32_t pid[PP];  // the pair each of the PP rounds works on
    uint32_t sbeg[PP], place[PP];  // PLACE: stream position of the pair's list; its place in the final stage (~0u: not in it)
#pragma unroll
    for (int pp = 0; pp < PP; ++pp) {
        const uint32_t pi = p0 + pp * PPW;
        live[pp] = pi < npairs;  // uniform over the pair's LP lanes
        pid[pp] = live_list ? (live[pp] ? live_list[pi] : 0u) : pi;
        const uint32_t p = pid[pp];
        cl[pp] = live[pp] ? pair_cluster[p] : 0xFFFFFFFFu;
        ycd_in[pp] = live[pp] ? pair_ycd[p] : 0.0f;
        sbeg[pp] = 0u, place[pp] = ~0u;
        if constexpr (PLACE) {
            sbeg[pp] = live[pp] ? pl.stream_begin[p] : 0u;
            place[pp] = live[pp] ? pl.rank[p] : ~0u;
        }
    }
    float4 cv[PP][R], yv[PP][R];
#pragma unroll
    for (int pp = 0; pp < PP; ++pp) {
        const uint32_t p = pid[pp], c = cl[pp];
        const bool in = live[pp] && c < nlists;
        lb[pp] = in ? offsets[c] : 0u;
        ll[pp] = in ? offsets[c + 1] - lb[pp] : 0u;
        if constexpr (PLACE) {
            if (in && place[pp] != ~0u) place[pp] += pl.grp_start[c] + pl.blk_base[(uint64_t)(p / RQ_RANK_ITEMS) * nlists + c];
            else place[pp] = ~0u;
        }
        const uint32_t row = live[pp] ? p / pairs_per_row : 0u;
        // skip_empty == 2 (an index with many empty lists: a shard of a multi-GPU deployment, where 7 of 8 probed lists live on
        // other ranks): the query and centroid rows of a pair are only fetched once its list is known to have members -- one more
        // dependent round trip for the pairs that stay, 1 KB less traffic for each that goes
        const bool fetch = skip_empty == 2 ? ll[pp] != 0 : true;
#pragma unroll
        for (int rd = 0; rd < R; ++rd) {
            if (fetch) {
                yv[pp][rd] = *reinterpret_cast<const float4 *>(y + (uint64_t)row * DIM + 4 * LP * rd + 4 * sub);
                cv[pp][rd] = *reinterpret_cast<const float4 *>(centroids + (uint64_t)(in ? c : 0u) * DIM + 4 * LP * rd + 4 * sub);
            } else {
                yv[pp][rd] = make_float4(0.0f, 0.0f, 0.0f, 0.0f), cv[pp][rd] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    }
#pragma unroll
    for (int pp = 0; pp < PP; ++pp) {
        const uint32_t p = pid[pp];
        if (!live[pp]) continue;
        const uint32_t row = p / pairs_per_row;
        if (ll[pp] == 0 && skip_empty) {  // nothing to scan for this pair (e.g. a list another shard owns)
            if (sub == 0) {
                PairScalars s;
                s.lower = 0.0f, s.delta = 0.0f, s.sumq = 0.0f, s.ycd = ycd_in[pp], s.ycd_sqrt = 0.0f;
                s.row = row, s.list_begin = 0, s.list_len = 0, s.stream_begin = sbeg[pp], s.pad = 0;
                scal[p] = s;
            }
            continue;
        }
        // where the fp6 operand row goes: the pair-major buffer, or (PLACE) the pair's row of the final stage's tile image
        uint32_t *q6row = qf6 ? qf6 + (uint64_t)p * 12 * W : nullptr;
        uint32_t *tail_dst = nullptr;
        if constexpr (PLACE) {
            q6row = nullptr;
            if (place[pp] != ~0u) {
                const bool additive = pl.tile_images == 2;
                const uint32_t opld = rq_img_opld(12 * W, additive), at = place[pp];
                uint32_t *base = pl.img + (uint64_t)(at >> 5) * rq_img_dwords(12 * W, additive);
                q6row = base + (at & 31u) * opld;
                tail_dst = base + 32 * opld + (at & 31u) * (additive ? RQ_RECA_TAIL : RQ_REC_TAIL);
            }
        }
        float r[R][4];
        float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
#pragma unroll
        for (int rd = 0; rd < R; ++rd) {
            r[rd][0] = yv[pp][rd].x - cv[pp][rd].x, r[rd][1] = yv[pp][rd].y - cv[pp][rd].y;
            r[rd][2] = yv[pp][rd].z - cv[pp][rd].z, r[rd][3] = yv[pp][rd].w - cv[pp][rd].w;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                mn = r[rd][e] < mn ? r[rd][e] : mn;
                mx = r[rd][e] > mx ? r[rd][e] : mx;
            }
        }
#pragma unroll
        for (int o = LP / 2; o >= 1; o >>= 1) {
            const float a = __shfl_xor(mn, o, LP), bb = __shfl_xor(mx, o, LP);
            mn = a < mn ? a : mn;
            mx = bb > mx ? bb : mx;
        }
        const float scalar = 1.0f / 15.0f;          // consts.rs:10
        const float delta = (mx - mn) * scalar;     // rabitq.rs:307
        const float one_over_delta = 1.0f / delta;  // :308 f32::recip
        uint32_t sum = 0;
#pragma unroll
        for (int rd = 0; rd < R; ++rd) {
            uint32_t nib16 = 0, f24 = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int32_t q = cvtps_epi32((r[rd][e] - mn) * one_over_delta);
                sum += (uint32_t)q;
                const uint32_t v = (uint32_t)q & 15u;
                nib16 |= v << (4 * e);
                f24 |= (v < 4 ? 4 * v : (v < 8 ? 8 + 2 * v : 16 + v)) << (6 * e);  // q/2 as fp6 e2m3
            }
            const uint32_t dsub = LP * rd + sub;  // this lane's 4-dimension group among the dim/4 of the vector
            {  // qnib: dword m <-> dims 8m..8m+7 = groups 2m (low half), 2m+1 (high half)
                const uint32_t other = __shfl_xor(nib16, 1, LP);
                if (qnib && (sub & 1) == 0 && p - row * pairs_per_row < qn_slots) qnib[(uint64_t)p * 8 * W + (dsub >> 1)] = nib16 | (other << 16);
            }
            {  // qf6: group t = dsub % 8 of a 32-dimension block holds stream bits [24t, 24t+24) of its 6 dwords
                const uint32_t nxt = __shfl_down(f24, 1, LP);
                const uint32_t t = dsub & 7, sh = 8 * (t & 3);
                if (q6row && (t & 3) != 3) {
                    const uint32_t w = dsub >> 4, h = (dsub >> 3) & 1;
                    q6row[h * 6 * W + 6 * w + 3 * (t >> 2) + (t & 3)] = (f24 >> sh) | (nxt << (24 - sh));
                }
            }
        }
#pragma unroll
        for (int o = LP / 2; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, LP);
        if (sub == 0) {
            PairScalars s;
            s.lower = mn;
            s.delta = delta;
            s.sumq = (float)sum;  // rabitq.rs:322 `scalar_sum as f32`
            s.ycd = ycd_in[pp];
            s.ycd_sqrt = sqrtf(ycd_in[pp]);  // :346
            s.row = row;
            s.list_begin = lb[pp];
            s.list_len = ll[pp];
            s.stream_begin = sbeg[pp];  // PLACE: known already; else filled by pair_prefix_kernel
            s.pad = 0;
            scal[p] = s;
            if constexpr (PLACE) {
                if (tail_dst) {  // the tail but for the threshold's part (stage_tail_kernel), 16-byte aligned in both image layouts
                    uint32_t t[12];
                    stage_tail_static(s, true, p - row * pairs_per_row, pl.s_lo, pl.s_hi, t);
                    t[RQ_REC_THR] = 0u;
#pragma unroll
                    for (int i = 0; i < 3; ++i) reinterpret_cast<uint4 *>(tail_dst)[i] = make_uint4(t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
                }
            }
        }
    }
}

template <int LP, int R, int PP>
__global__ __launch_bounds__(256) void prep_small_kernel(const float *__restrict__ y,
                                                         const float *__restrict__ centroids,
                                                         const uint32_t *__restrict__ offsets,
                                                         const uint32_t *__restrict__ pair_cluster,
                                                         const float *__restrict__ pair_ycd, uint32_t npairs,
                                                         uint32_t pairs_per_row, PairScalars *__restrict__ scal,
                                                         uint32_t *__restrict__ qnib, uint32_t *__restrict__ qf6,
                                                         uint32_t nlists, uint32_t skip_empty, uint32_t qn_slots) {
    constexpr uint32_t PPW = 64 / LP;
    const uint32_t p0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (PPW * PP) + (threadIdx.x & 63) / LP;
    prep_small_pairs<LP, R, PP>(y, centroids, offsets, pair_cluster, pair_ycd, npairs, pairs_per_row, scal, qnib, qf6, nlists,
                                skip_empty, p0, nullptr, qn_slots);
}

// The same quantisation with the final stage placed ahead of it (PrepPlace): no pair-major fp6 buffer
template <int LP, int R, int PP>
__global__ __launch_bounds__(256) void prep_small_placed_kernel(const float *__restrict__ y,
                                                                const float *__restrict__ centroids,
                                                                const uint32_t *__restrict__ offsets,
                                                                const uint32_t *__restrict__ pair_cluster,
                                                                const float *__restrict__ pair_ycd, uint32_t npairs,
                                                                uint32_t pairs_per_row, PairScalars *__restrict__ scal,
                                                                uint32_t *__restrict__ qnib, uint32_t nlists,
                                                                uint32_t skip_empty, uint32_t qn_slots, const PrepPlace pl) {
    constexpr uint32_t PPW = 64 / LP;
    const uint32_t p0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (PPW * PP) + (threadIdx.x & 63) / LP;
    prep_small_pairs<LP, R, PP, true>(y, centroids, offsets, pair_cluster, pair_ycd, npairs, pairs_per_row, scal, qnib, nullptr, nlists,
                                      skip_empty, p0, nullptr, qn_slots, pl);
}

// Sharded passes (a rank of a multi-GPU deployment: most probed lists live on other ranks, i.e. are empty here): one THREAD
// per pair writes the scalars of the pairs with nothing to scan and lists the others, and the quantisation kernel -- a lane
// group per pair -- then runs over that list only (7 of 8 lane groups did nothing but find their list empty).
__global__ __launch_bounds__(1024) void pair_split_kernel(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ pair_cluster,
                                                          const float *__restrict__ pair_ycd, uint32_t npairs, uint32_t pairs_per_row,
                                                          uint32_t nlists, PairScalars *__restrict__ scal,
                                                          uint32_t *__restrict__ live_list, uint32_t *__restrict__ live_count) {
    // 4096 pairs per block, ONE reservation per block on the list's counter (a wave-level reservation each was half a million
    // atomics on one address per pass: 3 ms)
    __shared__ uint32_t wcnt[4][16], s_base;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool keep[4];
    uint32_t rank[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t p = blockIdx.x * 4096 + u * 1024 + threadIdx.x;
        keep[u] = false;
        if (p < npairs) {
            const uint32_t c = pair_cluster[p];
            const uint32_t len = c < nlists ? offsets[c + 1] - offsets[c] : 0u;
            keep[u] = len != 0;
            if (!keep[u]) {  // exactly what prep_small_pairs writes for such a pair
                PairScalars s;
                s.lower = 0.0f, s.delta = 0.0f, s.sumq = 0.0f, s.ycd = pair_ycd[p], s.ycd_sqrt = 0.0f;
                s.row = p / pairs_per_row, s.list_begin = 0, s.list_len = 0, s.stream_begin = 0, s.pad = 0;
                scal[p] = s;
            }
        }
        const uint64_t m = __ballot(keep[u]);
        rank[u] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[u][wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int u = 0; u < 4; ++u)
            for (int w = 0; w < 16; ++w) {
                const uint32_t c = wcnt[u][w];
                wcnt[u][w] = tot;
                tot += c;
            }
        s_base = tot ? atomicAdd(live_count, tot) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (keep[u]) live_list[s_base + wcnt[u][wave] + rank[u]] = blockIdx.x * 4096 + u * 1024 + threadIdx.x;
}
template <int LP, int R, int PP>
__global__ __launch_bounds__(256) void prep_small_listed_kernel(const float *__restrict__ y,
                                                                const float *__restrict__ centroids,
                                                                const uint32_t *__restrict__ offsets,
                                                                const uint32_t *__restrict__ pair_cluster,
                                                                const float *__restrict__ pair_ycd, const uint32_t *__restrict__ live_list,
                                                                uint32_t nlive,
                                                                uint32_t pairs_per_row, PairScalars *__restrict__ scal,
                                                                uint32_t *__restrict__ qnib, uint32_t *__restrict__ qf6,
                                                                uint32_t nlists) {
    constexpr uint32_t PPW = 64 / LP;
    const uint32_t p0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (PPW * PP) + (threadIdx.x & 63) / LP;
    prep_small_pairs<LP, R, PP>(y, centroids, offsets, pair_cluster, pair_ycd, nlive, pairs_per_row, scal, qnib, qf6, nlists, 1u, p0, live_list);
}

// Position of every probed list in the query's candidate stream (the order the reference visits
// candidates: lists nearest-first, members in stored order) and the stream length, which is also
// what the reference adds to METRICS.rough for this query (src/rerank.rs:105).
// one wave, query row b: 64 slots per step, exclusive scan by shuffles, carry across steps
// Filtered passes (sub_off != nullptr): the stream keeps the index's positions, but the reference on the sub-index counts only the
// admitted rows of the probed lists (pair_cluster / sub_off: the probe lists and the sub-index's list offsets).
__device__ __forceinline__ void pair_prefix_row(PairScalars *__restrict__ scal, uint32_t b, uint32_t nprobe,
                                                unsigned long long *__restrict__ rough_count,
                                                const uint32_t *__restrict__ pair_cluster = nullptr,
                                                const uint32_t *__restrict__ sub_off = nullptr, uint32_t nlists = 0,
                                                unsigned long long *__restrict__ stream_len = nullptr,
                                                const uint32_t *__restrict__ offsets = nullptr /* ahead of the quantisation: list lengths from here (with pair_cluster, nlists) */,
                                                uint32_t *__restrict__ begin_out = nullptr /* ... and the positions go here, per pair */) {
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long carry = 0, admitted = 0;
    for (uint32_t s0 = 0; s0 < nprobe; s0 += 64) {
        const uint32_t s = s0 + lane;
        PairScalars *ps = scal + (uint64_t)b * nprobe + s;
        unsigned long long len = 0;
        if (offsets) {
            const uint32_t c = s < nprobe ? pair_cluster[(uint64_t)b * nprobe + s] : 0xFFFFFFFFu;
            len = c < nlists ? offsets[c + 1] - offsets[c] : 0u;
        } else
            len = s < nprobe ? ps->list_len : 0;
        const unsigned long long incl = wave_incl_scan(len);
        const unsigned long long begin = carry + incl - len;
        if (s < nprobe) *(begin_out ? begin_out + (uint64_t)b * nprobe + s : &ps->stream_begin) = begin > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)begin;
        carry += __shfl(incl, 63, 64);
        if (sub_off) {
            const uint32_t c = s < nprobe && len ? pair_cluster[(uint64_t)b * nprobe + s] : 0xFFFFFFFFu;
            unsigned long long ad = c < nlists ? sub_off[c + 1] - sub_off[c] : 0ull;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) ad += __shfl_xor(ad, o, 64);
            admitted += ad;
        }
    }
    if (lane == 0) rough_count[b] = sub_off ? admitted : carry;
    if (lane == 0 && stream_len) stream_len[b] = carry;  // (filtered passes: the stream's length, for the profile's matrix_pairs)
}
__global__ __launch_bounds__(256) void pair_prefix_kernel(PairScalars *__restrict__ scal, uint32_t nq, uint32_t nprobe,
                                                          unsigned long long *__restrict__ rough_count) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b < nq) pair_prefix_row(scal, b, nprobe, rough_count);
}
// ahead of the quantisation (PrepPlace): lengths from the index's offsets, positions into an array of their own
__global__ __launch_bounds__(256) void pair_prefix_lens_kernel(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ pair_cluster,
                                                               uint32_t nlists, uint32_t nq, uint32_t nprobe,
                                                               unsigned long long *__restrict__ rough_count, uint32_t *__restrict__ begin_out,
                                                               PairScalars *__restrict__ scal /* not touched */) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b < nq) pair_prefix_row(scal, b, nprobe, rough_count, pair_cluster, nullptr, nlists, nullptr, offsets, begin_out);
}
__global__ __launch_bounds__(256) void pair_prefix_filtered_kernel(PairScalars *__restrict__ scal, uint32_t nq, uint32_t nprobe,
                                                                   unsigned long long *__restrict__ rough_count,
                                                                   const uint32_t *__restrict__ pair_cluster,
                                                                   const uint32_t *__restrict__ sub_off, uint32_t nlists,
                                                                   unsigned long long *__restrict__ stream_len) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b < nq) pair_prefix_row(scal, b, nprobe, rough_count, pair_cluster, sub_off, nlists, stream_len);
}

// ---- filters (rq_filter_create) ----------------------------------------------------------------------------------------------
// Position bitmap: bit pos of word pos >> 5 = allow[map_ids[pos]] (ids >= nbits are not admitted).  One wave covers 64 positions:
// its bits come from ONE ballot and leave in two plain 32-bit stores.  Words past the last position are written as zero.
__global__ __launch_bounds__(256) void filter_positions_kernel(const uint32_t *__restrict__ map_ids, uint64_t n,
                                                               const uint32_t *__restrict__ allow_ids, uint64_t nbits,
                                                               uint32_t *__restrict__ pos_bits, uint64_t nwords) {
    const uint64_t pos = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    bool in = false;
    if (pos < n) {
        const uint32_t id = map_ids[pos];
        in = (uint64_t)id < nbits && ((allow_ids[id >> 5] >> (id & 31u)) & 1u);
    }
    const uint64_t m = __ballot(in);
    const uint64_t w = (pos - lane) >> 5;  // first of the wave's two words
    if (lane < 2 && w + lane < nwords) pos_bits[w + lane] = (uint32_t)(m >> (32 * lane));
}
// Admitted rows per list: one block per list, one word of the bitmap per lane and step (the list's first and last word masked to
// its range).
__global__ __launch_bounds__(256) void filter_lists_kernel(const uint32_t *__restrict__ pos_bits, const uint32_t *__restrict__ offsets,
                                                           uint32_t *__restrict__ list_adm) {
    __shared__ uint32_t s_cnt;
    const uint32_t c = blockIdx.x;
    const uint32_t b = offsets[c], e = offsets[c + 1];
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    uint32_t cnt = 0;
    if (e > b) {
        for (uint32_t w = (b >> 5) + threadIdx.x; w <= ((e - 1) >> 5); w += 256) {
            uint32_t bits = pos_bits[w];
            const uint32_t w0 = w << 5;
            if (w0 < b) bits &= ~0u << (b - w0);                    // positions before the list
            if (e - w0 < 32) bits &= (1u << (e - w0)) - 1u;         // positions after it
            cnt += (uint32_t)__popc(bits);
        }
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) list_adm[c] = s_cnt;
}

// ------------------------------------------------------------------------------------------------
// Work-list construction for a stage: the (query, slot) pairs with slot in [slot_lo, slot_hi).
// pair-major: one group per pair.  cluster-major: pairs bucketed by list so that a list is read
// from HBM once and scored against every query probing it.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pair_in_stage(const PairScalars &ps, uint32_t s_lo, uint32_t s_hi) {
    return stream_in_stage(ps.stream_begin, ps.list_len, s_lo, s_hi);
}

// `count` = nq * slot_hi work items: only the first slot_hi slots of every query can be in the stage
__global__ void group_count_kernel(const PairScalars *__restrict__ scal,
                                   const uint32_t *__restrict__ probe_cluster, uint32_t count, uint32_t nprobe,
                                   uint32_t slot_hi, uint32_t s_lo, uint32_t s_hi, uint32_t *__restrict__ grp_cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t b = i / slot_hi, p = b * nprobe + (i - b * slot_hi);
    if (pair_in_stage(scal[p], s_lo, s_hi)) atomicAdd(&grp_cnt[probe_cluster[p]], 1u);
}

// The same count for big stages, with the place of every pair inside its list's group decided on the way
// (cluster-major stages of large batches: ~16 pairs per list and block).  A block owns RQ_RANK_ITEMS consecutive work
// items and a histogram of the lists in LDS: an item's rank inside (block, list) comes from the LDS atomic, the
// block's base inside the list from ONE global atomic per (block, list) -- instead of one contended global atomic
// per pair here and a second one in stage_fill_kernel (4.2 M each at batch 65 536, on 4096 addresses).
//   rank[i]           place of item i among its block's pairs of the same list (~0u: not in the stage)
//   blk_base[blk][c]  first place of block blk's pairs in list c's group
// Dynamic LDS: k counters.
// begins / offsets (ahead of the quantisation, PrepPlace): the stream positions and list lengths come from there, not from scal.
__global__ __launch_bounds__(1024) void group_rank_kernel(const PairScalars *__restrict__ scal,
                                                          const uint32_t *__restrict__ probe_cluster, uint32_t count,
                                                          uint32_t nprobe, uint32_t slot_hi, uint32_t s_lo, uint32_t s_hi,
                                                          uint32_t k, uint32_t *__restrict__ grp_cnt,
                                                          uint32_t *__restrict__ rank, uint32_t *__restrict__ blk_base,
                                                          const uint32_t *__restrict__ begins = nullptr,
                                                          const uint32_t *__restrict__ offsets = nullptr) {
    extern __shared__ uint32_t rank_hist[];
    for (uint32_t c = threadIdx.x; c < k; c += 1024) rank_hist[c] = 0;
    __syncthreads();
    const uint32_t first = blockIdx.x * RQ_RANK_ITEMS;
    for (uint32_t j = threadIdx.x; j < RQ_RANK_ITEMS; j += 1024) {
        const uint32_t i = first + j;
        if (i >= count) break;
        const uint32_t b = i / slot_hi, p = b * nprobe + (i - b * slot_hi);
        uint32_t r = ~0u;
        if (begins) {
            const uint32_t c = probe_cluster[p];
            if (c < k && stream_in_stage(begins[p], offsets[c + 1] - offsets[c], s_lo, s_hi)) r = atomicAdd(&rank_hist[c], 1u);
        } else if (pair_in_stage(scal[p], s_lo, s_hi))
            r = atomicAdd(&rank_hist[probe_cluster[p]], 1u);
        rank[i] = r;
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < k; c += 1024) {
        const uint32_t h = rank_hist[c];
        blk_base[(uint64_t)blockIdx.x * k + c] = h ? atomicAdd(&grp_cnt[c], h) : 0u;
    }
}

// exclusive scan of cnt[0..k) into start[0..k]; single block, any k.  Also zeroes cnt for the
// fill pass (cnt is reused as the per-list cursor, so it holds the counts again afterwards).
// pad32 bit 0: every group starts at a multiple of 32 records (the matrix-core scan's query tiles).
// pad32 (matrix-core stages): the rows between a group's last record and its 32-row boundary are marked "no query"
// right here (their threshold operand: constant term -inf, so the accumulator of such a row starts at -inf and is
// never flagged): the scan then needs no per-tile masking.  recs / opdw: the stage's tile images.
__global__ __launch_bounds__(1024) void group_scan_kernel(uint32_t *__restrict__ cnt, uint32_t k,
                                                          uint32_t *__restrict__ start, uint32_t pad32,
                                                          uint32_t *__restrict__ recs, uint32_t opdw) {
    const uint32_t total = block_scan_chunked<uint32_t, uint32_t>(
        k, [&](uint32_t i) { return (pad32 & 1u) ? (cnt[i] + 31u) & ~31u : cnt[i]; },
        [&](uint32_t i, uint32_t st0, uint32_t v) {
            start[i] = st0;
            if ((pad32 & 1u) && recs) {
                const uint32_t real = cnt[i];
                const bool additive = (pad32 & 4u) != 0;  // bit 2: tile images of the additive gate (start value -inf)
                const uint32_t opld = rq_img_opld(opdw, additive), img = rq_img_dwords(opdw, additive);
                for (uint32_t at = st0 + real; at < st0 + v; ++at) {  // at most 31 rows
                    if (additive) {
                        recs[(uint64_t)(at >> 5) * img + 32 * opld + 32 * RQ_RECA_TAIL + (at & 31u)] = 0xFF800000u;
                        continue;
                    }
                    uint32_t *tl = recs + (uint64_t)(at >> 5) * img + 32 * opld + (at & 31u) * RQ_REC_TAIL + RQ_REC_V0;
                    *reinterpret_cast<uint4 *>(tl) = make_uint4(0u, 0u, 0u, 0x0000FF80u);  // slots 0..7: c0 = -inf
                    *reinterpret_cast<uint4 *>(tl + 4) = make_uint4(0u, 0u, 0u, 0u);        // slots 8..15
                }
            }
            if (!(pad32 & 2u)) cnt[i] = 0;  // bit 1: the places are already known (group_rank_kernel), cnt stays the count
        });
    if (threadIdx.x == 0) start[k] = total;
}

// f32 -> bf16 bits (round to nearest even) and back; finite inputs well inside the f32 range
__device__ __forceinline__ uint32_t bf16_rne(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ float bf16_to_f32(uint32_t b) { return __builtin_bit_cast(float, b << 16); }

// The threshold's part of a matrix-core stage record (comment in stage_fill_item): v'_q, the bound qb of the terms' magnitudes,
// whether the integer form is safe, and the bf16 form's margin.  Shared by stage_fill_item and stage_tail_kernel.
struct StageGate {
    float v[4], qb, margin;
    bool safe;
};
__device__ __forceinline__ StageGate stage_gate(float lower, float delta, float sumq, float ycd, float ycd_sqrt, float th,
                                                const FactorStats &fs) {
    StageGate g;
    const float inv2d = 0.5f / delta;
    g.v[0] = (th - ycd) * inv2d, g.v[1] = -inv2d, g.v[2] = -lower * inv2d, g.v[3] = ycd_sqrt * inv2d;
    g.qb = (fabsf(th - ycd) + fs.cds_max + fabsf(lower) * fs.ppc_absmax + ycd_sqrt * fs.eb_max) *
           fs.invfip_absmax * fabsf(inv2d);
    g.safe = delta > 0.0f && g.qb + sumq < 524288.0f;  // also false for NaN / inf
    g.margin = 2.0f + g.qb * (1.0f / 8192.0f) + (g.qb + sumq) * (1.0f / 262144.0f);
    return g;
}
// additive form: the row's accumulator start value C_q (u0: the list's reference U0)
__device__ __forceinline__ float stage_gate_cq(const StageGate &g, float sumq, const float4 u0) {
    float bq = u0.x * g.v[0];
    bq += u0.y * g.v[1];
    bq += u0.w * g.v[3];
    bq += 0.5f * sumq;
    const float margin_a = 2.0f + g.qb * (1.0f / 8192.0f) + (g.qb + sumq) * (1.0f / 65536.0f);
    float cq = -0.5f * (bq - margin_a);
    if (!g.safe || !(fabsf(cq) < 1.0e37f)) cq = __builtin_inff();  // always flagged: the exact path decides
    return cq;
}
// bf16 threshold form: the eight dwords at RQ_REC_V0
__device__ __forceinline__ void stage_gate_bf16(const StageGate &g, float sumq, uint32_t *__restrict__ t8) {
    const float v4 = -0.5f * (0.5f * sumq - g.margin);
    uint32_t vh[4], vl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x = -0.5f * g.v[i];
        vh[i] = bf16_rne(x);
        vl[i] = bf16_rne(x - bf16_to_f32(vh[i]));
    }
    uint32_t c0 = bf16_rne(v4);
    const float r1 = v4 - bf16_to_f32(c0);
    uint32_t c1 = bf16_rne(r1);
    uint32_t c2 = bf16_rne(r1 - bf16_to_f32(c1));
    if (!g.safe) {
#pragma unroll
        for (int i = 0; i < 4; ++i) vh[i] = 0, vl[i] = 0;
        c0 = 0x7F80u, c1 = 0, c2 = 0;  // +inf * 1: -S* = +inf
    }
    // A operand of the threshold MFMA, element e of lane half h = slot 8h + e:
    //   vh0 vh0 vl0 vh1 vh1 vl1 c0 c1 | vh2 vh2 vl2 vh3 vh3 vl3 c2 0     against the candidate side's
    //   uh0 ul0 uh0 uh1 ul1 uh1  1  1 | uh2 ul2 uh2 uh3 ul3 uh3  1 0
    t8[0] = vh[0] | (vh[0] << 16);
    t8[1] = vl[0] | (vh[1] << 16);
    t8[2] = vh[1] | (vl[1] << 16);
    t8[3] = c0 | (c1 << 16);
    t8[4] = vh[2] | (vh[2] << 16);
    t8[5] = vl[2] | (vh[3] << 16);
    t8[6] = vh[3] | (vl[3] << 16);
    t8[7] = c2;
}

// work item wi = (query, slot < slot_hi), handled by the 16 lanes threadIdx.x & ~15 .. | 15; thr_b: the query's threshold
template <int LPP = 16 /* lanes per work item: 16, or 8 for the additive tile images (16-byte aligned operand rows) */>
__device__ __forceinline__ void stage_fill_item(const PairScalars *__restrict__ scal,
                                                const uint32_t *__restrict__ probe_cluster,
                                                const uint32_t *__restrict__ operand /* opdw dwords per pair */,
                                                const float *__restrict__ thr, uint32_t wi,
                                                uint32_t nprobe, uint32_t slot_hi, uint32_t opdw, uint32_t s_lo,
                                                uint32_t s_hi,
                                                uint32_t cluster_major,
                                                const uint32_t *__restrict__ grp_start,
                                                uint32_t *__restrict__ grp_cursor,
                                                uint32_t *__restrict__ recs, const FactorStats &fs,
                                                uint32_t tile_images /* 0 record-major, 1 tile images, 2 tile images of the additive gate */,
                                                const uint32_t *__restrict__ rank /* group_rank_kernel, or null */,
                                                const uint32_t *__restrict__ blk_base, uint32_t k,
                                                const float4 *__restrict__ list_uref /* tile_images == 2: U0 per list */) {
    const uint32_t sub = threadIdx.x & (LPP - 1);                // LPP lanes per pair
    // (ranked placement: the counting pass has already decided which items are in the stage -- 7 of 8 are not when the pairs of
    // seven other shards' lists ride along in a multi-GPU pass; they leave before their 40-byte scalars are fetched)
    if (cluster_major && rank && rank[wi] == ~0u) return;
    const uint32_t wb = wi / slot_hi, p = wb * nprobe + (wi - wb * slot_hi);
    const PairScalars ps = scal[p];
    const bool in = pair_in_stage(ps, s_lo, s_hi);
    if (cluster_major && !in) return;
    uint32_t at = p;
    uint32_t list_id = 0;
    if (cluster_major) {
        const uint32_t c = probe_cluster[p];
        list_id = c;
        if (rank) {  // places were handed out by group_rank_kernel
            at = grp_start[c] + blk_base[(uint64_t)(wi / RQ_RANK_ITEMS) * k + c] + rank[wi];
        } else {
            uint32_t a = 0;
            if (sub == 0) a = atomicAdd(&grp_cursor[c], 1u);
            at = grp_start[c] + __shfl(a, 0, LPP);
        }
    }
    // record-major: record `at` = opdw operand dwords + RQ_REC_TAIL tail dwords.  tile images (matrix-core
    // scan): records in tiles of 32, each tile stored as the exact LDS image the kernel copies in with
    // LDS-DMA: 32 operand rows of opdw+2 dwords, then the 32 tails.
    const uint32_t stride = opdw + RQ_REC_TAIL;
    uint32_t *r = recs + (uint64_t)at * stride;
    uint32_t *tdst = r + opdw;
    float *cdst = nullptr;  // additive gate: the row's accumulator start value
    if (tile_images) {
        const uint32_t opld = rq_img_opld(opdw, tile_images == 2), img = rq_img_dwords(opdw, tile_images == 2);
        const uint32_t taild = tile_images == 2 ? RQ_RECA_TAIL : RQ_REC_TAIL;
        uint32_t *base = recs + (uint64_t)(at >> 5) * img;
        r = base + (at & 31u) * opld;
        tdst = base + 32 * opld + (at & 31u) * taild;
        if (tile_images == 2) cdst = reinterpret_cast<float *>(base + 32 * opld + 32 * taild + (at & 31u));
    }
    if constexpr (LPP == 8) {  // record-major records (stride opdw + 20 dwords) and additive tile images (rows of opdw + 4 dwords): 16-byte aligned like the operand itself (opdw = 8 W or 12 W)
        const uint4 *src = reinterpret_cast<const uint4 *>(operand + (uint64_t)p * opdw);
        uint4 *dst = reinterpret_cast<uint4 *>(r);
        for (uint32_t i = sub; i < opdw / 4; i += 8) dst[i] = src[i];
    } else {  // operand rows are 8-byte aligned in both layouts (opdw, the record stride and the image row stride are even)
        const uint2 *src = reinterpret_cast<const uint2 *>(operand + (uint64_t)p * opdw);
        uint2 *dst = reinterpret_cast<uint2 *>(r);
        for (uint32_t i = sub; i < opdw / 2; i += 16) dst[i] = src[i];
    }
    {  // the tail: computed by every lane of the pair (they would idle otherwise), stored 16 bytes per lane by lanes 0..4
        uint32_t t[RQ_REC_TAIL];
        stage_tail_static(ps, in, p - ps.row * nprobe, s_lo, s_hi, t);
        t[RQ_REC_THR] = __builtin_bit_cast(uint32_t, thr[ps.row]);
        // Integer form of the gate (used by the matrix-core scan).  With F = factor_ip * delta < 0,
        //   rough < thr  <=>  s > S* = [ (thr - ycd) + (-1) cds + (-lower) ppc + ysq eb ] / (2 F) + sumq / 2
        // (real arithmetic), a rank-5 bilinear form in u'_c = (1, cds, ppc, eb)/fip, 1  and v'_q.  The scan
        // starts its accumulator tile at -S*/2 (its dot products come out as s/2) with ONE
        // v_mfma_f32_32x32x16_bf16: every u', v' is split into bf16 hi + lo and the products
        // hi*hi + hi*lo + lo*hi are summed (12 slots), the constant term is split three ways (exact), 1
        // slot is unused; the gate is then "accumulator > 0".  S* is lowered by a margin that covers the
        // f32 rounding of the exact expression (2, safe while the terms stay below 2^19), the dropped
        // lo*lo products and split residues (< 2^-14 of the sum of |terms|) and the roundings of adding
        // s/2 onto -S*/2 inside the matrix unit (< 2^-19 of the magnitudes), so the test can never hide a
        // candidate the exact f32 expression would pass; where the scales make the bound unsafe (or
        // delta <= 0) the query is marked "always flagged" (-S* = +inf) and every candidate takes the
        // exact path.
        const StageGate g = stage_gate(ps.lower, ps.delta, ps.sumq, ps.ycd, ps.ycd_sqrt, thr[ps.row], fs);
        if (tile_images == 2) {
            // Additive gate (scan_mfma_kernel<.., ADD>): the query's side of  S* >= B_q + G_c,  B_q = sum_r U0[r] v'_q[r] + sumq / 2 with
            // the list's reference U0 (U0[2] = 0), as the accumulator's start value C_q = -(B_q - margin) / 2 (the dot products come
            // out as s / 2): "s/2 + C_q > G_c / 2" then holds for every candidate the exact f32 expression would pass.  The margin is
            // the bf16 form's (2 for the f32 rounding of the exact expression; qb 2^-13 covers, many times over, the f32 roundings
            // of B_q, of v' inside the list's V0 / DV and of the candidate's u' -- all relative 2^-22 of terms bounded by qb) with a
            // wider share for the matrix unit's own accumulation of C_q + s/2 (f32, magnitudes below qb + sumq).
            const float cq = stage_gate_cq(g, ps.sumq, list_uref[list_id]);
            if (sub == 5) *cdst = cq;
            if (sub < 3) *reinterpret_cast<uint4 *>(tdst + 4 * sub) = make_uint4(t[4 * sub], t[4 * sub + 1], t[4 * sub + 2], t[4 * sub + 3]);
            return;
        }
        stage_gate_bf16(g, ps.sumq, t + RQ_REC_V0);
        // Dense run directory of a VALU stage: list position p of this pair lives in cell CELL0 + p / 64.  Cells follow
        // the stream: floor(stream_begin / 64) + 2 slot + 1 - floor(s_lo / 64) leaves every list its own cells (the two
        // spare cells per slot absorb the roundings of stream_begin and of the list's length) and never goes negative
        // for a position inside the stage.
        if (!tile_images) t[RQ_REC_CELL0] = (ps.stream_begin >> 6) + 2u * (p - ps.row * nprobe) + 1u - (s_lo >> 6);
        static_assert(RQ_REC_TAIL == 20, "five 16-byte pieces");
        uint4 piece = make_uint4(t[0], t[1], t[2], t[3]);  // 16-byte aligned in both layouts
#pragma unroll
        for (int i = 1; i < 5; ++i)
            if (sub == (uint32_t)i) piece = make_uint4(t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
        if (sub < 5) *reinterpret_cast<uint4 *>(tdst + 4 * sub) = piece;
    }
}
template <int LPP = 16>
__global__ __launch_bounds__(256) void stage_fill_kernel(const PairScalars *__restrict__ scal,
                                                         const uint32_t *__restrict__ probe_cluster,
                                                         const uint32_t *__restrict__ operand /* opdw dwords per pair */,
                                                         const float *__restrict__ thr, uint32_t count,
                                                         uint32_t nprobe, uint32_t slot_hi, uint32_t opdw, uint32_t s_lo,
                                                         uint32_t s_hi,
                                                         uint32_t cluster_major,
                                                         const uint32_t *__restrict__ grp_start,
                                                         uint32_t *__restrict__ grp_cursor,
                                                         uint32_t *__restrict__ recs, const FactorStats fs,
                                                         uint32_t tile_images,
                                                         const uint32_t *__restrict__ rank /* group_rank_kernel, or null */,
                                                         const uint32_t *__restrict__ blk_base, uint32_t k,
                                                         const float4 *__restrict__ list_uref,
                                                         const uint32_t *__restrict__ items = nullptr /* the work items to visit (count of them), else all */) {
    uint32_t wi = blockIdx.x * (256 / LPP) + threadIdx.x / LPP;  // work item: (query, slot < slot_hi)
    if (wi >= count) return;
    if (items) wi = items[wi];
    stage_fill_item<LPP>(scal, probe_cluster, operand, thr, wi, nprobe, slot_hi, opdw, s_lo, s_hi, cluster_major, grp_start, grp_cursor,
                    recs, fs, tile_images, rank, blk_base, k, list_uref);
}

// block reduction of the per-thread min / max of v' (256 threads) and the list's V0 / DV
__device__ __forceinline__ void vrange_reduce_store(float *lo, float *hi, uint32_t c, float4 *__restrict__ vref, float (*red)[8] /* LDS: [4][8] */) {
    const float inf = __builtin_inff();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        for (int o = 32; o >= 1; o >>= 1) lo[r] = fminf(lo[r], __shfl_xor(lo[r], o, 64)), hi[r] = fmaxf(hi[r], __shfl_xor(hi[r], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[threadIdx.x >> 6][r] = lo[r], red[threadIdx.x >> 6][4 + r] = hi[r];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float v0[4], dv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float l = fminf(fminf(red[0][r], red[1][r]), fminf(red[2][r], red[3][r]));
            const float u = fmaxf(fmaxf(red[0][4 + r], red[1][4 + r]), fmaxf(red[2][4 + r], red[3][4 + r]));
            const bool any = l <= u && u < inf && l > -inf;
            v0[r] = any ? 0.5f * l + 0.5f * u : 0.0f;
            // half-range, widened so that |v - v0| <= dv survives the roundings of v0 and of the subtraction
            dv[r] = any ? fmaxf(u - v0[r], v0[r] - l) * 1.000001f : 0.0f;
        }
        vref[2 * c] = make_float4(v0[0], v0[1], v0[2], v0[3]);
        vref[2 * c + 1] = make_float4(dv[0], dv[1], dv[2], dv[3]);
    }
}
// Additive gate of the matrix-core scan: centre V0 and half-range DV of v'_q = ((thr - ycd), -1, -lower, sqrt(ycd)) / (2 delta)
// over the pairs of a stage that probe list c (the records of group c, tile images of the additive format), written as
// two float4 per list.  Pairs whose start value is +inf (always flagged: stage_fill_kernel) take no part.  One block per list.
__global__ __launch_bounds__(256) void group_vrange_kernel(const uint32_t *__restrict__ recs, const uint32_t *__restrict__ grp_start,
                                                           const uint32_t *__restrict__ grp_cnt, uint32_t opdw,
                                                           float4 *__restrict__ vref) {
    const uint32_t c = blockIdx.x, n = grp_cnt[c], st0 = grp_start[c];
    const uint32_t opld = rq_img_opld(opdw, true), img = rq_img_dwords(opdw, true);
    const float inf = __builtin_inff();
    float lo[4] = {inf, inf, inf, inf}, hi[4] = {-inf, -inf, -inf, -inf};
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint32_t at = st0 + i;
        const uint32_t *base = recs + (uint64_t)(at >> 5) * img + 32 * opld;
        const float cq = __builtin_bit_cast(float, base[32 * RQ_RECA_TAIL + (at & 31u)]);
        if (!(cq < inf)) continue;
        const uint32_t *t = base + (at & 31u) * RQ_RECA_TAIL;
        const float lower = __builtin_bit_cast(float, t[RQ_REC_LOWER]), delta = __builtin_bit_cast(float, t[RQ_REC_DELTA]);
        const float ycd = __builtin_bit_cast(float, t[RQ_REC_YCD]), ysq = __builtin_bit_cast(float, t[RQ_REC_YCD_SQRT]);
        const float th = __builtin_bit_cast(float, t[RQ_REC_THR]);
        const float inv2d = 0.5f / delta;  // the expressions of stage_fill_item
        const float v[4] = {(th - ycd) * inv2d, -inv2d, -lower * inv2d, ysq * inv2d};
#pragma unroll
        for (int r = 0; r < 4; ++r) lo[r] = fminf(lo[r], v[r]), hi[r] = fmaxf(hi[r], v[r]);
    }
    __shared__ float red[4][8];
    vrange_reduce_store(lo, hi, c, vref, red);
}

// The final stage's tails when the quantisation has placed the operand rows and the threshold-free tail dwords already
// (PrepPlace): one block per list walks the list's group in placement order, reads a row's tail and the query's threshold and
// writes what depends on the threshold -- t[RQ_REC_THR] and, bf16 form, the operand at RQ_REC_V0; additive form, C_q, and the
// list's V0 / DV on the way (group_vrange_kernel's result without its second read of the tails).  Operand rows are not touched.
__global__ __launch_bounds__(256) void stage_tail_kernel(uint32_t *__restrict__ recs, const uint32_t *__restrict__ grp_start,
                                                         const uint32_t *__restrict__ grp_cnt, const float *__restrict__ thr,
                                                         uint32_t opdw, const FactorStats fs, uint32_t tile_images,
                                                         const float4 *__restrict__ list_uref, float4 *__restrict__ vref) {
    const uint32_t c = blockIdx.x, n = grp_cnt[c], st0 = grp_start[c];
    const bool additive = tile_images == 2;
    const uint32_t opld = rq_img_opld(opdw, additive), img = rq_img_dwords(opdw, additive);
    const uint32_t taild = additive ? RQ_RECA_TAIL : RQ_REC_TAIL;
    const float inf = __builtin_inff();
    float lo[4] = {inf, inf, inf, inf}, hi[4] = {-inf, -inf, -inf, -inf};
    float4 u0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (additive && n) u0 = list_uref[c];
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint32_t at = st0 + i;
        uint32_t *base = recs + (uint64_t)(at >> 5) * img + 32 * opld;
        uint32_t *t = base + (at & 31u) * taild;
        const uint4 t0 = *reinterpret_cast<const uint4 *>(t), t1 = *reinterpret_cast<const uint4 *>(t + 4);
        const float lower = __builtin_bit_cast(float, t0.x), delta = __builtin_bit_cast(float, t0.y);
        const float sumq = __builtin_bit_cast(float, t0.z), ycd = __builtin_bit_cast(float, t0.w);
        const float ysq = __builtin_bit_cast(float, t1.x);
        static_assert(RQ_REC_LOWER == 0 && RQ_REC_DELTA == 1 && RQ_REC_SUMQ == 2 && RQ_REC_YCD == 3 && RQ_REC_YCD_SQRT == 4 && RQ_REC_THR == 5,
                      "the first six tail dwords");
        const float th = thr[t[RQ_REC_ROW]];
        t[RQ_REC_THR] = __builtin_bit_cast(uint32_t, th);
        const StageGate g = stage_gate(lower, delta, sumq, ycd, ysq, th, fs);
        if (additive) {
            const float cq = stage_gate_cq(g, sumq, u0);
            base[32 * RQ_RECA_TAIL + (at & 31u)] = __builtin_bit_cast(uint32_t, cq);
            if (!(cq < inf)) continue;  // always flagged: takes no part in the list's range
#pragma unroll
            for (int r = 0; r < 4; ++r) lo[r] = fminf(lo[r], g.v[r]), hi[r] = fmaxf(hi[r], g.v[r]);
        } else {
            uint32_t t8[8];
            stage_gate_bf16(g, sumq, t8);
            *reinterpret_cast<uint4 *>(t + RQ_REC_V0) = make_uint4(t8[0], t8[1], t8[2], t8[3]);
            *reinterpret_cast<uint4 *>(t + RQ_REC_V0 + 4) = make_uint4(t8[4], t8[5], t8[6], t8[7]);
        }
    }
    __shared__ float red[4][8];
    if (additive) vrange_reduce_store(lo, hi, c, vref, red);
}

// One launch for the words a pass wants zeroed before its first kernel (run_pass, option prep_placement)
struct ClearSpans {
    uint32_t *p[6];
    uint32_t n[6];
};
__global__ __launch_bounds__(256) void clear_words_kernel(const ClearSpans cs) {
#pragma unroll
    for (int j = 0; j < 6; ++j)
        for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < cs.n[j]; i += gridDim.x * 256) cs.p[j][i] = 0u;
}

// generic-W fallback (dim/64 not in the templated set): code words re-read per query (L1-resident).  FILT: the filtered form
// (scan_generic_filtered_kernel; a.x holds the filter's position bitmap)
template <bool FILT>
__device__ __forceinline__ void scan_generic_body(SCAN_PARAMS, uint32_t W) {
    const uint32_t STRIDE = 8 * W + RQ_REC_TAIL;
    const uint32_t gl = blockIdx.x / a.tiles_per_group;
    const uint32_t g = a.group_base + gl;
    const uint32_t tile = a.tile_base + (blockIdx.x - gl * a.tiles_per_group);
    uint32_t pb, pe;
    if (a.cluster_major) {
        pb = grp_start[g];
        pe = grp_start[g + 1];
    } else {
        pb = g;
        pe = g + 1;
    }
    if (pb >= pe) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t *rec = recs + (uint64_t)pb * STRIDE;
    const uint32_t list_begin = rec[8 * W + RQ_REC_LIST_BEGIN], list_len = rec[8 * W + RQ_REC_LIST_LEN];
    const uint32_t first = tile * 256;
    if (first >= list_len) return;
    if (!a.cluster_major && rec[8 * W + RQ_REC_LO] >= rec[8 * W + RQ_REC_HI]) return;
    const uint32_t local = first + threadIdx.x;
    const uint32_t pos = list_begin + (local < list_len ? local : 0);
    const uint32_t *cp = codes + (uint64_t)pos * (2 * W);
    const float4 fac = factors[pos];
    bool adm = true;
    if constexpr (FILT) {  // the lane's admission bit (once per block); a tile that admits nothing has nothing to scan
        adm = rq_admitted(load_scan_extra(a.x).allow, pos) != 0u;
        if (!__syncthreads_or(adm)) return;
    }
    for (uint32_t i = pb; i < pe; ++i, rec += STRIDE) {
        const uint32_t *pl = rec;  // the 4 bit planes (AND-popcount form)
        const uint32_t *t = rec + 8 * W;
        const uint32_t lo_p = t[RQ_REC_LO], hi_p = t[RQ_REC_HI];
        if (hi_p <= first || lo_p >= first + 256) continue;
        uint32_t s = 0;
        for (int pp = 0; pp < 4; ++pp) {
            uint32_t tt = 0;
            for (uint32_t w = 0; w < 2 * W; ++w) tt += __popc(cp[w] & pl[pp * 2 * W + w]);
            s += tt << pp;
        }
        float rough = rough_distance(s, fac, __builtin_bit_cast(float, t[RQ_REC_LOWER]),
                                     __builtin_bit_cast(float, t[RQ_REC_DELTA]), __builtin_bit_cast(float, t[RQ_REC_SUMQ]),
                                     __builtin_bit_cast(float, t[RQ_REC_YCD]), __builtin_bit_cast(float, t[RQ_REC_YCD_SQRT]));
        const uint32_t P0 = first + wave * 64;
        const uint32_t ra = lo_p > P0 ? (lo_p - P0 < 64 ? lo_p - P0 : 64) : 0;
        const uint32_t rb = hi_p > P0 ? (hi_p - P0 < 64 ? hi_p - P0 : 64) : 0;
        const uint64_t below_b = rb >= 64 ? ~0ull : ((1ull << rb) - 1ull);
        const uint64_t below_a = ra >= 64 ? ~0ull : ((1ull << ra) - 1ull);
        uint64_t m = __ballot(rough < __builtin_bit_cast(float, t[RQ_REC_THR]) && adm) & below_b & ~below_a;
        if (m) {
            const uint32_t b = t[RQ_REC_ROW], slot = t[RQ_REC_SLOT];
            const bool pass = (m >> lane) & 1ull;
            const uint32_t cntc = (uint32_t)__popcll(m);
            unsigned long long old = 0;
            if (lane == 0) old = atomicAdd(surv_cnt + b, (1ull << 32) | cntc);
            uint32_t base = __builtin_amdgcn_readfirstlane((uint32_t)old);
            uint32_t rbase = __builtin_amdgcn_readfirstlane((uint32_t)(old >> 32));
            if (pass) {
                uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (at < scan_seg(a).capof(b)) {
                    SurvRec r;
                    r.pos = pos, r.slot = slot, r.rough = rough, r.accurate = 0.0f;
                    surv[scan_seg(a).at(b) + at] = r;
                }
            }
            if (lane == 0 && rbase < scan_seg(a).capof(b)) {
                RunRec rr;
                rr.pos = list_begin + first + (threadIdx.x & ~63u);
                rr.slot = slot, rr.base = base, rr.cnt = cntc;
                runs[scan_seg(a).at(b) + rbase] = rr;
            }
        }
    }
}
__global__ __launch_bounds__(256) void scan_generic_kernel(SCAN_PARAMS, uint32_t W) {
    scan_generic_body<false>(codes, factors, offsets, grp_start, recs, surv, runs, surv_cnt, tile_table, a, W);
}
__global__ __launch_bounds__(256) void scan_generic_filtered_kernel(SCAN_PARAMS, uint32_t W) {
    scan_generic_body<true>(codes, factors, offsets, grp_start, recs, surv, runs, surv_cnt, tile_table, a, W);
}

// Dense variant for the per-stage test entry rq_scan: rough distance of every member of one list
// for one (query, list) pair; same device functions as the fused kernel.
__global__ __launch_bounds__(256) void scan_dense_kernel(const uint32_t *__restrict__ codes,
                                                         const float4 *__restrict__ factors,
                                                         uint32_t list_begin, uint32_t list_len,
                                                         uint32_t W, const uint32_t *__restrict__ pl,
                                                         float lower, float delta, float sumq, float ycd,
                                                         float *__restrict__ out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= list_len) return;
    const uint32_t *cp = codes + (uint64_t)(list_begin + i) * (2 * W);
    uint32_t s = 0;
    for (int p = 0; p < 4; ++p) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < 2 * W; ++w) t += __popc(cp[w] & pl[p * 2 * W + w]);
        s += t << p;
    }
    out[i] = rough_distance(s, factors[list_begin + i], lower, delta, sumq, ycd, sqrtf(ycd));
}

#include "kernels_rerank.h"  // the exact re-rank stage: exact distances, shadow rows, pre-filter kernels
#include "kernels_replay.h"  // survivor ordering, the rankers' replay, the result writers

// Rerank order of a large batch: queries grouped by their nearest list (counting sort: histogram, scan by
// group_scan_kernel, scatter).  Queries of one cluster rerank largely the same rows; handled back to back,
// the repeats are served by the L2 / Infinity Cache instead of HBM (measured: -15 % rerank time).
__global__ void order_count_kernel(const uint32_t *__restrict__ probe_cluster, uint32_t nprobe, uint32_t nq, uint32_t k,
                                   uint32_t *__restrict__ hist) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nq) return;
    const uint32_t c = probe_cluster[(uint64_t)b * nprobe];
    atomicAdd(&hist[c < k ? c : k], 1u);
}
__global__ void order_scatter_kernel(const uint32_t *__restrict__ probe_cluster, uint32_t nprobe, uint32_t nq, uint32_t k,
                                     const uint32_t *__restrict__ start, uint32_t *__restrict__ cursor,
                                     uint32_t *__restrict__ order) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nq) return;
    const uint32_t c = probe_cluster[(uint64_t)b * nprobe];
    const uint32_t g = c < k ? c : k;
    order[start[g] + atomicAdd(&cursor[g], 1u)] = b;
}

// Segment sizing of an arena stage: query b's segment = its exact survivor count (surv_cnt low word, counted by the scan)
// rounded up to 64 slots, at least floor_cap.
__global__ void seg_exact_kernel(unsigned long long *__restrict__ surv_cnt, uint32_t nq, uint32_t floor_cap,
                                 uint32_t *__restrict__ q_cap) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nq) return;
    const uint32_t cnt = (uint32_t)surv_cnt[b];
    const uint32_t cap = cnt > floor_cap ? cnt : floor_cap;
    q_cap[b] = cap > 0xFFFFFF80u ? 0xFFFFFFC0u : ((cap + 63u) & ~63u);
    // (the counter keeps its value: records | runs << 32 of the stage, what the kernels behind the scatter read)
}
// The arena's runs to their queries' segments.  A wave takes 64 runs of a shard at a time: lane r claims its run's place
// with the per-query 64-bit counter (exactly the reservation the direct path makes) and writes the descriptor; the records
// of all 64 runs are then copied by the whole wave, one record per lane and step (a lane finds its run by bisection over
// the chunk's prefix sums, like the replay's fetch), so reads and writes stay as coalesced as the runs are long.
__global__ __launch_bounds__(256) void arena_scatter_kernel(const SurvRec *__restrict__ arena_recs, const uint4 *__restrict__ arena_runs,
                                                            const unsigned long long *__restrict__ arena_cur,
                                                            const unsigned int *__restrict__ arena_fail, uint32_t arena_rsub,
                                                            const unsigned long long *__restrict__ q_base,
                                                            const uint2 *__restrict__ arena_places, SurvRec *__restrict__ surv,
                                                            RunRec *__restrict__ runs) {
    __shared__ uint32_t s_pref[4][65], s_src[4][64];
    __shared__ unsigned long long s_dst[4][64];
    // blocks 0 .. SHARDS-1: the shards (valid runs: up to the first append the shard turned away); block SHARDS: the common area
    // (the common area is walked by RQ_ARENA_COMMON_BLOCKS columns of blocks: it can hold a good part of the runs)
    const bool common = blockIdx.x >= RQ_ARENA_SHARDS;
    const uint32_t shard = common ? RQ_ARENA_SHARDS : blockIdx.x;
    uint32_t nr;
    if (!common) {
        nr = (uint32_t)(arena_cur[shard] >> 32);
        const uint32_t fl = arena_fail[shard];
        nr = nr < fl ? nr : fl;
    } else {
        nr = (uint32_t)(arena_cur[RQ_ARENA_SHARDS + 2] >> 32);
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint4 *src = arena_runs + (uint64_t)shard * arena_rsub;
    const uint2 *plc = arena_places + (uint64_t)shard * arena_rsub;
    const uint32_t col = common ? blockIdx.x - RQ_ARENA_SHARDS : 0u, ncol = common ? RQ_ARENA_COMMON_BLOCKS : 1u;
    // (a chain of dependent gathers per chunk -- descriptor -> the query's segment start -> the writes; records -> their copies --
    // so the next chunk's descriptors, places and segment starts are requested while this chunk's records move)
    const uint32_t rstep = ncol * gridDim.y * 256, rfirst = ((col * gridDim.y + blockIdx.y) * 4 + wave) * 64;
    uint4 d_n = make_uint4(0, 0, 0, 0);
    uint2 pl_n = make_uint2(0, 0);
    unsigned long long qat_n = 0;
    if (rfirst + lane < nr) {
        d_n = src[rfirst + lane], pl_n = plc[rfirst + lane];
        qat_n = q_base[d_n.z];
    }
    for (uint32_t r0 = rfirst; r0 < nr; r0 += rstep) {
        uint32_t cnt = 0;
        const uint4 d = d_n;
        const uint2 pl = pl_n;  // the run's place inside its query's segment, reserved by the scan
        const unsigned long long qat = qat_n;
        const bool more = r0 + rstep + lane < nr && r0 + rstep >= r0;
        if (more) d_n = src[r0 + rstep + lane], pl_n = plc[r0 + rstep + lane];
        if (r0 + lane < nr) {
            cnt = d.y >> 16;
            const uint32_t base = pl.x, rbase = pl.y;
            RunRec rr;
            rr.pos = d.x, rr.slot = d.y & 0xFFFFu, rr.base = base, rr.cnt = cnt;
            runs[qat + rbase] = rr;
            s_src[wave][lane] = d.w;
            s_dst[wave][lane] = qat + base;
        }
        const uint32_t incl = wave_incl_scan(cnt);
        s_pref[wave][lane + 1] = incl;
        if (lane == 0) s_pref[wave][0] = 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (more) qat_n = q_base[d_n.z];
        const uint32_t total = __shfl(incl, 63, 64);
        for (uint32_t e0 = 0; e0 < total; e0 += 128) {  // two records per lane in flight
            SurvRec rec[2];
            unsigned long long dst[2];
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const uint32_t e = e0 + 64 * v + lane;
                dst[v] = ~0ull;
                if (e < total) {
                    const uint32_t lo = run_of_prefix(s_pref[wave], e);
                    const uint32_t i = e - s_pref[wave][lo];
                    rec[v] = arena_recs[s_src[wave][lo] + i];
                    dst[v] = s_dst[wave][lo] + i;
                }
            }
#pragma unroll
            for (int v = 0; v < 2; ++v)
                if (dst[v] != ~0ull) surv[dst[v]] = rec[v];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the chunk's LDS rows are free again
    }
}

// exclusive scan of q_cap into q_base (u64); out_total[0] = the sum.  One block of 1024 threads, any nq.
__global__ __launch_bounds__(1024) void seg_scan_kernel(const uint32_t *__restrict__ q_cap, uint32_t nq,
                                                        unsigned long long *__restrict__ q_base, unsigned long long *__restrict__ out_total) {
    const unsigned long long total = block_scan_chunked<unsigned long long, uint32_t>(
        nq, [&](uint32_t i) { return q_cap[i]; }, [&](uint32_t i, unsigned long long at, unsigned long long) { q_base[i] = at; });
    if (threadIdx.x == 0) out_total[0] = total;
}

// dense run directory of a stage: cells [0, ncells) of every query start empty
__global__ void clear_dir_kernel(RunRec *__restrict__ runs, uint32_t nq, const QSeg seg, uint32_t ncells) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nq * ncells) return;
    const uint32_t b = (uint32_t)(i / ncells), c = (uint32_t)(i - (uint64_t)b * ncells);
    RunRec z;
    z.pos = 0, z.slot = 0, z.base = 0, z.cnt = 0;
    runs[seg.at(b) + c] = z;
}

// sums the matrix-core scan's 64 counter pairs into out[0] (sub-tile steps) and out[1] (steps that took the exact path)
__global__ __launch_bounds__(64) void stat_fold_kernel(const unsigned long long *__restrict__ stat, unsigned long long *__restrict__ out) {
    unsigned long long a = stat[2 * threadIdx.x], b = stat[2 * threadIdx.x + 1];
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64), b += __shfl_xor(b, o, 64);
    if (threadIdx.x == 0) out[0] = a, out[1] = b;
}
