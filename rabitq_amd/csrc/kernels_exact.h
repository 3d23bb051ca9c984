// kernels_exact.h -- exact (brute-force) top-k over the stored rows: rq_exact_search* of include/rabitq_hip.h.
//
// The answer of query q is the topk smallest (Ord32(e), id) over the admitted rows with e < f32::MAX, where e is the ONE exact-order
// distance of the library (exact_l2_row, kernels_rerank.h: what rq_rerank returns).  Computing e for every (query, row) pair would run
// the f32 chain n * nq times; instead one pass over the rows (exact_scan_kernel) approximates every pair on the matrix cores and keeps
// the pairs that can still be in the answer, and only those get their exact distance (exact_dist_kernel) and are ranked
// (exact_select_kernel).
//
// Bound.  T_q is an upper bound of the topk-th smallest e of query q: the topk-th smallest exact distance over a SAMPLE of the admitted
// rows (every stride-th position; the same kernels, run over the sample without a bound) -- topk exact distances of real admitted rows
// -- or f32::MAX where the sample holds fewer than topk.  Every row of the answer has e <= T_q, so T_q changes the work and never
// the answer.
//
// Approximation.  a = (|x|^2 + |q'|^2) - 2 <x~, q~>, x~ / q~ the operands rounded to bf16 (round to nearest even), the inner product
// from v_mfma_f32_32x32x16_bf16 with f32 accumulation.  It is within
//     m = (2^-8 + (2 dim + 64) 2^-24) 1.05 (|x| + |q'|)^2
// of e: the argument of prefilter_bound (kernels_coarse.h) with the row's own norm in the place of Cmax -- the bf16 rounding of the
// two operands moves -2<x, q'> by at most (2^-6 + 2^-15) |x||q'| <= (2^-8 + 2^-17)(|x| + |q'|)^2, the f32 accumulation, the two norms
// and the reference's own chain are inside the second term, and the factor 1.05 is the only slack over the bf16 bound (LOAD-BEARING:
// do not tighten it).  A row of the answer therefore has a <= e + m <= T_q + m, and the scan keeps a pair unless a > T_q + m (plus
// the rounding of the comparison itself).  The test is written so that a NaN on either side KEEPS the pair: it goes to the exact
// distance, which decides.  A row whose |x|^2 is not a finite f32 (overflow, inf or NaN elements) is always kept for the same reason:
// its e may still be finite (a huge row next to a huge query).
//
// This header has two parts: the launch interface, which the host unit sees (host_exact.h), and the kernels, compiled only by
// inst_exact.hip (RQ_EXACT_KERNELS) -- the host unit's compile time stays what it was.
#pragma once
#include "common.h"

#define RQ_EXACT_NO_SEED 1u       // rq_exact_params_t.flags bit 0: every bound is f32::MAX
#define RQ_EXACT_NO_PREFILTER 2u  // bit 1: every admitted pair gets its exact distance
#define RQ_EXACT_QGROUP 4096u     // queries one scan launch streams against every row tile (their bf16 image stays in the L2)
#define RQ_EXACT_SELECT_SLOTS 4096u

struct ExactArgs {
    BaseView base;              // untiered, not split: row p at its position
    uint32_t dim;
    uint32_t n;                 // stored rows (positions are u32)
    uint32_t rows, stride;      // the launch covers rows v = 0 .. rows - 1 at positions v * stride (the scan: n, 1; the bound's sample: every stride-th)
    const uint32_t *map_ids;    // position -> id
    const uint32_t *allow;      // the filter's position bitmap, or null
    const float *qpad;          // nq x dim: q' (transformed, padded)
    uint16_t *qbf;              // nq32 x dim bf16 image of q' (rows past nq: zeros)
    float *qn2, *qsn;           // nq32: |q'|^2 and sqrt(|q'|^2) * 1.000001
    float *thr;                 // nq: T_q
    uint32_t nq, nq32;          // queries of this launch, rounded up to whole 32-query MFMA tiles
    uint32_t cap;               // candidate slots per query (range form: records of the launch's shared arena)
    union {
        uint32_t *cand;         // nq x cap: positions
        uint2 *rec;             // range form: cap records, x = query of the launch, y = position
    };
    union {
        unsigned int *cnt;      // nq: candidates emitted (keeps counting past cap: the overflow is cnt > cap)
        unsigned long long *rec_count;  // range form: ONE count of the records appended (likewise past cap)
    };
    unsigned long long *keys;   // nq x cap: ord32_biased(e) << 32 | id, ~0 = not in the answer (range form: cap keys, one per record)
    uint32_t topk;
    float *out_dist;            // nq x topk
    uint32_t *out_id, *out_n;
};

// bytes of dynamic LDS exact_scan_kernel<RT> needs at this dim (the tile image, then |x|^2, its scaled root and the admitted flag per row)
static inline size_t exact_scan_lds_bytes(uint32_t rt, uint32_t dim) { return (size_t)rt * 32 * ((size_t)dim * 2 + 16) + (size_t)rt * 32 * 12; }
#define RQ_EXACT_LDS_MAX (156u * 1024u)   // one block per CU (RT = 1: the wide dimensions); the CU has 160 KiB, the kernel a little static LDS of its own
#define RQ_EXACT_LDS_HALF (64u * 1024u)   // RT = 2, 4: two blocks per CU, and what a launch may ask for without a function attribute
// 32-row sub-tiles per block: as many as leave room for two blocks per CU; 0 = the tile does not fit at all (dim > 2432: the caller
// runs without the pre-filter)
static inline uint32_t exact_scan_subtiles(uint32_t dim) {
    if (exact_scan_lds_bytes(4, dim) <= RQ_EXACT_LDS_HALF) return 4;
    if (exact_scan_lds_bytes(2, dim) <= RQ_EXACT_LDS_HALF) return 2;
    return exact_scan_lds_bytes(1, dim) <= RQ_EXACT_LDS_MAX ? 1 : 0;
}

// the launches (inst_exact.hip)
hipError_t exact_set_attributes();
void launch_exact_prep(const ExactArgs &a, hipStream_t st);                                      // qbf, qn2, qsn of the launch's queries
void launch_exact_thr(const float *seed_dist, const uint32_t *seed_n, uint32_t nq, uint32_t topk, float *thr,
                      unsigned int *unfilled, hipStream_t st);                                   // T_q (seed_dist == null: f32::MAX)
void launch_exact_scan(const ExactArgs &a, bool prefilter, hipStream_t st);
void launch_exact_dist(const ExactArgs &a, hipStream_t st);
void launch_exact_select(const ExactArgs &a, hipStream_t st);

// ---- the range form (rq_exact_range_search*, host_exact_range.h) ----
// T_q is the query's radius and nothing cuts at a topk, so the answers are wildly uneven: the scan appends its kept pairs as
// (query, position) records to ONE arena shared by the launch's queries (work memory follows the pairs kept, not nq x the largest
// answer), one pass gives every record its exact distance and key and counts the hits per query, and after the prefix sum of the
// counts (range_scan_kernel, kernels_range.h) the live keys are scattered into per-query segments of exactly the hits.
// ExactArgs::topk / out_* are not read by these launches.
struct ExactSegments {
    uint32_t *hits;                  // nq: live keys per query (zeroed by the host)
    uint32_t *cursor;                // nq: the scatter's next free slot of every segment (zeroed by the host)
    const unsigned long long *lims;  // nq + 1: the segments' offsets
    unsigned long long *out;         // lims[nq] keys: the segments
};
void launch_exact_range_thr(const float *radius, uint32_t nq, float *thr, hipStream_t st);  // T_q = r_q, or a bound that keeps nothing (NaN, r_q <= 0)
void launch_exact_range_scan(const ExactArgs &a, bool prefilter, hipStream_t st);
void launch_exact_range_dist(const ExactArgs &a, uint32_t *hits, uint32_t records, hipStream_t st);
void launch_exact_range_scatter(const ExactArgs &a, const ExactSegments &sg, uint32_t records, hipStream_t st);

#ifdef RQ_EXACT_KERNELS
#include "kernels_rerank.h"

typedef __bf16 ex_bf16x8 __attribute__((ext_vector_type(8)));
typedef float ex_f32x16 __attribute__((ext_vector_type(16)));

// two f32 -> packed bf16, round to nearest even (the rounding of asg_bf16_pair, kernels_coarse.h)
__device__ __forceinline__ uint32_t ex_bf16_pair(float lo, float hi) {
    uint32_t a = __builtin_bit_cast(uint32_t, lo), b = __builtin_bit_cast(uint32_t, hi);
    a += 0x7FFFu + ((a >> 16) & 1u);
    b += 0x7FFFu + ((b >> 16) & 1u);
    return (a >> 16) | (b & 0xFFFF0000u);
}
// T + m for one (row, query) pair and the comparison's own rounding: prefilter_bound's arithmetic with the two roots taken once per
// row and once per query (xs = sqrt(|x|^2) 1.000001, qs likewise) and one margin where the coarse ranking needs two.  inf / NaN in,
// inf / NaN out.
__device__ __forceinline__ float ex_pair_bound(float T, float xs, float qs, float c) {
    const float rad = xs + qs;
    const float thr = T + c * (rad * rad);
    return thr + fabsf(thr) * 1.0e-6f;
}
__device__ __forceinline__ float ex_margin_factor(uint32_t dim) { return (0.00390625f + (float)(2 * dim + 64) * 5.9604645e-8f) * 1.05f; }

// One wave per query row of the launch (rows nq .. nq32 - 1 are padding: zeros): the bf16 image and the two norm terms.
__global__ __launch_bounds__(256) void exact_prep_kernel(const ExactArgs a) {
    const uint32_t lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.nq32) return;
    float s = 0.0f;
    for (uint32_t e = 2 * lane; e < a.dim; e += 128) {
        float x0 = 0.0f, x1 = 0.0f;
        if (q < a.nq) x0 = a.qpad[(uint64_t)q * a.dim + e], x1 = a.qpad[(uint64_t)q * a.dim + e + 1];
        s = fmaf(x0, x0, s), s = fmaf(x1, x1, s);
        reinterpret_cast<uint32_t *>(a.qbf)[((uint64_t)q * a.dim + e) >> 1] = ex_bf16_pair(x0, x1);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) a.qn2[q] = s, a.qsn[q] = sqrtf(s) * 1.000001f;
}

// T_q: the largest distance of a filled sample answer, else f32::MAX
__global__ __launch_bounds__(256) void exact_thr_kernel(const float *__restrict__ seed_dist, const uint32_t *__restrict__ seed_n, uint32_t nq,
                                                        uint32_t topk, float *__restrict__ thr, unsigned int *__restrict__ unfilled) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    float t = 3.4028234663852886e38f;
    if (seed_dist && seed_n[q] >= topk) {
        float mx = seed_dist[(uint64_t)q * topk];
        for (uint32_t i = 1; i < topk; ++i) mx = fmaxf(mx, seed_dist[(uint64_t)q * topk + i]);
        if (mx == mx) t = mx;
    }
    if (unfilled && t == 3.4028234663852886e38f) atomicAdd(unfilled, 1u);  // (no bound at all: every query counts)
    thr[q] = t;
}

// The scan: block b owns rows [32 RT b, 32 RT (b + 1)) and reads them ONCE -- eight lanes per row, 8 elements per lane and step,
// through RowRef, rounded to bf16 into the LDS image (row stride 2 dim + 16 bytes: the 32 lanes of a fragment read hit different
// banks), |x|^2 in f32 beside it.  Then its four waves stream the launch's 32-query tiles against the image (wave w: tiles w, w + 4,
// ...): the query fragments come from the bf16 image in global memory (L2-resident, one 16-byte load per lane and 16-dimension
// slab), the row fragments from LDS, RT MFMAs per slab.  Accumulator register r of lane (col, kh) is row (r & 3) + 8 (r >> 2) + 4 kh of
// the sub-tile against query col: everything per query is lane-private.  Kept pairs are appended to the query's slots -- one atomic
// per lane and tile for the lane's whole count; the count runs on past the capacity while the stores stop, and the host runs the
// launch again with what the count has learnt.  PRE = false (no pre-filter: the test hook, and dimensions whose tile does not fit):
// no image, no MFMA, every admitted row is kept.
// RANGE (rq_exact_range_search*): the same tile, MFMAs and margin with T_q = the radius; kept pairs go to the launch's shared arena
// as (query, position) records.  The lanes' counts are summed over the wave (an inclusive scan by shuffles: six steps per tile, next
// to dim / 16 x RT MFMAs) and ONE lane reserves the wave's records with one 64-bit atomic; again the count runs on past the capacity
// while the stores stop.  A query whose bound is not above zero (NaN or non-positive radius) emits nothing, wild rows included.
template <int RT, bool PRE, bool RANGE = false>
__global__ __launch_bounds__(256, (RT == 1 ? 1 : 2)) void exact_scan_kernel(const ExactArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ex_lds[];
    const uint32_t dim = a.dim, ROWB = dim * 2 + 16;
    const uint32_t TILEB = PRE ? RT * 32 * ROWB : 0u;
    float *xn2 = reinterpret_cast<float *>(ex_lds + TILEB), *xsn = xn2 + RT * 32;
    uint32_t *adm = reinterpret_cast<uint32_t *>(xsn + RT * 32);
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, kh = lane >> 5;
    const uint64_t tile0 = (uint64_t)blockIdx.x * (32 * RT);
    {
        const uint32_t sub = t & 7, rrow = t >> 3;
        bool any = false;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint32_t lr = rt * 32 + rrow;
            const uint64_t p = (tile0 + lr) * a.stride;
            bool ok = tile0 + lr < a.rows;
            if (ok && a.allow) ok = (a.allow[p >> 5] >> (p & 31)) & 1u;
            any |= ok;
            float s = 0.0f;
            if constexpr (PRE) {
                const RowRef rr = a.base.row_at(ok ? p : 0, dim);
                unsigned char *img = ex_lds + lr * ROWB;
                for (uint32_t pc = sub; pc < dim / 8; pc += 8) {
                    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (ok) rq_row_get8(rr, 8 * pc, v);
#pragma unroll
                    for (int i = 0; i < 8; ++i) s = fmaf(v[i], v[i], s);
                    *reinterpret_cast<uint4 *>(img + 16 * pc) =
                        make_uint4(ex_bf16_pair(v[0], v[1]), ex_bf16_pair(v[2], v[3]), ex_bf16_pair(v[4], v[5]), ex_bf16_pair(v[6], v[7]));
                }
                s += __shfl_xor(s, 1, 8), s += __shfl_xor(s, 2, 8), s += __shfl_xor(s, 4, 8);
            }
            if (sub == 0) xn2[lr] = s, xsn[lr] = sqrtf(s) * 1.000001f, adm[lr] = ok ? 1u : 0u;
        }
        if (!__syncthreads_or(any ? 1 : 0)) return;  // (also the barrier behind the image) nothing admitted in this tile
    }
    // this lane's 16 rows of every sub-tile: admitted mask, and whether |x|^2 is a finite f32
    uint32_t amask[RT], wild[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        amask[rt] = 0u, wild[rt] = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t lr = rt * 32 + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
            amask[rt] |= adm[lr] ? (1u << r) : 0u;
            if constexpr (PRE) wild[rt] |= xn2[lr] < 3.0e38f ? 0u : (1u << r);
        }
    }
    const float cm = ex_margin_factor(dim);
    const uint32_t ngroups = a.nq32 / 32;
    for (uint32_t g = wave; g < ngroups; g += 4) {
        const uint32_t q = 32 * g + col;
        uint32_t mine[RT];
        if constexpr (PRE) {
            ex_f32x16 acc[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt] = ex_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            const uint16_t *qb = a.qbf + (uint64_t)q * dim + 8 * kh;
            const unsigned char *img = ex_lds + col * ROWB + 16 * kh;
            for (uint32_t m = 0; m < dim / 16; ++m) {
                const ex_bf16x8 bf = __builtin_bit_cast(ex_bf16x8, *reinterpret_cast<const uint4 *>(qb + 16 * m));
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const ex_bf16x8 af = *reinterpret_cast<const ex_bf16x8 *>(img + rt * 32 * ROWB + 32 * m);
                    acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[rt], 0, 0, 0);
                }
            }
            const float qn = a.qn2[q], qs = a.qsn[q], T = q < a.nq ? a.thr[q] : 0.0f;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                uint32_t keep = wild[rt];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t lr = rt * 32 + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
                    const float ap = fmaf(-2.0f, acc[rt][r], xn2[lr] + qn);
                    keep |= !(ap > ex_pair_bound(T, xsn[lr], qs, cm)) ? (1u << r) : 0u;
                }
                mine[rt] = keep & amask[rt];
            }
        } else {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) mine[rt] = amask[rt];
        }
        if constexpr (RANGE) {
            // (the wave is whole here: the loop over g is uniform and nothing above leaves it)
            const bool live = q < a.nq && a.thr[q] > 0.0f;
            uint32_t c = 0;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                if (!live) mine[rt] = 0u;
                c += (uint32_t)__popc(mine[rt]);
            }
            uint32_t inc = c;  // inclusive prefix of the lanes' counts
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(inc, o, 64);
                if (lane >= (uint32_t)o) inc += up;
            }
            const uint32_t total = __shfl(inc, 63, 64);
            if (total == 0) continue;
            unsigned long long first = 0;
            if (lane == 63) first = atomicAdd(a.rec_count, (unsigned long long)total);
            unsigned long long at = __shfl(first, 63, 64) + (inc - c);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                uint32_t mk = mine[rt];
                while (mk) {
                    const uint32_t r = (uint32_t)__builtin_ctz(mk);
                    mk &= mk - 1u;
                    if (at < a.cap) a.rec[at] = make_uint2(q, ((uint32_t)tile0 + rt * 32 + (r & 3u) + 8u * (r >> 2) + 4u * kh) * a.stride);
                    ++at;
                }
            }
            continue;
        }
        if (q >= a.nq) continue;
        uint32_t c = 0;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) c += (uint32_t)__popc(mine[rt]);
        if (c == 0) continue;
        uint32_t at = atomicAdd(&a.cnt[q], c);
        uint32_t *slots = a.cand + (uint64_t)q * a.cap;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            uint32_t mk = mine[rt];
            while (mk) {
                const uint32_t r = (uint32_t)__builtin_ctz(mk);
                mk &= mk - 1u;
                if (at < a.cap) slots[at] = ((uint32_t)tile0 + rt * 32 + (r & 3u) + 8u * (r >> 2) + 4u * kh) * a.stride;
                ++at;
            }
        }
    }
}

// The range form's bounds: T_q = the radius; a NaN or non-positive radius admits nothing and must not reach the scan's test, which
// keeps a pair on a NaN -- such a query gets -f32::MAX, and the scan emits nothing for a bound that is not above zero.
__global__ __launch_bounds__(256) void exact_range_thr_kernel(const float *__restrict__ radius, uint32_t nq, float *__restrict__ thr) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q < nq) thr[q] = radius[q] > 0.0f ? radius[q] : -3.4028234663852886e38f;
}

// Exact distances of the arena's records: one pass over the m records, 128 per block and round, a pair of lanes per record
// (exact_l2_row).  A block sees many queries, so q' is read from qpad in global memory (the L2 holds the launch's queries).  The key
// of a record with e < T_q (the radius) and e < f32::MAX, ~0 for every other one (a NaN fails both), and the hits counted per query:
// a wave whose 32 records belong to one query -- the scan writes a lane's pairs of a tile side by side -- adds its count once.
__global__ __launch_bounds__(256) void exact_range_dist_kernel(const ExactArgs a, uint32_t *__restrict__ hit_cnt, uint32_t m) {
    const uint32_t dim = a.dim, hf = threadIdx.x & 1, lane = threadIdx.x & 63;
    const uint32_t rounds = (uint32_t)(((uint64_t)m + 127) / 128);
    for (uint32_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const uint64_t i = (uint64_t)rd * 128 + (threadIdx.x >> 1);
        const bool have = i < m;  // (the same for the two lanes of a pair)
        const uint2 rec = have ? a.rec[i] : make_uint2(0xFFFFFFFFu, 0u);
        bool hit = false;
        if (have) {
            const float e = exact_l2_row(a.base.row_at(rec.y, dim), a.qpad + (uint64_t)rec.x * dim, dim, hf);
            if (hf == 0) {
                hit = e < a.thr[rec.x] && e < 3.4028234663852886e38f;
                a.keys[i] = hit ? ((unsigned long long)ord32_biased(e) << 32) | a.map_ids[rec.y] : ~0ull;
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

// The live keys into their query's segment [lims[q], lims[q + 1]): one thread per record, the place from the segment's cursor.  The
// order inside a segment is whatever the atomics give; the segments are sorted afterwards (keys are unique: one per id).
__global__ __launch_bounds__(256) void exact_range_scatter_kernel(const uint2 *__restrict__ rec, const unsigned long long *__restrict__ keys,
                                                                  uint32_t m, const ExactSegments sg) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const unsigned long long key = keys[i];
        if (key == ~0ull) continue;
        const uint32_t q = rec[i].x;
        const unsigned long long o = sg.lims[q] + atomicAdd(&sg.cursor[q], 1u);
        if (o < sg.lims[q + 1]) sg.out[o] = key;
    }
}

// Exact distances of a query's candidates: blockIdx.x = query, the blocks of a query (gridDim.y) stride over its slots; q' in LDS, a
// pair of lanes per candidate (exact_l2_row: the library's one exact-order routine).  The key of a candidate with e <= T_q and
// e < f32::MAX, ~0 for every other one (a NaN fails both).
__global__ __launch_bounds__(256) void exact_dist_kernel(const ExactArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ex_lds[];
    float *q_lds = reinterpret_cast<float *>(ex_lds);
    const uint32_t q = blockIdx.x, dim = a.dim, hf = threadIdx.x & 1;
    const uint32_t m = a.cnt[q] < a.cap ? a.cnt[q] : a.cap;
    if (blockIdx.y * 128u >= m) return;
    for (uint32_t e = threadIdx.x; e < dim; e += 256) q_lds[e] = a.qpad[(uint64_t)q * dim + e];
    __syncthreads();
    const float T = a.thr[q];
    for (uint32_t i = blockIdx.y * 128 + (threadIdx.x >> 1); i < m; i += gridDim.y * 128) {
        const uint32_t pos = a.cand[(uint64_t)q * a.cap + i];
        const float e = exact_l2_row(a.base.row_at(pos, dim), q_lds, dim, hf);
        if (hf == 0) {
            const bool in = e <= T && e < 3.4028234663852886e38f;
            a.keys[(uint64_t)q * a.cap + i] = in ? ((unsigned long long)ord32_biased(e) << 32) | a.map_ids[pos] : ~0ull;
        }
    }
}

// One block per query: the topk smallest keys of its slots, ascending.  Live keys are appended to an LDS buffer; when another round
// might not fit, the buffer is sorted and cut to its topk smallest (a key cut there has topk smaller ones: it is not in the answer).
// The keys are unique (one per id), so the result does not depend on the order they arrive in.
__global__ __launch_bounds__(256) void exact_select_kernel(const ExactArgs a) {
    __shared__ unsigned long long buf[RQ_EXACT_SELECT_SLOTS];
    __shared__ uint32_t fill;
    const uint32_t q = blockIdx.x, t = threadIdx.x, topk = a.topk;
    const uint32_t m = a.cnt[q] < a.cap ? a.cnt[q] : a.cap;
    const unsigned long long *keys = a.keys + (uint64_t)q * a.cap;
    if (t == 0) fill = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < m; i0 += 256) {
        const unsigned long long key = i0 + t < m ? keys[i0 + t] : ~0ull;
        if (key != ~0ull) buf[atomicAdd(&fill, 1u)] = key;
        __syncthreads();
        const uint32_t f = fill;
        __syncthreads();  // everybody has read the count before the next round adds to it
        if (f + 256 > RQ_EXACT_SELECT_SLOTS) {  // (uniform)
            bitonic_sort_block(buf, f, [](unsigned long long v) { return v; });
            if (t == 0) fill = f < topk ? f : topk;
            __syncthreads();
        }
    }
    const uint32_t f = fill;
    bitonic_sort_block(buf, f, [](unsigned long long v) { return v; });
    __syncthreads();
    const uint32_t take = f < topk ? f : topk;
    for (uint32_t e = t; e < take; e += 256) {
        a.out_dist[(uint64_t)q * topk + e] = ord32_unbias((uint32_t)(buf[e] >> 32));
        a.out_id[(uint64_t)q * topk + e] = (uint32_t)buf[e];
    }
    if (t == 0) a.out_n[q] = take;
}
#endif  // RQ_EXACT_KERNELS
