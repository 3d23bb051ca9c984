// kernels_keyed.h -- postings of an integer column and the keyed exact search over them (host_keyed.h), wave64.
// Nothing here writes an array of the index.
//
// POSTINGS: the live positions of an index grouped by the value of one integer column.  Three passes over the column and the live
// bitmap: (1) every value is claimed in an open-addressing table of 2^23 u64 keys (integer atomicCAS, linear probing) and counted,
// (2) the occupied slots are compacted to (value, count, slot) for the host, which sorts them in the column's order and sends back
// every slot's first place, (3) every live position is stored at its value's cursor.  Passes 1 and 3 aggregate per wave over EQUAL
// values before they touch memory: the wave walks its distinct values (the first lane still waiting is the leader, its value is
// broadcast by readlane) and the leader issues ONE atomicAdd for all lanes that hold it -- a value that owns half the index costs
// n / 128 atomics on its address, not n / 2.  Every 64-bit pattern is a legal value: the table's empty mark, ~0, has the side
// entry count[RQ_POST_SLOTS].  The order of positions inside a value is whatever the atomics give; no search output depends on it.
//
// KEYED SCAN: keyed_scan_kernel<MODE, PRE>, one block of four waves per work item (keyed_plan.h: a tile of at most 32 queries that
// share a key, and a chunk of that key's postings).  The block stages its query tile once -- the bf16 image, row stride
// 2 dim + 16 bytes, |q'|^2, its scaled root and T_q --, then its waves take the chunk's 32-row tiles in turn.  Per tile: the 32
// positions are ONE coalesced load from the postings (the dependent chain is position -> row, nothing else; the next tile's
// positions are loaded before this tile's gather), the filter bit comes from the position bitmap, the rows are gathered eight lanes
// per row through fetch_src / fetch_load / fetch_widen, rounded to bf16 into the wave's slab with |x|^2 and its root from the same
// registers (at dim 64 into one of TWO slabs: the next tile's loads are issued before this tile's matrix pass, SLABS = 2), and
// dim / 16 v_mfma_f32_32x32x16_bf16 give a = (|x|^2 + |q'|^2) - 2 acc.  A pair is kept unless
// a > T_q + ex_margin_factor(dim) (|x| + |q'|)^2 -- the exact scan's test, rule for rule (kernels_exact.h: a NaN on either side keeps,
// a row whose |x|^2 is not finite is always kept, an unadmitted row never).  Kept positions go to the query's candidate slots: the
// two lanes of a query add their counts and ONE of them reserves the places (an integer atomicAdd per wave, query and tile); the
// count runs on past the capacity while the stores stop, and the host runs the launch again with what the count has learnt.
// Items without RQ_KEYED_MATRIX (small segments, the bound's sample) and PRE = false (RQ_EXACT_NO_PREFILTER, and dimensions whose
// tiles do not fit in LDS) skip the gather and the matrix pass: every admitted pair is kept.
// The candidates then go through exact_dist_kernel and exact_select_kernel unchanged (kernels_exact.h, by their launch interface).
// Vector loads and stores only.
#pragma once
#include "common.h"
#include "keyed_plan.h"

#define RQ_POST_SLOTS (1u << 23)
#define RQ_POST_MAX_VALUES (1u << 22)
#define RQ_POST_EMPTY (~0ull)
#define RQ_POST_NO_SLOT 0xFFFFFFFFu
#define RQ_KEYED_LDS_MAX (156u * 1024u)  // as RQ_EXACT_LDS_MAX: what a block may take of a CU's 160 KiB

struct PostArgs {
    const void *col;            // n elements of 4 or 8 bytes
    const uint32_t *live;       // the live position bitmap, or null (every row is live)
    uint64_t n;
    unsigned long long *keys;   // RQ_POST_SLOTS
    uint32_t *count;            // RQ_POST_SLOTS + 1: the counts, then the cursors; the last one is the side entry of the value ~0
    uint32_t *distinct;         // slots claimed
    uint32_t *pos_out;          // pass 3: the postings
    uint64_t rows;              // pass 3: live rows counted by pass 1 (nothing is stored at or past it)
};

struct KeyedArgs {
    BaseView base;              // untiered, not split: row p at its position
    uint32_t dim, row_bytes;
    const uint32_t *post;       // the postings
    const uint32_t *allow;      // the filter's position bitmap, or null
    const uint4 *items;         // KeyedItem
    const uint32_t *order;      // 32 x tiles: plan slot -> query, or RQ_KEYED_PAD
    uint32_t tiles;
    const float *qpad;          // nq x dim: q' (transformed, padded), in the call's order
    uint16_t *qbf;              // 32 tiles x dim: the bf16 image in plan order, zero rows behind a short tile
    float *qn2, *qsn;           // 32 tiles: |q'|^2 and sqrt(|q'|^2) * 1.000001
    const float *thr;           // nq: T_q
    uint32_t cap;               // candidate slots per query
    uint32_t *cand;             // nq x cap: positions
    unsigned int *cnt;          // nq: candidates emitted (keeps counting past cap)
};

// ---- the LDS layout of keyed_scan_kernel, shared by the host (which sizes the launch and picks the form) and the kernel ----
struct KeyedLds {
    uint32_t rowb;                                // image row stride
    uint32_t qimg, qn2, qsn, thr, qb, wave0;      // block offsets
    uint32_t slab, xn2, xsn, pos, adm, slab_bytes;  // offsets inside one buffer of a wave's region; the buffer's size
    uint32_t wave_bytes, total;
};
__host__ __device__ inline KeyedLds keyed_lds(uint32_t dim, bool pre, uint32_t slabs) {
    KeyedLds l{};
    l.rowb = dim * 2 + 16;
    uint32_t o = 0;
    l.qimg = o, o += pre ? 32 * l.rowb : 0;
    l.qn2 = o, o += pre ? 128 : 0;
    l.qsn = o, o += pre ? 128 : 0;
    l.thr = o, o += pre ? 128 : 0;
    l.qb = o, o += 128;
    l.wave0 = o;
    uint32_t w = 0;
    l.slab = w, w += pre ? 32 * l.rowb : 0;
    l.xn2 = w, w += pre ? 128 : 0;
    l.xsn = w, w += pre ? 128 : 0;
    l.pos = w, w += 128;
    l.adm = w, w += 128;
    l.slab_bytes = w, l.wave_bytes = slabs * w, l.total = o + 4 * l.wave_bytes;
    return l;
}
#define RQ_KEYED_LDS_TWO (78u * 1024u)  // two blocks per CU
// buffers per wave: a second slab only at dim 64 (the double form holds a lane's pieces of that dimension in registers), where it
// still leaves two blocks per CU
static inline uint32_t keyed_slabs(uint32_t dim) { return dim == 64 && keyed_lds(dim, true, 2).total <= RQ_KEYED_LDS_TWO ? 2u : 1u; }

// the launches (inst_keyed.hip)
hipError_t keyed_set_attributes();
void launch_post_pass(const PostArgs &a, bool wide, bool scatter, hipStream_t st);
void launch_post_compact(const PostArgs &a, uint4 *pairs, uint32_t cap, uint32_t *out_n, hipStream_t st);
void launch_post_cursor(const uint2 *slot_start, uint32_t nv, uint32_t *count, hipStream_t st);
void launch_keyed_clear(unsigned int *cnt, uint32_t n, hipStream_t st);
void launch_keyed_prep(const KeyedArgs &a, hipStream_t st);
void launch_keyed_scan(const KeyedArgs &a, uint32_t nitems, int row_kind, bool pre, uint32_t slabs, hipStream_t st);

#ifdef RQ_KEYED_KERNELS
#include "kernels_rerank.h"
#include "kernels_directory.h"  // fetch_src / fetch_load / fetch_widen: the by-id gather's row access
#include "exact_margin.h"       // ex_bf16_pair, ex_margin_factor: the exact scan's own

typedef __bf16 ky_bf16x8 __attribute__((ext_vector_type(8)));
typedef float ky_f32x16 __attribute__((ext_vector_type(16)));

// ---- postings ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t post_hash(uint64_t v) {
    v ^= v >> 33, v *= 0xFF51AFD7ED558CCDull, v ^= v >> 33;
    return (uint32_t)v & (RQ_POST_SLOTS - 1u);
}
// the slot of value v (one lane calls); claim: an absent value takes the first empty slot of its probe sequence -- unless the table
// already holds more values than a postings object may (the host then refuses the column; nothing loops on a full table)
__device__ __forceinline__ uint32_t post_slot(const PostArgs &a, uint64_t v, bool claim) {
    if (v == RQ_POST_EMPTY) return RQ_POST_SLOTS;
    uint32_t h = post_hash(v);
    for (uint32_t probes = 0; probes < RQ_POST_SLOTS; ++probes, h = (h + 1u) & (RQ_POST_SLOTS - 1u)) {
        const unsigned long long cur = __atomic_load_n(a.keys + h, __ATOMIC_RELAXED);
        if (cur == v) return h;
        if (cur != RQ_POST_EMPTY) continue;
        if (!claim || __atomic_load_n(a.distinct, __ATOMIC_RELAXED) > RQ_POST_MAX_VALUES) return RQ_POST_NO_SLOT;
        const unsigned long long old = atomicCAS(a.keys + h, RQ_POST_EMPTY, (unsigned long long)v);
        if (old == RQ_POST_EMPTY) {
            atomicAdd(a.distinct, 1u);
            return h;
        }
        if (old == v) return h;
    }
    return RQ_POST_NO_SLOT;
}
// Passes 1 (SCATTER = false: claim and count) and 3 (true: place): a wave takes 64 consecutive positions a round.
template <bool WIDE, bool SCATTER>
__global__ __launch_bounds__(256) void post_pass_kernel(const PostArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t p0 = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; p0 < a.n; p0 += (uint64_t)gridDim.x * 256) {
        const uint64_t p = p0 + lane;
        bool live = p < a.n;
        if (live && a.live) live = (a.live[p >> 5] >> (p & 31u)) & 1u;
        uint64_t v = 0;
        if (live) v = WIDE ? static_cast<const uint64_t *>(a.col)[p] : (uint64_t)static_cast<const uint32_t *>(a.col)[p];
        unsigned long long rem = __ballot(live);
        while (rem) {  // (uniform) one distinct value of the wave per turn
            const uint32_t leader = __builtin_amdgcn_readfirstlane((uint32_t)__builtin_ctzll(rem));
            // (readlane returns a signed int: each half goes through u32 before it is widened, or a low word with bit 31 set would
            // smear into the high word and the leader would never meet its own value)
            const uint32_t v0_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)leader);
            const uint32_t v0_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)leader);
            const uint64_t v0 = ((uint64_t)v0_hi << 32) | (uint64_t)v0_lo;
            const bool same = live && v == v0;
            const unsigned long long m = __ballot(same) | (1ull << leader);  // (the leader leaves the loop whatever happens)
            uint32_t base = RQ_POST_NO_SLOT;
            if (lane == leader) {
                const uint32_t slot = post_slot(a, v0, !SCATTER);
                if (slot != RQ_POST_NO_SLOT) base = atomicAdd(a.count + slot, (uint32_t)__popcll(m));
            }
            if constexpr (SCATTER) {
                base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader);
                const uint64_t at = (uint64_t)base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (same && base != RQ_POST_NO_SLOT && at < a.rows) a.pos_out[at] = (uint32_t)p;
            }
            rem &= ~m;
        }
    }
}
// Pass 2: the occupied slots (and the side entry) as (value low, value high, count, slot), in any order.
__global__ __launch_bounds__(256) void post_compact_kernel(const PostArgs a, uint4 *__restrict__ pairs, uint32_t cap, uint32_t *__restrict__ out_n) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i <= RQ_POST_SLOTS; i += gridDim.x * 256) {
        const unsigned long long key = i < RQ_POST_SLOTS ? a.keys[i] : RQ_POST_EMPTY;
        const uint32_t c = a.count[i];
        if (i < RQ_POST_SLOTS ? key == RQ_POST_EMPTY : c == 0u) continue;
        const uint32_t at = atomicAdd(out_n, 1u);
        if (at < cap) pairs[at] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), c, i);
    }
}
// The counts become cursors: slot_start[i] = (slot, first place of its value)
__global__ __launch_bounds__(256) void post_cursor_kernel(const uint2 *__restrict__ slot_start, uint32_t nv, uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < nv && slot_start[i].x <= RQ_POST_SLOTS) count[slot_start[i].x] = slot_start[i].y;
}

// ---- keyed search --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void keyed_clear_kernel(unsigned int *__restrict__ cnt, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) cnt[i] = 0u;
}
// what one wave wrote to LDS is read by its other lanes behind this (the waves of a block walk different tiles: no block barrier)
__device__ __forceinline__ void ky_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}
// T + m and the comparison's own rounding: ex_pair_bound's arithmetic (kernels_exact.h), operation for operation
__device__ __forceinline__ float ky_pair_bound(float T, float xs, float qs, float c) {
    const float rad = xs + qs;
    const float thr = T + c * (rad * rad);
    return thr + fabsf(thr) * 1.0e-6f;
}

// One wave per plan slot: exact_prep_kernel's arithmetic on the slot's query (a padding slot: zeros).
__global__ __launch_bounds__(256) void keyed_prep_kernel(const KeyedArgs a) {
    const uint32_t lane = threadIdx.x & 63u, slot = blockIdx.x * 4 + (threadIdx.x >> 6), dim = a.dim;
    if (slot >= a.tiles * 32u) return;
    const uint32_t b = a.order[slot];
    float s = 0.0f;
    for (uint32_t e = 2 * lane; e < dim; e += 128) {
        float x0 = 0.0f, x1 = 0.0f;
        if (b != RQ_KEYED_PAD) x0 = a.qpad[(uint64_t)b * dim + e], x1 = a.qpad[(uint64_t)b * dim + e + 1];
        s = fmaf(x0, x0, s), s = fmaf(x1, x1, s);
        reinterpret_cast<uint32_t *>(a.qbf)[((uint64_t)slot * dim + e) >> 1] = ex_bf16_pair(x0, x1);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) a.qn2[slot] = s, a.qsn[slot] = sqrtf(s) * 1.000001f;
}

// SLABS = 2 (dim 64 only: the one dimension at which two slabs a wave still leave two blocks per CU): the raw loads of tile t + 1
// are issued into registers BEFORE the MFMAs, the test and the stores of tile t, and are widened into the other slab behind them
// -- the gather's latency runs under the matrix pass of the tile before.  At dim 64 a lane holds 2 pieces of each of its 4 rows.
template <int MODE, bool PRE, int SLABS>
__global__ __launch_bounds__(256) void keyed_scan_kernel(const KeyedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ky_lds[];
    const KeyedLds L = keyed_lds(a.dim, PRE, SLABS);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, dim = a.dim, col = lane & 31u, kh = lane >> 5;
    const uint4 it = a.items[blockIdx.x];
    const uint32_t tile = it.x, first = it.y, rows = it.z, stride = it.w & 0x7FFFFFFFu;
    const bool matrix = PRE && (it.w & RQ_KEYED_MATRIX);  // (uniform)
    uint32_t *qb = reinterpret_cast<uint32_t *>(ky_lds + L.qb);
    // ---- the query tile, once per block ----
    if (tid < 32) qb[tid] = a.order[tile * 32u + tid];
    if constexpr (PRE) {
        if (matrix) {
            const uint32_t per_row = dim / 8;  // 16-byte pieces of an image row
            for (uint32_t i = tid; i < 32 * per_row; i += 256) {
                const uint32_t r = i / per_row, c = i - r * per_row;
                *reinterpret_cast<uint4 *>(ky_lds + L.qimg + r * L.rowb + 16 * c) =
                    reinterpret_cast<const uint4 *>(a.qbf + ((uint64_t)tile * 32 + r) * dim)[c];
            }
            if (tid < 32) {
                const uint32_t slot = tile * 32u + tid, b = a.order[slot];
                reinterpret_cast<float *>(ky_lds + L.qn2)[tid] = a.qn2[slot];
                reinterpret_cast<float *>(ky_lds + L.qsn)[tid] = a.qsn[slot];
                reinterpret_cast<float *>(ky_lds + L.thr)[tid] = b != RQ_KEYED_PAD ? a.thr[b] : 0.0f;
            }
        }
    }
    __syncthreads();
    unsigned char *wl = ky_lds + L.wave0 + wave * L.wave_bytes;
    const uint32_t b = qb[col];  // this lane's query (lanes col and col + 32 share it: 16 rows of a tile each)
    const uint32_t ntiles = (rows + 31u) / 32u;
    const float cm = ex_margin_factor(dim);
    const uint32_t sub = lane & 7u, rr = lane >> 3;  // the gather: eight lanes per row, eight rows a pass
    // buffer s of the wave: positions, admitted flags, slab, norms
    const auto wpos = [&](uint32_t s) { return reinterpret_cast<uint32_t *>(wl + L.pos + s * L.slab_bytes); };
    const auto wadm = [&](uint32_t s) { return reinterpret_cast<uint32_t *>(wl + L.adm + s * L.slab_bytes); };
    const auto wslab = [&](uint32_t s) { return wl + L.slab + s * L.slab_bytes; };
    const auto wxn2 = [&](uint32_t s) { return reinterpret_cast<float *>(wl + L.xn2 + s * L.slab_bytes); };
    const auto wxsn = [&](uint32_t s) { return reinterpret_cast<float *>(wl + L.xsn + s * L.slab_bytes); };
    // the posting of this lane's row of tile tw, or RQ_KEYED_PAD behind the chunk's end (no position is 2^32 - 1: n fits a u32)
    const auto load_pos = [&](uint32_t tw) -> uint32_t {
        const uint32_t v = tw * 32u + col;
        return tw < ntiles && v < rows ? a.post[(uint64_t)first + (uint64_t)v * stride] : RQ_KEYED_PAD;
    };
    // positions and admitted flags of a tile into buffer s -> anything admitted (an unadmitted row is never kept: it gathers row 0)
    const auto publish = [&](uint32_t p, uint32_t s) -> bool {
        bool ok = p != RQ_KEYED_PAD;
        if (ok && a.allow) ok = (a.allow[p >> 5] >> (p & 31u)) & 1u;
        if (kh == 0) wpos(s)[col] = ok ? p : 0u, wadm(s)[col] = ok ? 1u : 0u;
        ky_wave_sync();
        return __any(ok);
    };
    // one widened piece of row lr into the slab of buffer s, its squares added to sum
    const auto put = [&](uint4 raw, uint32_t lr, uint32_t lp, uint32_t s, float &sum) {
        const uint4 v = fetch_keep(fetch_widen<MODE>(raw, false, a.base.fmt), wadm(s)[lr] != 0u);
        const float x0 = __builtin_bit_cast(float, v.x), x1 = __builtin_bit_cast(float, v.y);
        const float x2 = __builtin_bit_cast(float, v.z), x3 = __builtin_bit_cast(float, v.w);
        sum = fmaf(x0, x0, sum), sum = fmaf(x1, x1, sum), sum = fmaf(x2, x2, sum), sum = fmaf(x3, x3, sum);
        *reinterpret_cast<uint2 *>(wslab(s) + lr * L.rowb + 8 * lp) = make_uint2(ex_bf16_pair(x0, x1), ex_bf16_pair(x2, x3));
    };
    const auto put_norm = [&](float sum, uint32_t lr, uint32_t s) {
        sum += __shfl_xor(sum, 1, 8), sum += __shfl_xor(sum, 2, 8), sum += __shfl_xor(sum, 4, 8);
        if (sub == 0) wxn2(s)[lr] = sum, wxsn(s)[lr] = sqrtf(sum) * 1.000001f;
    };
    // the whole gather of buffer s in one go (SLABS = 1)
    const auto gather = [&](uint32_t s) {
#pragma unroll
        for (uint32_t ps = 0; ps < 4; ++ps) {
            const uint32_t lr = ps * 8 + rr;
            const FetchSrc src = fetch_src<MODE>(a.base, wpos(s)[lr], dim, a.row_bytes);
            float sum = 0.0f;
            for (uint32_t lp = sub; lp < dim / 4; lp += 8) put(fetch_load<MODE>(src, lp, dim), lr, lp, s, sum);
            put_norm(sum, lr, s);
        }
        ky_wave_sync();
    };
    // the matrix pass and the keep test of buffer s, or (no matrix pass) every admitted pair; then the kept positions to their slots
    const auto finish = [&](uint32_t s, bool mfma) {
        uint32_t amask = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) amask |= wadm(s)[(uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh] ? (1u << r) : 0u;
        uint32_t mine = amask;
        if constexpr (PRE) {
            if (mfma) {
                const float *xn2 = wxn2(s), *xsn = wxsn(s);
                // accumulator register r of lane (col, kh) is row (r & 3) + 8 (r >> 2) + 4 kh of the tile against query col (kernels_exact.h)
                ky_f32x16 acc = ky_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                const unsigned char *ai = wslab(s) + col * L.rowb + 16 * kh, *bi = ky_lds + L.qimg + col * L.rowb + 16 * kh;
                for (uint32_t m = 0; m < dim / 16; ++m) {
                    const ky_bf16x8 af = *reinterpret_cast<const ky_bf16x8 *>(ai + 32 * m), bf = *reinterpret_cast<const ky_bf16x8 *>(bi + 32 * m);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
                }
                const float qn = reinterpret_cast<const float *>(ky_lds + L.qn2)[col], qs = reinterpret_cast<const float *>(ky_lds + L.qsn)[col];
                const float T = reinterpret_cast<const float *>(ky_lds + L.thr)[col];
                uint32_t keep = 0u;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
                    const float ap = fmaf(-2.0f, acc[r], xn2[lr] + qn);
                    keep |= !(xn2[lr] < 3.0e38f) || !(ap > ky_pair_bound(T, xsn[lr], qs, cm)) ? (1u << r) : 0u;
                }
                mine = keep & amask;
            }
        }
        // the two lanes of a query add their counts, the lower one reserves the places of both
        if (b == RQ_KEYED_PAD) mine = 0u;
        const uint32_t c = (uint32_t)__popc(mine), other = __shfl_xor(c, 32, 64);
        uint32_t at = 0u;
        if (kh == 0 && c + other) at = atomicAdd(&a.cnt[b], c + other);
        at = __shfl(at, col, 64) + (kh ? other : 0u);
        uint32_t *slots = a.cand + (uint64_t)(b != RQ_KEYED_PAD ? b : 0u) * a.cap;
        const uint32_t *pos = wpos(s);
        while (mine) {
            const uint32_t r = (uint32_t)__builtin_ctz(mine);
            mine &= mine - 1u;
            if (at < a.cap) slots[at] = pos[(r & 3u) + 8u * (r >> 2) + 4u * kh];
            ++at;
        }
    };
    uint32_t nxt = load_pos(wave);
    if constexpr (PRE && SLABS == 2) {
        if (matrix) {  // (dim 64: pieces sub and sub + 8 of each of the lane's four rows)
            uint4 raw[4][2];
            const auto issue = [&](uint32_t s) {
#pragma unroll
                for (uint32_t ps = 0; ps < 4; ++ps) {
                    const FetchSrc src = fetch_src<MODE>(a.base, wpos(s)[ps * 8 + rr], dim, a.row_bytes);
                    raw[ps][0] = fetch_load<MODE>(src, sub, dim), raw[ps][1] = fetch_load<MODE>(src, sub + 8, dim);
                }
            };
            const auto land = [&](uint32_t s) {
#pragma unroll
                for (uint32_t ps = 0; ps < 4; ++ps) {
                    float sum = 0.0f;
                    put(raw[ps][0], ps * 8 + rr, sub, s, sum), put(raw[ps][1], ps * 8 + rr, sub + 8, s, sum);
                    put_norm(sum, ps * 8 + rr, s);
                }
                ky_wave_sync();
            };
            uint32_t s = 0;
            bool any = false;
            if (wave < ntiles) {  // (uniform per wave) the first tile: nothing to hide it under
                const uint32_t p = nxt;
                nxt = load_pos(wave + 4);
                any = publish(p, 0);
                issue(0), land(0);
            }
            for (uint32_t tw = wave; tw < ntiles; tw += 4, s ^= 1u) {
                const bool more = tw + 4 < ntiles;
                bool any_next = false;
                ky_wave_sync();  // the tile before this one has been read out of buffer s ^ 1
                if (more) {  // the next tile's rows are asked for before this tile's matrix pass
                    const uint32_t p = nxt;
                    nxt = load_pos(tw + 8);
                    any_next = publish(p, s ^ 1u);  // (buffer s ^ 1 was last read by the tile before this one: program order)
                    issue(s ^ 1u);
                }
                if (any) finish(s, true);
                if (more) land(s ^ 1u);
                any = any_next;
            }
            return;
        }
    }
    for (uint32_t tw = wave; tw < ntiles; tw += 4) {  // (uniform per wave)
        const uint32_t p = nxt;
        nxt = load_pos(tw + 4);  // the next tile's positions are on their way before this tile's rows are asked for
        ky_wave_sync();          // the previous tile's positions and fragments have been read
        if (!publish(p, 0)) continue;
        if constexpr (PRE) {
            if (matrix) gather(0);
        }
        finish(0, matrix);
    }
}
#endif  // RQ_KEYED_KERNELS
