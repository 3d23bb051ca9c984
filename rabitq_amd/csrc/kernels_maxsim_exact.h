// kernels_maxsim_exact.h -- exact multi-vector search (host_maxsim_exact.h), wave64: the true topk documents of a
// postings object by §4.23's chamfer, over ALL of its segments.  Nothing here writes an array of the index.
//
// THE CONTRACT (include/rabitq_hip.h states it; tests/maxsim_exact_model.py is its model): the topk segments with the smallest
// (ord32_biased(chamfer), segment number), chamfer bit for bit maxsim_score_keyed_kernel's.  Every score that reaches an output IS
// that kernel's: what this file adds decides only which documents it is asked for, and proves that the true topk are among them.
//
// PHASE 1, the bound pass.  maxsim_bound_prep_kernel writes, for the queries of a pass, the tokens' bf16 image in the operand layout
// of v_mfma_f32_32x32x16_bf16 (row stride 2 dim + 16, zero rows behind T_b up to the 32-token tile), |q'|^2 and its scaled root
// (ms_stage_tokens' arithmetic) into workspace memory.  maxsim_bound_kernel<MODE, SLABS>: blocks of four waves; grid x runs over
// work units -- unit u holds the segments whose first posting lies in [u R, (u + 1) R), found by two bisections of the segment
// starts, so a run of short documents is one unit and a long document shares its unit only with what starts before it --, grid y
// over chunks of Bc queries.  The block stages its chunk's image (LDS where it fits, else read through the L2) and norms; its waves
// take documents from a ticket counter (the return value schedules, nothing else) and a document is one wave's.  A wave loads 32
// positions of the postings in one coalesced load a tile ahead, gathers the rows through fetch_src / fetch_load / fetch_widen into
// its slab as bf16 with |x|^2 and its root (dim 64: the second slab takes the next tile's rows under this tile's matrix pass, by
// ms_tile_issue64 / ms_tile_land64), and multiplies the tile against EVERY token tile of the chunk's Bc queries: a gathered row
// serves Bc T tokens.  a = (|x|^2 + |q'|^2) - 2 acc, m = ex_margin_factor(dim) (|x| + |q'|)^2; per token the minimum of a - m and
// of a + m over the lane's 16 rows, one exchange between the lane halves, the minimum into the wave's own lo[Bc][T32] / hi[Bc][T32]
// (no atomic).  Masked rows take no part; a row whose |x|^2 is not finite, and a NaN bound, make lo = -inf and never lower hi.  At
// the document's end lane b sums its T_b lo and hi values in ascending t from +0.0f: L[b][seg] <= chamfer <= U[b][seg] (f32
// addition is monotone in each operand); a NaN sum gives L = -inf, U = +inf.
// PHASE 2.  maxsim_bound_threshold_kernel: tau_b = the topk-th smallest U[b][.] by its ordered image (radix select, four passes of
// LDS histograms; fewer than topk segments: +inf).  maxsim_bound_compact_kernel: the segments with !(L > tau_b) in ascending order.
// maxsim_exact_round_kernel hands a round of them to maxsim_score_keyed_kernel as it stands; maxsim_exact_merge_kernel sorts a
// round's scored documents together with the running topk (bitonic_sort_block, 2048 at a time) and writes the outputs at the end.
// Vector loads and stores only.
#pragma once
#include "kernels_maxsim.h"

#define RQ_MSX_MAX_BC 32u          // queries of a chunk (a lane per query sums at a document's end)
#define RQ_MSX_ROUND_SLOTS 16384u  // candidate slots per query of one scoring round
#define RQ_MSX_SORT 2048u          // scored documents the merge takes at a time

struct MaxsimBoundArgs {
    const float *tok;            // the pass's transformed, padded tokens: nq x T x dim
    const uint32_t *n_tokens;    // nq, nullable (= T)
    uint32_t nq, T, dim;         // nq: the queries of this pass
    uint32_t Bc, img_lds;        // queries per chunk; 1: the chunk's image is staged in LDS
    unsigned char *img;          // nq x T32 rows of 2 dim + 16 bytes
    float *qn2, *qsn;            // nq x T32
    const uint32_t *post, *starts;
    uint32_t nv, unit_rows;      // segments; R
    BaseView base;
    float *L, *U;                // nq x nv
    uint32_t topk, all;          // all: every segment survives (no bound pass ran)
    float *tau;                  // nq
    uint32_t *surv, *surv_n;     // nq x nv ascending; nq
    unsigned long long *totals;  // {the largest surv_n, their sum}, preset to 0
};

// ---- the block's LDS, shared by the host (which picks Bc and the form) and the kernel: MaxsimLds' fields where the tile routines
// of kernels_maxsim.h read them (slab, xn2, xsn, ring, buf2 of a wave; img, qn2, qsn of the block), lo / hi beside them ----
struct MaxsimBoundLds {
    MaxsimLds l;
    uint32_t lo, hi;  // offsets inside a wave's region: Bc x T32 floats each
};
__host__ __device__ inline MaxsimBoundLds maxsim_bound_lds(uint32_t dim, uint32_t T, uint32_t Bc, bool img_lds, uint32_t slabs) {
    MaxsimBoundLds b{};
    MaxsimLds &l = b.l;
    l.rowb = dim * 2 + 16, l.t32 = (T + 31u) & ~31u;
    uint32_t o = 0;
    l.img = o, o += img_lds ? Bc * l.t32 * l.rowb : 0;
    l.qn2 = o, o += Bc * l.t32 * 4;
    l.qsn = o, o += Bc * l.t32 * 4;
    l.wave0 = o;
    uint32_t w = 0;
    l.slab = w, w += 32 * l.rowb;
    l.xn2 = w, w += 128;
    l.xsn = w, w += 128;
    l.ring = w, w += 128 * 4;
    b.lo = w, w += Bc * l.t32 * 4;
    b.hi = w, w += Bc * l.t32 * 4;
    l.buf2 = w, w += slabs == 2 ? 32 * l.rowb + 256 : 0;
    l.wave_bytes = w, l.total = o + 4 * w;
    return b;
}
// Bc and the form: the largest chunk whose image fits beside the waves' regions with two blocks on a CU; where not even two queries'
// images do, the image stays in workspace memory (the L2 holds it) and Bc follows the lo / hi arrays alone; a shape whose one-query
// block passes RQ_MAXSIM_LDS_MAX has no bound pass (-> false).
static inline bool maxsim_bound_plan(uint32_t dim, uint32_t T, uint32_t *Bc, uint32_t *img_lds, uint32_t *slabs, uint32_t *lds) {
    const auto fit = [&](bool in_lds, uint32_t s, uint32_t cap) {
        uint32_t b = 0;
        while (b < RQ_MSX_MAX_BC && maxsim_bound_lds(dim, T, b + 1, in_lds, s).l.total <= cap) ++b;
        return b;
    };
    const uint32_t s = dim == 64 ? 2u : 1u;
    uint32_t b = fit(true, s, RQ_MAXSIM_LDS_TWO);
    *img_lds = 1u, *slabs = s;
    if (b < 2) {
        const uint32_t g = fit(false, s, RQ_MAXSIM_LDS_TWO);
        if (g > b) b = g, *img_lds = 0u;
    }
    if (b == 0) b = fit(false, 1u, RQ_MAXSIM_LDS_MAX) ? 1u : 0u, *img_lds = 0u, *slabs = 1u;
    *Bc = b;
    *lds = b ? maxsim_bound_lds(dim, T, b, *img_lds != 0, *slabs).l.total : 0u;
    return b != 0;
}

#define RQ_MSX_WORK_BYTES (256ull << 20)  // L, U and the survivors of one pass: 12 bytes per (query, segment)
// How a call is cut (plain host arithmetic): the queries of a pass from the work memory, a whole number of chunks where the bound
// pass runs; the rows of a work unit so that a large corpus gives a few thousand units and a small one still more than one block.
struct MaxsimExactCut {
    uint32_t pass_queries, unit_rows, units;
};
static inline MaxsimExactCut maxsim_exact_cut(uint32_t nq, uint64_t nv, uint64_t postings, uint32_t Bc /* 0: no bound pass */) {
    MaxsimExactCut c{};
    uint64_t p = RQ_MSX_WORK_BYTES / (12ull * (nv ? nv : 1ull));
    p = p < 1 ? 1 : p > 32768 ? 32768 : p;  // (a pass's queries are a grid's y extent, too)
    if (Bc && p > Bc) p -= p % Bc;
    c.pass_queries = (uint32_t)(p < nq ? p : nq ? nq : 1u);
    uint64_t r = postings / 8192;
    r = r < 1024 ? 1024 : r > 65536 ? 65536 : r;
    c.unit_rows = (uint32_t)r;
    c.units = (uint32_t)((postings + r - 1) / r);
    return c;
}

// the launches (inst_maxsim_exact.hip)
hipError_t maxsim_exact_set_attributes();
void launch_maxsim_bound_prep(const MaxsimBoundArgs &a, hipStream_t st);
void launch_maxsim_bound(const MaxsimBoundArgs &a, int row_kind, uint32_t slabs, uint32_t units, size_t lds, hipStream_t st);
void launch_maxsim_bound_threshold(const MaxsimBoundArgs &a, hipStream_t st);
void launch_maxsim_bound_compact(const MaxsimBoundArgs &a, hipStream_t st);
void launch_maxsim_exact_round(const MaxsimBoundArgs &a, uint32_t first, uint32_t slots, uint32_t *cand, uint32_t *cand_n, hipStream_t st);
void launch_maxsim_exact_merge(const MaxsimKeyedArgs &k, unsigned long long *run, uint32_t *run_n, bool first, bool last, hipStream_t st);

#ifdef RQ_MAXSIM_EXACT_KERNELS
// One wave per token row of the pass: the image row, |q'|^2 and its scaled root (ms_stage_tokens' arithmetic, token for token).
__global__ __launch_bounds__(256) void maxsim_bound_prep_kernel(const MaxsimBoundArgs a) {
    const uint32_t lane = threadIdx.x & 63u, dim = a.dim, t32 = (a.T + 31u) & ~31u, rowb = dim * 2 + 16;
    const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (uint64_t)a.nq * t32) return;
    const uint32_t b = (uint32_t)(g / t32), t = (uint32_t)(g % t32);
    const uint32_t tb = a.n_tokens ? a.n_tokens[b] : a.T, Tb = tb < a.T ? tb : a.T;
    const float *tg = a.tok + (uint64_t)b * a.T * dim;
    unsigned char *row = a.img + g * rowb;
    float s = 0.0f;
    for (uint32_t e = 2 * lane; e < dim; e += 128) {
        float x0 = 0.0f, x1 = 0.0f;
        if (t < Tb) x0 = tg[(uint64_t)t * dim + e], x1 = tg[(uint64_t)t * dim + e + 1];
        s = fmaf(x0, x0, s), s = fmaf(x1, x1, s);
        *reinterpret_cast<uint32_t *>(row + 2 * e) = ex_bf16_pair(x0, x1);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        a.qn2[g] = s, a.qsn[g] = sqrtf(s) * 1.000001f;
        *reinterpret_cast<uint4 *>(row + 2 * dim) = make_uint4(0u, 0u, 0u, 0u);  // (the row's padding: staged with it, never multiplied)
    }
}

// What a wave of the bound pass carries besides MaxsimWave.
struct MaxsimBoundWave {
    float *lo, *hi;          // the wave's Bc x T32 minima
    const uint32_t *tb;      // the chunk's T_b (block LDS)
    uint32_t nb, q0;         // queries of this chunk; the first of them
};

// The ring's rows [head, head + n) into the slab as bf16 with their norms: ms_tile_mfma's gather, operation for operation.
template <int MODE>
__device__ __forceinline__ void mb_gather(const MaxsimArgs &a, const MaxsimLds &L, MaxsimWave &w, uint32_t head, uint32_t n) {
    const uint32_t dim = a.dim, ROWB = L.rowb, sub = w.lane & 7u, rr = w.lane >> 3;
    const uint32_t *ring = reinterpret_cast<const uint32_t *>(w.lds + L.ring);
    unsigned char *slab = w.lds + L.slab;
    float *xn2 = reinterpret_cast<float *>(w.lds + L.xn2), *xsn = reinterpret_cast<float *>(w.lds + L.xsn);
    const uint32_t row_bytes = (uint32_t)RowSpec{a.base.fmt}.row_bytes(dim);
    ms_wave_sync();  // the previous tile's fragments have been read
#pragma unroll
    for (uint32_t ps = 0; ps < 4; ++ps) {
        const uint32_t lr = ps * 8 + rr;
        const bool ok = lr < n;
        const FetchSrc src = fetch_src<MODE>(a.base, ring[(head + (ok ? lr : 0u)) & 127u], dim, row_bytes);
        float s = 0.0f;
        for (uint32_t lp = sub; lp < dim / 4; lp += 8) {
            const uint4 v = fetch_keep(fetch_widen<MODE>(fetch_load<MODE>(src, lp, dim), false, a.base.fmt), ok);
            const float x0 = __builtin_bit_cast(float, v.x), x1 = __builtin_bit_cast(float, v.y);
            const float x2 = __builtin_bit_cast(float, v.z), x3 = __builtin_bit_cast(float, v.w);
            s = fmaf(x0, x0, s), s = fmaf(x1, x1, s), s = fmaf(x2, x2, s), s = fmaf(x3, x3, s);
            *reinterpret_cast<uint2 *>(slab + lr * ROWB + 8 * lp) = make_uint2(ex_bf16_pair(x0, x1), ex_bf16_pair(x2, x3));
        }
        s += __shfl_xor(s, 1, 8), s += __shfl_xor(s, 2, 8), s += __shfl_xor(s, 4, 8);
        if (sub == 0) xn2[lr] = s, xsn[lr] = sqrtf(s) * 1.000001f;
    }
    ms_wave_sync();
}

// A gathered tile of n rows (the slab at boff) against every token tile of the chunk's queries: the bounds into lo / hi.
// IMG_LDS: the image is the block's (blk + L.img), else the pass's in workspace memory.
template <bool IMG_LDS>
__device__ __forceinline__ void mb_tile_matrix(const MaxsimBoundArgs &a, const MaxsimLds &L, const MaxsimWave &w, const MaxsimBoundWave &bw,
                                               const unsigned char *blk, uint32_t boff, uint32_t n) {
    const uint32_t dim = a.dim, ROWB = L.rowb, col = w.lane & 31u, kh = w.lane >> 5;
    const unsigned char *slab = w.lds + L.slab + boff;
    const float *xn2 = reinterpret_cast<const float *>(w.lds + L.xn2 + boff), *xsn = reinterpret_cast<const float *>(w.lds + L.xsn + boff);
    const float *qn2 = reinterpret_cast<const float *>(blk + L.qn2), *qsn = reinterpret_cast<const float *>(blk + L.qsn);
    // this lane's 16 rows: register r is row (r & 3) + 8 (r >> 2) + 4 kh of the tile (the accumulator layout, kernels_exact.h)
    uint32_t valid = 0u, wild = 0u;
    float xn[16], xs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
        xn[r] = xn2[lr], xs[r] = xsn[lr];
        valid |= lr < n ? (1u << r) : 0u;
        wild |= xn[r] < 3.0e38f ? 0u : (1u << r);
    }
    const bool open = (valid & wild) != 0u;  // a row whose |x|^2 is not finite: no lower bound for any token
    const uint32_t plain = valid & ~wild;
    const float cm = ex_margin_factor(dim), inf = __builtin_inff();
    for (uint32_t b = 0; b < bw.nb; ++b) {
        const uint32_t ntt = (bw.tb[b] + 31u) >> 5;
        for (uint32_t tt = 0; tt < ntt; ++tt) {
            const uint32_t t = tt * 32 + col, at = b * L.t32 + t;
            ms_f32x16 acc = ms_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            const unsigned char *ai = slab + col * ROWB + 16 * kh;
            const unsigned char *bi = (IMG_LDS ? blk + L.img + (uint64_t)at * ROWB : a.img + ((uint64_t)(bw.q0 + b) * L.t32 + t) * ROWB) + 16 * kh;
            for (uint32_t m = 0; m < dim / 16; ++m) {
                const ms_bf16x8 af = *reinterpret_cast<const ms_bf16x8 *>(ai + 32 * m), bf = *reinterpret_cast<const ms_bf16x8 *>(bi + 32 * m);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
            }
            const float qn = qn2[at], qs = qsn[at];
            float l = inf, u = inf;
            bool nan = open;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float ap = fmaf(-2.0f, acc[r], xn[r] + qn), rad = xs[r] + qs, mg = cm * (rad * rad);
                const float h = ap + mg, g = ap - mg;
                if ((plain >> r) & 1u) {
                    u = h < u ? h : u;  // (a NaN bound never lowers hi)
                    l = g < l ? g : l;
                    nan |= g != g;
                }
            }
            l = nan ? -inf : l;
            {
                const float ou = __shfl_xor(u, 32, 64), ol = __shfl_xor(l, 32, 64);
                u = ou < u ? ou : u, l = ol < l ? ol : l;
            }
            if (kh == 0) {  // (a lane per token of the tile; the wave's own arrays: program order between tiles)
                const float pl = bw.lo[at], pu = bw.hi[at];
                bw.lo[at] = l < pl ? l : pl, bw.hi[at] = u < pu ? u : pu;
            }
        }
    }
}

// One document: the postings [start, start + len) walked once, 32 a tile, as ms_walk_keyed walks them (the position load a tile
// ahead; SLABS = 2: the next tile's raw rows in flight under this tile's matrix pass).
template <int MODE, int SLABS, bool IMG_LDS>
__device__ __forceinline__ void mb_walk(const MaxsimBoundArgs &a, const MaxsimArgs &ma, const MaxsimLds &L, MaxsimWave &w, const MaxsimBoundWave &bw,
                                        const unsigned char *blk, uint32_t start, uint32_t len) {
    uint32_t *ring = reinterpret_cast<uint32_t *>(w.lds + L.ring);
    const uint32_t ntile = (len + 31u) >> 5, col = w.lane & 31u;
    const auto load_pos = [&](uint32_t t) -> uint32_t {
        const uint64_t v = (uint64_t)t * 32u + col;
        return v < len ? a.post[(uint64_t)start + v] : 0u;
    };
    const auto publish = [&](uint32_t t, uint32_t p) {  // (ring segment t & 3 was last read by tile t - 4: program order)
        if (w.lane < 32) ring[(t & 3u) * 32u + col] = p;
        ms_wave_sync();
    };
    const auto rows_of = [&](uint32_t t) { return len - t * 32u < 32u ? len - t * 32u : 32u; };
    uint32_t nxt = load_pos(0);
    if constexpr (SLABS == 2) {
        uint4 raw[4][2];
        publish(0, nxt);
        nxt = load_pos(1);
        ms_tile_issue64<MODE>(ma, L, w, 0u, rows_of(0), raw);  // the first tile: nothing to hide it under
        ms_tile_land64<MODE>(ma, L, w, 0u, rows_of(0), raw);
        for (uint32_t t = 0; t < ntile; ++t) {
            const bool more = t + 1 < ntile;
            const uint32_t here = (t & 1u) * L.buf2, there = L.buf2 - here;
            ms_wave_sync();  // tile t's slab is written; the tile before has been read out of the other one
            if (more) {      // the next tile's rows are asked for before this tile's matrix pass
                const uint32_t p = nxt;
                nxt = load_pos(t + 2);
                publish(t + 1, p);
                ms_tile_issue64<MODE>(ma, L, w, ((t + 1) & 3u) * 32u, rows_of(t + 1), raw);
            }
            mb_tile_matrix<IMG_LDS>(a, L, w, bw, blk, here, rows_of(t));
            if (more) ms_tile_land64<MODE>(ma, L, w, there, rows_of(t + 1), raw);
        }
    } else {
        for (uint32_t t = 0; t < ntile; ++t) {
            const uint32_t p = nxt;
            nxt = load_pos(t + 1);  // on its way before this tile's rows are asked for
            publish(t, p);
            mb_gather<MODE>(ma, L, w, (t & 3u) * 32u, rows_of(t));
            mb_tile_matrix<IMG_LDS>(a, L, w, bw, blk, 0u, rows_of(t));
        }
    }
}

// the first segment whose first posting is at or behind row r (starts[0 .. nv) ascending)
__device__ __forceinline__ uint32_t mb_first_segment(const uint32_t *starts, uint32_t nv, uint64_t r) {
    uint32_t lo = 0, hi = nv;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (starts[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int MODE, int SLABS>
__global__ __launch_bounds__(256, 2) void maxsim_bound_kernel(const MaxsimBoundArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mb_lds[];
    __shared__ uint32_t s_ticket, s_tb[RQ_MSX_MAX_BC];
    const MaxsimBoundLds BL = maxsim_bound_lds(a.dim, a.T, a.Bc, a.img_lds != 0, SLABS);
    const MaxsimLds &L = BL.l;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q0 = blockIdx.y * a.Bc, nb = a.nq - q0 < a.Bc ? a.nq - q0 : a.Bc;
    // the unit: the segments whose first posting lies in [u R, (u + 1) R)  (uniform; a unit without one ends before any barrier)
    const uint64_t r0 = (uint64_t)blockIdx.x * a.unit_rows;
    const uint32_t s0 = __builtin_amdgcn_readfirstlane(mb_first_segment(a.starts, a.nv, r0));
    const uint32_t s1 = __builtin_amdgcn_readfirstlane(mb_first_segment(a.starts, a.nv, r0 + a.unit_rows));
    if (s0 >= s1) return;
    {   // ---- the chunk's image and norms, once per block ----
        const uint64_t g0 = (uint64_t)q0 * L.t32;
        if (a.img_lds) {
            const uint4 *src = reinterpret_cast<const uint4 *>(a.img + g0 * L.rowb);
            uint4 *dst = reinterpret_cast<uint4 *>(mb_lds + L.img);
            for (uint32_t i = tid; i < nb * L.t32 * (L.rowb / 16); i += 256) dst[i] = src[i];
        }
        float *qn2 = reinterpret_cast<float *>(mb_lds + L.qn2), *qsn = reinterpret_cast<float *>(mb_lds + L.qsn);
        for (uint32_t i = tid; i < nb * L.t32; i += 256) qn2[i] = a.qn2[g0 + i], qsn[i] = a.qsn[g0 + i];
        if (tid < nb) {
            const uint32_t tb = a.n_tokens ? a.n_tokens[q0 + tid] : a.T;
            s_tb[tid] = tb < a.T ? tb : a.T;
        }
        if (tid == 0) s_ticket = 0u;
    }
    __syncthreads();
    MaxsimArgs ma{};  // what the tile routines of kernels_maxsim.h read
    ma.dim = a.dim, ma.base = a.base;
    MaxsimWave w{};
    w.lds = mb_lds + L.wave0 + wave * L.wave_bytes, w.lane = lane;
    MaxsimBoundWave bw{reinterpret_cast<float *>(w.lds + BL.lo), reinterpret_cast<float *>(w.lds + BL.hi), s_tb, nb, q0};
    const float inf = __builtin_inff();
    for (;;) {  // the unit's documents, one ticket each (uniform per wave)
        uint32_t ticket = 0u;
        if (lane == 0) ticket = atomicAdd(&s_ticket, 1u);
        ticket = __builtin_amdgcn_readfirstlane(ticket);
        if (ticket >= s1 - s0) break;
        const uint32_t seg = s0 + ticket;
        const uint32_t start = __builtin_amdgcn_readfirstlane(a.starts[seg]), len = __builtin_amdgcn_readfirstlane(a.starts[seg + 1]) - start;
        for (uint32_t i = lane; i < nb * L.t32; i += 64) bw.lo[i] = inf, bw.hi[i] = inf;
        ms_wave_sync();
        if (a.img_lds) mb_walk<MODE, SLABS, true>(a, ma, L, w, bw, mb_lds, start, len);
        else mb_walk<MODE, SLABS, false>(a, ma, L, w, bw, mb_lds, start, len);
        ms_wave_sync();
        if (lane < nb) {  // lane b: the two sums in ascending t from +0.0f
            const uint32_t Tb = s_tb[lane];
            float sl = 0.0f, su = 0.0f;
            for (uint32_t t = 0; t < Tb; ++t) sl = sl + bw.lo[lane * L.t32 + t], su = su + bw.hi[lane * L.t32 + t];
            const bool nan = sl != sl || su != su;
            const uint64_t at = (uint64_t)(q0 + lane) * a.nv + seg;
            a.L[at] = nan ? -inf : sl, a.U[at] = nan ? inf : su;
        }
        ms_wave_sync();
    }
}

// tau_b: the topk-th smallest U[b][.] by its ordered image; one block per query, a radix select of four 8-bit passes.
__global__ __launch_bounds__(256) void maxsim_bound_threshold_kernel(const MaxsimBoundArgs a) {
    __shared__ uint32_t s_hist[256], s_prefix, s_rank;
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    if (a.nv < a.topk) {  // (uniform)
        if (tid == 0) a.tau[b] = __builtin_inff();
        return;
    }
    const float *U = a.U + (uint64_t)b * a.nv;
    if (tid == 0) s_prefix = 0u, s_rank = a.topk;  // (the rank among the keys that share the prefix, from 1)
    uint32_t mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        s_hist[tid] = 0u;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (uint32_t i = tid; i < a.nv; i += 256) {
            const uint32_t key = ord32_biased(U[i]);
            if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rank = s_rank, bin = 0;
            while (bin < 255u && s_hist[bin] < rank) rank -= s_hist[bin], ++bin;
            s_prefix = prefix | (bin << shift), s_rank = rank;
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    if (tid == 0) a.tau[b] = ord32_unbias(s_prefix);
}

// The survivors of a query -- the segments with !(L > tau_b), or every segment -- in ascending order, and their number.
__global__ __launch_bounds__(256) void maxsim_bound_compact_kernel(const MaxsimBoundArgs a) {
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, b = blockIdx.x;
    const float tau = a.all ? 0.0f : a.tau[b];
    const float *Lb = a.L + (uint64_t)b * a.nv;
    uint32_t *out = a.surv + (uint64_t)b * a.nv;
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < a.nv; i0 += 256) {  // (i0 + 256 may pass 2^32 only where nv does: it cannot)
        const uint32_t i = i0 + tid;
        const bool keep = i < a.nv && (a.all || !(Lb[i] > tau));
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t at = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        for (uint32_t v = 0; v < wave; ++v) at += s_wave[v];
        if (keep) out[at] = i;
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
        if (a.nv - i0 <= 256) break;
    }
    if (tid == 0) {
        a.surv_n[b] = base;
        atomicMax(a.totals + 0, (unsigned long long)base);
        atomicAdd(a.totals + 1, (unsigned long long)base);
    }
}

// A round of the exact scoring: the survivors [first, first + slots) of every query as its candidate row (stride `slots`).
__global__ __launch_bounds__(256) void maxsim_exact_round_kernel(const MaxsimBoundArgs a, uint32_t first, uint32_t slots, uint32_t *cand, uint32_t *cand_n) {
    const uint32_t b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = a.surv_n[b], cn = n > first ? (n - first < slots ? n - first : slots) : 0u;
    if (c < cn) cand[(uint64_t)b * slots + c] = a.surv[(uint64_t)b * a.nv + first + c];
    if (c == 0) cand_n[b] = cn;
}

// A round's scored documents into the query's running topk: (ord32_biased(chamfer), segment) keys, RQ_MSX_SORT of them at a time
// sorted together with the running ones.  last: the outputs, as maxsim_select_keyed_kernel writes them.
__global__ __launch_bounds__(256) void maxsim_exact_merge_kernel(const MaxsimKeyedArgs k, unsigned long long *run, uint32_t *run_n, uint32_t first, uint32_t last) {
    __shared__ unsigned long long s_key[2 * RQ_MSX_SORT];
    const MaxsimArgs &a = k.m;
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t cn = a.cand_n[b] < a.ncand ? a.cand_n[b] : a.ncand;
    const uint64_t in0 = (uint64_t)b * a.ncand, out0 = (uint64_t)b * a.topk;
    uint32_t n = first ? 0u : run_n[b];  // (<= topk <= 2048)
    for (uint32_t i = tid; i < n; i += 256) s_key[i] = run[out0 + i];
    for (uint32_t c0 = 0; c0 < cn; c0 += RQ_MSX_SORT) {
        const uint32_t m = cn - c0 < RQ_MSX_SORT ? cn - c0 : RQ_MSX_SORT;
        uint32_t live = 0;  // the slots that hold a scored document: an integer count, the same in every thread
        for (uint32_t i = 0; i < m; i += 256) {
            const bool in = i + tid < m, held = in && a.rows[in0 + c0 + i + tid] != 0u;
            if (in) s_key[n + i + tid] = held ? ((unsigned long long)ord32_biased(a.score[in0 + c0 + i + tid]) << 32) | a.cand[in0 + c0 + i + tid] : ~0ull;
            live += (uint32_t)__syncthreads_count(held);
        }
        __syncthreads();
        bitonic_sort_block(s_key, n + m, [](unsigned long long q) { return q; });
        __syncthreads();
        n = n + live < a.topk ? n + live : a.topk;
    }
    for (uint32_t i = tid; i < n; i += 256) run[out0 + i] = s_key[i];
    if (tid == 0) run_n[b] = n;
    if (last) {
        for (uint32_t s = tid; s < a.topk; s += 256) {
            const bool held = s < n;
            const unsigned long long q = s_key[held ? s : 0u];
            a.out_dist[out0 + s] = held ? ord32_unbias((uint32_t)(q >> 32)) : __builtin_bit_cast(float, RQ_MAXSIM_NAN_BITS);
            k.out_keys[out0 + s] = held ? k.values[(uint32_t)q] : 0ull;
        }
        if (tid == 0) a.out_n[b] = n;
    }
}
#endif  // RQ_MAXSIM_EXACT_KERNELS
