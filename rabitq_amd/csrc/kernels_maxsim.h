// kernels_maxsim.h -- multi-vector search (host_maxsim.h), wave64: a query is a set of token vectors, a document the
// stored rows whose ids lie in [D S, D S + S), and the score the Chamfer sum  chamfer(b, D) = sum_t min_x d(t, x)  (ascending
// chamfer = descending MaxSim).  Nothing here writes an array of the index.
//
// THE CONTRACT (include/rabitq_hip.h states it; tests/maxsim_model.py is its model).  d(t, x) = exact_l2_row (kernels_rerank.h) of
// the stored row against the transformed token, a NaN of any sign and payload counted as 0x7FC00000; the minimum of a token is the
// smallest ord32_biased(d) (a total order, that NaN last), the sum runs in f32 over t = 0 .. T_b - 1 from +0.0f, a NaN sum written
// as 0x7FC00000.  A document without a live row scores 0x7FC00000 with rows = 0.
// No output bit depends on the order threads run in or on an atomic's return value: the per-token minimum is an integer atomicMin
// whose result is not read, the sum is one lane's, the totals are integer sums.
//
// maxsim_score_kernel<MODE, PRE>.  One block of four waves per (query, group of `group` candidate slots); the block stages the
// query's tokens once, then every wave scores one document at a time (slots wave, wave + 4, ... of the group).
//   Block LDS: the tokens as f32 (only where they fit: tok_lds; else exact_l2_row reads them from global memory, the L2 holds them)
//   and, PRE, their bf16 image in 32-token tiles with zero rows behind T_b -- row stride 2 dim + 16 bytes, the B operand of
//   v_mfma_f32_32x32x16_bf16 as exact_scan_kernel lays its rows out -- with |q'|^2 and its scaled root (exact_prep_kernel's
//   arithmetic).
//   A wave walks its document's S ids 64 at a time (directory probe, live bit: group_probe_*), compacts the live positions into a
//   ring in LDS and takes them off 32 at a time:
//   PRE   the 32 rows go through fetch_src / fetch_load / fetch_widen into the wave's slab, rounded to bf16, |x|^2 and its root
//         from the same registers (eight lanes per row); dim / 16 MFMAs per 32-token tile give a = (|x|^2 + |q'|^2) - 2 acc and
//         m = ex_margin_factor(dim) (|x| + |q'|)^2, the exact scan's bound.  Per token U_t = min (a + m) is kept (an upper bound of
//         the token's true minimum: in the accumulator layout a lane holds 16 rows of one token, so the minimum is in-register plus
//         one exchange between the lane halves), and a row is appended to the wave's list (token, position, a - m) unless
//         a - m > U_t as it stands: a superset of the rows that can realise the minimum.  After the last tile the entries above the
//         final U_t are dropped and the rest get exact_l2_row, a pair of lanes per entry.  A list that is full marks the token: its
//         rows are walked again and every one gets its exact distance (never a pair dropped).  Every test keeps the pair when
//         either side is a NaN, and a row whose |x|^2 is not finite is always kept -- the exact scan's rules.
//   !PRE  (RQ_MAXSIM_NO_PREFILTER, and shapes whose tiles do not fit): every (token, row) pair gets exact_l2_row, 32 rows a round.
//   Both forms take the minimum of the same exact distances: the same bits.
// maxsim_score_keyed_kernel<MODE, PRE, SLABS> (host_maxsim_keyed.h; at the end of this file): the same scoring over
// documents named by a column -- a document is a segment of a postings object (kernels_keyed.h), walked as coalesced runs of positions.
// Vector loads and stores only.
#pragma once
#include "common.h"
#include "kernels_rerank.h"
#include "kernels_directory.h"
#include "kernels_group.h"  // GroupArgs and group_probe_*: the directory walk

#ifndef RQ_MAXSIM_NO_PREFILTER
#define RQ_MAXSIM_NO_PREFILTER 1u  // rq_maxsim_params_t.flags bit 0 (include/rabitq_hip.h)
#endif
#define RQ_MAXSIM_MAX_TOKENS 256u
#define RQ_MAXSIM_MAX_STRIDE 4096u
#define RQ_MAXSIM_MAX_SOURCE 2048u          // tokens x fetch of the end-to-end entry: one bitonic_sort_block
#define RQ_MAXSIM_NAN_BITS 0x7FC00000u
#define RQ_MAXSIM_PAD_DOC 0xFFFFFFFFu
#define RQ_MAXSIM_LDS_MAX (156u * 1024u)    // as RQ_EXACT_LDS_MAX: what a block may take of a CU's 160 KiB
#define RQ_MAXSIM_LDS_TWO (78u * 1024u)     // two blocks per CU

struct MaxsimArgs {
    const float *tok;           // nq x T x dim: the transformed, padded tokens
    const uint32_t *n_tokens;   // nq, nullable (= T)
    const uint32_t *cand;       // nq x ncand document numbers
    const uint32_t *cand_n;     // nq, nullable (= ncand)
    uint32_t nq, T, dim, ncand, S;
    uint32_t group, chunks;     // candidate slots per block; blocks per query
    uint32_t list_cap;          // PRE: entries of a wave's list
    uint32_t tok_lds;           // 1: the f32 tokens are staged in LDS
    GroupArgs dir;              // the directory, the live bitmap and the stored row count (the fields group_probe_* read; nothing else is set)
    BaseView base;
    float *score;               // nq x ncand
    uint32_t *rows;             // nq x ncand
    unsigned long long *stats;  // {rows gathered, pairs, exact distances, list overflows, documents scored}, preset to 0
    // the end-to-end entry: the source's rows (nq T x fetch), and what the selection writes
    const uint32_t *src_id, *src_n;
    uint32_t fetch, topk;
    uint32_t *cand_out, *cand_n_out;  // candidates kernel: nq x ncand, nq
    float *out_dist;                  // nq x topk
    uint32_t *out_docs, *out_n, *out_cand;
};

// ---- the LDS layout, shared by the host (which sizes the launch and picks the form) and the kernel ----
struct MaxsimLds {
    uint32_t rowb, t32;                                  // image row stride; T rounded up to whole 32-token tiles
    uint32_t tokf, img, qn2, qsn, wave0, wave_bytes;     // block offsets; the first wave's region and its size
    uint32_t slab, xn2, xsn, ubound, lpos, llo, ltok, ovf, ring, best;  // offsets inside a wave's region
    uint32_t total;
    uint32_t buf2;  // slabs = 2: the second (slab, xn2, xsn) of a wave, laid out as the first; its distance from the first
};
__host__ __device__ inline MaxsimLds maxsim_lds(uint32_t dim, uint32_t T, bool pre, bool tok_lds, uint32_t list_cap, uint32_t slabs = 1) {
    MaxsimLds l{};
    l.rowb = dim * 2 + 16, l.t32 = (T + 31u) & ~31u;
    uint32_t o = 0;
    l.tokf = o, o += tok_lds ? T * dim * 4 : 0;
    l.img = o, o += pre ? l.t32 * l.rowb : 0;
    l.qn2 = o, o += pre ? l.t32 * 4 : 0;
    l.qsn = o, o += pre ? l.t32 * 4 : 0;
    l.wave0 = o;
    uint32_t w = 0;
    l.slab = w, w += pre ? 32 * l.rowb : 0;
    l.xn2 = w, w += pre ? 128 : 0;
    l.xsn = w, w += pre ? 128 : 0;
    l.ubound = w, w += pre ? l.t32 * 4 : 0;
    l.lpos = w, w += pre ? list_cap * 4 : 0;
    l.llo = w, w += pre ? list_cap * 4 : 0;
    l.ltok = w, w += pre ? ((list_cap * 2 + 15u) & ~15u) : 0;
    l.ovf = w, w += pre ? 32 : 0;
    l.ring = w, w += 128 * 4;
    l.best = w, w += l.t32 * 4;
    l.buf2 = w, w += pre && slabs == 2 ? 32 * l.rowb + 256 : 0;
    l.wave_bytes = w, l.total = o + 4 * w;
    return l;
}
static inline uint32_t maxsim_list_cap(uint32_t T) { return 4u * ((T + 31u) & ~31u) < 128u ? 128u : 4u * ((T + 31u) & ~31u); }

// Documents named by a column: a candidate is a SEGMENT number of a postings object (kernels_keyed.h), the document
// the positions post[starts[s] .. starts[s + 1]).  m.cand / m.cand_out hold segment numbers (>= nv: a key the postings do not hold,
// a document without a row), m.S is not read, m.dir serves the end-to-end entry's id -> position -> column value only.
struct MaxsimKeyedArgs {
    MaxsimArgs m;
    const uint32_t *post;               // the postings: live positions grouped by value
    const uint32_t *starts;             // nv + 1
    const unsigned long long *values;   // nv: the values' u64 images, ascending in the column type's own order
    uint32_t nv, is_signed, wide;       // the column type: signed comparison; 8-byte elements
    unsigned long long *out_keys;       // the selection: nq x topk values (rq_attr_value_t images)
};
// two slabs a wave (the next tile's raw rows in flight under this tile's matrix pass): dim 64, where the pieces of a lane's four
// rows stay in registers and the block still leaves room for a second one on its CU
static inline uint32_t maxsim_keyed_slabs(uint32_t dim, uint32_t T, bool tok_lds, uint32_t list_cap) {
    return dim == 64 && maxsim_lds(dim, T, true, tok_lds, list_cap, 2).total <= RQ_MAXSIM_LDS_TWO ? 2u : 1u;
}

// the launches (inst_maxsim.hip)
void launch_keyed_lookup(const unsigned long long *keys, uint64_t m, const MaxsimKeyedArgs &k, uint32_t *seg, hipStream_t st);
void launch_maxsim_score_keyed(const MaxsimKeyedArgs &k, int row_kind, bool pre, uint32_t slabs, size_t lds, hipStream_t st);
void launch_maxsim_candidates_keyed(const MaxsimKeyedArgs &k, hipStream_t st);
void launch_maxsim_select_keyed(const MaxsimKeyedArgs &k, hipStream_t st);
hipError_t maxsim_set_attributes();
void launch_maxsim_score(const MaxsimArgs &a, int row_kind, bool pre, size_t lds, hipStream_t st);
void launch_maxsim_candidates(const MaxsimArgs &a, hipStream_t st);
void launch_maxsim_select(const MaxsimArgs &a, hipStream_t st);

#ifdef RQ_MAXSIM_KERNELS
#include "exact_margin.h"  // ex_bf16_pair, ex_margin_factor: the exact scan's own

typedef __bf16 ms_bf16x8 __attribute__((ext_vector_type(8)));
typedef float ms_f32x16 __attribute__((ext_vector_type(16)));

// what one wave wrote to LDS is read by its other lanes behind this (the waves of a block walk different documents: no block barrier)
__device__ __forceinline__ void ms_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}
// the ordered image of a distance; a NaN counts as 0x7FC00000 whatever its sign and payload (they are the hardware's, not the contract's)
__device__ __forceinline__ uint32_t ms_key(float e) { return ord32_biased(e != e ? __builtin_bit_cast(float, RQ_MAXSIM_NAN_BITS) : e); }
template <int MODE>
__device__ __forceinline__ float ms_exact(const BaseView &base, uint32_t pos, const float *tok, uint32_t dim, uint32_t hf) {
    if constexpr (MODE == FETCH_BYTE) return exact_l2_row_byte(base.row_at(pos, dim), tok, dim, hf);
    else if constexpr (MODE == FETCH_HALF) return exact_l2_row_half(base.row_at(pos, dim), tok, dim, hf);
    else return exact_l2_row_f32(RowRef{base.dev + (uint64_t)pos * dim, false, 0u}, tok, dim, hf);
}

// What a wave carries through one document.
struct MaxsimWave {
    unsigned char *lds;   // the wave's region
    const float *tokf;    // the query's f32 tokens (LDS or global)
    uint32_t Tb, ntt;     // tokens of the query; 32-token tiles
    uint32_t lane, list_n;
    unsigned long long n_exact, n_ovf;
};

// Exact distances of the ring's rows [head, head + n) (n <= 32) against every token of `mask_all` or of the wave's overflow words:
// a pair of lanes per row, the minimum per token by atomicMin on its ordered image.
template <int MODE>
__device__ __forceinline__ void ms_tile_exact(const MaxsimArgs &a, const MaxsimLds &L, MaxsimWave &w, uint32_t head, uint32_t n, bool marked_only) {
    const uint32_t *ring = reinterpret_cast<const uint32_t *>(w.lds + L.ring);
    uint32_t *best = reinterpret_cast<uint32_t *>(w.lds + L.best);
    const uint32_t *ovf = reinterpret_cast<const uint32_t *>(w.lds + L.ovf);
    const uint32_t i = w.lane >> 1, hf = w.lane & 1u;
    const bool have = i < n;  // (the same for the two lanes of a pair)
    const uint32_t pos = ring[(head + (have ? i : 0u)) & 127u];
    for (uint32_t t = 0; t < w.Tb; ++t) {
        if (marked_only && !((ovf[t >> 5] >> (t & 31u)) & 1u)) continue;  // (uniform)
        if (have) {
            const float e = ms_exact<MODE>(a.base, pos, w.tokf + (uint64_t)t * a.dim, a.dim, hf);
            if (hf == 0) atomicMin(best + t, ms_key(e));
        }
        w.n_exact += n;
    }
}

// ---- the two-slab form's tile routines (maxsim_score_keyed_kernel, SLABS = 2; boff: which (slab, xn2, xsn) of the wave, 0 or L.buf2).
// They are ms_tile_mfma below cut into its gather and its matrix pass, operation for operation; ms_tile_mfma itself stays one piece,
// as maxsim_score_kernel was built with it.
// One raw piece of row lr (a row past the tile's n: ok = false, zeros) widened and rounded to bf16 into the slab, its squares added to s ...
template <int MODE>
__device__ __forceinline__ void ms_put_piece(const MaxsimArgs &a, unsigned char *slab, uint32_t ROWB, uint4 raw, bool ok, uint32_t lr, uint32_t lp, float &s) {
    const uint4 v = fetch_keep(fetch_widen<MODE>(raw, false, a.base.fmt), ok);
    const float x0 = __builtin_bit_cast(float, v.x), x1 = __builtin_bit_cast(float, v.y);
    const float x2 = __builtin_bit_cast(float, v.z), x3 = __builtin_bit_cast(float, v.w);
    s = fmaf(x0, x0, s), s = fmaf(x1, x1, s), s = fmaf(x2, x2, s), s = fmaf(x3, x3, s);
    *reinterpret_cast<uint2 *>(slab + lr * ROWB + 8 * lp) = make_uint2(ex_bf16_pair(x0, x1), ex_bf16_pair(x2, x3));
}
// ... and the row's |x|^2 and its scaled root from the eight lanes' sums.
__device__ __forceinline__ void ms_put_norm(const MaxsimLds &L, MaxsimWave &w, uint32_t boff, float s, uint32_t lr) {
    s += __shfl_xor(s, 1, 8), s += __shfl_xor(s, 2, 8), s += __shfl_xor(s, 4, 8);
    if ((w.lane & 7u) == 0) reinterpret_cast<float *>(w.lds + L.xn2 + boff)[lr] = s, reinterpret_cast<float *>(w.lds + L.xsn + boff)[lr] = sqrtf(s) * 1.000001f;
}
// dim 64 (a lane holds pieces sub and sub + 8 of each of its four rows): the gather cut in two -- every raw load of the tile into
// registers, nothing consumed, and (later) their widening into the slab.  The same arithmetic in the same order as ms_tile_mfma's gather.
template <int MODE>
__device__ __forceinline__ void ms_tile_issue64(const MaxsimArgs &a, const MaxsimLds &L, const MaxsimWave &w, uint32_t head, uint32_t n, uint4 (&raw)[4][2]) {
    const uint32_t sub = w.lane & 7u, rr = w.lane >> 3;
    const uint32_t *ring = reinterpret_cast<const uint32_t *>(w.lds + L.ring);
    const uint32_t row_bytes = (uint32_t)RowSpec{a.base.fmt}.row_bytes(64u);
#pragma unroll
    for (uint32_t ps = 0; ps < 4; ++ps) {
        const uint32_t lr = ps * 8 + rr;
        const FetchSrc src = fetch_src<MODE>(a.base, ring[(head + (lr < n ? lr : 0u)) & 127u], 64u, row_bytes);
        raw[ps][0] = fetch_load<MODE>(src, sub, 64u), raw[ps][1] = fetch_load<MODE>(src, sub + 8, 64u);
    }
}
template <int MODE>
__device__ __forceinline__ void ms_tile_land64(const MaxsimArgs &a, const MaxsimLds &L, MaxsimWave &w, uint32_t boff, uint32_t n, const uint4 (&raw)[4][2]) {
    const uint32_t sub = w.lane & 7u, rr = w.lane >> 3;
#pragma unroll
    for (uint32_t ps = 0; ps < 4; ++ps) {
        const uint32_t lr = ps * 8 + rr;
        float s = 0.0f;
        ms_put_piece<MODE>(a, w.lds + L.slab + boff, L.rowb, raw[ps][0], lr < n, lr, sub, s);
        ms_put_piece<MODE>(a, w.lds + L.slab + boff, L.rowb, raw[ps][1], lr < n, lr, sub + 8, s);
        ms_put_norm(L, w, boff, s, lr);
    }
}

// A gathered tile (the ring's rows [head, head + n) in the slab at boff): ms_tile_mfma's matrix pass -- the MFMAs against every
// token tile, U_t and the list.
__device__ __forceinline__ void ms_tile_matrix(const MaxsimArgs &a, const MaxsimLds &L, MaxsimWave &w, const unsigned char *blk, uint32_t boff, uint32_t head, uint32_t n) {
    const uint32_t dim = a.dim, ROWB = L.rowb, lane = w.lane;
    const uint32_t *ring = reinterpret_cast<const uint32_t *>(w.lds + L.ring);
    const unsigned char *slab = w.lds + L.slab + boff;
    const float *xn2 = reinterpret_cast<const float *>(w.lds + L.xn2 + boff), *xsn = reinterpret_cast<const float *>(w.lds + L.xsn + boff);
    float *ub = reinterpret_cast<float *>(w.lds + L.ubound);
    uint32_t *lpos = reinterpret_cast<uint32_t *>(w.lds + L.lpos);
    float *llo = reinterpret_cast<float *>(w.lds + L.llo);
    uint16_t *ltok = reinterpret_cast<uint16_t *>(w.lds + L.ltok);
    uint32_t *ovf = reinterpret_cast<uint32_t *>(w.lds + L.ovf);
    const uint32_t col = lane & 31u, kh = lane >> 5;
    // this lane's 16 rows: register r is row (r & 3) + 8 (r >> 2) + 4 kh of the tile (the accumulator layout, kernels_exact.h)
    uint32_t valid = 0u, wild = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
        valid |= lr < n ? (1u << r) : 0u;
        wild |= xn2[lr] < 3.0e38f ? 0u : (1u << r);
    }
    const float cm = ex_margin_factor(dim);
    const float *qn2 = reinterpret_cast<const float *>(blk + L.qn2), *qsn = reinterpret_cast<const float *>(blk + L.qsn);
    for (uint32_t tt = 0; tt < w.ntt; ++tt) {
        const uint32_t t = tt * 32 + col;
        ms_f32x16 acc = ms_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const unsigned char *ai = slab + col * ROWB + 16 * kh, *bi = blk + L.img + t * ROWB + 16 * kh;
        for (uint32_t m = 0; m < dim / 16; ++m) {
            const ms_bf16x8 af = *reinterpret_cast<const ms_bf16x8 *>(ai + 32 * m), bf = *reinterpret_cast<const ms_bf16x8 *>(bi + 32 * m);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
        }
        const float qn = qn2[t], qs = qsn[t];
        float lo[16], u = ub[t];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
            const float ap = fmaf(-2.0f, acc[r], xn2[lr] + qn), rad = xsn[lr] + qs, mg = cm * (rad * rad);
            const float hi = ap + mg;
            lo[r] = ap - mg;
            if (((valid & ~wild) >> r) & 1u) u = hi < u ? hi : u;  // (a NaN bound never lowers U)
        }
        {
            const float o = __shfl_xor(u, 32, 64);
            u = o < u ? o : u;
        }
        if (kh == 0) ub[t] = u;
        const float cut = u + fabsf(u) * 1.0e-6f;  // (the comparison's own rounding, as ex_pair_bound)
        uint32_t keep = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) keep |= !(lo[r] > cut) ? (1u << r) : 0u;  // NaN on either side keeps
        keep = t < w.Tb ? (keep | wild) & valid : 0u;
        const uint32_t c = (uint32_t)__popc(keep);
        const uint32_t inc = wave_incl_scan(c);
        const uint32_t total = __shfl(inc, 63, 64);
        uint32_t at = w.list_n + (inc - c);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (!((keep >> r) & 1u)) continue;
            if (at < a.list_cap) {
                const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
                lpos[at] = ring[(head + lr) & 127u], llo[at] = lo[r], ltok[at] = (uint16_t)t;
            } else {
                atomicOr(ovf + (t >> 5), 1u << (t & 31u));
            }
            ++at;
        }
        w.list_n = w.list_n + total < a.list_cap ? w.list_n + total : a.list_cap;
    }
}
// PRE: the ring's rows [head, head + n) into the slab, the MFMAs against every token tile, U_t and the list.
template <int MODE>
__device__ __forceinline__ void ms_tile_mfma(const MaxsimArgs &a, const MaxsimLds &L, MaxsimWave &w, const unsigned char *blk, uint32_t head, uint32_t n) {
    const uint32_t dim = a.dim, ROWB = L.rowb, lane = w.lane;
    const uint32_t *ring = reinterpret_cast<const uint32_t *>(w.lds + L.ring);
    unsigned char *slab = w.lds + L.slab;
    float *xn2 = reinterpret_cast<float *>(w.lds + L.xn2), *xsn = reinterpret_cast<float *>(w.lds + L.xsn);
    float *ub = reinterpret_cast<float *>(w.lds + L.ubound);
    uint32_t *lpos = reinterpret_cast<uint32_t *>(w.lds + L.lpos);
    float *llo = reinterpret_cast<float *>(w.lds + L.llo);
    uint16_t *ltok = reinterpret_cast<uint16_t *>(w.lds + L.ltok);
    uint32_t *ovf = reinterpret_cast<uint32_t *>(w.lds + L.ovf);
    ms_wave_sync();  // the previous tile's fragments have been read
    {   // the gather: eight lanes per row, eight rows a pass; a row past n reads the tile's first row and stores zeros
        const uint32_t sub = lane & 7u, rr = lane >> 3;
        const uint32_t row_bytes = (uint32_t)RowSpec{a.base.fmt}.row_bytes(dim);
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
    }
    ms_wave_sync();
    const uint32_t col = lane & 31u, kh = lane >> 5;
    // this lane's 16 rows: register r is row (r & 3) + 8 (r >> 2) + 4 kh of the tile (the accumulator layout, kernels_exact.h)
    uint32_t valid = 0u, wild = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
        valid |= lr < n ? (1u << r) : 0u;
        wild |= xn2[lr] < 3.0e38f ? 0u : (1u << r);
    }
    const float cm = ex_margin_factor(dim);
    const float *qn2 = reinterpret_cast<const float *>(blk + L.qn2), *qsn = reinterpret_cast<const float *>(blk + L.qsn);
    for (uint32_t tt = 0; tt < w.ntt; ++tt) {
        const uint32_t t = tt * 32 + col;
        ms_f32x16 acc = ms_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const unsigned char *ai = slab + col * ROWB + 16 * kh, *bi = blk + L.img + t * ROWB + 16 * kh;
        for (uint32_t m = 0; m < dim / 16; ++m) {
            const ms_bf16x8 af = *reinterpret_cast<const ms_bf16x8 *>(ai + 32 * m), bf = *reinterpret_cast<const ms_bf16x8 *>(bi + 32 * m);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
        }
        const float qn = qn2[t], qs = qsn[t];
        float lo[16], u = ub[t];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
            const float ap = fmaf(-2.0f, acc[r], xn2[lr] + qn), rad = xsn[lr] + qs, mg = cm * (rad * rad);
            const float hi = ap + mg;
            lo[r] = ap - mg;
            if (((valid & ~wild) >> r) & 1u) u = hi < u ? hi : u;  // (a NaN bound never lowers U)
        }
        {
            const float o = __shfl_xor(u, 32, 64);
            u = o < u ? o : u;
        }
        if (kh == 0) ub[t] = u;
        const float cut = u + fabsf(u) * 1.0e-6f;  // (the comparison's own rounding, as ex_pair_bound)
        uint32_t keep = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) keep |= !(lo[r] > cut) ? (1u << r) : 0u;  // NaN on either side keeps
        keep = t < w.Tb ? (keep | wild) & valid : 0u;
        const uint32_t c = (uint32_t)__popc(keep);
        const uint32_t inc = wave_incl_scan(c);
        const uint32_t total = __shfl(inc, 63, 64);
        uint32_t at = w.list_n + (inc - c);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (!((keep >> r) & 1u)) continue;
            if (at < a.list_cap) {
                const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
                lpos[at] = ring[(head + lr) & 127u], llo[at] = lo[r], ltok[at] = (uint16_t)t;
            } else {
                atomicOr(ovf + (t >> 5), 1u << (t & 31u));
            }
            ++at;
        }
        w.list_n = w.list_n + total < a.list_cap ? w.list_n + total : a.list_cap;
    }
}

// One document: its live rows walked once (count only / exact / MFMA), -> live rows seen.
template <int MODE, int FORM /* 0: count, 1: exact for every token, 2: exact for the marked tokens, 3: MFMA */>
__device__ __forceinline__ uint32_t ms_walk(const MaxsimArgs &a, const MaxsimLds &L, MaxsimWave &w, const unsigned char *blk, uint32_t doc) {
    uint32_t *ring = reinterpret_cast<uint32_t *>(w.lds + L.ring);
    const GroupArgs &g = a.dir;
    const uint64_t id0 = (uint64_t)doc * a.S;
    uint32_t head = 0, count = 0, seen = 0;
    for (uint32_t j0 = 0; j0 < a.S; j0 += 64) {
        const uint32_t j = j0 + w.lane;
        const uint64_t id64 = id0 + j;
        const bool in = j < a.S && id64 < a.dir.top && a.dir.rows != 0;
        const uint32_t id = (uint32_t)id64;
        uint32_t p = RQ_DIR_ABSENT, lw = 0u;
        if (a.dir.rows) {  // (uniform)
            unsigned long long first = group_probe_first(g, id, in);
            group_pin(first);
            p = group_probe_finish(g, id, in, first);
            lw = group_live_word(g, p != RQ_DIR_ABSENT ? p : 0u);
        }
        const bool present = p != RQ_DIR_ABSENT && ((lw >> (p & 31u)) & 1u);
        const unsigned long long bal = __ballot(present);
        const uint32_t add = (uint32_t)__popcll(bal);
        if (add == 0) continue;
        seen += add;
        if constexpr (FORM == 0) continue;
        if (present) ring[(head + count + (uint32_t)__popcll(bal & ((1ull << w.lane) - 1ull))) & 127u] = p;
        count += add;
        ms_wave_sync();
        const bool last = j0 + 64 >= a.S;
        while (count >= 32 || (last && count)) {
            const uint32_t n = count < 32 ? count : 32u;
            if constexpr (FORM == 3) ms_tile_mfma<MODE>(a, L, w, blk, head, n);
            else ms_tile_exact<MODE>(a, L, w, head, n, FORM == 2);
            head = (head + n) & 127u, count -= n;
        }
    }
    if constexpr (FORM != 0) {  // (ids whose last chunk held no live row leave a tail in the ring)
        while (count) {
            const uint32_t n = count < 32 ? count : 32u;
            if constexpr (FORM == 3) ms_tile_mfma<MODE>(a, L, w, blk, head, n);
            else ms_tile_exact<MODE>(a, L, w, head, n, FORM == 2);
            head = (head + n) & 127u, count -= n;
        }
    }
    return seen;
}

// The query's tokens (tg: its T x dim f32 rows, T_b of them used) into the block's LDS, by all 256 threads; the caller meets the barrier.
template <bool PRE>
__device__ __forceinline__ void ms_stage_tokens(const MaxsimArgs &a, const MaxsimLds &L, unsigned char *blk, const float *tg, uint32_t Tb) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, dim = a.dim, ntt = (Tb + 31u) >> 5;
    if (a.tok_lds) {
        float4 *dst = reinterpret_cast<float4 *>(blk + L.tokf);
        for (uint32_t i = tid; i < Tb * dim / 4; i += 256) dst[i] = reinterpret_cast<const float4 *>(tg)[i];
    }
    if constexpr (PRE) {  // a wave per token: exact_prep_kernel's image and norms; the rows behind T_b are zeros
        float *qn2 = reinterpret_cast<float *>(blk + L.qn2), *qsn = reinterpret_cast<float *>(blk + L.qsn);
        for (uint32_t t = wave; t < ntt * 32; t += 4) {
            float s = 0.0f;
            for (uint32_t e = 2 * lane; e < dim; e += 128) {
                float x0 = 0.0f, x1 = 0.0f;
                if (t < Tb) x0 = tg[(uint64_t)t * dim + e], x1 = tg[(uint64_t)t * dim + e + 1];
                s = fmaf(x0, x0, s), s = fmaf(x1, x1, s);
                *reinterpret_cast<uint32_t *>(blk + L.img + t * L.rowb + 2 * e) = ex_bf16_pair(x0, x1);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) qn2[t] = s, qsn[t] = sqrtf(s) * 1.000001f;
        }
    }
}
// PRE, after a document's last tile: the list entries still at or below the final U_t get their exact distance, a pair of lanes per
// entry -> the tokens marked as overflowed (the caller walks the document again for them).
template <int MODE>
__device__ __forceinline__ uint32_t ms_list_pass(const MaxsimArgs &a, const MaxsimLds &L, MaxsimWave &w) {
    const uint32_t *lpos = reinterpret_cast<const uint32_t *>(w.lds + L.lpos);
    const float *llo = reinterpret_cast<const float *>(w.lds + L.llo), *ub = reinterpret_cast<const float *>(w.lds + L.ubound);
    const uint16_t *ltok = reinterpret_cast<const uint16_t *>(w.lds + L.ltok);
    const uint32_t *ovf = reinterpret_cast<const uint32_t *>(w.lds + L.ovf);
    uint32_t *best = reinterpret_cast<uint32_t *>(w.lds + L.best);
    const uint32_t hf = w.lane & 1u, dim = a.dim;
    uint32_t mine = 0;
    for (uint32_t i = w.lane >> 1; i < w.list_n; i += 32) {
        const uint32_t t = ltok[i];
        const float u = ub[t];
        if (llo[i] > u + fabsf(u) * 1.0e-6f) continue;       // (a pair shares its entry; a NaN keeps it)
        if ((ovf[t >> 5] >> (t & 31u)) & 1u) continue;        // (the second walk gives this token every row)
        const float e = ms_exact<MODE>(a.base, lpos[i], w.tokf + (uint64_t)t * dim, dim, hf);
        if (hf == 0) atomicMin(best + t, ms_key(e)), ++mine;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o, 64);
    w.n_exact += mine;
    uint32_t marked = 0;
    for (uint32_t k = 0; k < 8; ++k) marked += (uint32_t)__popc(ovf[k]);
    return marked;
}

template <int MODE, bool PRE>
__global__ __launch_bounds__(256) void maxsim_score_kernel(const MaxsimArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ms_lds[];
    const MaxsimLds L = maxsim_lds(a.dim, a.T, PRE, a.tok_lds != 0, a.list_cap);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, dim = a.dim;
    const uint32_t b = blockIdx.x / a.chunks, c0 = (blockIdx.x % a.chunks) * a.group;
    const uint32_t c1 = c0 + a.group < a.ncand ? c0 + a.group : a.ncand;
    uint32_t tb = a.n_tokens ? a.n_tokens[b] : a.T, cn = a.cand_n ? a.cand_n[b] : a.ncand;
    const uint32_t Tb = __builtin_amdgcn_readfirstlane(tb < a.T ? tb : a.T), cnum = __builtin_amdgcn_readfirstlane(cn < a.ncand ? cn : a.ncand);
    const uint64_t out0 = (uint64_t)b * a.ncand;
    if (c0 >= cnum) {  // a group of padding slots
        for (uint32_t c = c0 + tid; c < c1; c += 256) a.score[out0 + c] = __builtin_bit_cast(float, RQ_MAXSIM_NAN_BITS), a.rows[out0 + c] = 0u;
        return;
    }
    // ---- the tokens, once per block ----
    const float *tg = a.tok + (uint64_t)b * a.T * dim;
    const uint32_t ntt = (Tb + 31u) >> 5;
    ms_stage_tokens<PRE>(a, L, ms_lds, tg, Tb);
    __syncthreads();
    MaxsimWave w{};
    w.lds = ms_lds + L.wave0 + wave * L.wave_bytes;
    w.tokf = a.tok_lds ? reinterpret_cast<const float *>(ms_lds + L.tokf) : tg;
    w.Tb = Tb, w.ntt = ntt, w.lane = lane;
    uint32_t *best = reinterpret_cast<uint32_t *>(w.lds + L.best);
    unsigned long long n_rows = 0, n_pairs = 0, n_docs = 0;
    for (uint32_t c = c0 + wave; c < c1; c += 4) {  // (uniform per wave)
        if (c >= cnum) {
            if (lane == 0) a.score[out0 + c] = __builtin_bit_cast(float, RQ_MAXSIM_NAN_BITS), a.rows[out0 + c] = 0u;
            continue;
        }
        const uint32_t doc = a.cand[out0 + c];
        for (uint32_t t = lane; t < L.t32; t += 64) best[t] = 0xFFFFFFFFu;
        uint32_t seen;
        if (Tb == 0) {
            seen = ms_walk<MODE, 0>(a, L, w, ms_lds, doc);
        } else if constexpr (PRE) {
            float *ub = reinterpret_cast<float *>(w.lds + L.ubound);
            uint32_t *ovf = reinterpret_cast<uint32_t *>(w.lds + L.ovf);
            for (uint32_t t = lane; t < L.t32; t += 64) ub[t] = __builtin_inff();
            if (lane < 8) ovf[lane] = 0u;
            w.list_n = 0;
            ms_wave_sync();
            seen = ms_walk<MODE, 3>(a, L, w, ms_lds, doc);
            ms_wave_sync();
            const uint32_t marked = ms_list_pass<MODE>(a, L, w);
            if (marked) {  // (uniform)
                w.n_ovf += marked;
                (void)ms_walk<MODE, 2>(a, L, w, ms_lds, doc);
            }
        } else {
            seen = ms_walk<MODE, 1>(a, L, w, ms_lds, doc);
        }
        ms_wave_sync();
        if (lane == 0) {
            float s = 0.0f;
            for (uint32_t t = 0; t < Tb; ++t) s = s + ord32_unbias(best[t]);
            a.score[out0 + c] = seen && s == s ? s : __builtin_bit_cast(float, RQ_MAXSIM_NAN_BITS);  // (a NaN sum: the one NaN, too)
            a.rows[out0 + c] = seen;
        }
        n_rows += seen, n_pairs += (unsigned long long)seen * Tb, ++n_docs;
        ms_wave_sync();
    }
    if (lane == 0) {
        if (n_docs) atomicAdd(a.stats + 4, n_docs);
        if (n_rows) atomicAdd(a.stats + 0, n_rows), atomicAdd(a.stats + 1, n_pairs);
        if (w.n_exact) atomicAdd(a.stats + 2, w.n_exact);
        if (w.n_ovf) atomicAdd(a.stats + 3, w.n_ovf);
    }
}

// ---- the end-to-end entry's two small kernels: one block per query ----
// The documents id / S of the valid tokens' result rows, sorted and made unique: cand_out[b] ascending, cand_n_out[b] of them.
__global__ __launch_bounds__(256) void maxsim_candidates_kernel(const MaxsimArgs a) {
    __shared__ uint32_t s_doc[RQ_MAXSIM_MAX_SOURCE];
    __shared__ uint32_t s_valid, s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, b = blockIdx.x;
    const uint32_t tb = a.n_tokens ? a.n_tokens[b] : a.T, Tb = tb < a.T ? tb : a.T;
    const uint32_t slots = Tb * a.fetch;  // (<= 2048: the host checked T x fetch)
    if (tid == 0) s_valid = 0u;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = tid; i < slots; i += 256) {
        const uint64_t row = (uint64_t)b * a.T + i / a.fetch;
        const uint32_t j = i % a.fetch, n = a.src_n[row];
        const bool ok = j < (n < a.fetch ? n : a.fetch);
        s_doc[i] = ok ? a.src_id[row * a.fetch + j] / a.S : 0xFFFFFFFFu;  // (the slots without a row sort behind every document)
        mine += ok ? 1u : 0u;
    }
    if (mine) atomicAdd(&s_valid, mine);
    __syncthreads();
    bitonic_sort_block(s_doc, slots, [](uint32_t v) { return v; });
    __syncthreads();
    const uint32_t nv = s_valid;
    // thread t owns places 8 t .. 8 t + 7: its first occurrences, then their places among the whole row's
    uint32_t heads = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t i = tid * 8 + k;
        if (i < nv && (i == 0 || s_doc[i] != s_doc[i - 1])) heads |= 1u << k;
    }
    const uint32_t c = (uint32_t)__popc(heads), inc = wave_incl_scan(c);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t at = inc - c;
    for (uint32_t v = 0; v < wave; ++v) at += s_wave[v];
    uint32_t *out = a.cand_out + (uint64_t)b * a.ncand;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if ((heads >> k) & 1u) out[at++] = s_doc[tid * 8 + k];
    if (tid == 0) a.cand_n_out[b] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// The topk smallest (ord32_biased(chamfer), doc) of a query's scored candidates, ascending; padding behind.
__global__ __launch_bounds__(256) void maxsim_select_kernel(const MaxsimArgs a) {
    __shared__ unsigned long long s_key[RQ_MAXSIM_MAX_SOURCE];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t cn = a.cand_n[b] < a.ncand ? a.cand_n[b] : a.ncand;  // (<= 2048)
    const uint64_t in0 = (uint64_t)b * a.ncand, out0 = (uint64_t)b * a.topk;
    for (uint32_t i = tid; i < cn; i += 256)  // (a document without a live row is no candidate: it sorts behind every key and is cut below)
        s_key[i] = a.rows[in0 + i] ? ((unsigned long long)ord32_biased(a.score[in0 + i]) << 32) | a.cand[in0 + i] : ~0ull;
    __syncthreads();
    bitonic_sort_block(s_key, cn, [](unsigned long long k) { return k; });
    __syncthreads();
    uint32_t live = 0;  // the candidates that have a row: an integer count, the same in every thread
    for (uint32_t i = 0; i < cn; i += 256) live += (uint32_t)__syncthreads_count(i + tid < cn && a.rows[in0 + i + tid] != 0u);
    const uint32_t take = live < a.topk ? live : a.topk;
    for (uint32_t s = tid; s < a.topk; s += 256) {
        const bool held = s < take;
        const unsigned long long k = s_key[held ? s : 0u];
        a.out_dist[out0 + s] = held ? ord32_unbias((uint32_t)(k >> 32)) : __builtin_bit_cast(float, RQ_MAXSIM_NAN_BITS);
        a.out_docs[out0 + s] = held ? (uint32_t)k : RQ_MAXSIM_PAD_DOC;
    }
    if (tid == 0) a.out_n[b] = take, a.out_cand[b] = cn;
}

// ==== documents named by a column: MaxSim by postings ==================================================================
// THE CONTRACT is the one above with one change: the document of key v is the set of positions in v's segment of the postings --
// the rows that were live and held v when the postings were made.  Nothing here reads the live bitmap or (for the walk) the
// directory: the postings' generation / removal-epoch check (host) is what guarantees that every posting is still a live row.
// Documents have any length >= 1; a key the postings do not hold is a document without a row.
//
// maxsim_score_keyed_kernel<MODE, PRE, SLABS>: the block, the token staging, the per-tile routines, U_t, the list and its overflow
// are maxsim_score_kernel's (the proof that the kept set contains the minimum is about a tile's 32 ring positions and does not ask
// where they came from).  What differs is how work reaches the tiles:
//   the walk   a document's positions are ONE coalesced 32-lane load per tile from post[start + 32 t ...], written straight into
//              the ring (segment t & 3); the load for tile t + 1 is issued before tile t's gather is consumed.  The dependent chain
//              is position -> row.  Only the last tile of a segment is short.
//   SLABS = 2  (dim 64, PRE) keyed_scan_kernel's scheme: the raw row loads of tile t + 1 are issued into registers before the
//              MFMAs, the bound test and the list appends of tile t and widened into the wave's other slab behind them.
//   the split  documents differ in length by orders of magnitude, so the four waves take the group's slots from a ticket counter
//              in LDS.  The atomicAdd's return value schedules and nothing else: every document is scored wholly by one wave, in
//              the order of its postings' tiles, and every output is a minimum / an integer sum over them.  A very long document is
//              one wave's serial work (splitting a document over waves is not done here).
__device__ __forceinline__ bool ms_value_less(unsigned long long x, unsigned long long y, uint32_t is_signed, uint32_t wide) {
    if (!is_signed) return x < y;
    return wide ? (long long)x < (long long)y : (int)(uint32_t)x < (int)(uint32_t)y;
}
// the segment of the value image `key` (keyed_find, keyed_plan.h), or RQ_MAXSIM_PAD_DOC
__device__ __forceinline__ uint32_t ms_segment_of(const MaxsimKeyedArgs &k, unsigned long long key) {
    uint32_t lo = 0, hi = k.nv;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ms_value_less(k.values[mid], key, k.is_signed, k.wide)) lo = mid + 1;
        else hi = mid;
    }
    return lo < k.nv && k.values[lo] == key ? lo : RQ_MAXSIM_PAD_DOC;
}
// keys (rq_attr_value_t: 8 bytes each, a 4-byte value in the low 4) -> segment numbers
__global__ __launch_bounds__(256) void keyed_lookup_kernel(const unsigned long long *__restrict__ keys, uint64_t m, const MaxsimKeyedArgs k,
                                                           uint32_t *__restrict__ seg) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256)
        seg[i] = ms_segment_of(k, k.wide ? keys[i] : keys[i] & 0xFFFFFFFFull);
}

// One document: the postings [start, start + len) walked once, 32 a tile (FORM 1: exact for every token, 2: exact for the marked
// tokens, 3: MFMA).  A lane past the segment's end loads nothing and publishes position 0, which no tile routine reads (n is short).
template <int MODE, int FORM, int SLABS>
__device__ __forceinline__ void ms_walk_keyed(const MaxsimKeyedArgs &k, const MaxsimLds &L, MaxsimWave &w, const unsigned char *blk, uint32_t start, uint32_t len) {
    const MaxsimArgs &a = k.m;
    uint32_t *ring = reinterpret_cast<uint32_t *>(w.lds + L.ring);
    const uint32_t ntile = (len + 31u) >> 5, col = w.lane & 31u;
    const auto load_pos = [&](uint32_t t) -> uint32_t {
        const uint32_t v = t * 32u + col;
        return v < len ? k.post[(uint64_t)start + v] : 0u;
    };
    const auto publish = [&](uint32_t t, uint32_t p) {  // (ring segment t & 3 was last read by tile t - 4: program order)
        if (w.lane < 32) ring[(t & 3u) * 32u + col] = p;
        ms_wave_sync();
    };
    const auto rows_of = [&](uint32_t t) { return len - t * 32u < 32u ? len - t * 32u : 32u; };
    uint32_t nxt = load_pos(0);
    if constexpr (FORM == 3 && SLABS == 2) {
        uint4 raw[4][2];
        publish(0, nxt);
        nxt = load_pos(1);
        ms_tile_issue64<MODE>(a, L, w, 0u, rows_of(0), raw);  // the first tile: nothing to hide it under
        ms_tile_land64<MODE>(a, L, w, 0u, rows_of(0), raw);
        for (uint32_t t = 0; t < ntile; ++t) {
            const bool more = t + 1 < ntile;
            const uint32_t here = (t & 1u) * L.buf2, there = L.buf2 - here;
            ms_wave_sync();  // tile t's slab is written; the tile before has been read out of the other one
            if (more) {      // the next tile's rows are asked for before this tile's matrix pass
                const uint32_t p = nxt;
                nxt = load_pos(t + 2);
                publish(t + 1, p);
                ms_tile_issue64<MODE>(a, L, w, ((t + 1) & 3u) * 32u, rows_of(t + 1), raw);
            }
            ms_tile_matrix(a, L, w, blk, here, (t & 3u) * 32u, rows_of(t));
            if (more) ms_tile_land64<MODE>(a, L, w, there, rows_of(t + 1), raw);
        }
    } else {
        for (uint32_t t = 0; t < ntile; ++t) {
            const uint32_t p = nxt;
            nxt = load_pos(t + 1);  // on its way before this tile's rows are asked for
            publish(t, p);
            if constexpr (FORM == 3) ms_tile_mfma<MODE>(a, L, w, blk, (t & 3u) * 32u, rows_of(t));
            else ms_tile_exact<MODE>(a, L, w, (t & 3u) * 32u, rows_of(t), FORM == 2);
        }
    }
}

// (two waves a SIMD asked for: without the bound the byte form and the half two-slab form take more than 256 registers a lane and a CU
// holds one block; with it every form fits two, none spills)
template <int MODE, bool PRE, int SLABS>
__global__ __launch_bounds__(256, 2) void maxsim_score_keyed_kernel(const MaxsimKeyedArgs k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ms_lds[];
    __shared__ uint32_t s_ticket;
    const MaxsimArgs &a = k.m;
    const MaxsimLds L = maxsim_lds(a.dim, a.T, PRE, a.tok_lds != 0, a.list_cap, SLABS);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t b = blockIdx.x / a.chunks, c0 = (blockIdx.x % a.chunks) * a.group;
    const uint32_t c1 = c0 + a.group < a.ncand ? c0 + a.group : a.ncand;
    uint32_t tb = a.n_tokens ? a.n_tokens[b] : a.T, cn = a.cand_n ? a.cand_n[b] : a.ncand;
    const uint32_t Tb = __builtin_amdgcn_readfirstlane(tb < a.T ? tb : a.T), cnum = __builtin_amdgcn_readfirstlane(cn < a.ncand ? cn : a.ncand);
    const uint64_t out0 = (uint64_t)b * a.ncand;
    const float nan = __builtin_bit_cast(float, RQ_MAXSIM_NAN_BITS);
    if (c0 >= cnum) {  // a group of padding slots
        for (uint32_t c = c0 + tid; c < c1; c += 256) a.score[out0 + c] = nan, a.rows[out0 + c] = 0u;
        return;
    }
    const float *tg = a.tok + (uint64_t)b * a.T * a.dim;
    if (tid == 0) s_ticket = 0u;
    ms_stage_tokens<PRE>(a, L, ms_lds, tg, Tb);
    __syncthreads();
    MaxsimWave w{};
    w.lds = ms_lds + L.wave0 + wave * L.wave_bytes;
    w.tokf = a.tok_lds ? reinterpret_cast<const float *>(ms_lds + L.tokf) : tg;
    w.Tb = Tb, w.ntt = (Tb + 31u) >> 5, w.lane = lane;
    uint32_t *best = reinterpret_cast<uint32_t *>(w.lds + L.best);
    unsigned long long n_rows = 0, n_pairs = 0, n_docs = 0;
    for (;;) {  // the group's slots, one ticket a document (uniform per wave)
        uint32_t ticket = 0u;
        if (lane == 0) ticket = atomicAdd(&s_ticket, 1u);
        const uint32_t c = c0 + (uint32_t)__builtin_amdgcn_readfirstlane(ticket);
        if (c >= c1) break;
        const uint32_t seg = c < cnum ? __builtin_amdgcn_readfirstlane(a.cand[out0 + c]) : RQ_MAXSIM_PAD_DOC;
        uint32_t start = 0u, len = 0u;
        if (seg < k.nv) start = __builtin_amdgcn_readfirstlane(k.starts[seg]), len = __builtin_amdgcn_readfirstlane(k.starts[seg + 1]) - start;
        if (c < cnum) ++n_docs;
        if (len == 0u) {  // a padding slot, or a key the postings do not hold
            if (lane == 0) a.score[out0 + c] = nan, a.rows[out0 + c] = 0u;
            continue;
        }
        for (uint32_t t = lane; t < L.t32; t += 64) best[t] = 0xFFFFFFFFu;
        if (Tb == 0) {
            // (no token: +0.0f over the document's rows, nothing to walk)
        } else if constexpr (PRE) {
            float *ub = reinterpret_cast<float *>(w.lds + L.ubound);
            uint32_t *ovf = reinterpret_cast<uint32_t *>(w.lds + L.ovf);
            for (uint32_t t = lane; t < L.t32; t += 64) ub[t] = __builtin_inff();
            if (lane < 8) ovf[lane] = 0u;
            w.list_n = 0;
            ms_wave_sync();
            ms_walk_keyed<MODE, 3, SLABS>(k, L, w, ms_lds, start, len);
            ms_wave_sync();
            const uint32_t marked = ms_list_pass<MODE>(a, L, w);
            if (marked) {  // (uniform)
                w.n_ovf += marked;
                ms_walk_keyed<MODE, 2, 1>(k, L, w, ms_lds, start, len);
            }
        } else {
            ms_wave_sync();
            ms_walk_keyed<MODE, 1, 1>(k, L, w, ms_lds, start, len);
        }
        ms_wave_sync();
        if (lane == 0) {
            float s = 0.0f;
            for (uint32_t t = 0; t < Tb; ++t) s = s + ord32_unbias(best[t]);
            a.score[out0 + c] = s == s ? s : nan;  // (a NaN sum: the one NaN, too)
            a.rows[out0 + c] = len;
        }
        n_rows += len, n_pairs += (unsigned long long)len * Tb;
        ms_wave_sync();
    }
    if (lane == 0) {
        if (n_docs) atomicAdd(a.stats + 4, n_docs);
        if (n_rows) atomicAdd(a.stats + 0, n_rows), atomicAdd(a.stats + 1, n_pairs);
        if (w.n_exact) atomicAdd(a.stats + 2, w.n_exact);
        if (w.n_ovf) atomicAdd(a.stats + 3, w.n_ovf);
    }
}

// ---- the end-to-end entry's two small kernels: one block per query, as maxsim_candidates_kernel / maxsim_select_kernel ----
// The segments of the valid tokens' result rows -- id -> position (the directory) -> the column's value AS IT IS NOW -> its segment in
// the postings; a value the postings do not hold is no candidate --, sorted and made unique.
__global__ __launch_bounds__(256) void maxsim_candidates_keyed_kernel(const MaxsimKeyedArgs k) {
    __shared__ uint32_t s_doc[RQ_MAXSIM_MAX_SOURCE];
    __shared__ uint32_t s_valid, s_wave[4];
    const MaxsimArgs &a = k.m;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, b = blockIdx.x;
    const uint32_t tb = a.n_tokens ? a.n_tokens[b] : a.T, Tb = tb < a.T ? tb : a.T;
    const uint32_t slots = Tb * a.fetch;  // (<= 2048: the host checked T x fetch)
    if (tid == 0) s_valid = 0u;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = tid; i < slots; i += 256) {
        const uint64_t row = (uint64_t)b * a.T + i / a.fetch;
        const uint32_t j = i % a.fetch, n = a.src_n[row];
        const uint32_t id = j < (n < a.fetch ? n : a.fetch) ? a.src_id[row * a.fetch + j] : 0xFFFFFFFFu;
        const bool in = j < (n < a.fetch ? n : a.fetch) && id < a.dir.top && a.dir.rows != 0;
        uint32_t seg = RQ_MAXSIM_PAD_DOC;
        if (in) {
            const uint32_t p = group_probe_finish(a.dir, id, true, group_probe_first(a.dir, id, true));
            if (p != RQ_DIR_ABSENT) seg = ms_segment_of(k, group_column(a.dir, p));
        }
        s_doc[i] = seg;  // (the slots without a candidate sort behind every segment)
        mine += seg != RQ_MAXSIM_PAD_DOC ? 1u : 0u;
    }
    if (mine) atomicAdd(&s_valid, mine);
    __syncthreads();
    bitonic_sort_block(s_doc, slots, [](uint32_t v) { return v; });
    __syncthreads();
    const uint32_t nv = s_valid;
    uint32_t heads = 0;  // thread t owns places 8 t .. 8 t + 7: its first occurrences, then their places among the whole row's
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) {
        const uint32_t i = tid * 8 + q;
        if (i < nv && (i == 0 || s_doc[i] != s_doc[i - 1])) heads |= 1u << q;
    }
    const uint32_t c = (uint32_t)__popc(heads), inc = wave_incl_scan(c);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t at = inc - c;
    for (uint32_t v = 0; v < wave; ++v) at += s_wave[v];
    uint32_t *out = a.cand_out + (uint64_t)b * a.ncand;
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q)
        if ((heads >> q) & 1u) out[at++] = s_doc[tid * 8 + q];
    if (tid == 0) a.cand_n_out[b] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// The topk smallest (ord32_biased(chamfer), segment) of a query's scored candidates, ascending -- the segment number is the column
// type's own ascending order --, written as (chamfer, the segment's value); padding 0x7FC00000 / value 0 behind.
__global__ __launch_bounds__(256) void maxsim_select_keyed_kernel(const MaxsimKeyedArgs k) {
    __shared__ unsigned long long s_key[RQ_MAXSIM_MAX_SOURCE];
    const MaxsimArgs &a = k.m;
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t cn = a.cand_n[b] < a.ncand ? a.cand_n[b] : a.ncand;  // (<= 2048)
    const uint64_t in0 = (uint64_t)b * a.ncand, out0 = (uint64_t)b * a.topk;
    for (uint32_t i = tid; i < cn; i += 256)  // (an empty segment would be no candidate: it sorts behind every key and is cut below)
        s_key[i] = a.rows[in0 + i] ? ((unsigned long long)ord32_biased(a.score[in0 + i]) << 32) | a.cand[in0 + i] : ~0ull;
    __syncthreads();
    bitonic_sort_block(s_key, cn, [](unsigned long long q) { return q; });
    __syncthreads();
    uint32_t live = 0;  // the candidates that have a row: an integer count, the same in every thread
    for (uint32_t i = 0; i < cn; i += 256) live += (uint32_t)__syncthreads_count(i + tid < cn && a.rows[in0 + i + tid] != 0u);
    const uint32_t take = live < a.topk ? live : a.topk;
    for (uint32_t s = tid; s < a.topk; s += 256) {
        const bool held = s < take;
        const unsigned long long q = s_key[held ? s : 0u];
        a.out_dist[out0 + s] = held ? ord32_unbias((uint32_t)(q >> 32)) : __builtin_bit_cast(float, RQ_MAXSIM_NAN_BITS);
        k.out_keys[out0 + s] = held ? k.values[(uint32_t)q] : 0ull;
    }
    if (tid == 0) a.out_n[b] = take, a.out_cand[b] = cn;
}
#endif  // RQ_MAXSIM_KERNELS
