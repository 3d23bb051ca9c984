// kernels_exact_tiered.h -- the exact search on split-row and tiered indexes: rq_exact_search_tiered*, rq_exact_range_search_tiered* of
// include/rabitq_hip.h.  The contract, the phases and the append are kernels_exact.h's; what is new here is how a block
// gets its rows and what it knows about them.
//
// Rows.  A launch scans the PHYSICAL rows of one tier, linearly: the HBM array [0, n_dev) or the host array [0, n - n_dev) (an
// untiered split-row index: its one array, where a row lies at its position).  TierView turns a physical row back into its
// cluster-order position -- the filter bit, the candidate record and map_ids are by position -- from the list of the block's first
// row (a per-launch table, one bisection per block: tier_tile_list_kernel) and a walk over the lists the tile straddles.
//
// Plane 0.  A split row stores h_i = (bits(x_i) + 0x8000) >> 16 in its first 2 dim bytes (common.h): a bf16 image x~ of the row.  The
// plane scan reads those bytes alone and puts them into the LDS image UNCHANGED -- no conversion stands between the load and the
// matrix pass, and the second plane is never read.  Eight lanes share a row, 16 bytes per lane and load; every load of the tile is
// issued before the first is consumed, and the code is ORDERED so that sub-tile 0 is written to LDS and multiplied (the block's first
// query tiles) before the later sub-tiles are touched (RT = 1: the row in slices of 512 dimensions, two slices in registers).  What
// the compiled kernel does with that order today: the loads sit under predicates, and the wait in front of sub-tile 0 is vmcnt(0) --
// it drains the whole tile; and the query fragments are vector loads too, whose in-order counter would drain the tile at the first
// MFMA anyway.  The overlap of the first MFMAs with the later sub-tiles' loads is therefore NOT reached yet ("Open").
// The plain-f32 form of the same body (tiered, unsplit indexes) loads 32 bytes per lane and step and rounds as exact_scan_kernel does.
//
// Bound of the plane scan.  The scan computes  a = (|x~|^2 + |q'|^2) - 2 <x~, q~>  in f32, q~ = q' rounded to bf16 (nearest even),
// |x~|^2 the f32 sum of the squares of the plane-0 elements -- the true |x|^2 would need the second plane.  Let e = |x - q'|^2.
//   (1) x~_i = x_i (1 + d_i), |d_i| <= 2^-8: adding 0x8000 to the bit pattern and cutting 16 bits rounds the MAGNITUDE to the nearest
//       bf16, ties away from zero (the sign bit is above the carry); the error is half a bf16 ulp like round-to-nearest-even's, only
//       the tie rule differs.  q~_i = q'_i (1 + g_i), |g_i| <= 2^-8.
//   (2) | |x~|^2 - |x|^2 | = | sum x_i^2 (2 d_i + d_i^2) | <= (2^-7 + 2^-16) |x|^2.
//   (3) | <x~, q~> - <x, q'> | = | sum x_i q'_i (d_i + g_i + d_i g_i) | <= (2^-7 + 2^-16) |x| |q'|  (Cauchy-Schwarz).
//   (4) in exact arithmetic therefore |a - e| <= (2^-7 + 2^-16)(|x|^2 + 2 |x||q'|) <= (2^-7 + 2^-16)(|x| + |q'|)^2.
//   (5) the kernel holds |x~|, not |x|: |x| <= |x~| / (1 - 2^-8), so (|x| + |q'|)^2 <= (1 + 2^-7 + 2^-13)(|x~| + |q'|)^2, and
//       (2^-7 + 2^-16)(1 + 2^-7 + 2^-13) < 2^-7 + 2^-13.
//   (6) the f32 accumulation of the products, of the two norms and the reference's own chain: (2 dim + 64) 2^-24 (|x~| + |q'|)^2, the
//       term of kernels_exact.h ("Approximation") -- the same operations on operands of the same size.
//       m' = (2^-7 + 2^-13 + (2 dim + 64) 2^-24) 1.05 (|x~| + |q'|)^2  >=  |a - e|,
//   twice the plain scan's m in its leading term: the norm is now approximate too and its error adds to the product's.  The factor
//   1.05 is the slack kernels_exact.h keeps and is as load-bearing here.  A row of the answer has a <= e + m' <= T_q + m'.
// Non-finite values.  A pair is kept when either side of the test is NaN.  A row whose |x~|^2 is not below 3.0e38 is always kept
// (inf, NaN, a finite element that plane 0 rounds up to inf, overflow): its e may still be finite.  Below that threshold every x~_i
// is finite, so every x_i is (|x_i| <= |x~_i| (1 + 2^-8) -- but see the next sentence) and |x|^2 <= 1.008 x 3.0e38 < f32::MAX: the
// true norm of a row the test judges is finite, (1) - (6) apply, and an overflow of |x~|^2 + |q'|^2 or of the product makes the
// bound's (|x~| + |q'|)^2 overflow as well, which keeps the pair.  The one element plane 0 hides: a NaN whose bit pattern is at or
// above 0x7FFF8000 (either sign) wraps to -0 / +0.  Such a row is judged like a finite one and may be dropped; its e is NaN, and the
// contract never returns a row at NaN.
#pragma once
#include "kernels_exact.h"

// A physical row of one tier -> its position.  lt == null: an untiered index, row r is position r.
struct TierView {
    const ListTier *lt;
    uint32_t k;
    uint32_t tier;  // 0 = the HBM array, 1 = the host array
    uint32_t rows;  // rows of the tier's array
    __device__ __forceinline__ uint32_t first_row(uint32_t c) const { return tier ? lt[c].host_base : lt[c].hbm_base; }
    // the list row r belongs to: the largest c whose first row is <= r (lists without a row in this tier share theirs with the next one)
    __device__ __forceinline__ uint32_t list_of(uint32_t r) const {
        uint32_t lo = 0, hi = k;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (first_row(mid) <= r) lo = mid;
            else hi = mid;
        }
        return lo;
    }
    // position of row r, walking up from a list c at or before its own (the list of the tile's first row)
    __device__ __forceinline__ uint32_t position(uint32_t r, uint32_t c) const {
        if (!lt) return r;
        while (c + 1 < k && first_row(c + 1) <= r) ++c;
        const ListTier t = lt[c];
        return tier ? t.off + t.h + (r - t.host_base) : t.off + (r - t.hbm_base);
    }
};

struct TierScanArgs {
    ExactArgs a;                // base: the index's view (the exact distances resolve positions through BaseView::row)
    const float *rows;          // the tier's array: physical row r at rows + r dim
    TierView tv;
    const uint32_t *tile_list;  // per block of the scan: the list of its first row (null: untiered)
};

// c' of m' = c' (|x~| + |q'|)^2, the plane scan's margin (above); 1.05 is LOAD-BEARING as in ex_margin_factor
static inline __host__ __device__ float ex_plane_margin_factor(uint32_t dim) {
    return (0.0078125f + 0.0001220703125f + (float)(2 * dim + 64) * 5.9604645e-8f) * 1.05f;
}

// the launches (inst_exact_tiered.hip)
hipError_t exact_tiered_set_attributes();
void launch_tier_tile_list(const TierView &tv, uint32_t tile_rows, uint32_t tiles, uint32_t *tile_list, hipStream_t st);
void launch_exact_scan_tier(const TierScanArgs &ta, bool plane, bool range, hipStream_t st);  // the pre-filtered scan of one tier
void launch_exact_dist_tiered(const ExactArgs &a, hipStream_t st);
void launch_exact_range_dist_tiered(const ExactArgs &a, uint32_t *hits, uint32_t records, hipStream_t st);

#ifdef RQ_EXACT_TIERED_KERNELS
// (RQ_EXACT_KERNELS is defined by the unit: kernels_exact.h has brought kernels_rerank.h, exact_margin.h and ex_pair_bound)

__global__ __launch_bounds__(256) void tier_tile_list_kernel(const TierView tv, uint32_t tile_rows, uint32_t tiles, uint32_t *__restrict__ out) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < tiles) out[b] = tv.list_of(b * tile_rows);
}

// 8 elements of a row in flight: the 16 bytes of plane 0, or the 32 bytes of a plain row.  image(): the 16 bytes of the LDS image,
// and the squares of what the image holds (PLANE) / of the row itself (plain) added to s.
template <bool PLANE>
struct ExPiece;
template <>
struct ExPiece<true> {
    uint4 w;
    __device__ __forceinline__ void load(const float *row, uint32_t pc) { w = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(row) + 8 * pc); }
    __device__ __forceinline__ void zero() { w = make_uint4(0u, 0u, 0u, 0u); }
    __device__ __forceinline__ uint4 image(float &s) const {
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float lo = __builtin_bit_cast(float, ww[i] << 16), hi = __builtin_bit_cast(float, ww[i] & 0xFFFF0000u);
            s = fmaf(lo, lo, s), s = fmaf(hi, hi, s);
        }
        return w;
    }
};
template <>
struct ExPiece<false> {
    uint4 wa, wb;  // (the words as loaded)
    __device__ __forceinline__ void load(const float *row, uint32_t pc) {
        wa = *reinterpret_cast<const uint4 *>(row + 8 * pc), wb = *reinterpret_cast<const uint4 *>(row + 8 * pc + 4);
    }
    __device__ __forceinline__ void zero() { wa = make_uint4(0u, 0u, 0u, 0u), wb = wa; }
    __device__ __forceinline__ uint4 image(float &s) const {
        const uint32_t ww[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = __builtin_bit_cast(float, ww[i]), s = fmaf(f[i], f[i], s);
        return make_uint4(ex_bf16_pair(f[0], f[1]), ex_bf16_pair(f[2], f[3]), ex_bf16_pair(f[4], f[5]), ex_bf16_pair(f[6], f[7]));
    }
};

// The scan of one tier: block b owns physical rows [32 RT b, 32 RT (b + 1)) of ta.rows.  The LDS image (row stride 2 dim + 16), the
// fragment layout, the per-pair test and the append are exact_scan_kernel's; the rows' positions stand where that kernel keeps its
// admitted flags (~0 = not admitted).  Order of work:
//   (1) every row's position and filter bit; a tile with nothing admitted ends here;
//   (2) every load of the tile is issued (RT = 1: of the first two 512-dimension slices);
//   (3) per sub-tile (slice): its registers -> image and sum of squares, barrier, and the MFMAs of the block's FIRST query tiles
//       (wave w: tile w) over it (meant to run under the later sub-tiles' loads: see the header comment for what is reached);
//   (4) the first tiles' test and append, then the remaining query tiles as exact_scan_kernel streams them (RT MFMAs per slab).
// PLANE: rows are split rows and only plane 0 is read (margin m'); else plain f32 rows (margin m of kernels_exact.h).
template <int RT, bool PLANE, bool RANGE>
__global__ __launch_bounds__(256, (RT == 1 ? 1 : 2)) void exact_scan_plane_kernel(const TierScanArgs ta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ex_lds[];
    const ExactArgs &a = ta.a;
    const uint32_t dim = a.dim, ROWB = dim * 2 + 16, npc = dim / 8, nslab = dim / 16;
    float *xn2 = reinterpret_cast<float *>(ex_lds + RT * 32 * ROWB), *xsn = xn2 + RT * 32;
    uint32_t *rpos = reinterpret_cast<uint32_t *>(xsn + RT * 32);
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, kh = lane >> 5;
    const uint32_t sub = t & 7, rrow = t >> 3;
    const uint32_t tile0 = blockIdx.x * (32u * RT);  // (a tier has fewer than 2^32 rows, and the grid covers no more than them)
    const uint32_t ngroups = a.nq32 / 32;
    // (1)
    bool ok[RT];
    {
        const uint32_t hint = ta.tile_list ? ta.tile_list[blockIdx.x] : 0u;
        bool any = false;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint32_t lr = rt * 32 + rrow, r = tile0 + lr;
            ok[rt] = (uint64_t)tile0 + lr < ta.tv.rows;
            const uint32_t p = ok[rt] ? ta.tv.position(r, hint) : 0u;
            if (ok[rt] && a.allow) ok[rt] = (a.allow[p >> 5] >> (p & 31)) & 1u;
            if (sub == 0) rpos[lr] = ok[rt] ? p : 0xFFFFFFFFu;
            any |= ok[rt];
        }
        if (!__syncthreads_or(any ? 1 : 0)) return;
    }
    // the MFMAs of sub-tile rt against query tile g over the slabs [m0, m1)
    auto mfma_rows = [&](ex_f32x16 &acc, uint32_t g, uint32_t rt, uint32_t m0, uint32_t m1) {
        const uint16_t *qb = a.qbf + (uint64_t)(32 * g + col) * dim + 8 * kh;
        const unsigned char *img = ex_lds + (rt * 32 + col) * ROWB + 16 * kh;
        for (uint32_t m = m0; m < m1; ++m) {
            const ex_bf16x8 bf = __builtin_bit_cast(ex_bf16x8, *reinterpret_cast<const uint4 *>(qb + 16 * m));
            const ex_bf16x8 af = *reinterpret_cast<const ex_bf16x8 *>(img + 32 * m);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
        }
    };
    ex_f32x16 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = ex_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bool first = wave < ngroups;  // (wave-uniform) this wave has a first query tile: tile `wave`
    // (2), (3)
    if constexpr (RT > 1) {
        constexpr int PCS = RT == 4 ? 3 : 7;  // 16-byte pieces per lane and row: dim <= 192 (RT = 4), <= 448 (RT = 2)
        ExPiece<PLANE> v[RT][PCS];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const float *row = ta.rows + (uint64_t)(tile0 + rt * 32 + rrow) * dim;
#pragma unroll
            for (int i = 0; i < PCS; ++i) {
                if (ok[rt] && sub + 8u * i < npc) v[rt][i].load(row, sub + 8u * i);
                else v[rt][i].zero();
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint32_t lr = rt * 32 + rrow;
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < PCS; ++i)
                if (sub + 8u * i < npc) *reinterpret_cast<uint4 *>(ex_lds + lr * ROWB + 16 * (sub + 8u * i)) = v[rt][i].image(s);
            s += __shfl_xor(s, 1, 8), s += __shfl_xor(s, 2, 8), s += __shfl_xor(s, 4, 8);
            if (sub == 0) xn2[lr] = s, xsn[lr] = sqrtf(s) * 1.000001f;
            __syncthreads();
            if (first) mfma_rows(acc[rt], wave, rt, 0, nslab);
        }
    } else {
        const float *row = ta.rows + (uint64_t)(tile0 + rrow) * dim;
        const uint32_t nsl = (npc + 63) / 64;  // slices of 64 pieces: 512 dimensions, 32 slabs
        ExPiece<PLANE> va[8], vb[8];
        float s = 0.0f;
        auto fetch = [&](ExPiece<PLANE>(&v)[8], uint32_t sl) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t pc = 64 * sl + sub + 8u * i;
                if (ok[0] && pc < npc) v[i].load(row, pc);
                else v[i].zero();
            }
        };
        auto place = [&](const ExPiece<PLANE>(&v)[8], uint32_t sl) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t pc = 64 * sl + sub + 8u * i;
                if (pc < npc) *reinterpret_cast<uint4 *>(ex_lds + rrow * ROWB + 16 * pc) = v[i].image(s);
            }
            __syncthreads();
            if (first) mfma_rows(acc[0], wave, 0, 32 * sl, 32 * sl + 32 < nslab ? 32 * sl + 32 : nslab);
        };
        if constexpr (PLANE) {
            fetch(va, 0);
            for (uint32_t sl = 0; sl < nsl; sl += 2) {  // (block-uniform: every thread meets the same barriers)
                if (sl + 1 < nsl) fetch(vb, sl + 1);
                place(va, sl);
                if (sl + 1 < nsl) {
                    if (sl + 2 < nsl) fetch(va, sl + 2);
                    place(vb, sl + 1);
                }
            }
        } else {
            // (plain rows: one slice in registers -- 64 VGPRs a slice, and the compiler of this release does not survive the two-slice form)
            for (uint32_t sl = 0; sl < nsl; ++sl) {
                fetch(va, sl);
                place(va, sl);
            }
        }
        s += __shfl_xor(s, 1, 8), s += __shfl_xor(s, 2, 8), s += __shfl_xor(s, 4, 8);
        if (sub == 0) xn2[rrow] = s, xsn[rrow] = sqrtf(s) * 1.000001f;
    }
    __syncthreads();  // the norms of the last sub-tile
    // this lane's 16 rows of every sub-tile: admitted mask, and whether the norm is one the test may judge
    uint32_t amask[RT], wild[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        amask[rt] = 0u, wild[rt] = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t lr = rt * 32 + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
            amask[rt] |= rpos[lr] != 0xFFFFFFFFu ? (1u << r) : 0u;
            wild[rt] |= xn2[lr] < 3.0e38f ? 0u : (1u << r);
        }
    }
    const float cm = PLANE ? ex_plane_margin_factor(dim) : ex_margin_factor(dim);
    for (uint32_t g = wave; g < ngroups; g += 4) {
        const uint32_t q = 32 * g + col;
        if (g != wave) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt] = ex_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            const uint16_t *qb = a.qbf + (uint64_t)q * dim + 8 * kh;
            const unsigned char *img = ex_lds + col * ROWB + 16 * kh;
            for (uint32_t m = 0; m < nslab; ++m) {
                const ex_bf16x8 bf = __builtin_bit_cast(ex_bf16x8, *reinterpret_cast<const uint4 *>(qb + 16 * m));
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const ex_bf16x8 af = *reinterpret_cast<const ex_bf16x8 *>(img + rt * 32 * ROWB + 32 * m);
                    acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[rt], 0, 0, 0);
                }
            }
        }
        uint32_t mine[RT];
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
        if constexpr (RANGE) {
            // (the wave is whole here: the loop over g is uniform and nothing above leaves it)
            const bool live = q < a.nq && a.thr[q] > 0.0f;
            uint32_t c = 0;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                if (!live) mine[rt] = 0u;
                c += (uint32_t)__popc(mine[rt]);
            }
            const uint32_t inc = wave_incl_scan(c);
            const uint32_t total = __shfl(inc, 63, 64);
            if (total == 0) continue;
            unsigned long long start = 0;
            if (lane == 63) start = atomicAdd(a.rec_count, (unsigned long long)total);
            unsigned long long at = __shfl(start, 63, 64) + (inc - c);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                uint32_t mk = mine[rt];
                while (mk) {
                    const uint32_t r = (uint32_t)__builtin_ctz(mk);
                    mk &= mk - 1u;
                    if (at < a.cap) a.rec[at] = make_uint2(q, rpos[rt * 32 + (r & 3u) + 8u * (r >> 2) + 4u * kh]);
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
                if (at < a.cap) slots[at] = rpos[rt * 32 + (r & 3u) + 8u * (r >> 2) + 4u * kh];
                ++at;
            }
        }
    }
}

// exact_dist_kernel with the row resolved through BaseView::row (either tier, plain or split): exact_l2_row is called, not restated
__global__ __launch_bounds__(256) void exact_dist_tiered_kernel(const ExactArgs a) {
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
        const float e = exact_l2_row(a.base.row(pos, dim), q_lds, dim, hf);
        if (hf == 0) {
            const bool in = e <= T && e < 3.4028234663852886e38f;
            a.keys[(uint64_t)q * a.cap + i] = in ? ((unsigned long long)ord32_biased(e) << 32) | a.map_ids[pos] : ~0ull;
        }
    }
}

// exact_range_dist_kernel likewise
__global__ __launch_bounds__(256) void exact_range_dist_tiered_kernel(const ExactArgs a, uint32_t *__restrict__ hit_cnt, uint32_t m) {
    const uint32_t dim = a.dim, hf = threadIdx.x & 1, lane = threadIdx.x & 63;
    const uint32_t rounds = (uint32_t)(((uint64_t)m + 127) / 128);
    for (uint32_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const uint64_t i = (uint64_t)rd * 128 + (threadIdx.x >> 1);
        const bool have = i < m;  // (the same for the two lanes of a pair)
        const uint2 rec = have ? a.rec[i] : make_uint2(0xFFFFFFFFu, 0u);
        bool hit = false;
        if (have) {
            const float e = exact_l2_row(a.base.row(rec.y, dim), a.qpad + (uint64_t)rec.x * dim, dim, hf);
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
#endif  // RQ_EXACT_TIERED_KERNELS
