// kernels_keyed_tiered.h -- the keyed exact search on wide, split-row and tiered indexes: rq_exact_search_keyed_tiered* of
// include/rabitq_hip.h (host_keyed_tiered.h), wave64.  The contract, the plan (keyed_plan.h), the query images
// (keyed_prep_kernel), the items that read no row (keyed_scan_kernel<.., false, 1>), the exact distances (exact_dist_tiered_kernel) and
// the selection are the existing ones, reached by their launch interfaces.  What is new here is the matrix pass of an item:
//
// DIMENSION-SLICED SCAN: keyed_scan_sliced_kernel<PLANE, S>, one block of four waves per work item, as keyed_scan_kernel.  The block
// stages its query tile once, WHOLE (the bf16 image, row stride 2 dim + 16 bytes, |q'|^2, its scaled root, T_q); a wave's slab holds
// only S elements of its 32 rows (row stride 2 S + 16 bytes).  Per 32-row tile the wave walks the dimension in slices of S:
//   land   slice s from registers into the slab (PLANE: the words as loaded; plain rows: rounded by ex_bf16_pair), the squares added
//          to the sums the loading lanes keep across the slices;
//   issue  the raw loads of slice s + 1 -- behind the last slice, the NEXT tile's positions, row addresses and slice 0 -- into the
//          same registers;
//   mfma   S / 16 v_mfma_f32_32x32x16_bf16 of the slab against columns [s S, s S + S) of the query tile, into the SAME 16 accumulators.
// A row of 3 KB is never waited for as a whole: the loads of one slice run under the matrix pass of the slice before (the register
// double buffer of keyed_scan_kernel's SLABS = 2, across slices instead of tiles).  A position becomes a row address ONCE per row
// and tile (lanes 0 .. 31, BaseView::row: either tier, plain or split), shared through LDS; an unadmitted row reads position 0's row and is never kept.
// Eight lanes share a row, 16 bytes per lane and load.  The last slice of a dimension that S does not divide is short (64 elements).
//
// PLANE = true (split rows): the first plane alone is read, 2 dim bytes a row, and goes to the slab unchanged; |x~|^2 is summed from
// the same registers; the margin is ex_plane_margin_factor(dim) with exact_scan_plane_kernel's keep rules.  The proof is that
// kernel's (kernels_exact_tiered.h, "Bound of the plane scan" and "Non-finite values"): the same operands, the same rounding, the
// same test -- the order in which f32 sums are taken is free there ((6): any order of dim + O(1) operations).
// PLANE = false (plain f32 rows, the unsplit tiered layout included): ex_bf16_pair, |x|^2 from the f32 values, ex_margin_factor(dim)
// and §4.12's keep rules, word for word keyed_scan_kernel's: a NaN on either side keeps, a row whose |x|^2 is not below 3.0e38 is
// always kept, an unadmitted row never.
// The append is keyed_scan_kernel's: the two lanes of a query add their counts, one integer atomicAdd reserves, the count runs on
// past cap.  Vector loads and stores only.  Nothing here writes an array of the index.
#pragma once
#include "kernels_keyed.h"
#include "kernels_exact_tiered.h"  // ex_plane_margin_factor (and, for the host, the exact distances' launch)

// The LDS layout, shared by the host (which picks S and sizes the launch) and the kernel.
struct KeyedSlicedLds {
    uint32_t rowb, srowb;                     // row stride of the query image and of a slab
    uint32_t qimg, qn2, qsn, thr, qb, wave0;  // block offsets
    uint32_t slab, xn2, xsn, pos, row;        // offsets inside a wave's region (pos: two buffers of 32)
    uint32_t wave_bytes, total;
};
__host__ __device__ inline KeyedSlicedLds keyed_sliced_lds(uint32_t dim, uint32_t S) {
    KeyedSlicedLds l{};
    l.rowb = dim * 2 + 16, l.srowb = S * 2 + 16;
    uint32_t o = 0;
    l.qimg = o, o += 32 * l.rowb;
    l.qn2 = o, o += 128;
    l.qsn = o, o += 128;
    l.thr = o, o += 128;
    l.qb = o, o += 128;
    l.wave0 = o;
    uint32_t w = 0;
    l.slab = w, w += 32 * l.srowb;
    l.xn2 = w, w += 128;
    l.xsn = w, w += 128;
    l.pos = w, w += 256;
    l.row = w, w += 256;
    l.wave_bytes = w, l.total = o + 4 * w;
    return l;
}
// The table: S of a dimension, 0 = no matrix pass.  128 where two blocks still share a CU (dim <= 640), else 64 where that keeps two
// (dim <= 896); with one block per CU 128 while it fits (dim <= 1856), then 64.  2048 is where the table ends: dim 2112 would fit with
// 2 KB to spare and little for the small arrays to grow into.
#define RQ_KEYED_SLICED_MAX_DIM 2048u
static inline uint32_t keyed_sliced_slice(uint32_t dim) {
    if (dim > RQ_KEYED_SLICED_MAX_DIM) return 0u;
    if (keyed_sliced_lds(dim, 128).total <= RQ_KEYED_LDS_TWO) return 128u;
    if (keyed_sliced_lds(dim, 64).total <= RQ_KEYED_LDS_TWO) return 64u;
    return keyed_sliced_lds(dim, 128).total <= RQ_KEYED_LDS_MAX ? 128u : 64u;
}

// the launches (inst_keyed_tiered.hip)
hipError_t keyed_sliced_set_attributes();
void launch_keyed_scan_sliced(const KeyedArgs &a, uint32_t nitems, bool plane, hipStream_t st);  // every item takes the matrix pass

#ifdef RQ_KEYED_TIERED_KERNELS
// (RQ_KEYED_KERNELS is defined by the unit: kernels_keyed.h has brought ky_wave_sync, ky_pair_bound, the fragment types, exact_margin.h)

// a row piece as loaded: the address is known to be global memory (a generic pointer would make the loads flat ones, which count on
// the LDS counter too, and every wait for a fragment would then wait for the rows in flight)
typedef uint32_t kt_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) kt_u32x4 *kt_global_u32x4;

template <bool PLANE, int S>
__global__ __launch_bounds__(256) void keyed_scan_sliced_kernel(const KeyedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kt_lds[];
    constexpr uint32_t EPP = PLANE ? 8u : 4u;  // elements of a 16-byte piece
    constexpr uint32_t EB = PLANE ? 2u : 4u;   // bytes of an element as loaded
    constexpr int PCS = S / (8 * EPP);         // pieces per lane, row and slice
    const KeyedSlicedLds L = keyed_sliced_lds(a.dim, S);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, dim = a.dim, col = lane & 31u, kh = lane >> 5;
    const uint4 it = a.items[blockIdx.x];
    const uint32_t tile = it.x, first = it.y, rows = it.z, stride = it.w & 0x7FFFFFFFu;
    uint32_t *qb = reinterpret_cast<uint32_t *>(kt_lds + L.qb);
    // ---- the query tile, once per block, whole ----
    {
        const uint32_t per_row = dim / 8;  // 16-byte pieces of an image row
        for (uint32_t i = tid; i < 32 * per_row; i += 256) {
            const uint32_t r = i / per_row, c = i - r * per_row;
            *reinterpret_cast<uint4 *>(kt_lds + L.qimg + r * L.rowb + 16 * c) = reinterpret_cast<const uint4 *>(a.qbf + ((uint64_t)tile * 32 + r) * dim)[c];
        }
        if (tid < 32) {
            const uint32_t slot = tile * 32u + tid, b = a.order[slot];
            qb[tid] = b;
            reinterpret_cast<float *>(kt_lds + L.qn2)[tid] = a.qn2[slot];
            reinterpret_cast<float *>(kt_lds + L.qsn)[tid] = a.qsn[slot];
            reinterpret_cast<float *>(kt_lds + L.thr)[tid] = b != RQ_KEYED_PAD ? a.thr[b] : 0.0f;
        }
    }
    __syncthreads();
    unsigned char *wl = kt_lds + L.wave0 + wave * L.wave_bytes;
    unsigned char *slab = wl + L.slab;
    float *xn2 = reinterpret_cast<float *>(wl + L.xn2), *xsn = reinterpret_cast<float *>(wl + L.xsn);
    unsigned long long *wrow = reinterpret_cast<unsigned long long *>(wl + L.row);
    const auto wpos = [&](uint32_t s) { return reinterpret_cast<uint32_t *>(wl + L.pos) + 32u * s; };
    const uint32_t b = qb[col];  // this lane's query (lanes col and col + 32 share it: 16 rows of a tile each)
    const uint32_t ntiles = (rows + 31u) / 32u, ns = (dim + S - 1u) / S;
    const float cm = PLANE ? ex_plane_margin_factor(dim) : ex_margin_factor(dim);
    const uint32_t sub = lane & 7u, rr = lane >> 3;  // the gather: eight lanes per row, rows rr, rr + 8, rr + 16, rr + 24
    uintptr_t rowp[4];                               // their addresses (an unadmitted row: position 0's, as keyed_scan_kernel gathers it)
    kt_u32x4 raw[4][PCS];                            // the slice in flight
    float sum[4];
    ky_f32x16 acc;

    const auto load_pos = [&](uint32_t tw) -> uint32_t {
        const uint32_t v = tw * 32u + col;
        return tw < ntiles && v < rows ? a.post[(uint64_t)first + (uint64_t)v * stride] : RQ_KEYED_PAD;
    };
    // positions (RQ_KEYED_PAD = not admitted) of a tile into buffer pb, its row addresses -> anything admitted
    const auto publish = [&](uint32_t p, uint32_t pb) -> bool {
        bool ok = p != RQ_KEYED_PAD;
        if (ok && a.allow) ok = (a.allow[p >> 5] >> (p & 31u)) & 1u;
        if (kh == 0) {
            wpos(pb)[col] = ok ? p : RQ_KEYED_PAD;
            wrow[col] = (unsigned long long)reinterpret_cast<uintptr_t>(a.base.row(ok ? p : 0u, dim).p);
        }
        ky_wave_sync();
#pragma unroll
        for (uint32_t ps = 0; ps < 4; ++ps) rowp[ps] = (uintptr_t)wrow[ps * 8 + rr];
        return __any(ok);
    };
    // (no load sits under a predicate -- a select behind a load makes the compiler wait for it at once, §4.25: a piece past a short
    // last slice reads the row's first piece instead and is never landed)
    const auto issue = [&](uint32_t s) {
#pragma unroll
        for (uint32_t ps = 0; ps < 4; ++ps) {
#pragma unroll
            for (int i = 0; i < PCS; ++i) {
                const uint32_t e = s * S + (sub + 8u * i) * EPP;
                raw[ps][i] = *reinterpret_cast<kt_global_u32x4>(rowp[ps] + (uintptr_t)(e < dim ? e : 0u) * EB);
            }
        }
    };
    const auto land = [&](uint32_t s) {
#pragma unroll
        for (uint32_t ps = 0; ps < 4; ++ps) {
            const uint32_t lr = ps * 8 + rr;
#pragma unroll
            for (int i = 0; i < PCS; ++i) {
                const uint32_t pc = sub + 8u * i;
                if (s * S + pc * EPP >= dim) continue;
                const kt_u32x4 w = raw[ps][i];
                const uint32_t ww[4] = {w[0], w[1], w[2], w[3]};
                if constexpr (PLANE) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float lo = __builtin_bit_cast(float, ww[j] << 16), hi = __builtin_bit_cast(float, ww[j] & 0xFFFF0000u);
                        sum[ps] = fmaf(lo, lo, sum[ps]), sum[ps] = fmaf(hi, hi, sum[ps]);
                    }
                    *reinterpret_cast<kt_u32x4 *>(slab + lr * L.srowb + 16 * pc) = w;
                } else {
                    float x[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j] = __builtin_bit_cast(float, ww[j]), sum[ps] = fmaf(x[j], x[j], sum[ps]);
                    *reinterpret_cast<uint2 *>(slab + lr * L.srowb + 8 * pc) = make_uint2(ex_bf16_pair(x[0], x[1]), ex_bf16_pair(x[2], x[3]));
                }
            }
        }
    };
    // the keep test on the finished accumulators, then the kept positions of buffer pb to their slots
    const auto finish = [&](uint32_t pb) {
        const uint32_t *pos = wpos(pb);
        const float qn = reinterpret_cast<const float *>(kt_lds + L.qn2)[col], qs = reinterpret_cast<const float *>(kt_lds + L.qsn)[col];
        const float T = reinterpret_cast<const float *>(kt_lds + L.thr)[col];
        uint32_t mine = 0u;
        // accumulator register r of lane (col, kh) is row (r & 3) + 8 (r >> 2) + 4 kh of the tile against query col (kernels_exact.h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t lr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kh;
            const float ap = fmaf(-2.0f, acc[r], xn2[lr] + qn);
            const bool keep = !(xn2[lr] < 3.0e38f) || !(ap > ky_pair_bound(T, xsn[lr], qs, cm));
            mine |= keep && pos[lr] != RQ_KEYED_PAD ? (1u << r) : 0u;
        }
        // the two lanes of a query add their counts, the lower one reserves the places of both
        if (b == RQ_KEYED_PAD) mine = 0u;
        const uint32_t c = (uint32_t)__popc(mine), other = __shfl_xor(c, 32, 64);
        uint32_t at = 0u;
        if (kh == 0 && c + other) at = atomicAdd(&a.cnt[b], c + other);
        at = __shfl(at, col, 64) + (kh ? other : 0u);
        uint32_t *slots = a.cand + (uint64_t)(b != RQ_KEYED_PAD ? b : 0u) * a.cap;
        while (mine) {
            const uint32_t r = (uint32_t)__builtin_ctz(mine);
            mine &= mine - 1u;
            if (at < a.cap) slots[at] = pos[(r & 3u) + 8u * (r >> 2) + 4u * kh];
            ++at;
        }
    };
    uint32_t nxt = load_pos(wave);
    // positions, row addresses and slice 0 of tile tw into buffer pb; the positions of the tile behind it are on their way first
    const auto advance = [&](uint32_t tw, uint32_t pb) -> bool {
        const uint32_t p = nxt;
        nxt = load_pos(tw + 4);
        const bool any = publish(p, pb);
        if (any) issue(0);
        return any;
    };
    bool any = wave < ntiles ? advance(wave, 0) : false;  // (uniform per wave) the first tile: nothing to hide it under
    uint32_t pb = 0;
    for (uint32_t tw = wave; tw < ntiles; tw += 4, pb ^= 1u) {  // (uniform per wave)
        const bool more = tw + 4 < ntiles;
        bool any_next = false;
        if (any) {
            acc = ky_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            sum[0] = sum[1] = sum[2] = sum[3] = 0.0f;
            const unsigned char *ai = slab + col * L.srowb + 16 * kh, *bi = kt_lds + L.qimg + col * L.rowb + 16 * kh;
            for (uint32_t s = 0; s < ns; ++s) {
                ky_wave_sync();  // the slab has been read: the slice (the tile) before
                land(s);
                // the next loads are asked for behind the wave's fence (it would wait for them) and before this slice's matrix pass
                if (s + 1 < ns) ky_wave_sync(), issue(s + 1);
                else if (more) any_next = advance(tw + 4, pb ^ 1u);  // (publish has the fence)
                else ky_wave_sync();
                const uint32_t nm = (dim - s * S < (uint32_t)S ? dim - s * S : (uint32_t)S) / 16u;
                for (uint32_t m = 0; m < nm; ++m) {
                    const ky_bf16x8 af = *reinterpret_cast<const ky_bf16x8 *>(ai + 32 * m);
                    const ky_bf16x8 bf = *reinterpret_cast<const ky_bf16x8 *>(bi + 2 * s * S + 32 * m);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (uint32_t ps = 0; ps < 4; ++ps) {
                float t = sum[ps];
                t += __shfl_xor(t, 1, 8), t += __shfl_xor(t, 2, 8), t += __shfl_xor(t, 4, 8);
                if (sub == 0) xn2[ps * 8 + rr] = t, xsn[ps * 8 + rr] = sqrtf(t) * 1.000001f;
            }
            ky_wave_sync();
            finish(pb);
        } else if (more) {
            any_next = advance(tw + 4, pb ^ 1u);
        }
        any = any_next;
    }
}
#endif  // RQ_KEYED_TIERED_KERNELS
