// kernels_directory.h -- rows by id (host_directory.h), wave64: the id directory (build, lookup), the random-row gather
// behind rq_fetch_rows / rq_fetch_stored / rq_neighbours_of, the by-id exact distances and the kernel that drops a row from its own
// neighbours.  Nothing here writes an array of the index.
//
// THE DIRECTORY maps an id to its position in the layout.  Two forms, chosen from top = 1 + the largest stored id alone:
//   dense (top <= 4 n + 65536): pos_of_id[top], u32, RQ_DIR_ABSENT = no such id.
//   hash  (otherwise): open addressing, linear probing, cap = the power of two >= max(2 n, 16) slots of 64 bits, id << 32 | pos,
//         RQ_DIR_EMPTY = all ones (no stored row has position 2^32 - 1).  THE HASH FUNCTION (tests/by_id_model.py restates it):
//             home(id) = ((id * 0x9E3779B1) mod 2^32) >> (32 - log2(cap))
//         -- the multiplicative (Fibonacci) hash: the top log2(cap) bits of the 32-bit product.  A row is inserted with one 64-bit
//         atomicCAS per slot it looks at, from its home slot upwards (wrapping past the table's end), into the first empty one;
//         a lookup walks the same way until it meets the id or an empty slot.  The set of occupied slots, and so every lookup's
//         answer, does not depend on the order of the insertions; which id of a run sits in which of its slots does, and with
//         it the longest chain met while building (t ids that share a home slot give a chain of at least t).
// Ids are unique in an index (every entry that adds rows checks it), so an id has one position.
#pragma once

#define RQ_DIR_ABSENT 0xFFFFFFFFu
#define RQ_DIR_EMPTY (~0ull)
#define RQ_DIR_HASH_MUL 0x9E3779B1u
// the home slot of an id in a table of 2^bits slots (4 <= bits <= 31)
__host__ __device__ __forceinline__ uint32_t rq_dir_home(uint32_t id, uint32_t bits) { return (uint32_t)(id * RQ_DIR_HASH_MUL) >> (32u - bits); }

// The directory of map_ids[0 .. n): dense != nullptr -- dense[id] = position (dense preset to RQ_DIR_ABSENT, every id < its length);
// else the hash table `slots` of 2^bits slots, preset to RQ_DIR_EMPTY.  *longest (preset to 0): the longest probe chain, in slots
// looked at (1 = the row landed in its home slot).  A table of >= 2 n slots always has an empty one; the walk is bounded by the
// table's size all the same, and a row that found none is counted into *lost (the host refuses the directory).
__global__ __launch_bounds__(256) void directory_build_kernel(const uint32_t *__restrict__ map_ids, uint64_t n, uint32_t *__restrict__ dense,
                                                              unsigned long long *__restrict__ slots, uint32_t bits,
                                                              unsigned int *__restrict__ longest, unsigned int *__restrict__ lost) {
    uint32_t chain_max = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
        const uint32_t id = map_ids[p];
        if (dense) {
            dense[id] = (uint32_t)p;
            continue;
        }
        const unsigned long long val = ((unsigned long long)id << 32) | (uint32_t)p;
        const uint32_t mask = (1u << bits) - 1u;
        uint32_t s = rq_dir_home(id, bits), chain = 1;
        bool placed = false;
        for (; chain <= mask + 1u; ++chain, s = (s + 1u) & mask)
            if (atomicCAS(slots + s, RQ_DIR_EMPTY, val) == RQ_DIR_EMPTY) {
                placed = true;
                break;
            }
        if (!placed) atomicAdd(lost, 1u);
        else chain_max = chain > chain_max ? chain : chain_max;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t t = __shfl_xor(chain_max, o, 64);
        chain_max = t > chain_max ? t : chain_max;
    }
    if ((threadIdx.x & 63) == 0 && chain_max) atomicMax(longest, chain_max);
}

// ids[0 .. m) -> pos[0 .. m): the position of the stored row with that id, RQ_DIR_ABSENT if there is none (an id at or above `top`
// without a memory access) or if the row is dead (live: the position bitmap of the index's pending removals, nullable).
// Duplicates in the request are answered one by one.  *found (preset to 0) += the ids that have a live row.
__global__ __launch_bounds__(256) void directory_lookup_kernel(const uint32_t *__restrict__ ids, uint64_t m, uint64_t top,
                                                               const uint32_t *__restrict__ dense, const unsigned long long *__restrict__ slots,
                                                               uint32_t bits, const uint32_t *__restrict__ live, uint32_t *__restrict__ pos,
                                                               unsigned long long *__restrict__ found) {
    unsigned long long hits = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const uint32_t id = ids[i];
        uint32_t p = RQ_DIR_ABSENT;
        if ((uint64_t)id < top) {
            if (dense) {
                p = dense[id];
            } else {
                const uint32_t mask = (1u << bits) - 1u;
                uint32_t s = rq_dir_home(id, bits);
                for (uint32_t step = 0; step <= mask; ++step, s = (s + 1u) & mask) {
                    const unsigned long long slot = slots[s];
                    if (slot == RQ_DIR_EMPTY) break;
                    if ((uint32_t)(slot >> 32) == id) {
                        p = (uint32_t)slot;
                        break;
                    }
                }
            }
        }
        if (live && p != RQ_DIR_ABSENT && !((live[p >> 5] >> (p & 31u)) & 1u)) p = RQ_DIR_ABSENT;
        pos[i] = p;
        hits += p != RQ_DIR_ABSENT ? 1u : 0u;
    }
    for (int o = 32; o >= 1; o >>= 1) hits += __shfl_xor(hits, o, 64);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(found, hits);
}

// ---- the gather ------------------------------------------------------------------------------------------------------------------
// What a gather moves per row.  FETCH_F32 / FETCH_HALF / FETCH_BYTE: the row of an untiered index of that row kind, widened to dim
// f32 (rq_fetch_rows).  FETCH_RAW: the stored bytes of a typed row as they are (rq_fetch_stored).  FETCH_COLD: a tiered index's
// f32 row, found by BaseView::row() (a bisection over the lists; either tier, plain or split) -- an instantiation of its own, so
// that the untiered ones carry none of it.
enum { FETCH_F32 = 0, FETCH_HALF = 1, FETCH_BYTE = 2, FETCH_RAW = 3, FETCH_COLD = 4 };

struct FetchSrc {
    const uint8_t *p;  // the row's first byte
    bool split;        // FETCH_COLD: two 16-bit planes (common.h)
};
template <int MODE>
__device__ __forceinline__ FetchSrc fetch_src(const BaseView &base, uint32_t pos, uint32_t dim, uint32_t row_bytes) {
    if constexpr (MODE == FETCH_COLD) {
        const RowRef r = base.row(pos, dim);
        return FetchSrc{reinterpret_cast<const uint8_t *>(r.p), r.split};
    } else {
        return FetchSrc{reinterpret_cast<const uint8_t *>(base.dev) + (uint64_t)pos * row_bytes, false};
    }
}
// Lane piece lp of a row: the bytes that become 16 bytes of the destination -- 16 of an f32 or raw row, 8 of a half-precision row,
// 4 of a byte row, 8 + 8 of the two planes of a split row.  Always loaded (no branch around a load, see below).
template <int MODE>
__device__ __forceinline__ uint4 fetch_load(const FetchSrc s, uint32_t lp, uint32_t dim) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (MODE == FETCH_HALF) {
        const uint2 w = *reinterpret_cast<const uint2 *>(s.p + 8u * lp);
        r.x = w.x, r.y = w.y;
    } else if constexpr (MODE == FETCH_BYTE) {
        r.x = *reinterpret_cast<const uint32_t *>(s.p + 4u * lp);
    } else if constexpr (MODE == FETCH_COLD) {
        if (s.split) {  // (one row per sub-group: the branch does not split a row)
            const uint2 h = *reinterpret_cast<const uint2 *>(s.p + 8u * lp), lo = *reinterpret_cast<const uint2 *>(s.p + 2u * dim + 8u * lp);
            r.x = h.x, r.y = h.y, r.z = lo.x, r.w = lo.y;
        } else {
            r = *reinterpret_cast<const uint4 *>(s.p + 16u * lp);
        }
    } else {
        r = *reinterpret_cast<const uint4 *>(s.p + 16u * lp);
    }
    return r;
}
// (the same reason as merge_pin, kernels_relayout.h: the loads of a step stay ahead of its first store)
__device__ __forceinline__ void fetch_pin(uint4 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
__device__ __forceinline__ uint32_t fetch_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
// The 16 destination bytes of a lane piece: W of the stored elements (rows.h: exact), the joined planes of a split row.
template <int MODE>
__device__ __forceinline__ uint4 fetch_widen(const uint4 r, bool split, uint32_t fmt) {
    if constexpr (MODE == FETCH_HALF) {
        return make_uint4(fetch_bits(rq_widen_elem((uint16_t)r.x, fmt)), fetch_bits(rq_widen_elem((uint16_t)(r.x >> 16), fmt)),
                          fetch_bits(rq_widen_elem((uint16_t)r.y, fmt)), fetch_bits(rq_widen_elem((uint16_t)(r.y >> 16), fmt)));
    } else if constexpr (MODE == FETCH_BYTE) {
        return make_uint4(fetch_bits(rq_widen_byte((uint8_t)r.x, fmt)), fetch_bits(rq_widen_byte((uint8_t)(r.x >> 8), fmt)),
                          fetch_bits(rq_widen_byte((uint8_t)(r.x >> 16), fmt)), fetch_bits(rq_widen_byte((uint8_t)(r.x >> 24), fmt)));
    } else if constexpr (MODE == FETCH_COLD) {
        if (!split) return r;
        return make_uint4(rq_split_join(r.x & 0xFFFFu, r.z & 0xFFFFu), rq_split_join(r.x >> 16, r.z >> 16),
                          rq_split_join(r.y & 0xFFFFu, r.w & 0xFFFFu), rq_split_join(r.y >> 16, r.w >> 16));
    } else {
        return r;
    }
}
// v, or zeros: a mask per word (a ?: between two 16-byte values goes through scratch memory in hipcc's hands)
__device__ __forceinline__ uint4 fetch_keep(const uint4 v, bool keep) {
    const uint32_t k = keep ? 0xFFFFFFFFu : 0u;
    return make_uint4(v.x & k, v.y & k, v.z & k, v.w & k);
}

// Destination row q = the row at position pos[q], or (pos[q] == RQ_DIR_ABSENT) a row of zeros; found[q] (nullable) = 1 / 0.
// absent_row0: an absent id's destination receives row 0 of the index instead of zeros (rq_neighbours_of: the row becomes a query
// whose answer is thrown away, and a query of zeros is not one every metric takes).  The index has at least one row.
// A random-row gather, bandwidth-bound, shaped as merge_gather_kernel is (kernels_relayout.h) -- for bytes in flight: a wave is
// cut into 64 / G sub-groups of G lanes, one row each, R rows in flight per sub-group; a step has three phases with nothing
// consumed inside one -- (1) the R positions, (2) validity and source addresses, (3) every load of all R rows, pinned there by
// fetch_pin -- and only then the stores.  The loads are UNCONDITIONAL: a lane past the row's end reads the row's last piece again,
// a destination past m or an absent id reads row 0.  One instruction of a wave stores 64 / G ADJACENT destination rows: the wave
// owns R * 64 / G consecutive destinations per step and sub-group g takes rows g, g + 64 / G, ...
// What differs from merge_gather_kernel: a lane owns 16 bytes of the DESTINATION (LP of them per row: dim / 4 where the row is
// widened, row_bytes / 16 where it is copied), because a typed row writes 2 or 4 times the bytes it reads and the stores are what
// has to be contiguous; its load narrows to 8 or 4 bytes, which still covers the source row once, contiguously.  G = the power of
// two >= LP, at least 4 (a raw byte row at dim 64 is 4 pieces), at most 64; a row of more than 64 pieces takes further steps.
// dim is a multiple of 64 and `out` 16-byte aligned: every access is aligned.  Vector loads and stores only.
template <int MODE, int G, int R>
__global__ __launch_bounds__(256) void fetch_gather_kernel(const uint32_t *__restrict__ pos, uint64_t m, const BaseView base, uint32_t dim,
                                                           uint32_t LP, uint32_t absent_row0, uint4 *__restrict__ out,
                                                           uint32_t *__restrict__ found) {
    constexpr uint32_t SUBS = 64 / G, RPW = R * SUBS;
    const uint32_t lane = threadIdx.x & 63, sub = lane / G, l = lane % G;
    const uint32_t lc = l < LP ? l : LP - 1;  // this lane's piece, or the last one once more
    const uint32_t row_bytes = (uint32_t)RowSpec{base.fmt}.row_bytes(dim);
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t q0 = wave0 * RPW; q0 < m; q0 += nwaves * RPW) {
        uint64_t q[R];
        uint32_t p[R];
        bool in[R], ok[R];
        FetchSrc src[R];
        uint4 raw[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {  // phase 1: the positions
            q[r] = q0 + (uint32_t)r * SUBS + sub;
            p[r] = pos[q[r] < m ? q[r] : m - 1];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {  // phase 2: where each row comes from
            in[r] = q[r] < m;
            ok[r] = in[r] && p[r] != RQ_DIR_ABSENT;
            src[r] = fetch_src<MODE>(base, ok[r] ? p[r] : 0u, dim, row_bytes);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) raw[r] = fetch_load<MODE>(src[r], lc, dim);  // phase 3: every load, nothing used
#pragma unroll
        for (int r = 0; r < R; ++r) fetch_pin(raw[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!in[r]) continue;
            if (l < LP) out[q[r] * LP + l] = fetch_keep(fetch_widen<MODE>(raw[r], src[r].split, base.fmt), ok[r] || absent_row0);
            if (l == 0 && found) found[q[r]] = ok[r] ? 1u : 0u;
        }
        if (G == 64)  // rows of more than 64 pieces: the rest, R rows in flight again
            for (uint32_t e0 = 64; e0 < LP; e0 += 64) {
                const uint32_t e = e0 + l, ec = e < LP ? e : LP - 1;
#pragma unroll
                for (int r = 0; r < R; ++r) raw[r] = fetch_load<MODE>(src[r], ec, dim);
#pragma unroll
                for (int r = 0; r < R; ++r) fetch_pin(raw[r]);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (in[r] && e < LP) out[q[r] * LP + e] = fetch_keep(fetch_widen<MODE>(raw[r], src[r].split, base.fmt), ok[r] || absent_row0);
            }
    }
}

// ---- exact distances by id (rq_pair_distances) -------------------------------------------------------------------------------------
// Query b (prepared: transformed and padded to dim, as the rerank sees it) against the rows at pos[b * c .. b * c + c): one block per
// query, the query in LDS, a pair of lanes per row -- exact_l2_row (kernels_rerank.h), the one exact-distance routine, so every
// value is rq_rerank's for that position and query, bit for bit.  RQ_DIR_ABSENT gives +inf (the pair reads row 0 and drops the
// result: the fold exchanges between the two lanes, so neither may skip it).  The index has at least one row.
__global__ __launch_bounds__(256) void pair_distance_kernel(const float *__restrict__ q, const uint32_t *__restrict__ pos, uint32_t c,
                                                            const BaseView base, uint32_t dim, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float pair_q[];  // dim floats
    const uint64_t b = blockIdx.x;
    for (uint32_t e = threadIdx.x; e < dim; e += 256) pair_q[e] = q[b * dim + e];
    __syncthreads();
    const uint32_t hf = threadIdx.x & 1;
    for (uint32_t j = threadIdx.x >> 1; j < c; j += 128) {
        const uint32_t p = pos[b * c + j];
        const float d = exact_l2_row(base.row(p != RQ_DIR_ABSENT ? p : 0u, dim), pair_q, dim, hf);
        if (hf == 0) out[b * c + j] = p != RQ_DIR_ABSENT ? d : __builtin_inff();
    }
}

// ---- a row's neighbours without the row (rq_neighbours_of) -------------------------------------------------------------------------
// Row i of a plain call at topk + 1 (dist / id: m x (topk + 1), cnt[i] entries, in the plain call's order) -> row i of m x topk:
// the first entry whose id is ids[i] leaves, or the last one if there is none; the rest keep their order, and the slots behind them
// hold NaN / 0xFFFFFFFF.  An id without a row (pos[i] == RQ_DIR_ABSENT) gets a row of those.  One wave per row.
__global__ __launch_bounds__(256) void drop_self_kernel(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ pos, uint64_t m,
                                                        uint32_t topk, const float *__restrict__ dist, const uint32_t *__restrict__ id,
                                                        const uint32_t *__restrict__ cnt, float *__restrict__ out_dist,
                                                        uint32_t *__restrict__ out_id, uint32_t *__restrict__ out_found) {
    const uint32_t lane = threadIdx.x & 63, w = topk + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += (uint64_t)gridDim.x * 4) {
        const bool have = pos[i] != RQ_DIR_ABSENT;
        const uint32_t n = have ? (cnt[i] < w ? cnt[i] : w) : 0u, self = ids[i];
        uint32_t drop = n ? n - 1 : 0u;  // the last entry, unless the row itself is among them
        uint32_t first = 0xFFFFFFFFu;
        for (uint32_t e = lane; e < n; e += 64)
            if (id[i * w + e] == self) {
                first = e;  // (a lane's entries ascend: its first match is its smallest)
                break;
            }
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t t = __shfl_xor(first, o, 64);
            first = t < first ? t : first;
        }
        if (first != 0xFFFFFFFFu) drop = first;
        for (uint32_t e = lane; e < topk; e += 64) {
            const uint32_t s = e < drop ? e : e + 1;
            const bool valid = n != 0 && s < n;
            out_dist[i * topk + e] = valid ? dist[i * w + s] : __builtin_nanf("");
            out_id[i * topk + e] = valid ? id[i * w + s] : 0xFFFFFFFFu;
        }
        if (lane == 0) out_found[i] = have ? 1u : 0u;
    }
}
