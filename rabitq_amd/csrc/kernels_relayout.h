// kernels_relayout.h -- everything a relayout launches (host_relayout.h): rq_add, rq_remove, rq_compact,
// rq_merge_from and rq_extract, and, at the end, lazy removal (rq_remove_lazy, host_mutate.h), wave64.
// A relayout builds the arrays a fresh build of the live rows would produce.  Every list keeps the build's order, the 64-bit key
// ord32_biased(dist to the list's centroid) << 32 | id, so two sides over the same rotation and centroids (two indexes, or an
// index and a batch that has been through pass 1) merge list by list with a two-way merge by that key and one gather of whole
// rows; nothing stored is rotated, assigned or quantised again.
#pragma once

// ---- the order key ---------------------------------------------------------------------------------------------------------------
// The key word of stored rows p0 .. p0+m (rotated in xrot, m x dim): the distance to the row's own list's centroid in the
// lane order of assign_refine_kernel, with its clamp (a minimum that is not below f32::MAX is f32::MAX: NaN / inf rows, list 0).
__global__ __launch_bounds__(256) void row_key_kernel(const float *__restrict__ xrot, uint64_t p0, uint64_t m, uint32_t dim,
                                                      const float *__restrict__ centroids, const uint32_t *__restrict__ offsets,
                                                      uint32_t k, uint32_t *__restrict__ row_key) {
    const uint32_t hf = threadIdx.x & 1;
    const uint64_t v = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 1;
    if (v >= m) return;
    const uint64_t p = p0 + v;
    uint32_t lo = 0, hi = k;  // largest c with offsets[c] <= p (empty lists share their start with the next one)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= p) lo = mid;
        else hi = mid;
    }
    const float dd = pair_l2sq_exact(xrot + v * dim + 4 * hf, centroids + (uint64_t)lo * dim + 4 * hf, dim);
    if (hf == 0) row_key[p] = ord32_biased(dd < 3.402823466e+38f ? dd : 3.402823466e+38f);
}

// out[0] = 1 + the largest id in map_ids (0 if n == 0), out[1] = ids of map_ids found among the m ascending ids `sorted`
// (nullable); out preset to 0
__global__ __launch_bounds__(256) void id_scan_kernel(const uint32_t *__restrict__ map_ids, uint64_t n, const uint32_t *__restrict__ sorted,
                                                      uint32_t m, unsigned long long *__restrict__ out) {
    unsigned long long top = 0, hits = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
        const uint32_t id = map_ids[p];
        top = (unsigned long long)id + 1 > top ? (unsigned long long)id + 1 : top;
        if (sorted && m) {
            uint32_t lo = 0, hi = m;  // first batch id not below `id`
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (sorted[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            hits += lo < m && sorted[lo] == id ? 1u : 0u;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long t = __shfl_xor(top, o, 64), h = __shfl_xor(hits, o, 64);
        top = t > top ? t : top;
        hits += h;
    }
    if ((threadIdx.x & 63) == 0) {
        if (top) atomicMax(out, top);
        if (hits) atomicAdd(out + 1, hits);
    }
}

// Adjacent rows of a list out of the build's order (key not strictly above its predecessor's), one block per list, counted
// into *bad.  An index made by rq_build / rq_add never has one; rq_from_arrays / rq_load_dir take whatever order they are given.
__global__ __launch_bounds__(256) void list_order_kernel(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ row_key,
                                                         const uint32_t *__restrict__ map_ids, unsigned int *__restrict__ bad) {
    const uint32_t b = offsets[blockIdx.x], e = offsets[blockIdx.x + 1];
    uint32_t cnt = 0;
    for (uint32_t p = b + 1 + threadIdx.x; p < e; p += 256) {
        const unsigned long long k0 = ((unsigned long long)row_key[p - 1] << 32) | map_ids[p - 1];
        const unsigned long long k1 = ((unsigned long long)row_key[p] << 32) | map_ids[p];
        cnt += k0 < k1 ? 0u : 1u;
    }
    if (cnt) atomicAdd(bad, cnt);
}

// The batch of an rq_add as a side of the merge, in the shape of an index's arrays: sorted row j of the batch (keys: grouped by
// list, each list ascending by ord32_biased(dist) << 32 | rank of the row's id within the batch) gets its key word, its id
// (ids[rank], ascending; nullptr: id0 + rank), the codes and factors pass 1 left by input row (src[rank]; nullptr: rank) and its
// raw vector, m x d input rows zero-padded to dim as the build pads them.  One wave per row.
__global__ __launch_bounds__(256) void batch_side_kernel(const unsigned long long *__restrict__ keys, uint64_t m, uint32_t dim, uint32_t W,
                                                         const uint32_t *__restrict__ ids, uint32_t id0, const uint32_t *__restrict__ src,
                                                         const float *__restrict__ rows, uint32_t d, const uint64_t *__restrict__ codes_in,
                                                         const float4 *__restrict__ factors_in, float *__restrict__ base_o,
                                                         uint64_t *__restrict__ codes_o, float4 *__restrict__ factors_o,
                                                         uint32_t *__restrict__ map_ids_o, uint32_t *__restrict__ row_key_o) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < m; j += (uint64_t)gridDim.x * 4) {
        const unsigned long long k64 = keys[j];
        const uint32_t r = (uint32_t)k64, i = src ? src[r] : r;
        const float *in = rows + (uint64_t)i * d;
        float *out = base_o + j * dim;
        for (uint32_t e = lane; e < dim; e += 64) out[e] = e < d ? in[e] : 0.0f;
        for (uint32_t w = lane; w < W; w += 64) codes_o[j * W + w] = codes_in[(uint64_t)i * W + w];
        if (lane == 0) factors_o[j] = factors_in[i], map_ids_o[j] = ids ? ids[r] : id0 + r, row_key_o[j] = (uint32_t)(k64 >> 32);
    }
}

// ---- checks that run before anything is built ----------------------------------------------------------------------------------
// First element at which two arrays differ as bit patterns (NaNs compare too), *first preset to ~0.
__global__ __launch_bounds__(256) void bits_differ_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint64_t count,
                                                          unsigned long long *__restrict__ first) {
    unsigned long long at = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256)
        if (a[i] != b[i]) {
            at = i;  // (a thread's elements ascend: its first difference is its smallest)
            break;
        }
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long t = __shfl_xor(at, o, 64);
        at = t < at ? t : at;
    }
    if ((threadIdx.x & 63) == 0 && at != ~0ull) atomicMin(first, at);
}

// Bit id of `bits` (nbits of them, preset to 0) for every stored id below nbits.
__global__ __launch_bounds__(256) void id_bitmap_kernel(const uint32_t *__restrict__ map_ids, uint64_t n, uint64_t nbits,
                                                        uint32_t *__restrict__ bits) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
        const uint32_t id = map_ids[p];
        if ((uint64_t)id < nbits) atomicOr(bits + (id >> 5), 1u << (id & 31u));
    }
}
// Ids of map_ids that, shifted, have their bit set: counted into *hits (preset to 0).  The caller has checked that no shifted id
// passes 2^32 - 1.
__global__ __launch_bounds__(256) void id_hits_kernel(const uint32_t *__restrict__ map_ids, uint64_t n, uint32_t shift, uint64_t nbits,
                                                      const uint32_t *__restrict__ bits, unsigned long long *__restrict__ hits) {
    unsigned long long h = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
        const uint32_t id = map_ids[p] + shift;
        h += (uint64_t)id < nbits && ((bits[id >> 5] >> (id & 31u)) & 1u) ? 1u : 0u;
    }
    for (int o = 32; o >= 1; o >>= 1) h += __shfl_xor(h, o, 64);
    if ((threadIdx.x & 63) == 0 && h) atomicAdd(hits, h);
}

// ---- the merge -------------------------------------------------------------------------------------------------------------------
// Rows of [b, e) whose key row_key << 32 | (id + shift) is below `key` (the range ascends by that key).
__device__ __forceinline__ uint32_t merge_keys_below(const uint32_t *__restrict__ row_key, const uint32_t *__restrict__ ids, uint32_t shift,
                                                     uint32_t b, uint32_t e, unsigned long long key) {
    const uint32_t kw = (uint32_t)(key >> 32), kid = (uint32_t)key;
    uint32_t lo = b, hi = e;  // first row whose key is not below `key`
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t w = row_key[mid];
        if (w < kw || (w == kw && ids[mid] + shift < kid)) lo = mid + 1;  // (the id is read only where the key words tie)
        else hi = mid;
    }
    return lo - b;
}

// One block per list: the destination-to-source map of the merged list, src_of_dst[dst] = position p of index A (< n_a) or
// n_a + position of index B.  A kept row of A lands at (its rank among the list's kept rows of A) + (keys of B below its key);
// a row of B at (its rank in B's list) + (keys of A below its key): keys never tie (ids are unique across both, which the host
// has checked), so the places are a permutation of the merged list.  B's ids count with `shift_b` added.
// keep_a (nullable, position bitmap, read at positions inside a list only): the rows of A that stay -- rq_remove, rq_compact and
// rq_extract, which have no B (off_b == nullptr: every list of B is empty); rq_add and rq_merge_from keep every row of A.  With
// keep_a the ranks of B would have to count kept rows only: never both.
__global__ __launch_bounds__(256) void merge_lists_kernel(const uint32_t *__restrict__ off_a, const uint32_t *__restrict__ key_a,
                                                          const uint32_t *__restrict__ ids_a, const uint32_t *__restrict__ keep_a,
                                                          const uint32_t *__restrict__ off_b, const uint32_t *__restrict__ key_b,
                                                          const uint32_t *__restrict__ ids_b, uint32_t shift_b,
                                                          const uint32_t *__restrict__ out_off, uint32_t n_a,
                                                          uint32_t *__restrict__ src_of_dst) {
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t s_run;
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ab = off_a[c], ae = off_a[c + 1], out_b = out_off[c];
    const uint32_t bb = off_b ? off_b[c] : 0u, be = off_b ? off_b[c + 1] : 0u;
    if (keep_a) {  // ranks among the kept rows: a running count over 256-row steps (the keys are not read: there is no B)
        if (tid == 0) s_run = 0;
        __syncthreads();
        for (uint32_t t0 = ab; t0 < ae; t0 += 256) {
            const uint32_t p = t0 + tid;
            const bool keep = p < ae && ((keep_a[p >> 5] >> (p & 31u)) & 1u);
            const uint64_t mask = __ballot(keep);
            if (lane == 0) wsum[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t woff = 0, total = 0;
            for (uint32_t w = 0; w < 4; ++w) woff += w < wave ? wsum[w] : 0u, total += wsum[w];
            const uint32_t run = s_run;
            if (keep) src_of_dst[out_b + run + woff + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = p;
            __syncthreads();
            if (tid == 0) s_run = run + total;
            __syncthreads();
        }
        return;
    }
    for (uint32_t p = ab + tid; p < ae; p += 256) {
        const unsigned long long key = ((unsigned long long)key_a[p] << 32) | ids_a[p];
        src_of_dst[out_b + (p - ab) + merge_keys_below(key_b, ids_b, shift_b, bb, be, key)] = p;
    }
    for (uint32_t j = bb + tid; j < be; j += 256) {
        const unsigned long long key = ((unsigned long long)key_b[j] << 32) | (ids_b[j] + shift_b);
        src_of_dst[out_b + (j - bb) + merge_keys_below(key_a, ids_a, 0u, ab, ae, key)] = n_a + j;
    }
}

// ---- the gather ------------------------------------------------------------------------------------------------------------------
// The arrays of one source index, as the gather reads them (row_key nullable: rq_extract of an index without a key cache).
struct MergeSide {
    const float4 *base;
    const uint64_t *codes;
    const float4 *factors;
    const uint32_t *map_ids, *row_key;
};

// The loaded values are made "used" here, after the last load of a step: without it the compiler sinks each load into the
// predicated block of its store, and the rows move one after the other.  (An empty statement: no instruction is emitted.)
__device__ __forceinline__ void merge_pin(float4 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
__device__ __forceinline__ void merge_pin_row(float4 &v, float4 &f, uint64_t &cw, uint32_t &id, uint32_t &kw) {
    merge_pin(v), merge_pin(f);
    asm volatile("" : "+v"(cw), "+v"(id), "+v"(kw));
}

// Every destination row from one of two indexes: raw vector (dim x 4 B), codes (W x 8 B), factors (16 B), id (+ shift_b for rows
// of B) and key word.  Bandwidth-bound, so it is shaped for bytes in flight: a wave is cut into 64 / G sub-groups of G lanes, one
// row each (G = dim / 4 lanes of 16 B, at least 16, at most 64: two rows per wave at dim 128, four at dim 64), and every sub-group
// has R rows in flight.  A step has three phases with nothing consumed inside a phase, so that the compiler has no reason to wait
// between two loads: (1) the R map entries; (2) validity and source addresses; (3) every array's loads of all R rows, pinned
// there by merge_pin_row -- and only then the stores.  The loads of phase 3 are UNCONDITIONAL (a branch around a load makes hipcc drain the queue per row): a lane
// past the row's end reads the row's last piece again, and a row that is not to be moved (past n_out, or a hole) reads row 0 of a
// source that has rows -- n_out > 0 implies n_a + n_b > 0 -- and is not stored; the shift is added at store time.  A row longer
// than the 1 KiB a 64-lane sub-group moves at once takes further steps of R x 1 KiB.  One instruction of a wave stores 64 / G
// ADJACENT destination rows: the wave owns RPW = R * 64 / G consecutive destinations per step and sub-group g takes rows g,
// g + 64 / G, ...  A destination the merge left unset (or a source past both indexes) is counted into *holes and skipped; the
// host then refuses the result.  dim is a multiple of 64: every 16-byte access is aligned.  Vector loads and stores only.
template <int G, int R>
__global__ __launch_bounds__(256) void merge_gather_kernel(const uint32_t *__restrict__ src_of_dst, uint64_t n_out, uint32_t n_a, uint32_t n_b,
                                                           uint32_t dim, uint32_t W, const MergeSide a, const MergeSide b, uint32_t shift_b,
                                                           float4 *__restrict__ base_o, uint64_t *__restrict__ codes_o,
                                                           float4 *__restrict__ factors_o, uint32_t *__restrict__ map_ids_o,
                                                           uint32_t *__restrict__ row_key_o, unsigned int *__restrict__ holes) {
    constexpr uint32_t SUBS = 64 / G, RPW = R * SUBS;
    const uint32_t lane = threadIdx.x & 63, sub = lane / G, l = lane % G;
    const uint32_t V = dim >> 2;  // 16-byte pieces of a raw vector
    const uint32_t lv = l < V ? l : V - 1, lw = l < W ? l : W - 1;  // this lane's piece / code word, or the last one once more
    // without a key cache (rq_extract of an index that has none) the key loads read the ids instead: nothing of them is stored
    const uint32_t *key_a = a.row_key ? a.row_key : a.map_ids, *key_b = b.row_key ? b.row_key : b.map_ids;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t q0 = wave0 * RPW; q0 < n_out; q0 += nwaves * RPW) {
        uint64_t q[R];
        uint32_t s[R], sp[R];
        bool ok[R], fb[R];
        const float4 *vsrc[R];
        float4 v[R], f[R];
        uint64_t cw[R];
        uint32_t id[R], kw[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {  // phase 1: the map entries
            q[r] = q0 + (uint32_t)r * SUBS + sub;
            s[r] = src_of_dst[q[r] < n_out ? q[r] : n_out - 1];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {  // phase 2: where each row comes from
            const bool in = q[r] < n_out;
            bool from_b = s[r] >= n_a;
            uint32_t p = from_b ? s[r] - n_a : s[r];
            ok[r] = in && (!from_b || p < n_b);
            if (in && !ok[r] && l == 0) atomicAdd(holes, 1u);
            if (!ok[r]) from_b = n_a == 0, p = 0;  // a row to read (never stored)
            fb[r] = from_b, sp[r] = p;
            vsrc[r] = (from_b ? b.base : a.base) + (uint64_t)p * V;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {  // phase 3: every array's loads of every row, nothing used
            v[r] = vsrc[r][lv];
            cw[r] = (fb[r] ? b.codes : a.codes)[(uint64_t)sp[r] * W + lw];
            f[r] = (fb[r] ? b.factors : a.factors)[sp[r]];
            id[r] = (fb[r] ? b.map_ids : a.map_ids)[sp[r]];
            kw[r] = (fb[r] ? key_b : key_a)[sp[r]];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) merge_pin_row(v[r], f[r], cw[r], id[r], kw[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!ok[r]) continue;
            if (l < V) base_o[q[r] * V + l] = v[r];
            if (l < W) codes_o[q[r] * W + l] = cw[r];
            if (l == 0) {
                factors_o[q[r]] = f[r], map_ids_o[q[r]] = id[r] + (fb[r] ? shift_b : 0u);
                if (row_key_o) row_key_o[q[r]] = kw[r];
            }
        }
        if (G == 64)  // rows longer than one step of 64 x 16 B: the rest, R rows in flight again
            for (uint32_t e0 = 64; e0 < V; e0 += 64) {
                const uint32_t e = e0 + l, ec = e < V ? e : V - 1;
#pragma unroll
                for (int r = 0; r < R; ++r) v[r] = vsrc[r][ec];
#pragma unroll
                for (int r = 0; r < R; ++r) merge_pin(v[r]);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (ok[r] && e < V) base_o[q[r] * V + e] = v[r];
            }
    }
}

// ---- lazy removal (rq_remove_lazy / rq_compact) ----------------------------------------------------------------------
// The live bitmap of an index (the position bitmap of its owned filter) after marking the rows whose id bit is set in `drop_ids`:
// live' = live & ~drop, drop = drop_ids[map_ids[pos]] (ids >= nbits are not marked).  One wave covers 64 positions, as
// filter_positions_kernel does: the drop bits come from ONE ballot, the two new words leave in two plain 32-bit stores (lanes 0
// and 1).  live_in == nullptr: nothing was dead before -- the old words are "every position below n", so the bits past the last
// position stay clear.  *marked (preset to 0) += the rows that were live and are not any more: one LDS word per block, one
// integer atomic per block that marked anything.  live_out is another buffer than live_in (the host swaps them only when the
// whole call has succeeded); its words past the last wave are preset to zero by the host.
__global__ __launch_bounds__(256) void tombstone_positions_kernel(const uint32_t *__restrict__ map_ids, uint64_t n,
                                                                  const uint32_t *__restrict__ drop_ids, uint64_t nbits,
                                                                  const uint32_t *__restrict__ live_in, uint32_t *__restrict__ live_out,
                                                                  uint64_t nwords, unsigned long long *__restrict__ marked) {
    __shared__ uint32_t s_marked;
    const uint64_t pos = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    if (threadIdx.x == 0) s_marked = 0;
    __syncthreads();
    bool drop = false;
    if (pos < n) {
        const uint32_t id = map_ids[pos];
        drop = (uint64_t)id < nbits && ((drop_ids[id >> 5] >> (id & 31u)) & 1u);
    }
    const uint64_t d = __ballot(drop);
    const uint64_t w = (pos - lane) >> 5;  // first of the wave's two words (nwords is even: w < nwords covers both)
    uint64_t old = __ballot(pos < n);
    if (live_in) old = w < nwords ? ((uint64_t)live_in[w] | ((uint64_t)live_in[w + 1] << 32)) : 0ull;
    const uint64_t now = old & ~d;
    if (lane < 2 && w + lane < nwords) live_out[w + lane] = (uint32_t)(now >> (32 * lane));
    const uint32_t newly = (uint32_t)__popcll(old & d);
    if (lane == 0 && newly) atomicAdd(&s_marked, newly);
    __syncthreads();
    if (threadIdx.x == 0 && s_marked) atomicAdd(marked, (unsigned long long)s_marked);
}

// bits = (bits ^ flip) & live over the nwords words of two position bitmaps of one layout (live nullable: no removal is pending,
// every position counts as live).  flip == 0: a caller's filter made on an index with pending removals admits allowed AND live
// rows, rq_extract keeps requested AND live rows.  flip == ~0: the keep bits of rq_remove, NOT requested AND live; without a
// live bitmap the bits past the last position come out set, and every reader of keep bits looks at positions inside a list only
// (filter_lists_kernel masks each list's first and last word, merge_lists_kernel reads bit p for off[c] <= p < off[c + 1]).
__global__ __launch_bounds__(256) void bitmap_and_live_kernel(uint32_t *__restrict__ bits, uint32_t flip, const uint32_t *__restrict__ live,
                                                              uint64_t nwords) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * 256)
        bits[w] = (bits[w] ^ flip) & (live ? live[w] : ~0u);
}
