// kernels_attr.h -- device side of the attribute columns (host_attr.h): the scatter and gather of rq_attr_set /
// rq_attr_get, the gather that moves a column with a relayout, the predicate kernel of rq_filter_create_where, and the small passes
// over a filter's position bitmap (combine, id bitmap, id list).  A column is n elements of 4 or 8 bytes in position order.
#pragma once

// ---- columns -------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void attr_fill_kernel(T *__restrict__ col, uint64_t n, T fill) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) col[p] = fill;
}

// rq_attr_set, "the last occurrence wins" without relying on store order: three passes over the m requests.  (1) owner[pos] = 0 for
// every asked position (plain stores of one value: any order gives the same word); (2) owner[pos] = max(owner[pos], i + 1), an integer
// atomic; (3) request i stores its value only where owner[pos] == i + 1.  owner is n words, of which only the asked ones are ever read.
__global__ __launch_bounds__(256) void attr_owner_reset_kernel(const uint32_t *__restrict__ pos, uint64_t m, uint32_t *__restrict__ owner) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = pos[i];
        if (p != RQ_DIR_ABSENT) owner[p] = 0u;
    }
}
__global__ __launch_bounds__(256) void attr_owner_claim_kernel(const uint32_t *__restrict__ pos, uint64_t m, uint32_t *__restrict__ owner) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = pos[i];
        if (p != RQ_DIR_ABSENT) atomicMax(&owner[p], (uint32_t)i + 1u);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void attr_scatter_kernel(const uint32_t *__restrict__ pos, const T *__restrict__ values, uint64_t m,
                                                           const uint32_t *__restrict__ owner, T *__restrict__ col) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = pos[i];
        if (p != RQ_DIR_ABSENT && owner[p] == (uint32_t)i + 1u) col[p] = values[i];
    }
}
template <typename T>
__global__ __launch_bounds__(256) void attr_fetch_kernel(const uint32_t *__restrict__ pos, uint64_t m, const T *__restrict__ col, T fill,
                                                         T *__restrict__ out, uint32_t *__restrict__ found) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = pos[i];
        out[i] = p != RQ_DIR_ABSENT ? col[p] : fill;
        if (found) found[i] = p != RQ_DIR_ABSENT ? 1u : 0u;
    }
}

// A column follows a relayout: dst[q] = the value of the row merge_gather_kernel puts at q, by the same map (src_of_dst[q] < n_a: a
// row of side A; else row src_of_dst[q] - n_a of side B).  col_b == nullptr (the batch of an rq_add, a merge source without the
// column): the fill value.  A destination the merge left unset (the host refuses such a layout) gets the fill value too.  Four
// destinations per thread and step, their map entries and values loaded before any is stored.
template <typename T>
__global__ __launch_bounds__(256) void column_gather_kernel(const uint32_t *__restrict__ src_of_dst, uint64_t n_out, uint32_t n_a, uint32_t n_b,
                                                            const T *__restrict__ col_a, const T *__restrict__ col_b, T fill,
                                                            T *__restrict__ col_o) {
    constexpr int R = 4;
    for (uint64_t q0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * R; q0 < n_out; q0 += (uint64_t)gridDim.x * 256 * R) {
        uint32_t s[R];
        T v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] = q0 + r < n_out ? src_of_dst[q0 + r] : 0xFFFFFFFFu;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            v[r] = fill;
            if (s[r] < n_a) v[r] = col_a[s[r]];
            else if (col_b && s[r] - n_a < n_b) v[r] = col_b[s[r] - n_a];
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (q0 + r < n_out) col_o[q0 + r] = v[r];
    }
}

// ---- the predicate kernel --------------------------------------------------------------------------------------------------------------
// What travels by value in the kernel arguments (1.2 KB): everything in it is the same for every lane, so every branch on a type, an op
// or a token is a scalar branch.
struct WhereSlot {
    const void *col;  // the column's device array
    uint32_t type;    // RQ_ATTR_*
    uint32_t wide;    // 1: 8-byte elements
};
struct WhereTerm {
    uint64_t a, b;       // the constants as the union's u64 image (a 4-byte type: the high word is zero)
    const void *set;     // RQ_WHERE_IN: the sorted set on the device (elements of the column's type; F32: no NaN, -0 stored as +0)
    uint32_t set_count;
    uint32_t top;        //   the largest power of two <= set_count (0: an empty set)
    uint8_t slot, op;
    uint8_t pad[6];
};
struct WhereArgs {
    WhereSlot slots[RQ_WHERE_MAX_COLUMNS];
    WhereTerm terms[RQ_WHERE_MAX_TERMS];
    uint8_t tokens[RQ_WHERE_MAX_TOKENS];
    uint32_t nslots, ntokens;
};
static_assert(sizeof(WhereArgs) < 4096, "the predicate travels in the kernel arguments");

template <typename T>
__device__ __forceinline__ T where_value(uint64_t x) {
    if constexpr (sizeof(T) == 8) return (T)x;
    else if constexpr (std::is_same<T, float>::value) return __uint_as_float((uint32_t)x);
    else return (T)(uint32_t)x;
}
// v == s for some s of the ascending set: the number of elements below v by a search whose trip count depends on the set alone (one
// step per power of two <= count), then one comparison.  F32: -0 is looked up as +0, a NaN is below nothing and equal to nothing.
template <typename T>
__device__ __forceinline__ bool where_in(const WhereTerm &t, T v) {
    const T *s = static_cast<const T *>(t.set);
    if constexpr (std::is_same<T, float>::value) v = v + 0.0f;
    uint32_t lo = 0;
    for (uint32_t half = t.top; half; half >>= 1) {
        const uint32_t mid = lo + half;
        if (mid <= t.set_count && s[mid - 1] < v) lo = mid;
    }
    return lo < t.set_count && s[lo] == v;
}
// One term for the R runs a wave has in flight: stk[r] gets the truth value of x[r] pushed.  The switches on op and type sit outside
// the loops over the runs, so that each loop is a handful of instructions.
// (The per-run values are ext_vector_type vectors, not arrays: a vector is a value, so no pass can turn the constant-index selects on it
// back into an indexed access of private memory.)
template <typename T, int N>
struct WhereVec {
    typedef T type __attribute__((ext_vector_type(N)));
};
#define RQ_WHERE_EACH(expr)                                     \
    _Pragma("unroll") for (int r = 0; r < R; ++r) {             \
        const T v = where_value<T>(x[r]);                       \
        stk[r] = (stk[r] << 1) | ((expr) ? 1u : 0u);            \
    }                                                           \
    break
template <typename T, int R>
__device__ __forceinline__ void where_push_typed(const WhereTerm &t, const typename WhereVec<uint64_t, R>::type &x,
                                                 typename WhereVec<uint32_t, R>::type &stk) {
    const T a = where_value<T>(t.a), b = where_value<T>(t.b);
    switch (t.op) {
    case RQ_WHERE_EQ: RQ_WHERE_EACH(v == a);
    case RQ_WHERE_NE: RQ_WHERE_EACH(v != a);
    case RQ_WHERE_LT: RQ_WHERE_EACH(v < a);
    case RQ_WHERE_LE: RQ_WHERE_EACH(v <= a);
    case RQ_WHERE_GT: RQ_WHERE_EACH(v > a);
    case RQ_WHERE_GE: RQ_WHERE_EACH(v >= a);
    case RQ_WHERE_IN: RQ_WHERE_EACH(where_in<T>(t, v));
    default: RQ_WHERE_EACH(a <= v && v <= b);  // RQ_WHERE_BETWEEN
    }
}
#undef RQ_WHERE_EACH
template <int R>
__device__ __forceinline__ void where_push(const WhereTerm &t, uint32_t type, const typename WhereVec<uint64_t, R>::type &x,
                                           typename WhereVec<uint32_t, R>::type &stk) {
    if (t.op == RQ_WHERE_ANY_BITS || t.op == RQ_WHERE_ALL_BITS) {  // on the u64 image, whatever the integer type
        const uint64_t want = t.op == RQ_WHERE_ALL_BITS ? t.a : 0ull;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t got = x[r] & t.a;
            stk[r] = (stk[r] << 1) | ((t.op == RQ_WHERE_ALL_BITS ? got == want : got != 0) ? 1u : 0u);
        }
        return;
    }
    switch (type) {
    case RQ_ATTR_U32: return where_push_typed<uint32_t, R>(t, x, stk);
    case RQ_ATTR_I32: return where_push_typed<int32_t, R>(t, x, stk);
    case RQ_ATTR_F32: return where_push_typed<float, R>(t, x, stk);
    case RQ_ATTR_U64: return where_push_typed<uint64_t, R>(t, x, stk);
    default: return where_push_typed<int64_t, R>(t, x, stk);
    }
}
// slot `s` of a run's loaded values: a chain of selects on a scalar condition, never an indexed register array
template <int NS>
__device__ __forceinline__ uint32_t where_pick(const typename WhereVec<uint32_t, NS>::type &v, uint32_t s) {
    uint32_t x = v[0];
#pragma unroll
    for (int j = 1; j < NS; ++j) x = s == (uint32_t)j ? v[j] : x;
    return x;
}

// The position bitmap of a predicate, in filter_positions_kernel's layout: bit p of word p >> 5 = the program holds for the row at
// position p.  A wave owns runs of 64 positions, R of them in flight: every slot load of every run of a step is issued before any is
// used -- the loads are unconditional: a lane past the last row reads the last row again, the host rounds the slot count up to NS
// with copies of slot 0 (the same addresses: no further HBM traffic), and a column is read as 32-bit words (WIDE: some column has 8-byte
// elements; then every slot loads two words, at 2p and 2p + 1, a 4-byte column the word at p twice, the second masked away).  The
// boolean stack of a lane is one 32-bit register per run (bit 0 = top), and each run ends in ONE ballot that leaves as two plain 32-bit
// stores by lanes 0 and 1.  The grid covers pos_bitmap_words(n) / 2 runs, so the words past the last position are written, as zero.
// No atomics, no LDS, no scratch.  n > 0, and the program reads at least one column (the host answers an empty program itself).
template <int NS, bool WIDE, int R>
__global__ __launch_bounds__(256) void where_kernel(const WhereArgs a, uint64_t n, uint64_t nruns, uint32_t *__restrict__ pos_bits) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t run0 = wave0 * R; run0 < nruns; run0 += nwaves * R) {
        typename WhereVec<uint32_t, NS>::type lo[R], hi[R];  // (indexed by the unrolled r only)
        typename WhereVec<uint32_t, R>::type stk;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t p = (run0 + r) * 64 + lane, pc = p < n ? p : n - 1;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint32_t *col = static_cast<const uint32_t *>(a.slots[s].col);
                if constexpr (WIDE) {
                    const uint32_t wide = a.slots[s].wide;  // 1: 8-byte elements
                    const uint64_t at = pc << wide;
                    lo[r][s] = col[at], hi[r][s] = col[at + wide];
                } else
                    lo[r][s] = col[pc], hi[r][s] = 0u;
            }
            stk[r] = a.ntokens ? 0u : 1u;
        }
        if constexpr (WIDE) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int s = 0; s < NS; ++s) hi[r][s] &= 0u - a.slots[s].wide;
        }
        for (uint32_t i = 0; i < a.ntokens; ++i) {
            const uint32_t tok = a.tokens[i];
            if (tok < RQ_WHERE_MAX_TERMS) {
                const WhereTerm &t = a.terms[tok];
                const uint32_t type = a.slots[t.slot].type;
                typename WhereVec<uint64_t, R>::type x;
#pragma unroll
                for (int r = 0; r < R; ++r) x[r] = (uint64_t)where_pick<NS>(lo[r], t.slot) | ((uint64_t)where_pick<NS>(hi[r], t.slot) << 32);
                where_push<R>(t, type, x, stk);
            } else if (tok == RQ_WHERE_AND) {
#pragma unroll
                for (int r = 0; r < R; ++r) stk[r] = (stk[r] >> 1) & (stk[r] | ~1u);
            } else if (tok == RQ_WHERE_OR) {
#pragma unroll
                for (int r = 0; r < R; ++r) stk[r] = (stk[r] >> 1) | (stk[r] & 1u);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) stk[r] ^= 1u;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t run = run0 + r, p = run * 64 + lane;
            const uint64_t m = __ballot(p < n && (stk[r] & 1u));
            if (run < nruns && lane < 2) pos_bits[run * 2 + lane] = (uint32_t)(m >> (32 * lane));
        }
    }
}

// ---- passes over a filter's position bitmap ----------------------------------------------------------------------------------------
// out = op(a, b) & live, cut at n: word w keeps the bits of positions below n only (live nullable: every position below n is live).
__global__ __launch_bounds__(256) void filter_combine_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t op,
                                                             const uint32_t *__restrict__ live, uint64_t n, uint64_t nwords,
                                                             uint32_t *__restrict__ out) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * 256) {
        const uint32_t x = a[w], y = b ? b[w] : 0u;
        uint32_t r = op == RQ_FILTER_AND ? (x & y) : op == RQ_FILTER_OR ? (x | y) : op == RQ_FILTER_ANDNOT ? (x & ~y) : ~x;
        const uint64_t p0 = w << 5;
        const uint32_t in = p0 + 32 <= n ? ~0u : (p0 >= n ? 0u : (1u << (uint32_t)(n - p0)) - 1u);
        out[w] = r & in & (live ? live[w] : ~0u);
    }
}
// the id bitmap of the admitted rows (preset to zero): one integer atomic OR per admitted row whose id is below nbits
__global__ __launch_bounds__(256) void filter_id_bits_kernel(const uint32_t *__restrict__ pos_bits, const uint32_t *__restrict__ map_ids,
                                                             uint64_t n, uint64_t nbits, uint32_t *__restrict__ id_bits) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
        if (!((pos_bits[p >> 5] >> (p & 31u)) & 1u)) continue;
        const uint32_t id = map_ids[p];
        if ((uint64_t)id < nbits) atomicOr(&id_bits[id >> 5], 1u << (id & 31u));
    }
}
// The admitted ids in position order, in two passes over blocks of 256 bitmap words (8192 positions): the admitted rows of each block
// (the host turns the counts into offsets), then every word's place by a scan inside the block and its ids, cut at `cap`.
__device__ __forceinline__ uint32_t filter_word_below_n(const uint32_t *pos_bits, uint64_t w, uint64_t nwords, uint64_t n) {
    if (w >= nwords) return 0u;
    const uint64_t p0 = w << 5;
    return p0 + 32 <= n ? pos_bits[w] : (p0 >= n ? 0u : pos_bits[w] & ((1u << (uint32_t)(n - p0)) - 1u));
}
__global__ __launch_bounds__(256) void filter_block_counts_kernel(const uint32_t *__restrict__ pos_bits, uint64_t nwords, uint64_t n,
                                                                  uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    uint32_t c = (uint32_t)__popc(filter_word_below_n(pos_bits, (uint64_t)blockIdx.x * 256 + threadIdx.x, nwords, n));
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt;
}
__global__ __launch_bounds__(256) void filter_emit_ids_kernel(const uint32_t *__restrict__ pos_bits, uint64_t nwords, uint64_t n,
                                                              const uint32_t *__restrict__ map_ids, const unsigned long long *__restrict__ block_off,
                                                              uint64_t cap, uint32_t *__restrict__ out_ids) {
    __shared__ uint32_t s_scan[256];
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t bits = filter_word_below_n(pos_bits, w, nwords, n);
    s_scan[threadIdx.x] = (uint32_t)__popc(bits);
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {  // inclusive scan of the 256 word counts
        const uint32_t add = threadIdx.x >= o ? s_scan[threadIdx.x - o] : 0u;
        __syncthreads();
        s_scan[threadIdx.x] += add;
        __syncthreads();
    }
    uint64_t at = block_off[blockIdx.x] + s_scan[threadIdx.x] - (uint32_t)__popc(bits);
    while (bits) {
        const uint32_t bit = (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        if (at < cap) out_ids[at] = map_ids[(w << 5) + bit];
        ++at;
    }
}
