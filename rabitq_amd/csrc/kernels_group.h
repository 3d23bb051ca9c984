// kernels_group.h -- grouped search (host_group.h), wave64: from the result rows of a plain call at topk = fetch to "at most
// group_size rows per value of a column, the topk nearest values", one launch per batch.  Nothing here writes an array of the index.
//
// THE CONTRACT (include/rabitq_hip.h states it; tests/group_model.py is its model).  Query b brings cnt_b <= fetch pairs (dist, id)
// in ARBITRARY order.  A candidate whose id has no live row is absent: skipped and counted.  The others are sorted ascending by the
// 64-bit key ord32_biased(dist) << 32 | id -- the library's (distance, id) order -- and each carries the u64 image of its row's value
// in the column (a 4-byte type zero-extended).  With ord(key) = the number of distinct keys whose first occurrence in that order
// precedes this key's first occurrence, and rank(c) = the number of earlier candidates with c's key, candidate c is kept iff
// ord(key_c) < topk and rank(c) < group_size, and lands in out_id / out_dist[b, ord * group_size + rank]; out_key[b, ord] is the key,
// out_group_n[b, ord] the rows kept of it, out_n[b] the groups.  Every slot that holds no row is written all the same: id 0xFFFFFFFF,
// dist NaN, key 0, group_n 0.  ord and rank are functions of the sorted sequence alone, so the outputs do not depend on the order
// the candidates arrive in or the threads run in: no output value comes from an atomic's return value (the call's four totals are
// integer sums).
//
// Both shapes: (1) the sort, (2) id -> position as directory_lookup_kernel probes (dense array, or the hash table; the live bitmap
// where removals are pending), (3) the column value at that position, (4) first occurrences and ranks, (5) the scatter, (6) the
// padding.  The directory and column loads of all candidates a thread holds are issued before any is used and are UNCONDITIONAL: a
// candidate past cnt or past the directory's top reads entry 0, an absent one position 0 (a column is read as 32-bit words, so both
// element sizes are one code path).  An index without rows is the one exception: nothing is loaded (rows == 0, a scalar branch).
// Vector loads and stores only.
#pragma once

#define RQ_GROUP_PAD_ID 0xFFFFFFFFu
#define RQ_GROUP_WAVE_MAX 64u  // fetch up to here: group_select_wave_kernel

// What travels by value in the kernel arguments: the same for every lane, so every branch on it is a scalar branch.
struct GroupArgs {
    const float *dist;  // the source rows: nq x fetch, cnt[b] valid entries each
    const uint32_t *id;
    const uint32_t *cnt;
    uint32_t nq, fetch, topk, gsize;
    uint64_t rows;  // stored rows of the index (0: every candidate is absent)
    uint64_t top;   // the directory (kernels_directory.h)
    const uint32_t *dense;
    const unsigned long long *slots;
    uint32_t bits;
    uint32_t wide;         // 1: the column has 8-byte elements
    const uint32_t *live;  // nullable
    const uint32_t *col;   // the column, as 32-bit words
    float *out_dist;       // nq x topk x gsize
    uint32_t *out_id;
    unsigned long long *out_key;  // nq x topk
    uint32_t *out_group_n;
    uint32_t *out_n;        // nq
    uint32_t *out_fetched;  // nq, nullable
    unsigned long long *stats;  // {candidates, absent, kept, groups} of the call, preset to 0
};

__device__ __forceinline__ void group_pin(unsigned long long &v) {  // (as fetch_pin: the loads of a phase stay ahead of their first use)
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    v = ((unsigned long long)hi << 32) | lo;
}
// The first probe of an id: the dense entry (in the low word), or the id's home slot.  in: the id is a candidate's and below top.
__device__ __forceinline__ unsigned long long group_probe_first(const GroupArgs &a, uint32_t id, bool in) {
    const uint32_t safe = in ? id : 0u;
    if (a.dense) return a.dense[safe];
    return a.slots[rq_dir_home(safe, a.bits)];
}
// ... and the rest of the walk (directory_lookup_kernel's): the position, or RQ_DIR_ABSENT.
__device__ __forceinline__ uint32_t group_probe_finish(const GroupArgs &a, uint32_t id, bool in, unsigned long long first) {
    if (a.dense) return in ? (uint32_t)first : RQ_DIR_ABSENT;
    const uint32_t mask = (1u << a.bits) - 1u;
    uint32_t s = rq_dir_home(in ? id : 0u, a.bits), p = RQ_DIR_ABSENT;
    unsigned long long slot = first;
    for (uint32_t step = 0; in && step <= mask; ++step) {
        if (slot == RQ_DIR_EMPTY) break;
        if ((uint32_t)(slot >> 32) == id) {
            p = (uint32_t)slot;
            break;
        }
        s = (s + 1u) & mask;
        slot = a.slots[s];
    }
    return p;
}
// What is read at a position: its live word and the column's value (pc = the position, or 0 for none).
__device__ __forceinline__ uint32_t group_live_word(const GroupArgs &a, uint32_t pc) { return a.live ? a.live[pc >> 5] : 0xFFFFFFFFu; }
__device__ __forceinline__ unsigned long long group_column(const GroupArgs &a, uint32_t pc) {
    const uint64_t at = (uint64_t)pc << a.wide;
    const uint32_t lo = a.col[at], hi = a.col[at + a.wide] & (0u - a.wide);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long group_sort_key(float d, uint32_t id) { return ((unsigned long long)ord32_biased(d) << 32) | id; }

// ---- fetch <= 64: one wave per query, four queries per block, one candidate per lane ---------------------------------------------------
// The sort is range_sort_wave_kernel's network over the lanes.  One ballot per distinct key gives every lane of that key the mask of
// its group: the first occurrence is the mask's lowest bit, the rank the bits below the lane, ord the first occurrences below the
// group's.  The output row (at most 64 slots) is staged in LDS -- preset to the padding, the kept rows scattered in -- and leaves
// as coalesced stores.  Every wave of the block meets both barriers (a wave past the last query holds no candidate).
__global__ __launch_bounds__(256) void group_select_wave_kernel(const GroupArgs a) {
    __shared__ unsigned long long s_key[4][64];
    __shared__ float s_dist[4][64];
    __shared__ uint32_t s_id[4][64], s_gn[4][64];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t)blockIdx.x * 4 + w;
    const bool query = b < a.nq;
    const uint64_t row = (query ? b : 0u) * a.fetch;
    uint32_t cnt = query ? a.cnt[b] : 0u;
    cnt = __builtin_amdgcn_readfirstlane(cnt < a.fetch ? cnt : a.fetch);
    const uint32_t src = lane < cnt ? lane : 0u;
    const float d_in = a.dist[row + src];
    const uint32_t id_in = a.id[row + src];
    unsigned long long v = lane < cnt ? group_sort_key(d_in, id_in) : ~0ull;
    for (uint32_t k = 2; k <= 64; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const unsigned long long o = __shfl_xor(v, (int)j, 64);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            v = keep_min ? (o < v ? o : v) : (o > v ? o : v);
        }
    // (a key equal to the padding's is one more copy of the same bits: the first cnt lanes hold the candidates either way)
    const bool cand = lane < cnt;
    const uint32_t id = (uint32_t)v;
    bool present = false;
    unsigned long long ck = 0;
    if (a.rows) {
        const bool in = cand && (uint64_t)id < a.top;
        unsigned long long first = group_probe_first(a, id, in);
        group_pin(first);
        const uint32_t p = group_probe_finish(a, id, in, first);
        const uint32_t pc = p != RQ_DIR_ABSENT ? p : 0u;
        const uint32_t lw = group_live_word(a, pc);
        ck = group_column(a, pc);
        group_pin(ck);
        present = p != RQ_DIR_ABSENT && ((lw >> (pc & 31u)) & 1u);
    }
    const unsigned long long pm = __ballot(present);
    unsigned long long mine = 0, done = 0;
    for (uint32_t j = 0; j < cnt; ++j) {
        if (!(((pm & ~done) >> j) & 1ull)) continue;  // (scalar: absent, or its group is known)
        const uint32_t klo = __builtin_amdgcn_readlane((uint32_t)ck, j), khi = __builtin_amdgcn_readlane((uint32_t)(ck >> 32), j);
        const unsigned long long m = __ballot(present && (uint32_t)ck == klo && (uint32_t)(ck >> 32) == khi);
        if ((m >> lane) & 1ull) mine = m;
        done |= m;
    }
    const uint32_t first_lane = present ? (uint32_t)__builtin_ctzll(mine) : 0u;
    const uint32_t rank = (uint32_t)__popcll(mine & ((1ull << lane) - 1ull)), members = (uint32_t)__popcll(mine);
    const bool head = present && first_lane == lane;
    const unsigned long long heads = __ballot(head);
    const uint32_t ord = (uint32_t)__popcll(heads & ((1ull << first_lane) - 1ull));
    const uint32_t all = (uint32_t)__popcll(heads), ng = all < a.topk ? all : a.topk;
    const bool keep = present && ord < a.topk && rank < a.gsize;
    const unsigned long long km = __ballot(keep);
    s_key[w][lane] = 0ull, s_dist[w][lane] = __builtin_nanf(""), s_id[w][lane] = RQ_GROUP_PAD_ID, s_gn[w][lane] = 0u;
    __syncthreads();
    if (keep) {  // (ord * gsize + rank < topk * gsize <= fetch <= 64)
        const uint32_t slot = ord * a.gsize + rank;
        s_id[w][slot] = id, s_dist[w][slot] = ord32_unbias((uint32_t)(v >> 32));
    }
    if (head && ord < a.topk) s_key[w][ord] = ck, s_gn[w][ord] = members < a.gsize ? members : a.gsize;
    __syncthreads();
    if (!query) return;
    const uint32_t slots = a.topk * a.gsize;
    if (lane < slots) a.out_id[b * slots + lane] = s_id[w][lane], a.out_dist[b * slots + lane] = s_dist[w][lane];
    if (lane < a.topk) a.out_key[b * a.topk + lane] = s_key[w][lane], a.out_group_n[b * a.topk + lane] = s_gn[w][lane];
    if (lane == 0) {
        a.out_n[b] = ng;
        if (a.out_fetched) a.out_fetched[b] = cnt;
        atomicAdd(a.stats + 0, (unsigned long long)cnt);
        atomicAdd(a.stats + 1, (unsigned long long)(cnt - (uint32_t)__popcll(pm)));
        atomicAdd(a.stats + 2, (unsigned long long)__popcll(km));
        atomicAdd(a.stats + 3, (unsigned long long)ng);
    }
}

// ---- fetch <= CAP (256 or 2048): one block of 256 threads per query, the state in LDS ----------------------------------------------
// s_sk: the sort keys, sorted by bitonic_sort_block; index i below is a place in that order.  s_ck[i]: the column key of candidate i.
// First occurrences and ranks come from a SECOND SORT, of the candidates' indices by (absent, column key, index): the present
// candidates of one key become one run, in distance order, so a candidate's rank is its place minus the run's first place (found by
// bisection over the sorted column keys) and the run's first member is the key's first occurrence.  ord is a block-wide exclusive
// scan of the first-occurrence flags in distance order.  No atomic decides a value: the two LDS atomics are integer sums (the
// absent and the kept count).  A thread holds CAP / 256 candidates per phase.
// LDS: CAP x (8 + 8 + 4 x 2) bytes + 72: 6 KB at 256, 48 KB at 2048.
struct GroupRunKey {
    unsigned long long ck;
    uint32_t tag;  // absent << 15 | index
    __device__ __forceinline__ bool operator<(const GroupRunKey &o) const {
        const uint32_t ab = tag >> 15, oab = o.tag >> 15;
        if (ab != oab) return ab < oab;
        if (ck != o.ck) return ck < o.ck;
        return tag < o.tag;
    }
};
template <uint32_t CAP>
__global__ __launch_bounds__(256) void group_select_block_kernel(const GroupArgs a) {
    constexpr uint32_t R = CAP / 256;
    __shared__ unsigned long long s_sk[CAP], s_ck[CAP];
    __shared__ uint16_t s_perm[CAP], s_lb[CAP], s_ord[CAP], s_gn[CAP];
    __shared__ uint32_t s_wsum[16], s_absent, s_kept;
    const uint32_t tid = threadIdx.x;
    const uint64_t b = blockIdx.x, row = b * a.fetch;
    const uint32_t c0 = a.cnt[b], cnt = c0 < a.fetch ? c0 : a.fetch;  // (<= CAP: the host picks the instantiation by fetch)
    for (uint32_t i = tid; i < cnt; i += 256) s_sk[i] = group_sort_key(a.dist[row + i], a.id[row + i]);
    for (uint32_t o = tid; o < a.topk; o += 256) s_gn[o] = 0;
    if (tid == 0) s_absent = 0u, s_kept = 0u;
    __syncthreads();
    bitonic_sort_block(s_sk, cnt, [](unsigned long long k) { return k; });
    // the directory, the live bitmap, the column: R candidates per thread, every load of a phase before its first use
    uint32_t id[R], p[R];
    bool cand[R], in[R];
    unsigned long long raw[R], cv[R];
    uint32_t lw[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t i = tid + r * 256;
        cand[r] = i < cnt;
        id[r] = (uint32_t)s_sk[cand[r] ? i : 0u];
        in[r] = cand[r] && (uint64_t)id[r] < a.top;
        p[r] = RQ_DIR_ABSENT, lw[r] = 0u, cv[r] = 0ull;
    }
    if (a.rows) {
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) raw[r] = group_probe_first(a, id[r], in[r]);
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) group_pin(raw[r]);
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) p[r] = group_probe_finish(a, id[r], in[r], raw[r]);
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t pc = p[r] != RQ_DIR_ABSENT ? p[r] : 0u;
            lw[r] = group_live_word(a, pc);
            cv[r] = group_column(a, pc);
        }
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) group_pin(cv[r]);
    }
    uint32_t n_absent = 0;
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t i = tid + r * 256;
        const bool present = p[r] != RQ_DIR_ABSENT && ((lw[r] >> (p[r] & 31u)) & 1u);
        if (cand[r]) {
            s_ck[i] = cv[r];
            s_perm[i] = (uint16_t)(i | (present ? 0u : 0x8000u));
            n_absent += present ? 0u : 1u;
        }
    }
    if (n_absent) atomicAdd(&s_absent, n_absent);
    __syncthreads();
    const uint32_t mp = cnt - s_absent;  // the present candidates: places [0, mp) of the second sort
    bitonic_sort_block(s_perm, cnt, [&](uint16_t e) { return GroupRunKey{s_ck[e & 0x7FFFu], e}; });
    for (uint32_t j = tid; j < cnt; j += 256) {
        const uint32_t i = s_perm[j] & 0x7FFFu;
        uint32_t lo = j;
        if (j < mp) {  // the first place of this key's run: the lowest place in [0, j] whose column key is not below ck
            const unsigned long long ck = s_ck[i];
            uint32_t hi = j;
            lo = 0;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_ck[s_perm[mid]] < ck) lo = mid + 1;
                else hi = mid;
            }
        }
        s_lb[j] = (uint16_t)lo;
        s_ord[i] = j < mp && lo == j ? 1 : 0;  // in distance order: candidate i is its key's first occurrence
    }
    __syncthreads();
    const uint32_t all = block_scan_stretch<true>(cnt, s_wsum, [&](uint32_t i) { return (uint32_t)s_ord[i]; },
                                                  [&](uint32_t i, uint32_t excl) { s_ord[i] = (uint16_t)excl; });
    __syncthreads();
    const uint32_t ng = all < a.topk ? all : a.topk;
    const uint64_t slots = (uint64_t)a.topk * a.gsize;
    uint32_t n_kept = 0;
    for (uint32_t j = tid; j < mp; j += 256) {
        const uint32_t i = s_perm[j], lb = s_lb[j], ord = s_ord[s_perm[lb]], rank = j - lb;
        if (ord >= a.topk) continue;
        const unsigned long long ck = s_ck[i], sk = s_sk[i];
        if (rank < a.gsize) {
            const uint64_t at = b * slots + (uint64_t)ord * a.gsize + rank;
            a.out_id[at] = (uint32_t)sk, a.out_dist[at] = ord32_unbias((uint32_t)(sk >> 32));
            ++n_kept;
        }
        if (rank == 0) a.out_key[b * a.topk + ord] = ck;
        if (j + 1 == mp || s_ck[s_perm[j + 1]] != ck) s_gn[ord] = (uint16_t)(rank + 1 < a.gsize ? rank + 1 : a.gsize);  // the run's last member
    }
    if (n_kept) atomicAdd(&s_kept, n_kept);
    __syncthreads();
    // the padding: exactly the slots no row was scattered to
    for (uint32_t s = tid; s < slots; s += 256) {
        const uint32_t o = s / a.gsize, r = s - o * a.gsize;
        if (o >= ng || r >= s_gn[o]) a.out_id[b * slots + s] = RQ_GROUP_PAD_ID, a.out_dist[b * slots + s] = __builtin_nanf("");
    }
    for (uint32_t o = tid; o < a.topk; o += 256) {
        a.out_group_n[b * a.topk + o] = o < ng ? s_gn[o] : 0u;
        if (o >= ng) a.out_key[b * a.topk + o] = 0ull;
    }
    if (tid == 0) {
        a.out_n[b] = ng;
        if (a.out_fetched) a.out_fetched[b] = cnt;
        atomicAdd(a.stats + 0, (unsigned long long)cnt);
        atomicAdd(a.stats + 1, (unsigned long long)s_absent);
        atomicAdd(a.stats + 2, (unsigned long long)s_kept);
        atomicAdd(a.stats + 3, (unsigned long long)ng);
    }
}
