// kernels_diverse.h -- diverse search (host_diverse.h), wave64: from the result rows of a plain call at topk = fetch to
// "the topk rows that maximal marginal relevance takes, greedily", one launch per batch.  Nothing here writes an array of the index.
//
// THE CONTRACT (include/rabitq_hip.h states it; tests/diverse_model.py is its model).  Query b brings cnt_b <= fetch pairs (dist, id)
// in ARBITRARY order.  They are sorted ascending by the 64-bit key ord32_biased(dist) << 32 | id; a pair whose id has no live row
// is absent, one of the others whose distance is not finite is skipped, the rest are the candidates c_0 .. c_{m-1} in that order.
// D(c, s) = exact_l2_row (kernels_rerank.h) of the stored row of c against the row of s as rq_fetch_rows widens it.  Step 0 takes
// c_0; after taking s every candidate not yet taken has div = fminf(div, D(c, s)); step t >= 1 takes the one with the smallest
// ord32_biased(score) << 32 | place, score = (lambda * rel) - (mu * div) in three separately rounded f32 operations, a NaN score
// replaced by 0x7FC00000; min(topk, m) steps.  The outputs are in selection order, every slot without a row is written as padding.
// No output value comes from an atomic's return value or from the order threads run in: fminf and the 64-bit minimum are exact and
// commutative (the call's totals are integer sums).
//
// ONE kernel template, three shapes.  <64, 64>: a block is ONE wave, a candidate per lane, the sort is range_sort_wave_kernel's
// network over the lanes and the arg-min needs no LDS.  <256, 256> and <2048, 256>: a block of four waves, the sort is
// bitonic_sort_block, the arg-min crosses the waves through LDS.  MODE (the by-id gather's: FETCH_F32 / _HALF / _BYTE / _COLD) is how
// the index stores its rows: the launch picks it, as accurate_rows' KIND, so that an instantiation carries one row format's loads
// and only FETCH_COLD the bisection over the lists of a tiered index (BaseView::row).  A place below is an index into the SORTED pairs: the
// candidates keep their relative order there, so the smallest (score, index) is the smallest (score, place), and nothing is compacted.
// Per step: (1) the taken row goes into dynamic LDS as dim f32 -- the by-id gather's load and widen routines (kernels_directory.h),
// so the bits are rq_fetch_rows' -- (2) every PAIR of lanes takes candidates pair, pair + T / 2, ...: exact_l2_row issues the loads
// of its row before it consumes the first, (3) div, the score and the block-wide minimum.  Two barriers per step.
// LDS: CAP x (8 + 4 + 4 + 2 + 1) bytes + 48 static (1.3 KB / 4.9 KB / 38.0 KB) and 4 * dim dynamic: with dim <= RQ_DIVERSE_MAX_DIM
// (4096: 16 KB) the largest block holds 54 KB, inside the 64 KB a block gets without an attribute call.
// Vector loads and stores only.
#pragma once

#define RQ_DIVERSE_PAD_ID 0xFFFFFFFFu
#define RQ_DIVERSE_NAN_BITS 0x7FC00000u
#define RQ_DIVERSE_WAVE_MAX 64u    // fetch up to here: the one-wave block
#define RQ_DIVERSE_MAX_DIM 4096u  // the taken row in LDS: 16 KB beside the 38 KB of the 2048-wide state

// What travels by value in the kernel arguments: the same for every lane, so every branch on it is a scalar branch.
struct DiverseArgs {
    const float *dist;  // the source rows: nq x fetch, cnt[b] valid entries each
    const uint32_t *id;
    const uint32_t *cnt;
    uint32_t nq, fetch, topk, dim;
    float lambda, mu;  // mu = 1.0f - lambda, computed once on the host
    GroupArgs dir;     // the directory, the live bitmap and the stored row count (the fields group_probe_* read; nothing else is set)
    BaseView base;
    float *out_dist;  // nq x topk
    uint32_t *out_id;
    float *out_div;
    uint32_t *out_n;            // nq
    uint32_t *out_fetched;      // nq, nullable
    unsigned long long *stats;  // {candidates, absent, skipped, taken, pair_distances} of the call, preset to 0
};

// The row at `pos` into LDS as dim f32: lane piece lp is 16 bytes of the destination, loaded and widened as fetch_gather_kernel does.
template <int MODE, uint32_t T>
__device__ __forceinline__ void diverse_stage_row(const BaseView &base, uint32_t pos, uint32_t dim, uint4 *row_lds) {
    const FetchSrc src = fetch_src<MODE>(base, pos, dim, (uint32_t)RowSpec{base.fmt}.row_bytes(dim));
    for (uint32_t lp = threadIdx.x; lp < dim / 4; lp += T) row_lds[lp] = fetch_widen<MODE>(fetch_load<MODE>(src, lp, dim), src.split, base.fmt);
}
// D(c, s): exact_l2_row's piece for the row kind of MODE (kernels_rerank.h: the one accumulate step and the one fold)
template <int MODE>
__device__ __forceinline__ float diverse_pair_distance(const BaseView &base, uint32_t pos, const float *row_lds, uint32_t dim, uint32_t hf) {
    if constexpr (MODE == FETCH_COLD) return exact_l2_row_f32(base.row(pos, dim), row_lds, dim, hf);
    else if constexpr (MODE == FETCH_BYTE) return exact_l2_row_byte(base.row_at(pos, dim), row_lds, dim, hf);
    else if constexpr (MODE == FETCH_HALF) return exact_l2_row_half(base.row_at(pos, dim), row_lds, dim, hf);
    else return exact_l2_row_f32(RowRef{base.dev + (uint64_t)pos * dim, false, 0u}, row_lds, dim, hf);
}
__device__ __forceinline__ unsigned long long diverse_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o, 64);
        v = other < v ? other : v;
    }
    return v;
}

template <uint32_t CAP, uint32_t T, int MODE>
__global__ __launch_bounds__(T) void diverse_select_kernel(const DiverseArgs a) {
    constexpr uint32_t R = CAP / T, W = T / 64;
    static_assert(CAP % T == 0 && T % 64 == 0 && CAP <= 2048 && W <= 4, "a thread holds R candidates; a place fits 16 bits");
    static_assert(CAP * 19u + 48u + RQ_DIVERSE_MAX_DIM * 4u <= 65536u, "the state and the taken row share 64 KB of LDS");
    extern __shared__ __attribute__((aligned(16))) float s_row[];  // dim floats: the row taken last
    __shared__ unsigned long long s_key[CAP];                      // the sorted pairs: rel in the high word (ord32_biased), the id below
    __shared__ float s_div[CAP];
    __shared__ uint32_t s_pos[CAP];
    __shared__ uint16_t s_sel[CAP];  // the place taken at step t
    __shared__ uint8_t s_out[CAP];   // 1: taken, or never a candidate
    __shared__ unsigned long long s_red[4];
    __shared__ uint32_t s_absent, s_skipped;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t b = blockIdx.x, row = b * a.fetch;
    uint32_t c0 = a.cnt[b];
    const uint32_t cnt = __builtin_amdgcn_readfirstlane(c0 < a.fetch ? c0 : a.fetch);  // (<= CAP: the host picks the instantiation by fetch)
    if (tid == 0) s_absent = 0u, s_skipped = 0u;
    // ---- the sort ----
    if constexpr (CAP == 64 && T == 64) {
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
        s_key[lane] = v;  // (the first cnt lanes hold the pairs, as in group_select_wave_kernel)
        __syncthreads();
    } else {
        for (uint32_t i = tid; i < cnt; i += T) s_key[i] = group_sort_key(a.dist[row + i], a.id[row + i]);
        __syncthreads();
        bitonic_sort_block(s_key, cnt, [](unsigned long long k) { return k; });
    }
    // ---- the directory and the live bitmap: R pairs per thread, every load of a phase before its first use ----
    uint32_t id[R], p[R], lw[R];
    bool cand[R], in[R];
    unsigned long long raw[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t i = tid + r * T;
        cand[r] = i < cnt;
        id[r] = (uint32_t)s_key[cand[r] ? i : 0u];
        in[r] = cand[r] && (uint64_t)id[r] < a.dir.top;
        p[r] = RQ_DIR_ABSENT, lw[r] = 0u;
    }
    if (a.dir.rows) {
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) raw[r] = group_probe_first(a.dir, id[r], in[r]);
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) group_pin(raw[r]);
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) p[r] = group_probe_finish(a.dir, id[r], in[r], raw[r]);
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) lw[r] = group_live_word(a.dir, p[r] != RQ_DIR_ABSENT ? p[r] : 0u);
    }
    uint32_t n_absent = 0, n_skipped = 0;
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t i = tid + r * T;
        const bool present = p[r] != RQ_DIR_ABSENT && ((lw[r] >> (p[r] & 31u)) & 1u);
        if (cand[r]) {
            const uint32_t rel_bits = __builtin_bit_cast(uint32_t, ord32_unbias((uint32_t)(s_key[i] >> 32)));
            const bool finite = (rel_bits & 0x7F800000u) != 0x7F800000u;
            s_pos[i] = present ? p[r] : 0u;
            s_div[i] = __builtin_inff();
            s_out[i] = present && finite ? 0 : 1;
            n_absent += present ? 0u : 1u;
            n_skipped += present && !finite ? 1u : 0u;
        }
    }
    if (n_absent) atomicAdd(&s_absent, n_absent);
    if (n_skipped) atomicAdd(&s_skipped, n_skipped);
    __syncthreads();
    const uint32_t m = cnt - s_absent - s_skipped;  // the candidates
    const uint32_t steps = m < a.topk ? m : a.topk;
    // ---- the selection: `steps` dependent steps ----
    const uint32_t hf = tid & 1u;
    uint32_t last_pos = 0;
    const float lambda = a.lambda, mu = a.mu;
    for (uint32_t t = 0; t < steps; ++t) {
        unsigned long long best = ~0ull;
        if (t == 0) {  // c_0: the first place that holds a candidate
            for (uint32_t i = tid; i < cnt; i += T)
                if (!s_out[i]) best = best < i ? best : (unsigned long long)i;
        } else {
            diverse_stage_row<MODE, T>(a.base, last_pos, a.dim, reinterpret_cast<uint4 *>(s_row));
            __syncthreads();  // (also: the previous step's s_out / s_sel stores, and everybody has read s_red)
            for (uint32_t i = tid >> 1; i < cnt; i += T / 2) {
                if (s_out[i]) continue;  // (a pair of lanes shares its candidate: the branch does not split the pair)
                const float d = diverse_pair_distance<MODE>(a.base, s_pos[i], s_row, a.dim, hf);
                const float div = fminf(s_div[i], d);
                if (hf == 0) s_div[i] = div;
                const float rel = ord32_unbias((uint32_t)(s_key[i] >> 32));
                const float score = __fsub_rn(__fmul_rn(lambda, rel), __fmul_rn(mu, div));
                const uint32_t sb = score != score ? RQ_DIVERSE_NAN_BITS : __builtin_bit_cast(uint32_t, score);
                const unsigned long long key = ((unsigned long long)ord32_biased(__builtin_bit_cast(float, sb)) << 32) | i;
                best = key < best ? key : best;
            }
        }
        best = diverse_wave_min(best);
        if constexpr (W > 1) {
            if (lane == 0) s_red[wave] = best;
            __syncthreads();
#pragma unroll
            for (uint32_t w = 0; w < W; ++w) best = s_red[w] < best ? s_red[w] : best;
        }
        const uint32_t taken = (uint32_t)best;  // (t < steps <= m: a candidate is left, so `best` is a key)
        last_pos = s_pos[taken];
        if (tid == 0) s_sel[t] = (uint16_t)taken, s_out[taken] = 1;  // (read behind the next step's barrier, or the one below)
    }
    __syncthreads();
    // ---- the outputs: in selection order, the padding in the slots behind ----
    const uint64_t out = b * a.topk;
    for (uint32_t s = tid; s < a.topk; s += T) {
        const bool held = s < steps;
        const uint32_t i = held ? s_sel[s] : 0u;
        const unsigned long long k = s_key[i];
        a.out_id[out + s] = held ? (uint32_t)k : RQ_DIVERSE_PAD_ID;
        a.out_dist[out + s] = held ? ord32_unbias((uint32_t)(k >> 32)) : __builtin_bit_cast(float, RQ_DIVERSE_NAN_BITS);
        a.out_div[out + s] = held ? s_div[i] : __builtin_bit_cast(float, RQ_DIVERSE_NAN_BITS);
    }
    if (tid == 0) {
        a.out_n[b] = steps;
        if (a.out_fetched) a.out_fetched[b] = cnt;
        // D is evaluated for every candidate left after each step but the last: (m - 1) + ... + (m - steps + 1)
        const unsigned long long pairs = steps ? (unsigned long long)(steps - 1) * m - (unsigned long long)(steps - 1) * steps / 2 : 0ull;
        atomicAdd(a.stats + 0, (unsigned long long)cnt);
        atomicAdd(a.stats + 1, (unsigned long long)s_absent);
        atomicAdd(a.stats + 2, (unsigned long long)s_skipped);
        atomicAdd(a.stats + 3, (unsigned long long)steps);
        atomicAdd(a.stats + 4, pairs);
    }
}
