// kernels_replay.h -- what happens to a stage's survivors after the exact distances (kernels_rerank.h): their ordering,
// the replay of the reference's rankers, and the result writers.  Included by kernels_query.h.
//
//   ordering   the reference visits a query's candidates by ascending (probe slot, position) (src/rabitq.rs:304, :348).  The
//              scans append survivors in runs (RunRec, common.h) that never interleave, so only the run DIRECTORY is ordered.
//              Three strategies, each for a measured regime, and they stay three: a bitonic sort (sort_segment: short
//              directories in LDS, and the last resort in global memory), slot buckets + rank counting (sort_runs_by_slot),
//              and the cell bitmap (order_runs_bitmap: long directories, O(n)).  sort_runs_kernel / sort_runs_mid_kernel
//              choose per query; sort_survivors_kernel orders the heuristic ranker's accepted array.
//   replay     ReplayState (the rankers' state across stages), replay_wave (HeapReRanker / HeuristicReRanker::rank_batch,
//              src/rerank.rs:81-106 / :143-168, by one wave per query), stage_begin (a stage's per-query preamble),
//              stage_finish_kernel (small batches: rerank + order + replay in one block), replay_kernel (large batches).
//   results    init_state_kernel, finalize_heap_kernel / finalize_heuristic_kernel (heap_result_entry: one element of a heap
//              ranker's row), metrics_sum_kernel.
#pragma once

// ------------------------------------------------------------------------------------------------
// Restore the reference's visiting order among a query's survivors: ascending (slot, position)
// (src/rabitq.rs:304 outer loop, :348 inner loop).  One block per query; LDS when it fits.
// ------------------------------------------------------------------------------------------------
#define RQ_SORT_LDS_RECS 2048
template <typename T, uint32_t LDS_RECS = RQ_SORT_LDS_RECS>
__device__ __forceinline__ void sort_segment(T *recs, uint32_t n, const T *src = nullptr /* the unsorted records, when not in place */) {
    __shared__ T lds[LDS_RECS];
    if (!src) src = recs;
    if (n < 2 && src == recs) return;
    auto key = [](const T &r) { return surv_key(r); };
    if (n <= LDS_RECS) {
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lds[i] = src[i];
        __syncthreads();
        bitonic_sort_block(lds, n, key);
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) recs[i] = lds[i];
    } else {
        if (src != recs) {
            for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) recs[i] = src[i];
            __threadfence_block();
        }
        __syncthreads();
        bitonic_sort_block(recs, n, key);  // in global memory (L2), rare
    }
}
// The run directory ordered by (slot, position) without a comparison sort over the whole directory: runs are
// bucketed by probe slot into a second buffer (LDS histogram + scatter: O(n)), then every bucket -- the runs one list
// contributed -- is ordered by position by ONE wave through rank counting (a run's final place is the number of
// smaller positions in its bucket; the bucket's positions are staged through LDS in chunks and compared four at a
// time) and written back to the directory at its final index.  Block-cooperative; needs nslots <= MAX_SLOTS.
#define RQ_BUCKET_CHUNK 1024u
#define RQ_SORT_MID_LDS_WORDS 14336u  // dwords of each of the two dynamic-LDS arrays of order_runs_bitmap: 458 752 cells = 14.7M list positions per query
template <uint32_t MAX_SLOTS>
__device__ __forceinline__ void sort_runs_by_slot(RunRec *__restrict__ dir, RunRec *__restrict__ tmp, uint32_t n, uint32_t nslots) {
    __shared__ uint32_t start[MAX_SLOTS + 1], cursor[MAX_SLOTS];
    __shared__ uint32_t wsum[16];
    __shared__ __attribute__((aligned(16))) uint32_t keys[4][RQ_BUCKET_CHUNK];  // per wave (blocks of 256 threads)
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = nthr >> 6;
    for (uint32_t i = tid; i < nslots; i += nthr) cursor[i] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += nthr) atomicAdd(&cursor[dir[i].slot], 1u);
    __syncthreads();
    // exclusive scan of the bucket sizes: a bucket's start, and its cursor for the scatter
    block_scan_stretch(nslots, wsum, [&](uint32_t i) { return cursor[i]; }, [&](uint32_t i, uint32_t at) { start[i] = at, cursor[i] = at; });
    if (tid == 0) start[nslots] = n;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += nthr) {
        const RunRec r = dir[i];
        tmp[atomicAdd(&cursor[r.slot], 1u)] = r;
    }
    __threadfence_block();
    __syncthreads();  // every record is in tmp (bucketed); dir is free to receive the final order
    for (uint32_t sl = wave; sl < nslots; sl += nwaves) {  // one wave per bucket
        const uint32_t b0 = start[sl], m = start[sl + 1] - b0;
        if (m == 0) continue;
        const RunRec *seg = tmp + b0;
        if (m == 1) {
            if (lane == 0) dir[b0] = seg[0];
            continue;
        }
        const bool one_chunk = m <= RQ_BUCKET_CHUNK;  // the usual case: the bucket's positions are staged once
        auto stage_keys = [&](uint32_t c0, uint32_t cm) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();  // the previous contents have been consumed by every lane
            for (uint32_t t = lane; t < ((cm + 3) & ~3u); t += 64) keys[wave][t] = t < cm ? seg[c0 + t].pos : 0xFFFFFFFFu;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };
        if (one_chunk) stage_keys(0, m);
        for (uint32_t e0 = 0; e0 < m; e0 += 64) {  // 64 runs of the bucket at a time, one per lane
            RunRec mine;
            mine.pos = 0xFFFFFFFFu;
            if (e0 + lane < m) mine = seg[e0 + lane];
            uint32_t rank = 0;
            for (uint32_t c0 = 0; c0 < m; c0 += RQ_BUCKET_CHUNK) {
                const uint32_t cm = m - c0 < RQ_BUCKET_CHUNK ? m - c0 : RQ_BUCKET_CHUNK;
                if (!one_chunk) stage_keys(c0, cm);
                for (uint32_t t = 0; t < cm; t += 4) {
                    const uint4 kq = *reinterpret_cast<const uint4 *>(&keys[wave][t]);  // same address in every lane: broadcast
                    rank += (kq.x < mine.pos ? 1u : 0u) + (kq.y < mine.pos ? 1u : 0u) + (kq.z < mine.pos ? 1u : 0u) +
                            (kq.w < mine.pos ? 1u : 0u);
                }
            }
            if (e0 + lane < m) dir[b0 + rank] = mine;  // positions are unique within a bucket: ranks are a permutation
        }
    }
}

// The same ordering in O(n), for directories whose position span fits an LDS bitmap (the usual case: the final stage of a
// batch on an index with very unequal lists leaves tens of thousands of runs per query, thousands per list, where the rank
// counting above is quadratic).  Within a probe slot (= one list) the runs of one stage sit on distinct 32-position
// cells of the list (a run = one query x one 32- or 64-position sub-tile, common.h), so a run's final index is the number
// of occupied cells before its own: cell = cellbase[slot] + (pos - minpos[slot]) / 32 over a bitmap of the query's cells
// (one bit per 32 list positions of every probed list that contributed), rank = popcount prefix.  Three passes over the
// descriptors (L2), no comparison.  `src` are the unsorted descriptors, `out` receives the order (out != src).  Returns
// false -- nothing written -- when the bitmap does not fit `cap_words` or two runs share a cell (not produced by the
// scans; the caller then falls back to the bucket ranking).
template <uint32_t MAX_SLOTS>
__device__ __forceinline__ bool order_runs_bitmap(const RunRec *src, RunRec *out, uint32_t n, uint32_t nslots, uint32_t *words /* [cap_words] */,
                                                  uint32_t *wpre /* [cap_words] */, uint32_t cap_words) {
    __shared__ uint32_t minpos[MAX_SLOTS], cellbase[MAX_SLOTS];  // cellbase holds the slot's largest position first
    __shared__ uint32_t bsum[17];
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    for (uint32_t i = tid; i < nslots; i += nthr) minpos[i] = 0xFFFFFFFFu, cellbase[i] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += nthr) {
        const RunRec r = src[i];
        atomicMin(&minpos[r.slot], r.pos);
        atomicMax(&cellbase[r.slot], r.pos);
    }
    __syncthreads();
    // exclusive scan of the slots' cell counts: a slot's first cell
    const uint32_t total_cells = block_scan_stretch<true>(
        nslots, bsum, [&](uint32_t i) { return minpos[i] == 0xFFFFFFFFu ? 0u : ((cellbase[i] - minpos[i]) >> 5) + 1u; },
        [&](uint32_t i, uint32_t at) { cellbase[i] = at; });
    const uint32_t nwords = (total_cells + 31) >> 5;
    if (nwords > cap_words) return false;  // (block-uniform)
    for (uint32_t i = tid; i < nwords; i += nthr) words[i] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += nthr) {
        const RunRec r = src[i];
        const uint32_t cell = cellbase[r.slot] + ((r.pos - minpos[r.slot]) >> 5);
        atomicOr(&words[cell >> 5], 1u << (cell & 31u));
    }
    __syncthreads();
    // exclusive popcount prefix over the words (bsum is free again: two barriers since the scan above read it); wpre is scratch,
    // so a directory that fails the test below has still written nothing to `out`
    const uint32_t occupied = block_scan_stretch<true>(
        nwords, bsum, [&](uint32_t i) { return (uint32_t)__popc(words[i]); }, [&](uint32_t i, uint32_t at) { wpre[i] = at; });
    if (occupied != n) return false;  // two runs on one cell (block-uniform)
    __syncthreads();
    for (uint32_t i = tid; i < n; i += nthr) {
        const RunRec r = src[i];
        const uint32_t cell = cellbase[r.slot] + ((r.pos - minpos[r.slot]) >> 5);
        out[wpre[cell >> 5] + (uint32_t)__popc(words[cell >> 5] & ((1u << (cell & 31u)) - 1u))] = r;
    }
    return true;
}

// heuristic ranker's accepted array (src/rerank.rs:170-176): by (Ord32(accurate), arrival)
__global__ __launch_bounds__(256) void sort_survivors_kernel(SurvRec *__restrict__ surv,
                                                             const uint32_t *__restrict__ surv_cnt,
                                                             uint32_t cap) {
    const uint32_t b = blockIdx.x;
    uint32_t n = surv_cnt[b];
    n = n < cap ? n : cap;
    sort_segment(surv + (uint64_t)b * cap, n);
}

// ------------------------------------------------------------------------------------------------
// Ordered replay of the re-rankers over (rough, accurate) pairs: HeapReRanker::rank_batch
// (src/rerank.rs:81-106) and HeuristicReRanker::rank_batch (:143-168), with Rust's
// std BinaryHeap push / pop (sift_up; sift_down_to_bottom + sift_up) on (Ord32, AlwaysEqual) items
// so that evictions among equal keys match.  One wave per query; survivors are taken 64 at a time
// and only lanes with rough < threshold are visited (ballot), the threshold being re-applied after
// every change.  State persists across stages in global memory.
// ------------------------------------------------------------------------------------------------
struct ReplayState {
    float *thr;              // nq
    uint32_t *heap_len;      // nq
    int32_t *heap_key;       // nq * topk
    uint32_t *heap_id;       // nq * topk
    uint32_t *precise;       // nq   (rerank.rs:91 / :153)
    uint32_t *need;          // nq   max survivor count of a stage (sizes re-runs and the learnt capacities)
    uint32_t *ovf;           // nq   1 = a stage dropped records (count > the query's capacity): the query is re-run
    uint32_t *nsurv;         // nq   survivors replayed (= accurate distances computed)
    uint32_t *nshadow;       // nq   of those: rejected by the fp16 shadow rows, f32 row never read
    // heuristic ranker
    float *recent_max;       // nq
    uint32_t *win_count;     // nq
    uint32_t *arr_len;       // nq   accepted so far (may exceed hcap -> overflow)
    SurvRec *arr;            // nq * hcap : {pos = arrival index, slot = biased Ord32(acc), accurate = id bits}
    uint32_t hcap;
};

#define RQ_MAX_TOPK 2048

// One wave replays a query's survivors (run directory `dir`, records `recs`) through the ranker.
// CONTIG: the survivors are recs[0 .. nruns) in visiting order already (no run directory: `dir` is unused and `nruns`
// counts records) -- the small-batch kernel's LDS-resident survivors.
template <bool HEURISTIC, bool REGHEAP = false, bool CONTIG = false>
__device__ __forceinline__ void replay_wave(const SurvRec *__restrict__ recs, const RunRec *__restrict__ dir,
                                            uint32_t nruns, uint32_t topk,
                                            uint32_t b, const ReplayState &st, int32_t *hkey, uint32_t *hid) {
    const uint32_t lane = threadIdx.x & 63;
    // Everything that steers the loops below is the same in every lane; saying so (v_readfirstlane / v_readlane) keeps the
    // loop counters, the heap indices and the branch conditions in scalar registers.  Left to the compiler's divergence
    // analysis, a bound that came out of a memory load or a cross-lane shuffle made the survivor loop "divergent" and with
    // it every value it carries: the sift loops then ran under exec masks with their indices in vector registers.
    nruns = __builtin_amdgcn_readfirstlane(nruns);
    topk = __builtin_amdgcn_readfirstlane(topk);
    float thr = st.thr[b];
    uint32_t precise = 0;
    uint32_t hlen = 0, wcount = 0, alen = 0;
    float recent = 0.0f;
    // REGHEAP (topk < 64: BinaryHeap::push before pop holds topk + 1 elements): the heap lives in one register pair, element i in lane i, read and written with
    // v_readlane / a lane-select at wave-uniform indices: a sift step is a few scalar instructions instead of a chain of
    // dependent LDS round trips (the replay of a stage was bound by exactly that latency)
    int32_t rk = 0;
    uint32_t ri = 0;
    auto HK = [&](uint32_t idx) -> int32_t {
        if constexpr (REGHEAP) return __builtin_amdgcn_readlane(rk, (int)idx);
        else return hkey[idx];
    };
    auto HI = [&](uint32_t idx) -> uint32_t {
        if constexpr (REGHEAP) return (uint32_t)__builtin_amdgcn_readlane((int)ri, (int)idx);
        else return hid[idx];
    };
    auto SETH = [&](uint32_t idx, int32_t k, uint32_t i) {
        if constexpr (REGHEAP) {
            rk = lane == idx ? k : rk;  // (no writelane builtin in this toolchain: a compare and two selects)
            ri = lane == idx ? i : ri;
        } else {
            hkey[idx] = k, hid[idx] = i;
        }
    };
    if constexpr (!HEURISTIC) {
        hlen = __builtin_amdgcn_readfirstlane(st.heap_len[b]);
        if constexpr (REGHEAP) {
            if (lane < hlen) rk = st.heap_key[(uint64_t)b * topk + lane], ri = st.heap_id[(uint64_t)b * topk + lane];
        } else {
            for (uint32_t i = lane; i < hlen; i += 64) {
                hkey[i] = st.heap_key[(uint64_t)b * topk + i];
                hid[i] = st.heap_id[(uint64_t)b * topk + i];
            }
        }
    } else {
        recent = st.recent_max[b];
        wcount = __builtin_amdgcn_readfirstlane(st.win_count[b]);
        alen = __builtin_amdgcn_readfirstlane(st.arr_len[b]);
    }
    // The survivors are replayed in stream order = directory order, then record order inside a run.  The
    // directory is read 64 descriptors at a time; within such a chunk the stream is cut into batches of 64
    // survivors (whatever runs they belong to): lane i finds its (run, offset) by a binary search over
    // the chunk's prefix sums in LDS, so a batch costs one round trip however many short runs it spans,
    // and batch k+1 is in flight while batch k is replayed.
    __shared__ uint32_t s_pref[CONTIG ? 1 : 65], s_base[CONTIG ? 1 : 64];
    for (uint32_t c0 = 0; c0 < (CONTIG ? (nruns ? 1u : 0u) : nruns); c0 += 64) {
        uint32_t total = nruns;
        if constexpr (!CONTIG) {
            uint32_t dbase = 0, dcnt = 0;
            if (c0 + lane < nruns) dbase = dir[c0 + lane].base, dcnt = dir[c0 + lane].cnt;
            const uint32_t incl = wave_incl_scan(dcnt);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // previous chunk's readers are done (one wave)
            s_pref[lane + 1] = incl;
            s_base[lane] = dbase;
            if (lane == 0) s_pref[0] = 0;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        auto fetch = [&](uint32_t off, SurvRec &rec) {
            const uint32_t t = off + lane;
            rec.pos = 0, rec.slot = 0, rec.rough = 0.0f, rec.accurate = 0.0f;
            if (t < total) {
                if constexpr (CONTIG) {
                    rec = recs[t];
                } else {
                    const uint32_t lo = run_of_prefix(s_pref, t);
                    rec = recs[s_base[lo] + (t - s_pref[lo])];
                }
            }
        };
        SurvRec nxt;
        fetch(0, nxt);
        for (uint32_t off = 0; off < total; off += 64) {
            const bool have = off + lane < total;
            const SurvRec r = nxt;
            if (off + 64 < total) fetch(off + 64, nxt);  // wave-uniform
            uint64_t m = __ballot(have && r.rough < thr);  // rerank.rs:84 / :146: candidates the reference reranks
            while (m) {
                // the threshold only moves when a candidate is accepted (rerank.rs:92 / :154), so everything before
                // the next acceptance is counted in one step instead of visited one by one
                const uint64_t acc_m = __ballot(have && r.rough < thr && r.accurate < thr) & m;
                if (acc_m == 0) {
                    precise += (uint32_t)__popcll(m);
                    break;
                }
                const int i = __builtin_ctzll(acc_m);
                const uint64_t upto = (2ull << i) - 1ull;  // lanes 0..i (i = 63 wraps to all ones)
                precise += (uint32_t)__popcll(m & upto);
                m &= ~upto;
                // (lane i's values through v_readlane: i is wave-uniform, a shuffle would go through LDS)
                const float acc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r.accurate), i));
                // the rankers carry the cluster-order POSITION; finalize_* maps it to the original id (rabitq.rs:324)
                const uint32_t id = (uint32_t)__builtin_amdgcn_readlane((int)r.pos, i);
                if constexpr (!HEURISTIC) {
                    // push: append + sift_up(0, old_len)
                    int32_t key = ord32_from_f32(acc);
                    uint32_t idv = id;
                    if constexpr (REGHEAP) {  // every lane holds the same values: keep them (and the control flow) scalar
                        key = (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)key);
                        idv = __builtin_amdgcn_readfirstlane(idv);
                    }
                    uint32_t p = hlen++;
                    while (p > 0) {
                        uint32_t parent = (p - 1) >> 1;
                        int32_t pk = HK(parent);
                        if (key <= pk) break;
                        uint32_t pid = HI(parent);
                        SETH(p, pk, pid);
                        p = parent;
                    }
                    SETH(p, key, idv);
                    if (hlen > topk) {  // pop: last -> root, sift_down_to_bottom(0), sift_up
                        --hlen;
                        int32_t hk = HK(hlen);
                        uint32_t hi = HI(hlen);
                        if (hlen > 0) {
                            const uint32_t end = hlen;
                            uint32_t q = 0, child = 1;
                            while (child + 1 < end) {
                                int32_t kl = HK(child), kr = HK(child + 1);
                                if (kl <= kr) child += 1;
                                int32_t ck = HK(child);
                                uint32_t ci = HI(child);
                                SETH(q, ck, ci);
                                q = child;
                                child = 2 * q + 1;
                            }
                            if (child == end - 1) {
                                int32_t ck = HK(child);
                                uint32_t ci = HI(child);
                                SETH(q, ck, ci);
                                q = child;
                            }
                            while (q > 0) {  // sift_up(0, q) of the hole element
                                uint32_t parent = (q - 1) >> 1;
                                int32_t pk = HK(parent);
                                if (hk <= pk) break;
                                uint32_t pid = HI(parent);
                                SETH(q, pk, pid);
                                q = parent;
                            }
                            SETH(q, hk, hi);
                        }
                    }
                    if (hlen == topk) thr = ord32_to_f32(HK(0));  // rerank.rs:98-100
                } else {
                    if (alen < st.hcap && lane == 0) {
                        SurvRec e;
                        e.pos = alen;
                        e.slot = ord32_biased(acc);
                        e.rough = acc;
                        e.accurate = __builtin_bit_cast(float, id);
                        st.arr[(uint64_t)b * st.hcap + alen] = e;
                    }
                    ++alen;
                    ++wcount;
                    recent = (acc > recent || recent != recent) ? acc : recent;  // f32::max
                    if (wcount >= 12) {                                          // consts.rs:12
                        thr = recent;
                        wcount = 0;
                        recent = -3.402823466e+38f;
                    }
                }
                m &= __ballot(have && r.rough < thr);
            }
        }
    }
    if constexpr (!HEURISTIC) {
        if constexpr (REGHEAP) {
            if (lane < hlen) st.heap_key[(uint64_t)b * topk + lane] = rk, st.heap_id[(uint64_t)b * topk + lane] = ri;
        } else {
            for (uint32_t i = lane; i < hlen; i += 64) {
                st.heap_key[(uint64_t)b * topk + i] = hkey[i];
                st.heap_id[(uint64_t)b * topk + i] = hid[i];
            }
        }
        if (lane == 0) st.heap_len[b] = hlen;
    } else if (lane == 0) {
        st.recent_max[b] = recent;
        st.win_count[b] = wcount;
        st.arr_len[b] = alen;
    }
    if (lane == 0) {
        st.thr[b] = thr;
        st.precise[b] += precise;
    }
}

// A stage's per-query preamble, shared by every kernel that finishes one: the scan's counter (records | runs << 32) against
// the query's capacity.  A query whose records were dropped (count > capacity) takes no part in the stage (n = nruns = 0) and
// is re-run with a larger buffer; need / ovf / nsurv are updated and the counter is reset for the next stage by thread 0.
// BARRIER: the block is more than one wave, so every thread reads the counter before thread 0 resets it (a one-wave block
// reads it in one instruction, ahead of the reset in program order).
struct StageCounts {
    uint32_t n, nruns;  // survivor records and run descriptors to finish
    uint32_t cap;       // the query's capacity
    uint64_t qat;       // its first slot in the survivor buffer / the run directory
    bool overflow;
};
template <bool BARRIER>
__device__ __forceinline__ StageCounts stage_begin(unsigned long long *__restrict__ surv_cnt, const QSeg &seg, uint32_t b, const ReplayState &st) {
    const unsigned long long cnt64 = surv_cnt[b];
    const uint32_t cnt = (uint32_t)cnt64;
    StageCounts c;
    c.cap = seg.capof(b);
    if constexpr (BARRIER) c.qat = seg.at(b);
    c.overflow = cnt > c.cap;
    c.n = c.overflow ? 0 : cnt;
    c.nruns = c.overflow ? 0 : (uint32_t)(cnt64 >> 32);
    if constexpr (BARRIER) __syncthreads();
    if (threadIdx.x == 0) {
        if (cnt > st.need[b]) st.need[b] = cnt;
        if (c.overflow) st.ovf[b] = 1u;
        st.nsurv[b] += c.n;
        surv_cnt[b] = 0;  // ready for the next stage
    }
    // (the one-wave replay fetches its segment start behind the reset, where it did before the preamble was shared: fetched
    // ahead of the counter, replay_kernel's launch measured 2 % longer on the default benchmark, 184 us against 181)
    if constexpr (!BARRIER) c.qat = seg.at(b);
    return c;
}

// One block per query finishes a stage: (A) exact rerank distances of the stage's survivors
// (src/rerank.rs:85-90, 8 lanes = the 8 AVX lanes of src/simd.rs:14-73), (B) sort of the run
// directory into the reference's visiting order, (C) wave 0 replays the ranker.
template <bool HEURISTIC, int KIND>
__device__ __forceinline__ void stage_finish_body(SurvRec *__restrict__ surv, RunRec *__restrict__ runs,
                                                           unsigned long long *__restrict__ surv_cnt, const QSeg &seg,
                                                           const BaseView &base,
                                                           const float *__restrict__ qpad, uint32_t dim, uint32_t topk,
                                                           const ReplayState &st, const uint32_t *__restrict__ probe_cluster,
                                                           uint32_t nprobe, uint32_t presorted) {
    // (+ 1: replay_wave pushes before it pops, so a full heap holds topk + 1 elements for a moment -- at topk == RQ_MAX_TOPK the
    // element one past the arrays landed in whatever LDS follows them)
    __shared__ int32_t hkey[HEURISTIC ? 1 : RQ_MAX_TOPK + 1];
    __shared__ uint32_t hid[HEURISTIC ? 1 : RQ_MAX_TOPK + 1];
    extern __shared__ __attribute__((aligned(16))) float fin_q[];  // dim floats: the padded query
    const uint32_t b = blockIdx.x;
    const StageCounts sc = stage_begin<true>(surv_cnt, seg, b, st);
    const uint32_t n = sc.n, nruns = sc.nruns;
    const uint64_t qat = sc.qat;
    if (n == 0) return;
    SurvRec *recs = surv + qat;
    {  // (A)
        for (uint32_t c = threadIdx.x * 4; c < dim; c += blockDim.x * 4)
            *reinterpret_cast<float4 *>(fin_q + c) = *reinterpret_cast<const float4 *>(qpad + (uint64_t)b * dim + c);
        __syncthreads();
        accurate_rows<KIND>(recs, n, base, fin_q, dim, threadIdx.x >> 1, blockDim.x >> 1, probe_cluster + (uint64_t)b * nprobe);  // 256 or 1024 threads per query
    }
    // (B): up to RQ_SORT_LDS_RECS descriptors in LDS; longer directories were already ordered by sort_runs_mid_kernel
    // when the host launched it ahead of this kernel (presorted != 0), else (rare) bitonic in global memory
    if (nruns <= RQ_SORT_LDS_RECS || !presorted) sort_segment(runs + qat, nruns);
    __syncthreads();                                  // (A)'s stores and (B)'s order visible to wave 0
    if (threadIdx.x < 64)                             // (C)
        replay_wave<HEURISTIC>(recs, runs + qat, nruns, topk, b, st, hkey, hid);
}
// KIND: the row kind of the index, phase (A)'s accurate_rows<KIND> (the launch: with_row_kind).  The body is a function of its own
// because the kernels were compiled that way: written into the kernel, the same statements schedule differently.
template <bool HEURISTIC, int KIND>
__global__ __launch_bounds__(1024) void stage_finish_kernel(SurvRec *__restrict__ surv, RunRec *__restrict__ runs,
                                                           unsigned long long *__restrict__ surv_cnt, const QSeg seg,
                                                           const BaseView base,
                                                           const float *__restrict__ qpad, uint32_t dim, uint32_t topk,
                                                           ReplayState st, const uint32_t *__restrict__ probe_cluster,
                                                           uint32_t nprobe, uint32_t presorted) {
    stage_finish_body<HEURISTIC, KIND>(surv, runs, surv_cnt, seg, base, qpad, dim, topk, st, probe_cluster, nprobe, presorted);
}

// `runs_src`: where the stage's unsorted descriptors are when not in `runs` itself (an arena stage scatters them into the
// second directory buffer, so that the ordering pass is the one that writes the directory); same geometry.
__global__ __launch_bounds__(64) void sort_runs_kernel(RunRec *__restrict__ runs,
                                                        const unsigned long long *__restrict__ surv_cnt,
                                                        const QSeg seg, uint32_t *__restrict__ big_list,
                                                        uint32_t *__restrict__ big_count, uint32_t list_above,
                                                        const RunRec *runs_src) {
    const uint32_t b = blockIdx.x;
    const unsigned long long c = surv_cnt[b];
    if ((uint32_t)c > seg.capof(b)) return;
    // early stages leave a few dozen runs per query, the stages around one list's worth a few hundred (more at dim 64,
    // where the estimates are noisier): 512 descriptors = 8 KiB of LDS per 64-thread block keep them out of global memory
    const uint32_t nruns = (uint32_t)(c >> 32);
    if (list_above != 512u) {  // small-batch path: only list the directories stage_finish_kernel cannot sort in LDS
        if (nruns > list_above && threadIdx.x == 0) big_list[atomicAdd(big_count, 1u)] = b;
        return;
    }
    if (nruns > 512) {  // a loose threshold: handed to sort_runs_mid_kernel (cell bitmap, or slot buckets + rank counting)
        if (threadIdx.x == 0) big_list[atomicAdd(big_count, 1u)] = b;
        return;
    }
    sort_segment<RunRec, 512>(runs + seg.at(b), nruns, runs_src ? runs_src + seg.at(b) : nullptr);
}

// Directories of more than 512 runs, listed by sort_runs_kernel, are ordered by a persistent launch that walks the
// list (it exits at once when the list is empty, the common case): the cell bitmap (order_runs_bitmap, dynamic LDS:
// 2 x lds_words dwords), else slot-bucketing + per-bucket rank counting through the second directory buffer; the last
// block out resets the counter for the next stage.  src_is_tmp: the unsorted descriptors are in runs_tmp.
// The three orderings are kept apart on purpose: each covers a measured regime (bitonic: short directories, or no second
// buffer; buckets: the bitmap does not fit; bitmap: the rest).  lds_words = 0 (option scan_debug bit 2048, a test hook)
// withholds the bitmap, so that the other two are exercised on directories a test can produce.
__global__ __launch_bounds__(256) void sort_runs_mid_kernel(RunRec *__restrict__ runs, RunRec *__restrict__ runs_tmp,
                                                            const unsigned long long *__restrict__ surv_cnt, const QSeg seg,
                                                            const uint32_t *__restrict__ big_list,
                                                            uint32_t *__restrict__ big_count /* [0] entries, [1] blocks done, [2] most entries of a stage */,
                                                            uint32_t nslots, uint32_t src_is_tmp, uint32_t lds_words) {
    extern __shared__ __attribute__((aligned(16))) uint32_t mid_lds[];
    const uint32_t total = big_count[0];
    for (uint32_t i = blockIdx.x; i < total; i += gridDim.x) {
        const uint32_t b = big_list[i], n = (uint32_t)(surv_cnt[b] >> 32);
        RunRec *dir = runs + seg.at(b), *tmp = runs_tmp ? runs_tmp + seg.at(b) : nullptr;
        bool done = false;
        if (nslots <= 1024 && tmp && lds_words) {
            if (src_is_tmp) {
                done = order_runs_bitmap<1024>(tmp, dir, n, nslots, mid_lds, mid_lds + lds_words, lds_words);
            } else {
                done = order_runs_bitmap<1024>(dir, tmp, n, nslots, mid_lds, mid_lds + lds_words, lds_words);
                if (done) {  // back into the directory (the block's own writes: L2)
                    __threadfence_block();
                    __syncthreads();
                    for (uint32_t e = threadIdx.x; e < n; e += blockDim.x) dir[e] = tmp[e];
                }
            }
        }
        if (!done) {
            if (src_is_tmp && tmp) {  // the fall-backs order the directory itself
                __syncthreads();
                for (uint32_t e = threadIdx.x; e < n; e += blockDim.x) dir[e] = tmp[e];
                __threadfence_block();
                __syncthreads();
            }
            if (nslots <= 1024 && tmp) sort_runs_by_slot<1024>(dir, tmp, n, nslots);
            else sort_segment<RunRec, 16>(dir, n);  // more than 1024 probe slots, or no second buffer yet: bitonic sort in global memory
        }
        __syncthreads();
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // every block reads `total` before it counts itself done: the last one out may reset both
        __threadfence();
        if (atomicAdd(big_count + 1, 1u) + 1 == gridDim.x) {
            if (total > big_count[2]) big_count[2] = total;  // for the host: sizes the next pass's launch
            big_count[0] = 0;
            big_count[1] = 0;
        }
    }
}

template <bool HEURISTIC, bool REGHEAP = false>
__global__ __launch_bounds__(64) void replay_kernel(const SurvRec *__restrict__ surv, const RunRec *__restrict__ runs,
                                                    unsigned long long *__restrict__ surv_cnt, const QSeg seg, uint32_t topk,
                                                    ReplayState st, uint32_t dense_cells) {
    extern __shared__ __attribute__((aligned(16))) unsigned char replay_smem[];  // topk * 8 bytes (heap ranker)
    int32_t *hkey = reinterpret_cast<int32_t *>(replay_smem);
    uint32_t *hid = reinterpret_cast<uint32_t *>(replay_smem) + topk;
    const uint32_t b = blockIdx.x;
    const StageCounts sc = stage_begin<false>(surv_cnt, seg, b, st);  // one wave: no block barrier
    if (sc.n == 0) return;
    // dense directory: every cell of the stage is a descriptor (count 0 where nothing survived), already in order
    const uint32_t nruns = dense_cells ? dense_cells : sc.nruns;
    replay_wave<HEURISTIC, REGHEAP>(surv + sc.qat, runs + sc.qat, nruns, topk, b, st, hkey, hid);
}

// ranker state of a fresh query (src/rerank.rs:70-77, :129-139) + per-query counters, one launch
// thr_init (seeded passes): the threshold a query starts with instead of f32::MAX, row_map: pass row -> row of thr_init
__global__ void init_state_kernel(ReplayState st, unsigned long long *__restrict__ surv_cnt, uint32_t nq,
                                  const float *__restrict__ thr_init, const uint32_t *__restrict__ row_map) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nq) return;
    st.thr[b] = thr_init ? thr_init[row_map ? row_map[b] : b] : 3.402823466e+38f;  // f32::MAX
    st.recent_max[b] = -3.402823466e+38f;  // f32::MIN
    st.heap_len[b] = 0, st.precise[b] = 0, st.need[b] = 0, st.ovf[b] = 0, st.nsurv[b] = 0, st.nshadow[b] = 0, st.win_count[b] = 0, st.arr_len[b] = 0;
    surv_cnt[b] = 0;
}

// ------------------------------------------------------------------------------------------------
// Results (src/rerank.rs:108-113 heap Vec order; :170-176 the topk smallest, here sorted).
// ------------------------------------------------------------------------------------------------
// element e of the heap ranker's row sb (the heap's Vec order) into result row ob; the rankers carry positions
__device__ __forceinline__ void heap_result_entry(const ReplayState &st, uint32_t sb, uint32_t ob, uint32_t e, uint32_t topk,
                                                  const uint32_t *__restrict__ map_ids, float *__restrict__ out_dist,
                                                  uint32_t *__restrict__ out_id) {
    out_dist[(uint64_t)ob * topk + e] = ord32_to_f32(st.heap_key[(uint64_t)sb * topk + e]);
    out_id[(uint64_t)ob * topk + e] = map_ids[st.heap_id[(uint64_t)sb * topk + e]];  // position -> original id
}
__global__ void finalize_heap_kernel(const ReplayState st, uint32_t nq, uint32_t topk,
                                     const uint32_t *__restrict__ row_map, const uint32_t *__restrict__ map_ids,
                                     float *__restrict__ out_dist, uint32_t *__restrict__ out_id,
                                     uint32_t *__restrict__ out_n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * topk) return;
    uint32_t b = i / topk, e = i - b * topk;
    uint32_t ob = row_map ? row_map[b] : b;
    uint32_t len = st.heap_len[b];
    if (e < len) heap_result_entry(st, b, ob, e, topk, map_ids, out_dist, out_id);
    if (e == 0) out_n[ob] = len;
}

__global__ void finalize_heuristic_kernel(const ReplayState st, uint32_t nq, uint32_t topk,
                                          const uint32_t *__restrict__ row_map, const uint32_t *__restrict__ map_ids,
                                          float *__restrict__ out_dist, uint32_t *__restrict__ out_id,
                                          uint32_t *__restrict__ out_n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * topk) return;
    uint32_t b = i / topk, e = i - b * topk;
    uint32_t ob = row_map ? row_map[b] : b;
    uint32_t len = st.arr_len[b];
    len = len < st.hcap ? len : st.hcap;
    uint32_t take = len < topk ? len : topk;
    if (e < take) {
        const SurvRec &r = st.arr[(uint64_t)b * st.hcap + e];
        out_dist[(uint64_t)ob * topk + e] = r.rough;
        out_id[(uint64_t)ob * topk + e] = map_ids[__builtin_bit_cast(uint32_t, r.accurate)];  // position -> original id
    }
    if (e == 0) out_n[ob] = take;
}

// per-batch totals for METRICS (src/metrics.rs:44-53): sums of the per-query counters.
// out4[0..5) = {rough, precise (queries without overflow only), #overflowed queries, accurate distances
// computed, max buffer need}
__global__ __launch_bounds__(256) void metrics_sum_kernel(const unsigned long long *__restrict__ rough,
                                                          const uint32_t *__restrict__ precise,
                                                          const uint32_t *__restrict__ need,
                                                          const uint32_t *__restrict__ arr_len,
                                                          const uint32_t *__restrict__ nsurv,
                                                          const uint32_t *__restrict__ nshadow, uint32_t nq,
                                                          const uint32_t *__restrict__ ovf, uint32_t hcap,
                                                          unsigned long long *__restrict__ out4) {
    __shared__ unsigned long long s[6];
    if (threadIdx.x < 6) s[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long r = 0, p = 0, o = 0, a = 0, mx = 0, sh = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nq; i += gridDim.x * 256) {
        const bool ok = !ovf[i] && (!arr_len || arr_len[i] <= hcap);
        r += rough[i];
        p += ok ? precise[i] : 0;
        o += ok ? 0 : 1;
        a += nsurv[i];
        sh += nshadow[i];
        const unsigned long long al = arr_len ? arr_len[i] : 0ull;
        unsigned long long nd = need[i] > al ? (unsigned long long)need[i] : al;
        mx = nd > mx ? nd : mx;
    }
    atomicAdd(&s[0], r);
    atomicAdd(&s[1], p);
    atomicAdd(&s[2], o);
    atomicAdd(&s[3], a);
    atomicMax(&s[4], mx);
    atomicAdd(&s[5], sh);
    __syncthreads();
    if (threadIdx.x < 4) atomicAdd(&out4[threadIdx.x], s[threadIdx.x]);
    if (threadIdx.x == 5) atomicAdd(&out4[5], s[5]);
    if (threadIdx.x == 4) atomicMax(&out4[4], s[4]);
}
