// host_range.h -- part of the host side of librabitq_hip.so (one translation unit, see rabitq_hip.hip).  Range search: every
// candidate of the probed lists with rough < r_b and accurate < r_b, per query ascending by (distance, id), as a result object
// the library sizes itself (rq_range_search*, include/rabitq_hip.h).
//
// A call = passes of run_pass in range mode (rotate, coarse ranking, quantisation, ONE scan stage under thr = r_b, the top-k
// path's exact-distance kernels, the hit counts), each followed by its "piece": offsets from the counts, one allocation of
// exactly the pass's hits, the keys written to their segments.  Survivor storage: uniform buffers of the default capacity; the
// queries whose candidates below the radius exceed it are run again -- alone, grouped by need, with the capacity their exact
// count asks for -- which cannot change a set.  The pieces are then united (one piece covering the call in order: adopted as it
// is), the segments sorted by length class, and the keys split into the result's arrays.
#pragma once

// Words of a workspace's pinned block (Workspace::h_totals, 16 words; [0..10] belong to a pass's totals, [15] to its pair split)
// that the range tail reads results back through.  The two uses share words: they are strictly sequential on one workspace
// (a piece is made, and waited for, before anything is sorted), each ending in a stream synchronisation.
enum { RQ_HT_RANGE_BINS = 11 /* 4 words: the three segment lists' lengths, the longest segment */, RQ_HT_RANGE_TOTAL = 13 /* 1 word: a prefix sum's total */ };

struct rq_range_result {
    uint32_t nq = 0;
    uint64_t total = 0;
    DevBuf<unsigned long long> lims;  // nq + 1
    DevBuf<float> dist;               // total
    DevBuf<uint32_t> id;              // total
};

// what one run (a pass, or a re-run of overflowed queries) contributed: run-local query j = query q0 + (rows ? rows[j] : j) of the call
struct RangePiece {
    DevBuf<unsigned long long> keys, lims;  // lims: m + 1 run-local offsets into keys
    DevBuf<uint32_t> rows;
    bool has_rows = false;
    uint32_t q0 = 0, m = 0;
    uint64_t total = 0;
};

struct RangeTimer {  // wall time of the launches behind a pass's profile spans, when profiling is on (adds to ms_sort / ms_total)
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st = nullptr;
    void begin(hipStream_t s) {
        st = s;
        if (!g_profiling.load()) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            a = nullptr;
            return;
        }
        (void)hipEventRecord(a, st);
    }
    void end(rq_profile_t &prof) {  // (the stream has been waited for by the caller once the end event is recorded)
        if (!a || !b) return;
        (void)hipEventRecord(b, st);
        (void)hipEventSynchronize(b);
        float ms = 0;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess) prof.ms_sort += ms, prof.ms_total += ms;
    }
    ~RangeTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// The piece of the run that has just finished on `ws` (its survivors, exact distances and hit counts are still in the workspace).
static rq_status range_make_piece(const rq_index *idx, Workspace &ws, uint32_t m, uint32_t cap, uint32_t q0, const uint32_t *d_rows,
                                  rq_profile_t &prof, std::unique_ptr<RangePiece> *out) {
    std::unique_ptr<RangePiece> p(new RangePiece());
    hipStream_t st = ws.stream;
    RangeTimer tm;
    tm.begin(st);
    p->q0 = q0, p->m = m;
    RQC(p->lims.alloc((size_t)m + 1));
    range_scan_kernel<uint32_t><<<1, 1024, 0, st>>>(ws.range_hits.p, m, p->lims.p);
    unsigned long long *h_total = ws.h_totals + RQ_HT_RANGE_TOTAL;
    HIPC(hipMemcpyAsync(h_total, p->lims.p + m, 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    p->total = *h_total;
    RQC(p->keys.alloc(p->total));  // exactly the run's hits: nothing is guessed, nothing runs twice for a short guess
    if (p->total)
        range_emit_kernel<<<ceil_div(m, 4), 256, 0, st>>>(ws.surv.p, ws.surv_cnt.p, cap, ws.thr.p, m, idx->map_ids.p, p->lims.p, p->keys.p);
    if (d_rows) {
        p->has_rows = true;
        RQC(p->rows.alloc(m));
        HIPC(hipMemcpyAsync(p->rows.p, d_rows, (size_t)m * 4, hipMemcpyDeviceToDevice, st));
    }
    tm.end(prof);
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    *out = std::move(p);
    return RQ_OK;
}

// The queries of a finished pass (`c`: its call, at query q0 of the range call) whose survivors did not fit `cap`: again, grouped by
// need (ascending: a query that admits a whole list does not size the buffers of the ones that missed by a little), every group with
// the capacity its largest exact count asks for.  One re-run always suffices: the count under a fixed radius does not depend on the capacity.
static rq_status range_rerun_overflowed(Workspace &ws, const QueryCall &c, const QueryParams &qp, uint32_t q0, CallTotals &tot,
                                        std::vector<std::unique_ptr<RangePiece>> &pieces) {
    rq_index *idx = c.idx;
    Overflowed ov;
    RQC(read_overflowed(ws, qp.nq, false, false, 0, ov));
    std::vector<uint32_t> &over = ov.rows, &h_need = ov.need;
    std::sort(over.begin(), over.end(), [&](uint32_t a, uint32_t b) { return h_need[a] != h_need[b] ? h_need[a] < h_need[b] : a < b; });
    // A workload most of whose queries admit more than the buffers hold (loose radii everywhere) should not scan twice from now
    // on: when an eighth of the pass overflowed, remember the capacity the overflowed queries needed -- up to RQ_MAX_CAP_HINT, the
    // bound the top-k passes use for theirs, and judged by the largest need BELOW that bound: an outlier that admits a whole list
    // is re-run alone whatever is remembered, and must neither size every later pass nor stop the others from being learnt
    if ((uint64_t)over.size() * 8 >= qp.nq) {
        uint32_t need = 0;
        for (uint32_t b : over)
            if (h_need[b] <= RQ_MAX_CAP_HINT) need = std::max(need, h_need[b]);
        if (need > qp.cap) {
            const uint32_t want = pow2_ceil(need);
            uint32_t cur = idx->range_cap_hint.load();
            while (cur < want && !idx->range_cap_hint.compare_exchange_weak(cur, want)) {}
        }
    }
    const uint64_t budget = 4ull << 30;  // survivor records + run directories of one re-run (48 B per slot), unless one query alone needs more
    const uint64_t max_m = std::max<uint64_t>(1, std::min<uint64_t>(RQ_MAX_NQ_PER_PASS, (1ull << 22) / c.npb()));
    WsLease lease(idx, ws_acquire(idx));  // (pooled: its buffers persist across calls)
    Workspace &rws = *lease.w;
    for (size_t o = 0; o < over.size();) {
        size_t e = o;
        uint32_t ncap = 0;
        while (e < over.size() && e - o < max_m) {
            const uint32_t need = h_need[over[e]];
            if (need > (1u << 31)) return fail(RQ_ERR_OOM, "a query admits more than 2^31 candidates: the result does not fit");
            const uint32_t cap = std::max(2 * RQ_DEFAULT_CAP, pow2_ceil(need));
            if (e > o && (uint64_t)(e - o + 1) * cap * 48ull > budget) break;
            ncap = cap, ++e;
        }
        const uint32_t m = (uint32_t)(e - o);
        tot.prof.retries += m;
        QueryParams rq = pass_params(c, m, ncap, ncap);
        rq.range = true;
        PassResult rr;
        // (the profile takes the re-run in: its launches and times, the rows it scans AGAIN -- scan_candidates is what was scanned,
        // the rough counter what the reference counts -- and the candidates and shadow rejects the first pass could not keep)
        RQC(rerun_rows(rws, c, rq, over.data() + o, &rr, &tot.prof));
        if (rr.overflowed) return fail(RQ_ERR_HIP, "range re-run: survivor count changed between runs");
        tot.precise += rr.precise;
        std::unique_ptr<RangePiece> piece;
        RQC(range_make_piece(idx, rws, m, ncap, q0, rws.retry_rows.p, tot.prof, &piece));
        pieces.push_back(std::move(piece));
        o = e;
    }
    return RQ_OK;
}

// Sort every segment [lims[b], lims[b + 1]) of keys ascending, by length class (kernels_range.h).
static rq_status range_sort_segments(Workspace &ws, unsigned long long *keys, const unsigned long long *lims, uint32_t nq, uint64_t total) {
    hipStream_t st = ws.stream;
    DevBuf<uint32_t> &lists = ws.range_lists;  // (kept with the workspace: no allocation per call)
    DevBuf<unsigned long long> &counters = ws.range_counters;
    RQC(lists.ensure(3 * (size_t)nq));
    RQC(counters.ensure(4));
    HIPC(hipMemsetAsync(counters.p, 0, 32, st));
    range_bin_kernel<<<ceil_div(nq, 256), 256, 0, st>>>(lims, nq, lists.p, counters.p);
    range_sort_wave_kernel<<<ceil_div(nq, 4), 256, 0, st>>>(keys, lims, nq);
    unsigned long long *h = ws.h_totals + RQ_HT_RANGE_BINS;
    HIPC(hipMemcpyAsync(h, counters.p, 32, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    const uint32_t n_small = (uint32_t)h[0], n_mid = (uint32_t)h[1], n_big = (uint32_t)h[2];
    const uint64_t longest = h[3];
    if (n_small) range_sort_block_kernel<256, RQ_RANGE_SMALL_MAX><<<n_small, 256, RQ_RANGE_SMALL_MAX * 8, st>>>(keys, lims, lists.p, n_small);
    if (n_mid) range_sort_block_kernel<1024, RQ_RANGE_TILE><<<n_mid, 1024, RQ_RANGE_TILE * 8, st>>>(keys, lims, lists.p + nq, n_mid);
    if (n_big) {
        // tiles in LDS, then log2(tiles of the longest segment) merge passes between the key array and a second one (an even
        // number of passes: a pass whose runs cover a whole segment copies it, so the result ends in the key array)
        DevBuf<unsigned long long> tmp;
        RQC(tmp.alloc(total));
        const uint32_t *big = lists.p + 2 * (size_t)nq;
        const uint32_t tiles = ceil_div(longest, RQ_RANGE_TILE), blocks = ceil_div(longest, 256);
        for (uint32_t y0 = 0; y0 < n_big; y0 += 32768) {  // (grid.y is bounded)
            const uint32_t ny = std::min(32768u, n_big - y0);
            range_sort_tile_kernel<<<dim3(tiles, ny), 1024, RQ_RANGE_TILE * 8, st>>>(keys, lims, big + y0, ny);
        }
        unsigned long long *src = keys, *dst = tmp.p;
        uint32_t passes = 0;
        for (uint64_t width = RQ_RANGE_TILE; width < longest || (passes & 1u); width *= 2, ++passes) {
            for (uint32_t y0 = 0; y0 < n_big; y0 += 32768) {
                const uint32_t ny = std::min(32768u, n_big - y0);
                range_merge_kernel<<<dim3(blocks, ny), 256, 0, st>>>(src, dst, lims, big + y0, ny, width);
            }
            std::swap(src, dst);
        }
        HIPC(hipStreamSynchronize(st));  // (the second key array is freed here)
    }
    HIPC(hipStreamSynchronize(st));  // (nothing of the sort is in flight when its buffers are reused or freed)
    HIPC(hipGetLastError());
    return RQ_OK;
}

// The tail of a range call: the runs' pieces united into the call's offsets and keys (one piece covering the call in order: adopted
// as it is), the segments sorted, the keys split into the result's arrays.  Also the tail of the exact range search
// (host_exact_range.h), whose pieces are built from keys that are already segmented.
static rq_status range_finish_pieces(Workspace &ws, std::vector<std::unique_ptr<RangePiece>> &pieces, uint32_t nq, rq_range_result *res) {
    hipStream_t st = ws.stream;
    DevBuf<unsigned long long> keys;
    if (pieces.size() == 1 && !pieces[0]->has_rows) {  // one pass, nothing re-run: its offsets and keys are the call's
        res->lims.take(pieces[0]->lims);
        keys.take(pieces[0]->keys);
        res->total = pieces[0]->total;
    } else {
        DevBuf<unsigned long long> counts;
        RQC(counts.alloc(nq));
        RQC(res->lims.alloc((size_t)nq + 1));
        HIPC(hipMemsetAsync(counts.p, 0, (size_t)nq * 8, st));
        for (auto &p : pieces)
            if (p->total) range_piece_counts_kernel<<<ceil_div(p->m, 256), 256, 0, st>>>(p->lims.p, p->has_rows ? p->rows.p : nullptr, p->q0, p->m, counts.p);
        range_scan_kernel<unsigned long long><<<1, 1024, 0, st>>>(counts.p, nq, res->lims.p);
        unsigned long long *h_total = ws.h_totals + RQ_HT_RANGE_TOTAL;
        HIPC(hipMemcpyAsync(h_total, res->lims.p + nq, 8, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        res->total = *h_total;
        RQC(keys.alloc(res->total));
        for (auto &p : pieces)
            if (p->total)
                range_piece_scatter_kernel<<<ceil_div(p->m, 4), 256, 0, st>>>(p->keys.p, p->lims.p, p->has_rows ? p->rows.p : nullptr, p->q0, p->m,
                                                                            res->lims.p, keys.p);
        HIPC(hipStreamSynchronize(st));
        pieces.clear();
    }
    if (res->total) RQC(range_sort_segments(ws, keys.p, res->lims.p, nq, res->total));
    RQC(res->dist.alloc(res->total));
    RQC(res->id.alloc(res->total));
    if (res->total)
        range_split_kernel<<<(uint32_t)std::min<uint64_t>(4096, (res->total + 255) / 256), 256, 0, st>>>(keys.p, res->total, res->dist.p, res->id.p);
    return RQ_OK;  // (the key array is freed here: hipFree waits for the split)
}

static rq_status range_device_impl(rq_index *idx, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len, uint32_t probe,
                                   const float *d_radius, rq_range_result **out) {
    std::unique_ptr<rq_range_result> res(new rq_range_result());
    res->nq = nq;
    CallTotals tot;
    rq_profile_t &prof = tot.prof;
    Workspace *ws = ws_acquire(idx);
    WsLease rel(idx, ws);
    RQC(ws_ensure_stream(*ws));
    hipStream_t st = ws->stream;
    const QueryCall call{idx, filter, len, probe, 1u, false, QueryIO{d_q, nullptr, nullptr, nullptr, nullptr, nullptr, d_radius}};
    std::vector<std::unique_ptr<RangePiece>> pieces;
    for (uint32_t q0 = 0, step_nq = 0; q0 < nq; q0 += step_nq) {
        const QueryCall pc = call.at(q0);
        const uint32_t cap0 = std::max(RQ_DEFAULT_CAP, idx->range_cap_hint.load());
        step_nq = pass_queries(pc, nq - q0, cap0, false);
        QueryParams qp = pass_params(pc, step_nq, cap0, cap0);
        qp.range = true;
        RQC(ws_prepare(idx, *ws, qp));
        PassResult pr;
        RQC(run_pass(*ws, pc, qp, nullptr, &pr, &prof, false));
        tot.rough += pr.rough, tot.precise += pr.precise;
        std::unique_ptr<RangePiece> piece;
        RQC(range_make_piece(idx, *ws, step_nq, cap0, q0, nullptr, prof, &piece));
        pieces.push_back(std::move(piece));
        if (pr.overflowed) RQC(range_rerun_overflowed(*ws, pc, qp, q0, tot, pieces));
    }
    RangeTimer tm;
    tm.begin(st);
    RQC(range_finish_pieces(*ws, pieces, nq, res.get()));
    tm.end(prof);
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    count_call(nq, tot);
    *out = res.release();
    return RQ_OK;
}

static rq_status range_device(rq_index *idx, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len, uint32_t probe,
                              const float *d_radius, rq_range_result **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    if (nq == 0) {  // (as the other query entries: validated only as far as an empty call can be wrong)
        RQC(ensure_device());
        if (!idx) return fail(RQ_ERR_INVALID, "null argument");
    } else {
        RQC(validate_call(idx, !d_q || !d_radius, len, probe, 1u, filter));
    }
    if (nq == 0) {
        std::unique_ptr<rq_range_result> res(new rq_range_result());
        RQC(res->lims.alloc(1));
        HIPC(hipMemset(res->lims.p, 0, 8));
        RQC(res->dist.alloc(0));
        RQC(res->id.alloc(0));
        *out = res.release();
        return RQ_OK;
    }
    const rq_status s = range_device_impl(idx, filter, d_q, nq, len, probe, d_radius, out);
    if (s == RQ_ERR_OOM) (void)hipGetLastError();  // (a failed hipMalloc's error is sticky: the caller's next call must not pick it up)
    return s;
}
