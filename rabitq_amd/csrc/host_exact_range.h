// host_exact_range.h -- part of the host side of librabitq_hip.so (one translation unit, see rabitq_hip.hip; after host_exact.h and
// host_range.h).  The exact range search (rq_exact_range_search*, include/rabitq_hip.h): every admitted row with e < r_b, as an
// ordinary rq_range_result.  The exact search's scan with T_q = the radius (kernels_exact.h, the RANGE instantiations), its kept pairs
// in one arena per launch, one exact-distance pass over the arena, then the range path's own tail: hit counts -> offsets
// (range_scan_kernel) -> one allocation of exactly the hits -> the keys in their segments -> range_finish_pieces (host_range.h).
//
// Arena and overflow.  A launch's arena holds `cap` (query, position) records and as many keys (16 bytes a record).  The scan counts
// every kept pair, stored or not; a launch whose count exceeds cap stops there and is run again with exactly the count it learnt (the
// radii are fixed, so the count does not depend on the capacity: one re-run suffices).  When the count's arena would exceed the slot
// budget the group is halved instead, down to one query; a single query's arena is allocated whatever it takes and is RQ_ERR_OOM when
// that fails.  Work memory therefore follows the pairs kept, never nq x the largest answer.
#pragma once

#define RQ_EXRANGE_RECORD_BYTES 16ull   // a record of the arena and its key
#define RQ_EXRANGE_PER_QUERY 1024u      // arena records per query of a launch a call starts from (or the hint, when that is larger)

// a result whose counts are all zero
static rq_status exact_range_empty(uint32_t nq, rq_range_result **out) {
    std::unique_ptr<rq_range_result> res(new rq_range_result());
    res->nq = nq;
    RQC(res->lims.alloc((size_t)nq + 1));
    HIPC(hipMemset(res->lims.p, 0, ((size_t)nq + 1) * 8));
    RQC(res->dist.alloc(0));
    RQC(res->id.alloc(0));
    *out = res.release();
    return RQ_OK;
}

static rq_status exact_range_impl(rq_index *idx, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len, const float *d_radius,
                                  const rq_exact_params_t &prm, rq_range_result **out) {
    rq_exact_stats_t &stats = g_exact_stats;
    const uint64_t admitted = filter ? filter->rows : idx->n;
    if (idx->n == 0 || admitted == 0) return exact_range_empty(nq, out);  // (nothing to scan: a launch of no blocks is not a launch)
    RQC(exact_ensure_attributes());
    std::unique_ptr<rq_range_result> res(new rq_range_result());
    res->nq = nq;
    Workspace *ws = ws_acquire(idx);  // (for its stream, its pinned words and the segmented sort's lists: nothing of a query pass is touched)
    WsLease rel(idx, ws);
    RQC(ws_ensure_stream(*ws));
    hipStream_t st = ws->stream;
    struct Events {
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } g;
    for (hipEvent_t &e : g.ev) HIPC(hipEventCreate(&e));
    auto elapsed = [&](int from, int to, float *acc) -> rq_status {
        float ms = 0.0f;
        HIPC(hipEventElapsedTime(&ms, g.ev[from], g.ev[to]));
        *acc += ms;
        return RQ_OK;
    };
    const bool prefilter = !(prm.flags & RQ_EXACT_NO_PREFILTER) && exact_scan_subtiles(idx->dim) != 0;
    stats.scan_subtiles = prefilter ? exact_scan_subtiles(idx->dim) : 0u;  // (the decision launch_exact_range_scan takes)
    // the records per query earlier calls on this index / filter learnt -- a hint of its own: the exact top-k's slots and the range
    // passes' survivor buffers are sized by theirs; the test hook overrides it
    std::atomic<uint32_t> &cap_hint = filter ? const_cast<rq_filter *>(filter)->exact_range_cap_hint : idx->exact_range_cap_hint;
    const uint64_t per_query = std::min<uint64_t>(admitted, prm.cand_per_query ? prm.cand_per_query : std::max(RQ_EXRANGE_PER_QUERY, cap_hint.load()));
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = std::max<uint64_t>(64ull << 20, std::min<uint64_t>(RQ_EXACT_SLOT_BUDGET, free_b / 3)) / RQ_EXRANGE_RECORD_BYTES;  // records

    DevBuf<float> qscratch, thr, qn2, qsn;
    DevBuf<uint16_t> qbf;
    DevBuf<uint2> rec;
    DevBuf<unsigned long long> keys, count;
    DevBuf<uint32_t> hits, cursor;
    RQC(count.alloc(1));
    unsigned long long *h_word = ws->h_totals + RQ_HT_RANGE_TOTAL;
    std::vector<std::unique_ptr<RangePiece>> pieces;
    for (uint32_t q0 = 0; q0 < nq; q0 += RQ_EXACT_CHUNK) {
        const uint32_t m = std::min<uint32_t>(RQ_EXACT_CHUNK, nq - q0);
        const float *qp = nullptr;  // q': transformed, padded
        RQC(transform_queries(idx, d_q + (uint64_t)q0 * len, m, len, /*want_padded=*/true, qscratch, st, &qp));
        RQC(thr.ensure(m));
        launch_exact_range_thr(d_radius + q0, m, thr.p, st);
        uint32_t limit = RQ_EXACT_QGROUP;  // queries of a launch: halved while a group's arena exceeds the budget
        uint64_t learnt = 0;               // the pairs the group's last launch counted (it overflowed): the next one's capacity
        for (uint32_t g0 = 0; g0 < m;) {
            const uint32_t step = std::min<uint32_t>(m - g0, limit);
            uint64_t cap = learnt ? learnt : per_query * step;
            if (step > 1) cap = std::min(cap, budget);
            cap = std::max<uint64_t>(1, std::min<uint64_t>(cap, admitted * step));
            if (cap > 0xFFFFFFFFull) return fail(RQ_ERR_OOM, "a launch's arena of more than 2^32 records does not fit");  // (step == 1: cap <= n < 2^32)
            ExactArgs a{};
            a.base = idx->view(), a.dim = idx->dim, a.n = (uint32_t)idx->n, a.rows = a.n, a.stride = 1, a.map_ids = idx->map_ids.p;
            a.allow = filter ? filter->pos_bits.p : nullptr;
            a.nq = step, a.nq32 = (step + 31) / 32 * 32;
            RQC(qbf.ensure((uint64_t)a.nq32 * idx->dim));
            RQC(qn2.ensure(a.nq32));
            RQC(qsn.ensure(a.nq32));
            RQC(rec.ensure(cap));
            RQC(keys.ensure(cap));
            a.qpad = qp + (uint64_t)g0 * idx->dim, a.qbf = qbf.p, a.qn2 = qn2.p, a.qsn = qsn.p, a.thr = thr.p + g0;
            a.cap = (uint32_t)cap, a.rec = rec.p, a.rec_count = count.p, a.keys = keys.p;
            // (1) the scan, and what it counted
            HIPC(hipMemsetAsync(count.p, 0, 8, st));
            launch_exact_prep(a, st);
            HIPC(hipEventRecord(g.ev[0], st));
            launch_exact_range_scan(a, prefilter, st);
            HIPC(hipEventRecord(g.ev[1], st));
            HIPC(hipMemcpyAsync(h_word, count.p, 8, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            HIPC(hipGetLastError());
            const uint64_t kept = *h_word;
            RQC(elapsed(0, 1, &stats.ms_scan));
            stats.row_bytes_read += idx->n * idx->row_bytes(), stats.scan_launches += 1;
            if (kept > cap) {  // overflowed: nothing downstream runs on this launch
                stats.reruns += 1;
                if (step > 1 && kept > budget) {
                    limit = std::max(1u, step / 2), learnt = 0;
                    continue;
                }
                learnt = kept;
                if (!prm.cand_per_query) {
                    const uint64_t mean = (kept + step - 1) / step;
                    const uint32_t want = (uint32_t)std::min<uint64_t>(admitted, mean + mean / 8);
                    uint32_t cur = cap_hint.load();
                    while (cur < want && !cap_hint.compare_exchange_weak(cur, want)) {}
                }
                continue;
            }
            const uint32_t records = (uint32_t)kept;
            stats.candidates += kept, stats.exact += kept;
            // (2) exact distances, keys and hit counts; (3) offsets, one allocation of exactly the hits, the keys into their segments
            RQC(hits.ensure(step));
            RQC(cursor.ensure(step));
            HIPC(hipMemsetAsync(hits.p, 0, (size_t)step * 4, st));
            HIPC(hipMemsetAsync(cursor.p, 0, (size_t)step * 4, st));
            std::unique_ptr<RangePiece> p(new RangePiece());
            p->q0 = q0 + g0, p->m = step;
            RQC(p->lims.alloc((size_t)step + 1));
            HIPC(hipEventRecord(g.ev[0], st));
            launch_exact_range_dist(a, hits.p, records, st);
            HIPC(hipEventRecord(g.ev[1], st));
            range_scan_kernel<uint32_t><<<1, 1024, 0, st>>>(hits.p, step, p->lims.p);
            HIPC(hipMemcpyAsync(h_word, p->lims.p + step, 8, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            p->total = *h_word;
            RQC(p->keys.alloc(p->total));
            if (p->total) launch_exact_range_scatter(a, ExactSegments{hits.p, cursor.p, p->lims.p, p->keys.p}, records, st);
            HIPC(hipEventRecord(g.ev[2], st));
            HIPC(hipStreamSynchronize(st));
            HIPC(hipGetLastError());
            RQC(elapsed(0, 1, &stats.ms_exact));
            RQC(elapsed(1, 2, &stats.ms_select));
            pieces.push_back(std::move(p));
            g0 += step, limit = RQ_EXACT_QGROUP, learnt = 0;
        }
    }
    rec.release(), keys.release();  // (the arena is not needed behind the last piece)
    HIPC(hipEventRecord(g.ev[0], st));
    RQC(range_finish_pieces(*ws, pieces, nq, res.get()));
    HIPC(hipEventRecord(g.ev[1], st));
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    RQC(elapsed(0, 1, &stats.ms_select));
    *out = res.release();
    return RQ_OK;
}

static rq_status exact_range_device(const rq_index *idx, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len,
                                    const float *d_radius, const rq_exact_params_t *params, rq_range_result **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    g_exact_stats = rq_exact_stats_t{};
    g_exact_stats.struct_size = sizeof(rq_exact_stats_t);
    if (nq == 0) {  // (as rq_range_search: validated only as far as an empty call can be wrong)
        RQC(ensure_device());
        if (!idx) return fail(RQ_ERR_INVALID, "null argument");
        return exact_range_empty(0, out);
    }
    rq_exact_params_t prm{};
    RQC(exact_validate(idx, !d_q || !d_radius, len, 1u, filter, params, &prm));
    const rq_status s = exact_range_impl(const_cast<rq_index *>(idx), filter, d_q, nq, len, d_radius, prm, out);
    if (s == RQ_ERR_OOM) (void)hipGetLastError();  // (a failed hipMalloc's error is sticky: the caller's next call must not pick it up)
    return s;
}

static rq_status exact_range_host(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                  const float *radius, const rq_exact_params_t *params, rq_range_result **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    RQC(ensure_device());
    if (!idx || (nq && (!queries || !radius))) return fail(RQ_ERR_INVALID, "null argument");
    if (nq) {  // (refused before anything is allocated)
        rq_exact_params_t prm{};
        RQC(exact_validate(idx, false, len, 1u, filter, params, &prm));
    }
    DevBuf<float> dq, dr;
    RQC(dq.upload(queries, (uint64_t)nq * len));
    RQC(dr.upload(radius, nq));
    return exact_range_device(idx, filter, dq.p, nq, len, dr.p, params, out);
}
