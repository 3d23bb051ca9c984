// host_exact_tiered.h -- part of the host side of librabitq_hip.so (one translation unit, see rabitq_hip.hip; after host_exact.h and
// host_exact_range.h, whose phases, overflow protocol, learnt capacities and stats these entries keep).  The exact search and the
// exact range search on every f32-row index: plain, split rows, tiered, tiered + split (rq_exact_search_tiered*,
// rq_exact_range_search_tiered*, include/rabitq_hip.h; kernels: kernels_exact_tiered.h, compiled in inst_exact_tiered.hip).
// What differs from host_exact.h: the pre-filtered scan is one launch per TIER over that tier's physical rows, the two on two streams
// (the host-link reads run under the HBM scan; both append to the same slots), and the exact distances resolve a position through
// BaseView::row.  The sample of the bound and the scan without a pre-filter read no row: they are inst_exact.hip's launches as they are.
#pragma once
#include "kernels_exact_tiered.h"  // (the launch interface only)

static rq_status exact_tiered_ensure_attributes() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] { err = exact_tiered_set_attributes(); });
    if (err != hipSuccess) return fail(RQ_ERR_HIP, std::string("hipFuncSetAttribute(exact_scan_plane_kernel): ") + hipGetErrorString(err));
    return RQ_OK;
}

// exact_validate without its two layout refusals
static rq_status exact_tiered_validate(const rq_index *idx, bool args_null, uint32_t len, uint32_t topk, const rq_filter *filter,
                                       const rq_exact_params_t *params, rq_exact_params_t *prm) {
    RQC(validate_call(idx, args_null, len, 1u, topk, filter));
    *prm = rq_exact_params_t{};
    if (params) {
        if (params->struct_size < 4) return fail(RQ_ERR_INVALID, "struct_size is not set (set it to sizeof(rq_exact_params_t) before the call)");
        memcpy(prm, params, std::min<size_t>(params->struct_size, sizeof *prm));
    }
    if (prm->flags & ~(RQ_EXACT_NO_SEED | RQ_EXACT_NO_PREFILTER)) return fail(RQ_ERR_INVALID, "unknown bit in rq_exact_params_t.flags");
    return RQ_OK;
}
// indexes the plain entries serve as they are: half-precision and byte rows (never tiered or split), and plain f32 rows all in HBM
static bool exact_tiered_forwards(const rq_index *idx) {
    return idx->rows.typed() || (!idx->base_host && idx->n_dev >= idx->n && !idx->split_rows);
}

// The pre-filtered scan of every tier: the HBM array on `st`, the host array on a stream of its own, joined before anything reads the
// counts.  Owns the second stream, the join events and the per-tier tile tables of one call.
struct TierScan {
    const rq_index *idx;
    hipStream_t st2 = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    DevBuf<uint32_t> tiles[2];
    uint32_t rt = 0;
    ~TierScan() {
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        if (st2) (void)hipStreamDestroy(st2);
    }
    bool tiered() const { return idx->base_host != nullptr; }
    uint64_t tier_rows(int tier) const { return !tiered() ? (tier ? 0 : idx->n) : tier ? idx->n - idx->n_dev : idx->n_dev; }
    TierView view(int tier) const { return TierView{tiered() ? idx->list_tier.p : nullptr, idx->k, (uint32_t)tier, (uint32_t)tier_rows(tier)}; }
    rq_status prepare(hipStream_t st) {
        rt = exact_scan_subtiles(idx->dim);
        if (!tiered() || rt == 0) return RQ_OK;
        HIPC(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&join, hipEventDisableTiming));
        for (int tier = 0; tier < 2; ++tier) {
            const uint32_t n_tiles = (uint32_t)((tier_rows(tier) + 32 * rt - 1) / (32 * rt));
            RQC(tiles[tier].alloc(std::max<uint32_t>(n_tiles, 1u)));
            launch_tier_tile_list(view(tier), 32 * rt, n_tiles, tiles[tier].p, st);
        }
        return RQ_OK;
    }
    // bytes of raw rows one scan reads: the first plane of a split row, the whole of a plain one
    uint64_t bytes() const { return idx->n * (uint64_t)idx->dim * (idx->split_rows ? 2u : 4u); }
    rq_status launch(const ExactArgs &a, bool range, hipStream_t st) {
        TierScanArgs ta{a, idx->base.p, view(0), tiered() ? tiles[0].p : nullptr};
        if (!tiered()) {
            launch_exact_scan_tier(ta, idx->split_rows, range, st);
            return RQ_OK;
        }
        HIPC(hipEventRecord(fork, st));
        HIPC(hipStreamWaitEvent(st2, fork, 0));
        TierScanArgs th{a, idx->base_host_dev, view(1), tiles[1].p};
        launch_exact_scan_tier(th, idx->split_rows, range, st2);
        HIPC(hipEventRecord(join, st2));
        launch_exact_scan_tier(ta, idx->split_rows, range, st);
        HIPC(hipStreamWaitEvent(st, join, 0));
        return RQ_OK;
    }
};

static rq_status exact_tiered_search_device(const rq_index *idx, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len, uint32_t topk,
                                            const rq_exact_params_t *params, float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n) {
    if (!idx || !d_out_dist || !d_out_id || !d_out_n || (nq && !d_q)) return fail(RQ_ERR_INVALID, "null argument");
    g_exact_stats = rq_exact_stats_t{};
    g_exact_stats.struct_size = sizeof(rq_exact_stats_t);
    if (nq == 0) return RQ_OK;
    rq_exact_params_t prm{};
    RQC(exact_tiered_validate(idx, false, len, topk, filter, params, &prm));
    if (exact_tiered_forwards(idx)) return exact_search_device(idx, filter, d_q, nq, len, topk, params, d_out_dist, d_out_id, d_out_n);
    RQC(exact_ensure_attributes());
    RQC(exact_tiered_ensure_attributes());
    hipStream_t st = nullptr;
    HIPC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct Guard {
        hipStream_t s;
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        ~Guard() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
            (void)hipStreamDestroy(s);
        }
    } g{st};
    for (hipEvent_t &e : g.ev) HIPC(hipEventCreate(&e));
    if (idx->n == 0) {
        HIPC(hipMemsetAsync(d_out_n, 0, (size_t)nq * 4, st));
        HIPC(hipStreamSynchronize(st));
        return RQ_OK;
    }
    TierScan ts{idx};
    RQC(ts.prepare(st));
    const bool prefilter = !(prm.flags & RQ_EXACT_NO_PREFILTER) && ts.rt != 0;
    const bool no_seed = (prm.flags & RQ_EXACT_NO_SEED) || !prefilter;
    const uint64_t admitted = filter ? filter->rows : idx->n;
    uint32_t sample_rows = 0;
    const uint32_t stride = exact_sample_stride(idx->n, admitted, topk, prm.seed_probe, &sample_rows);
    const uint32_t cap_max = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(admitted, idx->n));
    std::atomic<uint32_t> &cap_hint = filter ? const_cast<rq_filter *>(filter)->exact_cap_hint : const_cast<rq_index *>(idx)->exact_cap_hint;
    uint32_t cap = std::min<uint32_t>(cap_max, prm.cand_per_query ? prm.cand_per_query : std::max<uint32_t>(std::max<uint32_t>(4 * topk, 1024u), cap_hint.load()));
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const uint64_t slot_budget = std::max<uint64_t>(64ull << 20, std::min<uint64_t>(RQ_EXACT_SLOT_BUDGET, free_b / 3));
    rq_exact_stats_t &stats = g_exact_stats;
    stats.seed_probe = no_seed ? 0u : sample_rows;
    stats.scan_subtiles = prefilter ? ts.rt : 0u;

    DevBuf<float> seed_dist, qscratch, thr, qn2, qsn;
    DevBuf<uint32_t> seed_id, seed_n, cand;
    DevBuf<unsigned int> cnt, unfilled;
    DevBuf<uint16_t> qbf;
    DevBuf<unsigned long long> keys;
    std::vector<unsigned int> h_cnt;
    RQC(unfilled.alloc(1));
    HIPC(hipMemsetAsync(unfilled.p, 0, 4, st));
    // scan (+ capacity check), exact distances and selection of one launch, as host_exact.h runs them
    auto run = [&](ExactArgs &a, bool pre, bool counted, bool *over, uint64_t *total) -> rq_status {
        RQC(cnt.ensure(a.nq));
        RQC(cand.ensure((uint64_t)a.nq * a.cap));
        RQC(keys.ensure((uint64_t)a.nq * a.cap));
        a.cand = cand.p, a.cnt = cnt.p, a.keys = keys.p;
        HIPC(hipMemsetAsync(cnt.p, 0, (size_t)a.nq * 4, st));
        HIPC(hipEventRecord(g.ev[0], st));
        if (pre) RQC(ts.launch(a, false, st));
        else launch_exact_scan(a, false, st);  // (positions and filter bits only: no row is read)
        HIPC(hipEventRecord(g.ev[1], st));
        h_cnt.resize(a.nq);
        HIPC(hipMemcpyAsync(h_cnt.data(), cnt.p, (size_t)a.nq * 4, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        HIPC(hipGetLastError());
        float ms = 0.0f;
        HIPC(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
        if (counted) stats.ms_scan += ms, stats.row_bytes_read += pre ? ts.bytes() : 0ull, stats.scan_launches += 1;
        else stats.ms_seed += ms;
        unsigned int most = 0;
        *total = 0;
        for (unsigned int c : h_cnt) *total += c, most = std::max(most, c);
        *over = most > a.cap;
        if (*over) {
            cap = (uint32_t)std::min<uint64_t>(cap_max, ((uint64_t)most + most / 8 + 255) / 256 * 256);
            return RQ_OK;
        }
        HIPC(hipEventRecord(g.ev[0], st));
        launch_exact_dist_tiered(a, st);
        HIPC(hipEventRecord(g.ev[1], st));
        launch_exact_select(a, st);
        HIPC(hipEventRecord(g.ev[2], st));
        HIPC(hipStreamSynchronize(st));
        HIPC(hipGetLastError());
        float ms2 = 0.0f;
        HIPC(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
        HIPC(hipEventElapsedTime(&ms2, g.ev[1], g.ev[2]));
        if (counted) stats.ms_exact += ms, stats.ms_select += ms2;
        else stats.ms_seed += ms + ms2;
        return RQ_OK;
    };
    uint32_t bound_g0 = 0xFFFFFFFFu, bound_step = 0;
    for (uint32_t q0 = 0; q0 < nq; q0 += RQ_EXACT_CHUNK) {
        const uint32_t m = std::min<uint32_t>(RQ_EXACT_CHUNK, nq - q0);
        bound_g0 = 0xFFFFFFFFu;
        const float *qp = nullptr;
        RQC(transform_queries(idx, d_q + (uint64_t)q0 * len, m, len, /*want_padded=*/true, qscratch, st, &qp));
        RQC(thr.ensure(m));
        for (uint32_t g0 = 0; g0 < m;) {
            const uint32_t slots = std::max(cap, no_seed ? 1u : sample_rows);
            const uint32_t step = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(m - g0, RQ_EXACT_QGROUP),
                                                               std::max<uint64_t>(1, slot_budget / (RQ_EXACT_SLOT_BYTES * slots)));
            ExactArgs a{};
            a.base = idx->view(), a.dim = idx->dim, a.n = (uint32_t)idx->n, a.map_ids = idx->map_ids.p;
            a.allow = filter ? filter->pos_bits.p : nullptr;
            a.nq = step, a.nq32 = (step + 31) / 32 * 32, a.topk = topk;
            RQC(qbf.ensure((uint64_t)a.nq32 * idx->dim));
            RQC(qn2.ensure(a.nq32));
            RQC(qsn.ensure(a.nq32));
            a.qpad = qp + (uint64_t)g0 * idx->dim, a.qbf = qbf.p, a.qn2 = qn2.p, a.qsn = qsn.p, a.thr = thr.p + g0;
            bool over = false;
            uint64_t total = 0;
            const bool have_bound = bound_g0 == g0 && bound_step == step;
            if (!no_seed && !have_bound) {  // the sample: positions p stride, resolved through BaseView::row by the exact distances
                RQC(seed_dist.ensure((uint64_t)step * topk));
                RQC(seed_id.ensure((uint64_t)step * topk));
                RQC(seed_n.ensure(step));
                launch_exact_thr(nullptr, nullptr, step, topk, a.thr, nullptr, st);
                ExactArgs sa = a;
                sa.stride = stride, sa.rows = sample_rows, sa.cap = sample_rows;
                sa.out_dist = seed_dist.p, sa.out_id = seed_id.p, sa.out_n = seed_n.p;
                RQC(run(sa, false, false, &over, &total));
                stats.exact += total;
            }
            if (!have_bound) launch_exact_thr(no_seed ? nullptr : seed_dist.p, seed_n.p, step, topk, a.thr, unfilled.p, st);
            bound_g0 = g0, bound_step = step;
            launch_exact_prep(a, st);
            a.stride = 1, a.rows = a.n, a.cap = cap;
            a.out_dist = d_out_dist + (uint64_t)(q0 + g0) * topk, a.out_id = d_out_id + (uint64_t)(q0 + g0) * topk, a.out_n = d_out_n + q0 + g0;
            RQC(run(a, prefilter, true, &over, &total));
            if (over) {
                stats.reruns += 1;
                if (!prm.cand_per_query) {
                    uint32_t cur = cap_hint.load();
                    while (cur < cap && !cap_hint.compare_exchange_weak(cur, cap)) {}
                }
                continue;
            }
            stats.candidates += total, stats.exact += total;
            g0 += step;
        }
    }
    HIPC(hipMemcpy(&stats.seed_unfilled, unfilled.p, 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

static rq_status exact_tiered_search_host(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len, uint32_t topk,
                                          const rq_exact_params_t *params, float *out_dist, uint32_t *out_id, uint32_t *out_n) {
    if (!idx || !out_dist || !out_id || !out_n || (nq && !queries)) return fail(RQ_ERR_INVALID, "null argument");
    if (nq == 0) {
        g_exact_stats = rq_exact_stats_t{};
        g_exact_stats.struct_size = sizeof(rq_exact_stats_t);
        return RQ_OK;
    }
    rq_exact_params_t prm{};
    RQC(exact_tiered_validate(idx, false, len, topk, filter, params, &prm));
    const uint64_t cells = (uint64_t)nq * topk;
    DevBuf<float> dq, dd;
    DevBuf<uint32_t> di, dn;
    RQC(dq.upload(queries, (uint64_t)nq * len));
    RQC(dd.upload(out_dist, cells));  // the caller's arrays travel both ways: slots past out_n stay as they were
    RQC(di.upload(out_id, cells));
    RQC(dn.alloc(nq));
    RQC(exact_tiered_search_device(idx, filter, dq.p, nq, len, topk, params, dd.p, di.p, dn.p));
    HIPC(hipMemcpy(out_dist, dd.p, cells * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_id, di.p, cells * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_n, dn.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

// ---- the range form: exact_range_impl (host_exact_range.h) with the tiers' scan and the position-resolving distances ----
static rq_status exact_tiered_range_impl(rq_index *idx, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len, const float *d_radius,
                                         const rq_exact_params_t &prm, rq_range_result **out) {
    rq_exact_stats_t &stats = g_exact_stats;
    const uint64_t admitted = filter ? filter->rows : idx->n;
    if (idx->n == 0 || admitted == 0) return exact_range_empty(nq, out);
    RQC(exact_ensure_attributes());
    RQC(exact_tiered_ensure_attributes());
    std::unique_ptr<rq_range_result> res(new rq_range_result());
    res->nq = nq;
    Workspace *ws = ws_acquire(idx);
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
    TierScan ts{idx};
    RQC(ts.prepare(st));
    const bool prefilter = !(prm.flags & RQ_EXACT_NO_PREFILTER) && ts.rt != 0;
    stats.scan_subtiles = prefilter ? ts.rt : 0u;
    std::atomic<uint32_t> &cap_hint = filter ? const_cast<rq_filter *>(filter)->exact_range_cap_hint : idx->exact_range_cap_hint;
    const uint64_t per_query = std::min<uint64_t>(admitted, prm.cand_per_query ? prm.cand_per_query : std::max(RQ_EXRANGE_PER_QUERY, cap_hint.load()));
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = std::max<uint64_t>(64ull << 20, std::min<uint64_t>(RQ_EXACT_SLOT_BUDGET, free_b / 3)) / RQ_EXRANGE_RECORD_BYTES;

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
        const float *qp = nullptr;
        RQC(transform_queries(idx, d_q + (uint64_t)q0 * len, m, len, /*want_padded=*/true, qscratch, st, &qp));
        RQC(thr.ensure(m));
        launch_exact_range_thr(d_radius + q0, m, thr.p, st);
        uint32_t limit = RQ_EXACT_QGROUP;
        uint64_t learnt = 0;
        for (uint32_t g0 = 0; g0 < m;) {
            const uint32_t step = std::min<uint32_t>(m - g0, limit);
            uint64_t cap = learnt ? learnt : per_query * step;
            if (step > 1) cap = std::min(cap, budget);
            cap = std::max<uint64_t>(1, std::min<uint64_t>(cap, admitted * step));
            if (cap > 0xFFFFFFFFull) return fail(RQ_ERR_OOM, "a launch's arena of more than 2^32 records does not fit");
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
            HIPC(hipMemsetAsync(count.p, 0, 8, st));
            launch_exact_prep(a, st);
            HIPC(hipEventRecord(g.ev[0], st));
            if (prefilter) RQC(ts.launch(a, true, st));
            else launch_exact_range_scan(a, false, st);  // (positions and filter bits only: no row is read)
            HIPC(hipEventRecord(g.ev[1], st));
            HIPC(hipMemcpyAsync(h_word, count.p, 8, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            HIPC(hipGetLastError());
            const uint64_t kept = *h_word;
            RQC(elapsed(0, 1, &stats.ms_scan));
            stats.row_bytes_read += prefilter ? ts.bytes() : 0ull, stats.scan_launches += 1;
            if (kept > cap) {
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
            RQC(hits.ensure(step));
            RQC(cursor.ensure(step));
            HIPC(hipMemsetAsync(hits.p, 0, (size_t)step * 4, st));
            HIPC(hipMemsetAsync(cursor.p, 0, (size_t)step * 4, st));
            std::unique_ptr<RangePiece> p(new RangePiece());
            p->q0 = q0 + g0, p->m = step;
            RQC(p->lims.alloc((size_t)step + 1));
            HIPC(hipEventRecord(g.ev[0], st));
            launch_exact_range_dist_tiered(a, hits.p, records, st);
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
    rec.release(), keys.release();
    HIPC(hipEventRecord(g.ev[0], st));
    RQC(range_finish_pieces(*ws, pieces, nq, res.get()));
    HIPC(hipEventRecord(g.ev[1], st));
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    RQC(elapsed(0, 1, &stats.ms_select));
    *out = res.release();
    return RQ_OK;
}

static rq_status exact_tiered_range_device(const rq_index *idx, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len,
                                           const float *d_radius, const rq_exact_params_t *params, rq_range_result **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!idx || (nq && (!d_q || !d_radius))) return fail(RQ_ERR_INVALID, "null argument");
    if (nq == 0 || exact_tiered_forwards(idx)) return exact_range_device(idx, filter, d_q, nq, len, d_radius, params, out);
    g_exact_stats = rq_exact_stats_t{};
    g_exact_stats.struct_size = sizeof(rq_exact_stats_t);
    rq_exact_params_t prm{};
    RQC(exact_tiered_validate(idx, false, len, 1u, filter, params, &prm));
    const rq_status s = exact_tiered_range_impl(const_cast<rq_index *>(idx), filter, d_q, nq, len, d_radius, prm, out);
    if (s == RQ_ERR_OOM) (void)hipGetLastError();  // (a failed hipMalloc's error is sticky: the caller's next call must not pick it up)
    return s;
}

static rq_status exact_tiered_range_host(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                         const float *radius, const rq_exact_params_t *params, rq_range_result **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!idx || (nq && (!queries || !radius))) return fail(RQ_ERR_INVALID, "null argument");
    RQC(ensure_device());
    if (nq) {  // (refused before anything is allocated)
        rq_exact_params_t prm{};
        RQC(exact_tiered_validate(idx, false, len, 1u, filter, params, &prm));
    }
    DevBuf<float> dq, dr;
    RQC(dq.upload(queries, (uint64_t)nq * len));
    RQC(dr.upload(radius, nq));
    return exact_tiered_range_device(idx, filter, dq.p, nq, len, dr.p, params, out);
}
