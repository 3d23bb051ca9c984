// host_call.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  From a call to its passes: validation, capacities and pass sizes, the overflow re-runs, one pass
// in flight (PassFlight), the call's loop over its passes (query_device) and the begin / end halves of a batch call (rq_ticket).
#pragma once

// The checks every query entry shares (args_null: one of the entry's own pointer arguments is null; a range call has topk = 1).
static rq_status validate_call(const rq_index *idx, bool args_null, uint32_t len, uint32_t probe, uint32_t topk, const rq_filter *filter) {
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    if (!idx || args_null) return fail(RQ_ERR_INVALID, "null argument");
    RQC(raw_len_check(idx, "query", len));
    if (probe == 0 || idx->k == 0) return fail(RQ_ERR_INVALID, "probe == 0 (the reference panics at rabitq.rs:295)");
    if (topk == 0 || topk > RQ_MAX_TOPK) return fail(RQ_ERR_UNSUPPORTED, "topk must be in [1, 2048]");
    if (std::min(probe, idx->k) > RQ_MAX_PROBE) return fail(RQ_ERR_UNSUPPORTED, "probe > 16384 not supported");
    if (idx->dim > 4096) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
    if (filter && filter->idx != idx) return fail(RQ_ERR_INVALID, "the filter was made for another index");
    if (filter && filter->generation != idx->generation)
        return fail(RQ_ERR_INVALID, "the filter was made before the index was last mutated (rq_add / rq_remove): make it again");
    if (filter && filter->removal_epoch != idx->removal_epoch)
        return fail(RQ_ERR_INVALID, "the filter was made before rows of the index were last marked dead (rq_remove_lazy): make it again");
    return RQ_OK;
}
static rq_status validate_query(const QueryCall &c) {
    return validate_call(c.idx, !c.io.d_q || !c.io.out_dist || !c.io.out_id || !c.io.out_n, c.len, c.probe, c.topk, c.filter);
}

// What a call adds up over its passes: the reference's counters and the profile.
struct CallTotals {
    uint64_t rough = 0, precise = 0;
    rq_profile_t prof{};
};
// tail of every query call: the reference's counters (rerank.rs:105, :104, rabitq.rs:331) and the profile of the last call
static void count_call(uint32_t nq, const CallTotals &tot) {
    g_rough.fetch_add(tot.rough, std::memory_order_relaxed);
    g_precise.fetch_add(tot.precise, std::memory_order_relaxed);
    g_query.fetch_add(nq, std::memory_order_relaxed);
    g_profile = tot.prof;
}

// Uniform survivor capacity of a pass over `remaining` queries, and whether its final stage is segmented.  An index whose
// batches overflowed the default capacity (cap_hint) used to size EVERY query of a pass for the worst one (learnt capacity
// 32 768: 100 GB for a 65 536-query pass of the hard benchmark distribution); large batches now keep the default
// capacity for the stages that cannot exceed it and give every other stage per-query segments.
// (a seeded call -- it carries initial thresholds -- is never segmented)
static uint32_t pass_capacity(const QueryCall &c, uint32_t remaining, bool *seg) {
    const uint32_t hint = hints_of(c.idx, c.filter).cap.load();
    const int opt = g_seg_opt.load();
    *seg = !c.io.thr_init && rq_large_batch(remaining) && scan_is_fused(c.idx->W) && (opt >= 2 || (opt == 1 && hint > RQ_DEFAULT_CAP));
    if (*seg) return RQ_DEFAULT_CAP;  // stages that cannot exceed it stay uniform, the others are segmented
    return std::max(RQ_DEFAULT_CAP, hint);
}

// queries per pass: survivor / run buffers are 32 B per slot per query (keep one pass under ~24 GiB) and
// (query, list) pairs per pass <= 2^22 (bounds the per-pair buffers and every launch size)
static uint32_t pass_queries(const QueryCall &c, uint32_t remaining, uint32_t cap0, bool seg) {
    const rq_index *idx = c.idx;
    // survivor records + run directory: 32 B per slot per query, 48 B when the pass also keeps the second directory buffer
    // (ws_prepare: capacities beyond the default, segmented passes, long directories); the budget is a third of the HBM that
    // was free once the index was resident (at least 4 GiB: an index that fills the HBM -- 100M x 768 -- still answers a
    // 32 768-query batch in ONE pass; split in two, every block of the matrix-core scan paid its start-up twice: a third
    // of that launch at dim 768)
    const uint64_t slot_bytes = cap0 > RQ_DEFAULT_CAP || seg || hints_of(idx, c.filter).big_dirs.load() > 0 ? 48 : 32;
    // Probe lists supplied by the caller = a shard of a multi-GPU deployment: most of a query's probed lists live on other ranks
    // (empty here: skipped before any per-pair work), and the step's batch grows with the number of ranks so that a list still
    // meets as many queries as on one GPU -- cut into passes of 65 536 queries, each pass of an 8-GPU step would bring a list
    // 128 queries instead of 1024 and the matrix-core scan would run at half its rate (one-rank-of-eight rehearsal: 0.19 of
    // peak).  Such passes may hold 16 x the queries / pairs (per-pair buffers: ~200 B per pair, 6.7 GB at 2^25 pairs).
    const bool ext_lists = c.io.ext_cluster != nullptr;
    const uint64_t max_nq = ext_lists ? 16ull * RQ_MAX_NQ_PER_PASS : RQ_MAX_NQ_PER_PASS, max_pairs = ext_lists ? (1ull << 26) : (1ull << 22);
    uint32_t step_nq = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(remaining, max_nq),
                                                    std::max<uint64_t>(1, idx->pass_budget / ((uint64_t)cap0 * slot_bytes)));
    return std::min<uint32_t>(step_nq, (uint32_t)std::max<uint64_t>(1, max_pairs / c.npb()));
}

// The parameters of the next top-k pass of a call (advanced to that pass) with `remaining` queries to go: how many of them it takes
// and its capacities.
static QueryParams topk_pass_params(const QueryCall &c, uint32_t remaining) {
    bool seg = false;
    const uint32_t cap0 = pass_capacity(c, remaining, &seg);
    const uint32_t step_nq = pass_queries(c, remaining, cap0, seg);
    QueryParams qp = pass_params(c, step_nq, cap0, std::max(cap0, std::max(RQ_DEFAULT_CAP, hints_of(c.idx, c.filter).cap.load())));
    qp.seg_final = seg && rq_large_batch(step_nq);
    qp.ext_lists = c.io.ext_cluster != nullptr;
    return qp;
}

// Runs a first pass of a call (prepared workspace, no row map).  When it gives up inside an arena stage -- no room for the survivor
// arena, or it kept overflowing -- the pass is run once more on the uniform buffers (qp.seg_final is cleared), where a query that
// overflows is simply re-run with the capacity it asks for: slower, never wrong.
static rq_status run_pass_or_uniform(Workspace &ws, const QueryCall &c, QueryParams &qp, PassResult *pr, rq_profile_t *prof, bool defer) {
    ws.arena_failed = false;
    const rq_status st = run_pass(ws, c, qp, nullptr, pr, prof, defer);
    if (st == RQ_OK || !ws.arena_failed || !qp.seg_final) return st;
    (void)hipStreamSynchronize(ws.stream);
    // a failed hipMalloc leaves hipErrorOutOfMemory as the thread's last error (sticky on ROCm 7.2): the repeat's own
    // hipGetLastError() check must not pick it up; the arena of earlier batches goes back to the pool the repeat allocates from
    (void)hipGetLastError();
    ws.arena_recs.release(), ws.arena_runs.release(), ws.scan_extra.release(), ws.arena_places.release();
    ws.arena_failed = false;
    qp.seg_final = false;
    RQC(ws_prepare(c.idx, ws, qp));
    *pr = PassResult();
    return run_pass(ws, c, qp, nullptr, pr, prof, defer);
}

// ------------------------------------------------------------------------------------------------
// overflow re-runs: the mechanics top-k calls (after_pass) and range calls (range_rerun_overflowed) share
// ------------------------------------------------------------------------------------------------
// What a finished pass of m queries, still in `ws`, says about its survivor buffers.  need / alen: per run-local row, the survivors
// it asked for and (top-k passes) the length of the heuristic ranker's array; rows: the ones to run again, ascending -- their overflow
// flag is set, or (heuristic) their array outgrew hcap.
struct Overflowed {
    std::vector<uint32_t> need, alen, rows;
};
static rq_status read_overflowed(Workspace &ws, uint32_t m, bool topk_pass, bool heuristic, uint32_t hcap, Overflowed &o) {
    std::vector<uint32_t> h_ovf(m);
    o.need.assign(m, 0), o.alen.assign(m, 0), o.rows.clear();
    HIPC(hipMemcpy(o.need.data(), ws.need.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    if (topk_pass) HIPC(hipMemcpy(o.alen.data(), ws.arr_len.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(h_ovf.data(), ws.ovf.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < m; ++b)
        if (h_ovf[b] || (heuristic && o.alen[b] > hcap)) o.rows.push_back(b);
    return RQ_OK;
}

// Runs rows h_rows[0 .. rq.nq) of the pass `c` again on the pooled workspace `rws` with the parameters rq: the rows (and their probe
// lists, if the call brings them) are gathered into the workspace's retry buffers, the pass reads thresholds and writes results
// through the row map.
static rq_status rerun_rows(Workspace &rws, const QueryCall &c, const QueryParams &rq, const uint32_t *h_rows, PassResult *rr,
                            rq_profile_t *prof_acc) {
    const uint32_t m = rq.nq, npb = c.npb();
    RQC(ws_prepare(c.idx, rws, rq));
    RQC(rws.retry_q.ensure((uint64_t)m * c.len));
    RQC(rws.retry_rows.ensure(m));
    HIPC(hipMemcpy(rws.retry_rows.p, h_rows, (size_t)m * 4, hipMemcpyHostToDevice));
    gather_rows_kernel<<<ceil_div((uint64_t)m * c.len, 256), 256, 0, rws.stream>>>(c.io.d_q, rws.retry_rows.p, m, c.len, rws.retry_q.p);
    QueryCall sub = c;
    sub.io.d_q = rws.retry_q.p;
    if (c.io.ext_cluster) {  // the caller's probe lists, restricted to the re-run queries
        RQC(rws.retry_pc.ensure((uint64_t)m * npb));
        RQC(rws.retry_pd.ensure((uint64_t)m * npb));
        gather_rows_kernel<<<ceil_div((uint64_t)m * npb, 256), 256, 0, rws.stream>>>(reinterpret_cast<const float *>(c.io.ext_cluster),
                                                                                      rws.retry_rows.p, m, npb, rws.retry_pc.p);
        gather_rows_kernel<<<ceil_div((uint64_t)m * npb, 256), 256, 0, rws.stream>>>(c.io.ext_dist, rws.retry_rows.p, m, npb, rws.retry_pd.p);
        sub.io.ext_cluster = reinterpret_cast<const uint32_t *>(rws.retry_pc.p), sub.io.ext_dist = rws.retry_pd.p;
    }
    return run_pass(rws, sub, rq, rws.retry_rows.p, rr, prof_acc, false);
}

// After a finished pass (still in `ws`): remember the capacity it needed and re-run exactly the queries whose survivor
// buffers overflowed, with the capacity they asked for.  `c` is the pass's call (already advanced).
static rq_status after_pass(Workspace &ws, const QueryCall &c, const QueryParams &qp, const PassResult &pr, CallTotals &tot) {
    rq_index *idx = c.idx;
    if (pr.max_need > qp.cap) {  // remember (with headroom) so that later batches do not overflow
        // ... but only up to RQ_MAX_CAP_HINT: survivor buffers are cap x 32 B for EVERY query of the pass, so one outlier
        // query (a loose threshold after an unlucky nearest list) must not shrink the passes of all later batches; beyond
        // the bound the outliers are simply re-run below with the capacity they asked for
        uint32_t want = pow2_ceil((uint32_t)std::min<uint64_t>(pr.max_need + pr.max_need / 4, RQ_MAX_CAP_HINT));
        std::atomic<uint32_t> &cap_hint = hints_of(idx, qp.filter).cap;
        uint32_t cur = cap_hint.load();
        while (cur < want && !cap_hint.compare_exchange_weak(cur, want)) {}
    }
    if (!pr.overflowed) return RQ_OK;
    // a cut pass (adaptive probing): the re-runs must see the same cut lists -- the pass's rows, still in `ws`, are their probe lists
    // (gathered through the row map like a caller's), and they carry no rule
    QueryCall rc = c;
    if (c.rule.on() && !c.io.ext_cluster) rc.io.ext_cluster = ws.probe_cluster.p, rc.io.ext_dist = ws.probe_dist.p;
    rc.rule = ProbeRule{};
    uint32_t cap = qp.cap, hcap = qp.hcap, max_need = 0, max_alen = 0;
    std::vector<uint32_t> over_rows;
    Overflowed ov;
    // the rows of a run of m queries (run-local row b = row from[b] of the pass, or b) that overflowed the capacities it ran with
    auto collect = [&](Workspace &w, uint32_t m, const uint32_t *from, std::vector<uint32_t> &into) -> rq_status {
        RQC(read_overflowed(w, m, true, qp.heuristic, hcap, ov));
        for (uint32_t b : ov.rows) {
            into.push_back(from ? from[b] : b);
            max_need = std::max(max_need, ov.need[b]);
            max_alen = std::max(max_alen, ov.alen[b]);
        }
        return RQ_OK;
    };
    RQC(collect(ws, qp.nq, nullptr, over_rows));
    int guard = 0;
    while (!over_rows.empty() && guard++ < 8) {
        tot.prof.retries += (uint32_t)over_rows.size();
        cap = std::max(cap * 2, pow2_ceil(max_need));
        if (qp.heuristic) hcap = std::max(hcap * 2, pow2_ceil(std::max(max_alen, max_need)));
        // bound the retry workspace to ~4 GiB of survivor records
        uint32_t chunk = (uint32_t)std::max<uint64_t>(1, (4ull << 30) / ((uint64_t)(cap + hcap) * sizeof(SurvRec)));
        std::vector<uint32_t> still;
        // a pooled workspace (its buffers persist: a workload whose outliers overflow every batch must not pay
        // hipMalloc / hipFree of gigabytes per batch)
        WsLease lease(idx, ws_acquire(idx));
        for (size_t o = 0; o < over_rows.size(); o += chunk) {
            uint32_t m = (uint32_t)std::min<size_t>(chunk, over_rows.size() - o);
            PassResult rr;
            RQC(rerun_rows(*lease.w, rc, pass_params(rc, m, cap, hcap), over_rows.data() + o, &rr, nullptr));
            tot.precise += rr.precise;
            if (rr.overflowed) RQC(collect(*lease.w, m, over_rows.data() + o, still));
        }
        over_rows.swap(still);
    }
    if (!over_rows.empty()) return fail(RQ_ERR_OOM, "survivor buffers kept overflowing");
    return RQ_OK;
}

// ------------------------------------------------------------------------------------------------
// one pass in flight
// ------------------------------------------------------------------------------------------------
// A pass of a top-k call on a workspace (and stream) of its own, in two halves: begin enqueues the whole pass and returns, end waits
// for it, adds it to the call's totals and does the (rare) overflow re-runs.  Whatever happens in between, the destructor waits for
// an enqueued pass and hands the workspace back.  A flight keeps its workspace from one pass to the next until release().
struct PassFlight {
    rq_index *idx = nullptr;
    Workspace *ws = nullptr;
    bool borrowed = false;  // ws is the caller's (set together with ws): never released here
    bool enqueued = false;
    QueryCall call;  // the pass's: advanced to its first query
    QueryParams qp{};
    PassFlight() = default;
    PassFlight(const PassFlight &) = delete;
    PassFlight &operator=(const PassFlight &) = delete;
    ~PassFlight() { release(); }

    rq_status begin(const QueryCall &pass_call, const QueryParams &params, CallTotals &tot) {
        call = pass_call, qp = params, idx = call.idx;
        if (!ws) ws = ws_acquire(idx);
        RQC(ws_prepare(idx, *ws, qp));
        enqueued = true;
        PassResult pr;
        return run_pass_or_uniform(*ws, call, qp, &pr, &tot.prof, true);
    }
    rq_status end(CallTotals &tot) {  // (nothing enqueued: nothing to do)
        if (!enqueued) return RQ_OK;
        enqueued = false;
        PassResult pr;
        RQC(finish_pass(idx, *ws, &pr, &tot.prof));
        tot.rough += pr.rough, tot.precise += pr.precise;
        return after_pass(*ws, call, qp, pr, tot);
    }
    void release() {
        if (enqueued) (void)hipStreamSynchronize(ws->stream);  // (an error path: nothing may stay in flight)
        if (ws && !borrowed) ws_release(idx, ws);
        ws = nullptr, enqueued = false, borrowed = false;
    }
};

// tail of every top-k call: the reference's panics and counters
static rq_status conclude_query(const QueryCall &c, uint32_t nq, const CallTotals &tot) {
    bool any_empty = false;
    if (c.heuristic) {  // rerank.rs:171-173: an empty array panics in the reference
        std::vector<uint32_t> h_n(nq);
        HIPC(hipMemcpy(h_n.data(), c.io.out_n, nq * 4, hipMemcpyDefault));  // out_n may be device or mapped host memory
        for (uint32_t v : h_n) any_empty |= (v == 0);
    }
    count_call(nq, tot);
    if (any_empty) return fail(RQ_ERR_EMPTY, "heuristic ranker accepted no candidate for at least one query");
    return RQ_OK;
}

// A top-k call over nq queries, queries / outputs in device memory: its passes, one after the other through a ring of flights.
// use_ws: the caller holds (and releases) the workspace every pass runs on.
static rq_status query_device(const QueryCall &call, uint32_t nq, Workspace *use_ws) {
    RQC(validate_query(call));
    if (nq == 0) return RQ_OK;
    const rq_index *idx = call.idx;
    CallTotals tot;
    PassFlight fl[2];
    fl[0].ws = use_ws, fl[0].borrowed = use_ws != nullptr;
    // A call of several passes (more than 65 536 queries) keeps TWO passes in flight, each on a workspace and stream of its own -- what
    // rq_query_batch_device_begin / _end let a caller do with two batches, done here for one large batch: pass i + 1 is enqueued
    // before pass i is waited for, so the thin launches at either end of a pass overlap the other pass's wide ones (+4 %: 131 072
    // queries 33.9 -> 32.6 ms per call).  Results are those of the passes run one after the other.  Every other call has ONE flight,
    // which keeps its workspace for the whole call.
    uint32_t depth = 1;
    if (!use_ws && !call.io.ext_cluster && !call.io.thr_init && g_pass_overlap.load()) {
        const QueryParams first = topk_pass_params(call, nq);
        // (only with room for a second workspace: an index that fills the HBM -- configs[3] -- runs its passes one after the other;
        // rough size of a pass's buffers: survivor records + directories, per-pair records and operands, distances, ranker state)
        size_t free_b = 0, total_b = 0;
        if (first.nq < nq && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const uint64_t need = (uint64_t)first.nq * ((uint64_t)first.cap * 48 + (uint64_t)call.npb() * 320 + (uint64_t)idx->dim * 8 + (uint64_t)idx->k * 4 + 4096);
            if (free_b > need + (6ull << 30)) depth = 2;
        }
    }
    uint32_t slot = 0;
    for (uint32_t q0 = 0, step_nq = 0; q0 < nq; q0 += step_nq, slot = (slot + 1) % depth) {
        PassFlight &f = fl[slot];
        // the pass that had this slot (the one before the previous one, or the previous one) is finished BEFORE the next one's
        // parameters are computed: they read the capacity hints it may just have learnt
        RQC(f.end(tot));
        if (depth > 1) f.release();  // (the passes take workspaces of their own from the pool, this one among them)
        const QueryCall pc = call.at(q0);
        const QueryParams qp = topk_pass_params(pc, nq - q0);
        step_nq = qp.nq;
        RQC(f.begin(pc, qp, tot));
    }
    for (uint32_t i = 0; i < depth; ++i, slot = (slot + 1) % depth) RQC(fl[slot].end(tot));  // oldest first
    return conclude_query(call, nq, tot);
}

// Adaptive probing's look at a rule (rq_probe_counts_device): the query transform, the rotation, the coarse ranking and the cut of
// every query -- the front of a pass (Pass::rotate_coarse), nothing behind it.  call.rule.out_nprobe receives the counts; no counter of
// rq_metrics moves.
static rq_status probe_counts_device(const QueryCall &call, uint32_t nq) {
    RQC(validate_call(call.idx, !call.io.d_q || !call.rule.out_nprobe, call.len, call.probe, 1, nullptr));
    if (nq == 0) return RQ_OK;
    rq_index *idx = call.idx;
    WsLease lease(idx, ws_acquire(idx));
    Workspace &ws = *lease.w;
    RQC(ws_ensure_stream(ws));
    const uint32_t m = call.npb();
    const uint32_t step = (uint32_t)std::min<uint64_t>(RQ_MAX_NQ_PER_PASS, std::max<uint64_t>(1, (1ull << 22) / m));  // (a top-k pass's bounds)
    for (uint64_t q0 = 0; q0 < nq; q0 += step) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(step, nq - q0);
        const QueryCall pc = call.at(q0);
        const QueryParams qp = pass_params(pc, n, 0, 0);
        RQC(ws.qpad.ensure((uint64_t)n * idx->dim));
        RQC(ws.y.ensure((uint64_t)n * idx->dim));
        RQC(ws.dist.ensure((uint64_t)n * idx->k));
        RQC(ws.probe_dist.ensure((uint64_t)n * m));
        RQC(ws.probe_cluster.ensure((uint64_t)n * m));
        RQC(ws.totals.ensure(16));
        PassPlan pl{};
        pl.nprobe = m, pl.npairs = n * m;
        ws.prof.reset(0, ws.stream);
        Pass c{idx, ws, qp, pl, ws.prof, ws.stream, idx->dim, idx->k, idx->W, n, 1u, m, n * m, pc.io, nullptr, nullptr, pc.io.d_q,
               ws.probe_cluster.p, ws.probe_dist.p};
        RQC(c.rotate_coarse());
        HIPC(hipStreamSynchronize(ws.stream));
        HIPC(hipGetLastError());
    }
    return RQ_OK;
}

// The same call split in two, so that a caller can keep several batches in flight (each on its own workspace and HIP stream): a
// ticket is one flight and its totals.  Calls that need more than one pass run synchronously inside begin.
struct rq_ticket {
    rq_index *idx = nullptr;  // (counted in idx->open_tickets until _end)
    PassFlight flight;
    CallTotals tot;
    bool done = false;
    rq_status status = RQ_OK;
};

static rq_status query_device_begin(const QueryCall &call, uint32_t nq, rq_ticket **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    RQC(validate_query(call));
    std::unique_ptr<rq_ticket> t(new rq_ticket());
    t->idx = call.idx;
    struct Open {  // counted while the ticket is outstanding (rq_add / rq_remove refuse to relayout under it)
        rq_index *i;
        bool keep = false;
        explicit Open(rq_index *x) : i(x) { i->open_tickets.fetch_add(1); }
        ~Open() { if (!keep) i->open_tickets.fetch_sub(1); }
    } open(call.idx);
    const QueryParams qp = topk_pass_params(call, nq);
    if (nq == 0 || qp.nq < nq) {  // nothing to overlap / several passes: synchronous
        t->status = query_device(call, nq, nullptr);
        t->done = true;
    } else {
        RQC(t->flight.begin(call, qp, t->tot));  // (on failure the ticket goes, and with it the flight: waited for, workspace returned)
    }
    open.keep = true;
    *out = t.release();
    return RQ_OK;
}

static rq_status query_device_end(rq_ticket *tk) {
    if (!tk) return fail(RQ_ERR_INVALID, "null ticket");
    std::unique_ptr<rq_ticket> t(tk);
    t->idx->open_tickets.fetch_sub(1);
    if (t->done) return t->status;
    RQC(t->flight.end(t->tot));
    return conclude_query(t->flight.call, t->flight.qp.nq, t->tot);
}
