// host_group_full.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in
// order; they are not stand-alone headers; after host_exact_range.h, host_group.h, host_keyed.h and host_maxsim_keyed.h).  The complete
// form of the exact grouped search (rq_exact_search_grouped_full*; kernels: kernels_group_full.h, compiled in
// inst_group_full.hip): the true topk groups of every query from ONE pass over all rows.
//   (1) position -> segment of the postings, once per postings object;
//   (2) T_q from the exact search's own sample launches (an upper bound of the topk-th smallest group minimum);
//   (3) the exact scan's range form at thr = T_q, its records in one arena, one re-run with the learnt capacity on overflow
//       (host_exact_range.h's scheme, word for word), the queries streamed in groups of RQ_EXACT_QGROUP;
//   (4) exact distance and segment of every record, the hits into per-query segments;
//   (5) the distinct-minimum selection: with group_size == 1 it writes the final outputs and the call ends here;
//   (6) group_size > 1: the chosen segments are read back once and the keyed exact search runs over nq x topk plan-queries --
//       plan-query b topk + ord is query b against the ord-th chosen value at topk = group_size -- straight into the outputs, which (5)
//       has preset to the padding; a slot behind out_n[b] carries a value the postings do not hold and gets nothing.
// No existing kernel or launch changes; every entry reads the index and writes nothing of it.
#pragma once
#include "kernels_group_full.h"  // (the launch interface only: the kernels are inst_group_full.hip's)

static thread_local rq_group_full_stats_t g_group_full_stats;  // the calling thread's last complete grouped call (rq_last_group_full_stats)

// The checks that need no device: nulls, the struct, fetch, the limits.
static rq_status group_full_checks(const rq_index *idx, const rq_postings *post, const float *q, uint32_t nq, const rq_group_params_t *gp,
                                   const GroupOut &out) {
    if (!idx || !post || !gp || !out.dist || !out.id || !out.key || !out.group_n || !out.n || (nq && !q)) return fail(RQ_ERR_INVALID, "null argument");
    if (gp->struct_size != sizeof(rq_group_params_t))
        return fail(RQ_ERR_INVALID, "struct_size is not sizeof(rq_group_params_t) (set it before the call)");
    if (gp->flags) return fail(RQ_ERR_INVALID, "unknown bit in rq_group_params_t.flags");
    if (gp->fetch) return fail(RQ_ERR_INVALID, "rq_group_params_t.fetch must be 0: the complete form sees every row");
    if (gp->topk == 0 || gp->group_size == 0 || (uint64_t)gp->topk * gp->group_size > RQ_MAX_TOPK)
        return fail(RQ_ERR_UNSUPPORTED, "topk and group_size must be at least 1 and topk * group_size <= 2048");
    return RQ_OK;
}

// (1): made by the first complete grouped call by these postings and kept on the object (4 bytes per stored position)
static rq_status group_full_inverse(const rq_index *idx, const rq_postings *cp, hipStream_t st, uint32_t *built) {
    RQC(postings_device_copy(cp));
    rq_postings *p = const_cast<rq_postings *>(cp);
    std::lock_guard<std::mutex> lock(p->dev_mu);
    if (p->inverse_ready) return RQ_OK;
    RQC(p->inverse.alloc(idx->n));
    launch_group_full_inverse(p->pos.p, p->d_starts.p, (uint32_t)p->values.size(), p->starts.back(), p->inverse.p, idx->n, st);
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    p->inverse_ready = true, *built = 1;
    return RQ_OK;
}

static rq_status group_full_device(const rq_index *idx, const rq_postings *post, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len,
                                   const rq_exact_params_t *exact, const rq_group_params_t *gp, const GroupOut &out) {
    RQC(group_full_checks(idx, post, d_q, nq, gp, out));
    g_group_full_stats = rq_group_full_stats_t{};
    g_group_full_stats.struct_size = sizeof(rq_group_full_stats_t);
    const uint32_t topk = gp->topk, gsize = gp->group_size, slots = topk * gsize;
    rq_exact_params_t prm{};
    RQC(ensure_device());
    RQC(keyed_validate(idx, post, false, len, slots, filter, exact, &prm));
    if (nq == 0) return RQ_OK;
    RQC(exact_ensure_attributes());
    hipStream_t st = nullptr;
    HIPC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct Guard {
        hipStream_t s;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Guard() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
            (void)hipStreamDestroy(s);
        }
    } g{st};
    for (hipEvent_t &e : g.ev) HIPC(hipEventCreate(&e));
    auto elapsed = [&](int from, int to, float *acc) -> rq_status {
        float ms = 0.0f;
        HIPC(hipEventElapsedTime(&ms, g.ev[from], g.ev[to]));
        *acc += ms;
        return RQ_OK;
    };
    rq_group_full_stats_t &stats = g_group_full_stats;
    {
        PhaseClock clk;
        RQC(group_full_inverse(idx, post, st, &stats.inverse_built));
        stats.ms_inverse = clk.lap(), stats.inverse_bytes = idx->n * 4;
    }
    const uint32_t *inverse = post->inverse.p;
    const uint64_t admitted = filter ? filter->rows : idx->n;
    const bool scannable = idx->n && admitted && post->starts.back();  // (nothing to scan: a launch of no blocks is not a launch)
    const bool prefilter = !(prm.flags & RQ_EXACT_NO_PREFILTER) && exact_scan_subtiles(idx->dim) != 0;
    const bool seeded = prefilter && !(prm.flags & RQ_EXACT_NO_SEED);  // (without the pre-filter the scan keeps every pair whatever the bound)
    uint32_t sample_rows = 0;
    const uint32_t stride = exact_sample_stride(idx->n, admitted, topk, prm.seed_probe, &sample_rows);
    std::atomic<uint32_t> &cap_hint = const_cast<rq_postings *>(post)->full_cap_hint;  // arena records per query earlier calls learnt
    const uint64_t per_query = std::min<uint64_t>(admitted, prm.cand_per_query ? prm.cand_per_query : std::max(RQ_EXRANGE_PER_QUERY, cap_hint.load()));
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const uint64_t slot_budget = std::max<uint64_t>(64ull << 20, std::min<uint64_t>(RQ_EXACT_SLOT_BUDGET, free_b / 3));
    const uint64_t budget = slot_budget / (RQ_EXRANGE_RECORD_BYTES + 4);  // records: the arena's 16 bytes and the segment
    const uint32_t sample_fit = (uint32_t)std::max<uint64_t>(1, slot_budget / (RQ_EXACT_SLOT_BYTES * std::max(sample_rows, 1u)));

    DevBuf<float> qscratch, thr, qn2, qsn;
    DevBuf<uint16_t> qbf;
    DevBuf<uint2> rec;
    DevBuf<unsigned long long> keys, count, lims, hit_keys, sample_keys;
    DevBuf<uint32_t> segs, hits, cursor, hit_segs, chosen, sample_cand;
    DevBuf<unsigned int> sample_cnt;
    RQC(count.alloc(1));
    RQC(chosen.alloc((uint64_t)nq * topk));
    unsigned long long h_word = 0;
    for (uint32_t q0 = 0; q0 < nq; q0 += RQ_EXACT_CHUNK) {
        const uint32_t m = std::min<uint32_t>(RQ_EXACT_CHUNK, nq - q0);
        const float *qp = nullptr;  // q': transformed, padded
        RQC(transform_queries(idx, d_q + (uint64_t)q0 * len, m, len, /*want_padded=*/true, qscratch, st, &qp));
        RQC(thr.ensure(m));
        uint32_t limit = RQ_EXACT_QGROUP;  // queries of a launch: halved while a group's arena exceeds the budget
        uint64_t learnt = 0;               // the pairs the group's last launch counted (it overflowed): the next one's capacity
        uint32_t bound_g0 = 0xFFFFFFFFu, bound_step = 0;  // the queries whose bounds thr holds (a repeated launch keeps them)
        for (uint32_t g0 = 0; g0 < m;) {
            const uint32_t step = std::min(std::min<uint32_t>(m - g0, limit), seeded ? sample_fit : limit);
            ExactArgs a{};
            a.base = idx->view(), a.dim = idx->dim, a.n = (uint32_t)idx->n, a.rows = a.n, a.stride = 1, a.map_ids = idx->map_ids.p;
            a.allow = filter ? filter->pos_bits.p : nullptr;
            a.nq = step, a.nq32 = (step + 31) / 32 * 32;
            a.qpad = qp + (uint64_t)g0 * idx->dim, a.thr = thr.p + g0;
            uint32_t records = 0;
            if (scannable) {
                RQC(qbf.ensure((uint64_t)a.nq32 * idx->dim));
                RQC(qn2.ensure(a.nq32));
                RQC(qsn.ensure(a.nq32));
                a.qbf = qbf.p, a.qn2 = qn2.p, a.qsn = qsn.p;
                // (2) the bounds, unless this launch repeats the last one's queries
                const bool bound_now = bound_g0 != g0 || bound_step != step;
                if (bound_now) {
                    launch_exact_thr(nullptr, nullptr, step, topk, a.thr, nullptr, st);  // f32::MAX (the sample's own pass runs without a bound)
                    HIPC(hipEventRecord(g.ev[0], st));
                    if (seeded) {
                        ExactArgs sa = a;
                        sa.stride = stride, sa.rows = sample_rows, sa.cap = sample_rows;
                        RQC(sample_cand.ensure((uint64_t)step * sample_rows));
                        RQC(sample_keys.ensure((uint64_t)step * sample_rows));
                        RQC(sample_cnt.ensure(step));
                        sa.cand = sample_cand.p, sa.cnt = sample_cnt.p, sa.keys = sample_keys.p;
                        HIPC(hipMemsetAsync(sample_cnt.p, 0, (size_t)step * 4, st));
                        launch_exact_scan(sa, false, st);  // every sampled admitted row of every query (a query keeps at most sample_rows: no overflow)
                        launch_exact_dist(sa, st);
                        launch_group_full_bound(sa, inverse, topk, a.thr, st);
                    }
                    HIPC(hipEventRecord(g.ev[1], st));
                    bound_g0 = g0, bound_step = step;
                }
                // (3) the scan, and what it counted
                uint64_t cap = learnt ? learnt : per_query * step;
                if (step > 1) cap = std::min(cap, budget);
                cap = std::max<uint64_t>(1, std::min<uint64_t>(cap, admitted * step));
                if (cap > 0xFFFFFFFFull) return fail(RQ_ERR_OOM, "a launch's arena of more than 2^32 records does not fit");  // (step == 1: cap <= n < 2^32)
                RQC(rec.ensure(cap));
                RQC(keys.ensure(cap));
                RQC(segs.ensure(cap));
                a.cap = (uint32_t)cap, a.rec = rec.p, a.rec_count = count.p, a.keys = keys.p;
                HIPC(hipMemsetAsync(count.p, 0, 8, st));
                launch_exact_prep(a, st);
                HIPC(hipEventRecord(g.ev[2], st));
                launch_exact_range_scan(a, prefilter, st);
                HIPC(hipEventRecord(g.ev[3], st));
                HIPC(hipMemcpyAsync(&h_word, count.p, 8, hipMemcpyDeviceToHost, st));
                HIPC(hipStreamSynchronize(st));
                HIPC(hipGetLastError());
                if (bound_now && seeded) RQC(elapsed(0, 1, &stats.ms_bound));
                RQC(elapsed(2, 3, &stats.ms_scan));
                const uint64_t kept = h_word;
                if (kept > cap) {  // overflowed: nothing downstream runs on this launch
                    stats.scan_reruns += 1;
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
                records = (uint32_t)kept;
                stats.records += kept;
            }
            // (4) exact distances, segments and hit counts; offsets; the hits into their segments
            RQC(hits.ensure(step));
            RQC(cursor.ensure(step));
            RQC(lims.ensure((size_t)step + 1));
            HIPC(hipMemsetAsync(hits.p, 0, (size_t)step * 4, st));
            HIPC(hipMemsetAsync(cursor.p, 0, (size_t)step * 4, st));
            HIPC(hipEventRecord(g.ev[0], st));
            launch_group_full_dist(a, inverse, segs.p, hits.p, records, st);
            HIPC(hipEventRecord(g.ev[1], st));
            range_scan_kernel<uint32_t><<<1, 1024, 0, st>>>(hits.p, step, lims.p);
            HIPC(hipMemcpyAsync(&h_word, lims.p + step, 8, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            const uint64_t total = h_word;
            RQC(hit_keys.ensure(total));
            RQC(hit_segs.ensure(total));
            if (total) launch_group_full_scatter(a, segs.p, ExactSegments{hits.p, cursor.p, lims.p, hit_keys.p}, hit_segs.p, records, st);
            // (5) the selection, and every output slot of the launch's queries
            const uint64_t b0 = (uint64_t)q0 + g0;
            GroupFullSelectArgs sa{};
            sa.keys = hit_keys.p, sa.segs = hit_segs.p, sa.lims = lims.p, sa.values = reinterpret_cast<const unsigned long long *>(post->d_values.p);
            sa.topk = topk, sa.gsize = gsize;
            sa.out_dist = out.dist + b0 * slots, sa.out_id = out.id + b0 * slots;
            sa.out_key = reinterpret_cast<unsigned long long *>(out.key) + b0 * topk, sa.out_group_n = out.group_n + b0 * topk;
            sa.out_n = out.n + b0, sa.out_fetched = out.fetched ? out.fetched + b0 : nullptr, sa.chosen = chosen.p + b0 * topk;
            HIPC(hipEventRecord(g.ev[2], st));
            launch_group_full_select(sa, step, st);
            HIPC(hipEventRecord(g.ev[3], st));
            HIPC(hipStreamSynchronize(st));
            HIPC(hipGetLastError());
            RQC(elapsed(0, 1, &stats.ms_exact));
            RQC(elapsed(1, 2, &stats.ms_scatter));
            RQC(elapsed(2, 3, &stats.ms_select));
            stats.hits += total;
            g0 += step, limit = RQ_EXACT_QGROUP, learnt = 0;
        }
    }
    if (gsize == 1) return RQ_OK;

    // (6) the rows of the chosen groups
    PhaseClock clk;
    const uint64_t groups = (uint64_t)nq * topk;
    std::vector<uint32_t> h_chosen(groups);
    HIPC(hipMemcpy(h_chosen.data(), chosen.p, groups * 4, hipMemcpyDeviceToHost));
    const uint32_t nv = (uint32_t)post->values.size();
    uint64_t none = 0;  // a value the postings do not hold: one of nv + 1 candidates is free
    while (keyed_find(post->values.data(), nv, none, post->is_signed(), post->wide()) != nv) ++none;
#ifdef RQ_DEV_ABLATIONS
    std::vector<uint32_t> head_id((uint64_t)nq * slots), row_id((uint64_t)nq * slots);
    HIPC(hipMemcpy(head_id.data(), out.id, head_id.size() * 4, hipMemcpyDeviceToHost));
#endif
    const rq_keyed_stats_t keyed_before = g_keyed_stats;  // (rq_last_keyed_stats keeps naming the caller's own last keyed search)
    const uint32_t per_call = std::max(1u, RQ_EXACT_CHUNK / topk);  // queries whose plan-queries one keyed call takes
    DevBuf<float> qexp;
    std::vector<rq_attr_value_t> pkeys;
    rq_status s = RQ_OK;
    for (uint32_t b0 = 0; b0 < nq && s == RQ_OK; b0 += per_call) {
        const uint32_t mb = std::min(per_call, nq - b0), pq = mb * topk;
        pkeys.resize(pq);
        for (uint32_t i = 0; i < pq; ++i) {
            const uint32_t seg = h_chosen[(uint64_t)b0 * topk + i];
            pkeys[i].u64 = seg == RQ_GF_NO_SEG ? none : post->values[seg];
        }
        RQC(qexp.ensure((uint64_t)pq * len));
        launch_group_full_expand(d_q + (uint64_t)b0 * len, len, topk, (uint64_t)pq * len, qexp.p, st);
        HIPC(hipStreamSynchronize(st));
        HIPC(hipGetLastError());
        s = keyed_search_device(idx, post, filter, qexp.p, pq, len, pkeys.data(), gsize, exact, out.dist + (uint64_t)b0 * slots,
                                out.id + (uint64_t)b0 * slots, out.group_n + (uint64_t)b0 * topk);
        stats.plan_queries += pq, stats.rows_listed += g_keyed_stats.rows_listed;
    }
    g_keyed_stats = keyed_before;
    RQC(s);
#ifdef RQ_DEV_ABLATIONS
    HIPC(hipMemcpy(row_id.data(), out.id, row_id.size() * 4, hipMemcpyDeviceToHost));
    for (uint64_t gi = 0; gi < groups; ++gi)  // row 0 of every group is the minimum the selection found
        if (head_id[gi * gsize] != row_id[gi * gsize]) return fail(RQ_ERR_HIP, "complete grouped search: a group's first keyed row is not its selected minimum");
#endif
    stats.ms_rows = clk.lap();
    return RQ_OK;
}

// The host-pointer form: the queries go up, group_full_device runs, the outputs come down.
static rq_status group_full_host(const rq_index *idx, const rq_postings *post, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                 const rq_exact_params_t *exact, const rq_group_params_t *gp, const GroupOut &out) {
    RQC(group_full_checks(idx, post, queries, nq, gp, out));
    RQC(ensure_device());
    const uint64_t groups = (uint64_t)nq * gp->topk, cells = groups * gp->group_size;
    DevBuf<float> d_q, d_od;
    DevBuf<uint32_t> d_oi, d_gn, d_n, d_f;
    DevBuf<uint64_t> d_key;
    RQC(d_q.upload(queries, (uint64_t)nq * len));
    RQC(d_od.alloc(cells));
    RQC(d_oi.alloc(cells));
    RQC(d_key.alloc(groups));
    RQC(d_gn.alloc(groups));
    RQC(d_n.alloc(nq));
    RQC(d_f.alloc(nq));
    RQC(group_full_device(idx, post, filter, d_q.p, nq, len, exact, gp, GroupOut{d_od.p, d_oi.p, d_key.p, d_gn.p, d_n.p, d_f.p}));
    if (nq) {
        HIPC(hipMemcpy(out.dist, d_od.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.id, d_oi.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.key, d_key.p, groups * 8, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.group_n, d_gn.p, groups * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.n, d_n.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
        if (out.fetched) HIPC(hipMemcpy(out.fetched, d_f.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    }
    return RQ_OK;
}
