// host_keyed_tiered.h -- part of the host side of librabitq_hip.so (one translation unit, see rabitq_hip.hip; after host_exact_tiered.h
// and host_keyed.h, whose plan, phases, overflow protocol, learnt capacity (cap_hint on the postings) and stats these entries keep).
// The keyed exact search on every f32-row index at every dimension: rq_exact_search_keyed_tiered* (include/rabitq_hip.h; DESIGN §4.30;
// kernel: kernels_keyed_tiered.h, compiled in inst_keyed_tiered.hip).  What differs from host_keyed.h: the items with a matrix pass
// go to the dimension-sliced scan (plane 0 of a split row, rows of either tier), the items without one (small segments, the bound's
// sample, RQ_EXACT_NO_PREFILTER, dim > 2048) to keyed_scan_kernel's form that reads no row, both into the same slots; and the exact
// distances resolve a position through BaseView::row (launch_exact_dist_tiered).
#pragma once
#include "kernels_keyed_tiered.h"  // (the launch interface only)

static rq_status keyed_tiered_ensure_attributes() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] { err = keyed_sliced_set_attributes(); });
    if (err != hipSuccess) return fail(RQ_ERR_HIP, std::string("hipFuncSetAttribute(keyed_scan_sliced_kernel): ") + hipGetErrorString(err));
    return RQ_OK;
}
// keyed_validate without the exact search's two layout refusals
static rq_status keyed_tiered_validate(const rq_index *idx, const rq_postings *post, bool args_null, uint32_t len, uint32_t topk,
                                       const rq_filter *filter, const rq_exact_params_t *params, rq_exact_params_t *prm) {
    if (!idx || !post || args_null) return fail(RQ_ERR_INVALID, "null argument");
    if (post->idx != idx) return fail(RQ_ERR_INVALID, "the postings were made for another index");
    RQC(postings_current(post));
    return exact_tiered_validate(idx, false, len, topk, filter, params, prm);
}
// indexes rq_exact_search_keyed serves as they are: typed rows at any dimension, and plain f32 rows all in HBM where its own matrix
// pass exists (dim <= 448)
static bool keyed_tiered_forwards(const rq_index *idx) {
    if (idx->rows.typed()) return true;
    return !idx->base_host && idx->n_dev >= idx->n && !idx->split_rows && keyed_lds(idx->dim, true, 1).total <= RQ_KEYED_LDS_MAX;
}

static rq_status keyed_tiered_search_device(const rq_index *idx, const rq_postings *post, const rq_filter *filter, const float *d_q, uint32_t nq,
                                            uint32_t len, const rq_attr_value_t *keys, uint32_t topk, const rq_exact_params_t *params,
                                            float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n) {
    g_keyed_stats = rq_keyed_stats_t{};
    g_keyed_stats.struct_size = sizeof(rq_keyed_stats_t);
    rq_exact_params_t prm{};
    RQC(keyed_tiered_validate(idx, post, !d_out_dist || !d_out_id || !d_out_n || (nq && (!d_q || !keys)), len, topk, filter, params, &prm));
    if (keyed_tiered_forwards(idx)) return keyed_search_device(idx, post, filter, d_q, nq, len, keys, topk, params, d_out_dist, d_out_id, d_out_n);
    if (nq == 0) return RQ_OK;
    RQC(exact_ensure_attributes());
    RQC(keyed_tiered_ensure_attributes());
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
    rq_keyed_stats_t &stats = g_keyed_stats;
    const uint32_t chunk_rows = g_keyed_chunk.load() ? g_keyed_chunk.load() : RQ_KEYED_CHUNK_ROWS;
    const uint32_t small_rows = g_keyed_small.load() ? g_keyed_small.load() : RQ_KEYED_SMALL_ROWS;
    const bool prefilter = !(prm.flags & RQ_EXACT_NO_PREFILTER) && keyed_sliced_slice(idx->dim) != 0;
    const bool seeded = prefilter && !(prm.flags & RQ_EXACT_NO_SEED);  // (without the matrix pass a bound saves nothing: none is made)
    std::atomic<uint32_t> &cap_hint = const_cast<rq_postings *>(post)->cap_hint;
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const uint64_t slot_budget = std::max<uint64_t>(64ull << 20, std::min<uint64_t>(RQ_EXACT_SLOT_BUDGET, free_b / 3));

    DevBuf<float> qscratch, thr, qn2, qsn, seed_dist;
    DevBuf<uint32_t> cand, order, seed_id, seed_n;
    DevBuf<unsigned int> cnt;
    DevBuf<uint16_t> qbf;
    DevBuf<unsigned long long> ekeys;
    DevBuf<uint4> items;
    std::vector<unsigned int> h_cnt;
    std::vector<uint64_t> images;
    std::vector<KeyedItem> all;
    KeyedPlan plan;
    const uint32_t nv = (uint32_t)post->values.size();
    uint32_t cap_learnt = 0;  // what a re-run of this call learnt

    for (uint32_t g0 = 0; g0 < nq;) {
        // the queries [g0, g0 + step), as host_keyed.h: plan, prep, (1) the bounds from the sample, (2) the scan, (3) exact distances
        // and selection; (2) is run again when a query's candidates did not fit its slots
        uint32_t step = std::min<uint32_t>(nq - g0, RQ_EXACT_CHUNK);
        const auto plan_step = [&](uint32_t m) {
            PhaseClock clk;
            images.resize(m);
            for (uint32_t i = 0; i < m; ++i) images[i] = attr_image(post->type, keys[g0 + i]);
            keyed_plan(post->values.data(), post->starts.data(), nv, post->is_signed(), post->wide(), images.data(), m, topk, prm.seed_probe,
                       prefilter, seeded, chunk_rows, small_rows, keyed_stride_of, &plan);
            stats.ms_plan += clk.lap();
        };
        plan_step(step);
        const auto cap_of = [&]() {
            const uint32_t cap_max = std::max(plan.largest_segment, 1u);  // (a query keeps at most every row of its segment)
            const uint32_t want = prm.cand_per_query ? prm.cand_per_query : std::max(std::max<uint32_t>(4 * topk, 1024u), cap_hint.load());
            return std::min(cap_max, std::max(want, cap_learnt));
        };
        uint32_t cap = cap_of();
        const uint64_t slots = std::max<uint64_t>(cap, plan.largest_sample);
        const uint32_t fit = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(step, slot_budget / (RQ_EXACT_SLOT_BYTES * std::max<uint64_t>(slots, 1))));
        if (fit < step) {  // fewer queries a launch: plan them again
            step = fit;
            plan_step(step);
            cap = cap_of();
        }
        const float *qp = nullptr;  // q': transformed, padded
        RQC(transform_queries(idx, d_q + (uint64_t)g0 * len, step, len, /*want_padded=*/true, qscratch, st, &qp));
        RQC(thr.ensure(step));
        RQC(cnt.ensure(step));
        // the upload: the scan's items with a matrix pass, those without, the sample's
        all.clear();
        for (const KeyedItem &it : plan.scan)
            if (it.stride & RQ_KEYED_MATRIX) all.push_back(it);
        const uint32_t nsliced = (uint32_t)all.size(), nscan = (uint32_t)plan.scan.size(), nseed = (uint32_t)plan.seed.size();
        for (const KeyedItem &it : plan.scan)
            if (!(it.stride & RQ_KEYED_MATRIX)) all.push_back(it);
        all.insert(all.end(), plan.seed.begin(), plan.seed.end());
        RQC(order.ensure(plan.order.size()));  // (the buffers of an earlier step are kept: the host arrays live until the step's last wait)
        RQC(items.ensure(all.size()));
        if (!plan.order.empty()) HIPC(hipMemcpyAsync(order.p, plan.order.data(), plan.order.size() * 4, hipMemcpyHostToDevice, st));
        if (!all.empty()) HIPC(hipMemcpyAsync(items.p, all.data(), all.size() * sizeof(KeyedItem), hipMemcpyHostToDevice, st));
        RQC(qbf.ensure((uint64_t)std::max(plan.tiles, 1u) * 32 * idx->dim));
        RQC(qn2.ensure((uint64_t)std::max(plan.tiles, 1u) * 32));
        RQC(qsn.ensure((uint64_t)std::max(plan.tiles, 1u) * 32));

        KeyedArgs ka{};
        ka.base = idx->view(), ka.dim = idx->dim, ka.row_bytes = (uint32_t)idx->row_bytes();
        ka.post = post->pos.p, ka.allow = filter ? filter->pos_bits.p : nullptr;
        ka.order = order.p, ka.tiles = plan.tiles, ka.qpad = qp, ka.qbf = qbf.p, ka.qn2 = qn2.p, ka.qsn = qsn.p, ka.thr = thr.p, ka.cnt = cnt.p;
        ExactArgs ea{};  // the exact distances and the selection, from per-query candidate positions
        ea.base = idx->view(), ea.dim = idx->dim, ea.n = (uint32_t)idx->n, ea.map_ids = idx->map_ids.p;
        ea.qpad = qp, ea.thr = thr.p, ea.nq = step, ea.topk = topk, ea.cnt = cnt.p;
        if (plan.any_matrix) launch_keyed_prep(ka, st);

        // scan (+ capacity check), exact distances and selection: the first `sliced` of the n items take the matrix pass, the others read
        // no row; *over: the scan's candidates did not fit (nothing else ran)
        const auto run = [&](const uint4 *its, uint32_t sliced, uint32_t n, uint32_t slots_q, bool counted, bool *over, uint64_t *total) -> rq_status {
            RQC(cand.ensure((uint64_t)step * slots_q));
            RQC(ekeys.ensure((uint64_t)step * slots_q));
            ka.cap = slots_q, ka.cand = cand.p;
            ea.cap = slots_q, ea.cand = cand.p, ea.keys = ekeys.p;
            launch_keyed_clear(cnt.p, step, st);
            HIPC(hipEventRecord(g.ev[0], st));
            ka.items = its;
            launch_keyed_scan_sliced(ka, sliced, idx->split_rows, st);
            ka.items = its + sliced;
            launch_keyed_scan(ka, n - sliced, idx->rows.kind(), false, 1, st);
            HIPC(hipEventRecord(g.ev[1], st));
            h_cnt.resize(step);
            HIPC(hipMemcpyAsync(h_cnt.data(), cnt.p, (size_t)step * 4, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            HIPC(hipGetLastError());
            float ms = 0.0f, ms2 = 0.0f;
            HIPC(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
            if (counted) stats.ms_scan += ms;
            else stats.ms_seed += ms;
            unsigned int most = 0;
            *total = 0;
            for (unsigned int c : h_cnt) *total += c, most = std::max(most, c);
            *over = most > slots_q;
            if (*over) {
                cap_learnt = (uint32_t)std::min<uint64_t>(0xFFFFFFFFu, ((uint64_t)most + most / 8 + 255) / 256 * 256);
                return RQ_OK;
            }
            HIPC(hipEventRecord(g.ev[0], st));
            launch_exact_dist_tiered(ea, st);
            HIPC(hipEventRecord(g.ev[1], st));
            launch_exact_select(ea, st);
            HIPC(hipEventRecord(g.ev[2], st));
            HIPC(hipStreamSynchronize(st));
            HIPC(hipGetLastError());
            HIPC(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
            HIPC(hipEventElapsedTime(&ms2, g.ev[1], g.ev[2]));
            if (counted) stats.ms_exact += ms, stats.ms_select += ms2;
            else stats.ms_seed += ms + ms2;
            return RQ_OK;
        };
        bool over = false;
        uint64_t total = 0;
        launch_exact_thr(nullptr, nullptr, step, topk, thr.p, nullptr, st);  // every bound f32::MAX (the sample's own pass runs without one)
        if (nseed) {  // (1): every sampled admitted row of the seeded segments' queries, exactly; the topk-th smallest is the bound
            RQC(seed_dist.ensure((uint64_t)step * topk));
            RQC(seed_id.ensure((uint64_t)step * topk));
            RQC(seed_n.ensure(step));
            ea.out_dist = seed_dist.p, ea.out_id = seed_id.p, ea.out_n = seed_n.p;
            RQC(run(items.p + nscan, 0, nseed, std::max(plan.largest_sample, 1u), false, &over, &total));
            stats.exact += total;
            launch_exact_thr(seed_dist.p, seed_n.p, step, topk, thr.p, nullptr, st);  // (a query outside the sample: seed_n = 0, f32::MAX)
        }
        ea.out_dist = d_out_dist + (uint64_t)g0 * topk, ea.out_id = d_out_id + (uint64_t)g0 * topk, ea.out_n = d_out_n + g0;
        bool replan = false;
        for (;;) {  // (2) again, and only (2), while a query's candidates do not fit its slots: the plan, the images and the bounds stay
            RQC(run(items.p, nsliced, nscan, cap, true, &over, &total));
            if (!over) break;
            stats.reruns += 1;
            if (!prm.cand_per_query) {
                uint32_t cur = cap_hint.load();
                while (cur < cap_learnt && !cap_hint.compare_exchange_weak(cur, cap_learnt)) {}
            }
            cap = cap_of();
            if ((uint64_t)step * cap * RQ_EXACT_SLOT_BYTES > slot_budget && step > 1) {  // the learnt capacity needs fewer queries a launch
                replan = true;
                break;
            }
        }
        if (replan) continue;
        stats.keys_distinct += plan.keys_distinct, stats.queries_absent += plan.queries_absent;
        stats.items += nscan + nseed, stats.rows_gathered += plan.rows_matrix, stats.rows_listed += plan.rows_scan, stats.candidates += total, stats.exact += total;
        if (plan.any_matrix) stats.prefilter = 1;
        g0 += step;
    }
    return RQ_OK;
}

static rq_status keyed_tiered_search_host(const rq_index *idx, const rq_postings *post, const rq_filter *filter, const float *queries, uint32_t nq,
                                          uint32_t len, const rq_attr_value_t *keys, uint32_t topk, const rq_exact_params_t *params, float *out_dist,
                                          uint32_t *out_id, uint32_t *out_n) {
    rq_exact_params_t prm{};
    RQC(keyed_tiered_validate(idx, post, !out_dist || !out_id || !out_n || (nq && (!queries || !keys)), len, topk, filter, params, &prm));
    const uint64_t cells = (uint64_t)nq * topk;
    DevBuf<float> dq, dd;
    DevBuf<uint32_t> di, dn;
    RQC(dq.upload(queries, (uint64_t)nq * len));
    RQC(dd.upload(out_dist, cells));  // the caller's arrays travel both ways: slots past out_n stay as they were
    RQC(di.upload(out_id, cells));
    RQC(dn.alloc(nq));
    RQC(keyed_tiered_search_device(idx, post, filter, dq.p, nq, len, keys, topk, params, dd.p, di.p, dn.p));
    if (cells) {
        HIPC(hipMemcpy(out_dist, dd.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out_id, di.p, cells * 4, hipMemcpyDeviceToHost));
    }
    if (nq) HIPC(hipMemcpy(out_n, dn.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}
