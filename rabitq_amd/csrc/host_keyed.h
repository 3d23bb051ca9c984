// host_keyed.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  Postings of an integer column (rq_postings_*) and the keyed exact search over them
// (rq_exact_search_keyed*; kernels: kernels_keyed.h, compiled in inst_keyed.hip; the plan: keyed_plan.h).  Every entry
// reads the index and writes nothing of it; an index on which no postings are made allocates nothing here.
#pragma once
#include "kernels_keyed.h"  // (the launch interface only: the kernels are inst_keyed.hip's)

// The tuning numbers (DESIGN §4.24 has the sweep they come from); rq_keyed_tuning overrides them for measurements, results never
// depend on them.
#define RQ_KEYED_CHUNK_ROWS 1024u   // postings per work item
#define RQ_KEYED_SMALL_ROWS 1024u   // segments below it take neither the bound nor the matrix pass
static std::atomic<uint32_t> g_keyed_chunk{0}, g_keyed_small{0}, g_keyed_slabs{0};  // 0 = the default / automatic

// A value -> positions directory of one column: a snapshot, as a filter is.
static_assert(sizeof(KeyedItem) == sizeof(uint4), "a work item is uploaded as one uint4");
struct rq_postings {
    const rq_index *idx = nullptr;
    uint64_t generation = 0, removal_epoch = 0;  // the index's when it was made (a relayout or a marking rq_remove_lazy since then: refused)
    uint32_t type = 0;                           // RQ_ATTR_*
    std::vector<uint64_t> values;                // the distinct values' u64 images, ascending in the column type's own order
    std::vector<uint64_t> starts;                // values.size() + 1
    DevBuf<uint32_t> pos;                        // the live positions, grouped by value
    std::atomic<uint32_t> cap_hint{0};           // candidate slots per query the keyed search learnt on these postings
    std::string column;                          // the column's name (multi-vector search by postings reads its values as they are now)
    // the device copy of values / starts, made by the first multi-vector call by these postings and kept (host_maxsim_keyed.h)
    std::mutex dev_mu;
    bool dev_ready = false;
    DevBuf<uint64_t> d_values;
    DevBuf<uint32_t> d_starts;
    // position -> segment, made by the first complete grouped call by these postings and kept (host_group_full.h; under dev_mu too)
    bool inverse_ready = false;
    DevBuf<uint32_t> inverse;
    std::atomic<uint32_t> full_cap_hint{0};      // arena records per query the complete grouped search learnt on these postings
    bool is_signed() const { return type == RQ_ATTR_I32 || type == RQ_ATTR_I64; }
    bool wide() const { return type >= RQ_ATTR_U64; }
};
static thread_local rq_keyed_stats_t g_keyed_stats;  // the calling thread's last keyed search (rq_last_keyed_stats)

static rq_status keyed_ensure_attributes() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] { err = keyed_set_attributes(); });
    if (err != hipSuccess) return fail(RQ_ERR_HIP, std::string("hipFuncSetAttribute(keyed_scan_kernel): ") + hipGetErrorString(err));
    return RQ_OK;
}
// postings the entries of idx would accept (the filter's three checks, in its words)
static rq_status postings_current(const rq_postings *p) {
    if (p->generation != p->idx->generation)
        return fail(RQ_ERR_INVALID, "the postings were made before the index was last mutated (rq_add / rq_remove): make them again");
    if (p->removal_epoch != p->idx->removal_epoch)
        return fail(RQ_ERR_INVALID, "the postings were made before rows of the index were last marked dead (rq_remove_lazy): make them again");
    return RQ_OK;
}

static rq_status postings_create(const rq_index *idx, const char *column, rq_postings **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    AttrColumn *c = nullptr;
    RQC(attr_named(idx, column, false, &c));
    if (c->type == RQ_ATTR_F32) return fail(RQ_ERR_INVALID, "postings are for integer columns (column " + c->name + " is f32)");
    RQC(ensure_device());
    std::unique_ptr<rq_postings> p(new rq_postings());
    p->idx = idx, p->generation = idx->generation, p->removal_epoch = idx->removal_epoch, p->type = c->type;
    p->column = c->name;
    p->starts.assign(1, 0);
    if (idx->n == 0) {
        *out = p.release();
        return RQ_OK;
    }
    DevBuf<unsigned long long> keys;
    DevBuf<uint32_t> count, small;  // small: {slots claimed, pairs written}
    RQC(keys.alloc(RQ_POST_SLOTS));
    RQC(count.alloc((size_t)RQ_POST_SLOTS + 1));
    RQC(small.alloc(2));
    HIPC(hipMemsetAsync(keys.p, 0xFF, (size_t)RQ_POST_SLOTS * 8, nullptr));
    HIPC(hipMemsetAsync(count.p, 0, ((size_t)RQ_POST_SLOTS + 1) * 4, nullptr));
    HIPC(hipMemsetAsync(small.p, 0, 8, nullptr));
    PostArgs a{};
    a.col = c->data.p, a.live = idx->live ? idx->live->pos_bits.p : nullptr, a.n = idx->n;
    a.keys = keys.p, a.count = count.p, a.distinct = small.p;
    launch_post_pass(a, p->wide(), false, nullptr);
    uint32_t h_small[2] = {0, 0};
    HIPC(hipMemcpy(h_small, small.p, 8, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    if (h_small[0] > RQ_POST_MAX_VALUES) return fail(RQ_ERR_UNSUPPORTED, "the column holds more than 2^22 distinct values");
    const uint32_t cap = h_small[0] + 1;  // (+ the side entry)
    DevBuf<uint4> pairs;
    RQC(pairs.alloc(cap));
    launch_post_compact(a, pairs.p, cap, small.p + 1, nullptr);
    HIPC(hipMemcpy(h_small, small.p, 8, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    const uint32_t nv = std::min(h_small[1], cap);
    if (nv > RQ_POST_MAX_VALUES) return fail(RQ_ERR_UNSUPPORTED, "the column holds more than 2^22 distinct values");
    std::vector<uint4> h_pairs(nv);
    if (nv) HIPC(hipMemcpy(h_pairs.data(), pairs.p, (size_t)nv * 16, hipMemcpyDeviceToHost));
    const bool sg = p->is_signed(), wd = p->wide();
    std::sort(h_pairs.begin(), h_pairs.end(), [&](const uint4 &x, const uint4 &y) {
        return keyed_less(((uint64_t)x.y << 32) | x.x, ((uint64_t)y.y << 32) | y.x, sg, wd);
    });
    std::vector<uint2> slot_start(nv);
    p->values.resize(nv), p->starts.resize((size_t)nv + 1);
    uint64_t at = 0;
    for (uint32_t i = 0; i < nv; ++i) {
        p->values[i] = ((uint64_t)h_pairs[i].y << 32) | h_pairs[i].x, p->starts[i] = at;
        slot_start[i] = make_uint2(h_pairs[i].w, (uint32_t)at);
        at += h_pairs[i].z;
    }
    p->starts[nv] = at;
    RQC(p->pos.alloc(at));
    DevBuf<uint2> d_ss;
    RQC(d_ss.upload(slot_start.data(), nv));
    launch_post_cursor(d_ss.p, nv, count.p, nullptr);
    a.pos_out = p->pos.p, a.rows = at;
    launch_post_pass(a, wd, true, nullptr);
    HIPC(hipStreamSynchronize(nullptr));
    HIPC(hipGetLastError());
    *out = p.release();
    return RQ_OK;
}
static rq_status postings_info(const rq_postings *p, rq_postings_info_t *out) {
    if (!p || !out) return fail(RQ_ERR_INVALID, "null argument");
    rq_postings_info_t full{};
    full.type = p->type, full.values = p->values.size(), full.rows = p->starts.back();
    full.bytes = p->starts.back() * 4 + (p->values.size() * 2 + 1) * 8;
    return copy_out_sized(out, full);
}
static rq_status postings_values(const rq_postings *p, rq_attr_value_t *out_values, uint64_t *out_counts, uint64_t cap) {
    if (!p || (cap && (!out_values || !out_counts))) return fail(RQ_ERR_INVALID, "null argument");
    RQC(postings_current(p));
    for (uint64_t i = 0; i < std::min<uint64_t>(cap, p->values.size()); ++i)
        out_values[i].u64 = p->values[i], out_counts[i] = p->starts[i + 1] - p->starts[i];
    return RQ_OK;
}
static rq_status postings_counts(const rq_postings *p, const rq_attr_value_t *keys, uint64_t m, uint64_t *out_counts) {
    if (!p || (m && (!keys || !out_counts))) return fail(RQ_ERR_INVALID, "null argument");
    RQC(postings_current(p));
    const uint32_t nv = (uint32_t)p->values.size();
    for (uint64_t i = 0; i < m; ++i) {
        const uint32_t s = keyed_find(p->values.data(), nv, attr_image(p->type, keys[i]), p->is_signed(), p->wide());
        out_counts[i] = s < nv ? p->starts[s + 1] - p->starts[s] : 0;
    }
    return RQ_OK;
}
static rq_status postings_positions_device(const rq_postings *p, rq_attr_value_t key, uint32_t *d_out, uint64_t cap, uint64_t *out_count) {
    if (!p || !out_count) return fail(RQ_ERR_INVALID, "null argument");
    *out_count = 0;
    if (cap && !d_out) return fail(RQ_ERR_INVALID, "null output with cap > 0");
    RQC(postings_current(p));
    const uint32_t nv = (uint32_t)p->values.size();
    const uint32_t s = keyed_find(p->values.data(), nv, attr_image(p->type, key), p->is_signed(), p->wide());
    if (s == nv) return RQ_OK;
    *out_count = p->starts[s + 1] - p->starts[s];
    const uint64_t take = std::min(cap, *out_count);
    if (take) HIPC(hipMemcpy(d_out, p->pos.p + p->starts[s], take * 4, hipMemcpyDeviceToDevice));
    return RQ_OK;
}

// ---- the keyed exact search ----------------------------------------------------------------------------------------------------------
static uint32_t keyed_stride_of(uint64_t rows, uint32_t topk, uint32_t asked, uint32_t *sample_rows) {
    return exact_sample_stride(rows, rows, topk, asked, sample_rows);
}
// The checks of both entries, before anything is allocated: nulls and the sized params first (they need no device), then the exact
// search's own.
static rq_status keyed_validate(const rq_index *idx, const rq_postings *post, bool args_null, uint32_t len, uint32_t topk, const rq_filter *filter,
                                const rq_exact_params_t *params, rq_exact_params_t *prm) {
    if (!idx || !post || args_null) return fail(RQ_ERR_INVALID, "null argument");
    if (post->idx != idx) return fail(RQ_ERR_INVALID, "the postings were made for another index");
    RQC(postings_current(post));
    return exact_validate(idx, false, len, topk, filter, params, prm);
}

static rq_status keyed_search_device(const rq_index *idx, const rq_postings *post, const rq_filter *filter, const float *d_q, uint32_t nq,
                                     uint32_t len, const rq_attr_value_t *keys, uint32_t topk, const rq_exact_params_t *params, float *d_out_dist,
                                     uint32_t *d_out_id, uint32_t *d_out_n) {
    g_keyed_stats = rq_keyed_stats_t{};
    g_keyed_stats.struct_size = sizeof(rq_keyed_stats_t);
    rq_exact_params_t prm{};
    RQC(keyed_validate(idx, post, !d_out_dist || !d_out_id || !d_out_n || (nq && (!d_q || !keys)), len, topk, filter, params, &prm));
    if (nq == 0) return RQ_OK;
    RQC(exact_ensure_attributes());
    RQC(keyed_ensure_attributes());
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
    const bool fits = keyed_lds(idx->dim, true, 1).total <= RQ_KEYED_LDS_MAX;
    const uint32_t slabs_opt = g_keyed_slabs.load(), slabs = slabs_opt == 1 ? 1u : keyed_slabs(idx->dim);  // (2 only where it fits)
    const uint32_t chunk_rows = g_keyed_chunk.load() ? g_keyed_chunk.load() : RQ_KEYED_CHUNK_ROWS;
    const uint32_t small_rows = g_keyed_small.load() ? g_keyed_small.load() : RQ_KEYED_SMALL_ROWS;
    const bool prefilter = !(prm.flags & RQ_EXACT_NO_PREFILTER) && fits;
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
        // the queries [g0, g0 + step): plan, prep, (1) the bounds from the sample, (2) one scan launch, (3) exact distances and selection;
        // (2) is run again when a query's candidates did not fit its slots
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
        all.assign(plan.scan.begin(), plan.scan.end());
        all.insert(all.end(), plan.seed.begin(), plan.seed.end());
        RQC(order.ensure(plan.order.size()));  // (the buffers of an earlier step are kept: the host arrays live until the step's last wait)
        RQC(items.ensure(all.size()));
        if (!plan.order.empty()) HIPC(hipMemcpyAsync(order.p, plan.order.data(), plan.order.size() * 4, hipMemcpyHostToDevice, st));
        if (!all.empty()) HIPC(hipMemcpyAsync(items.p, all.data(), all.size() * sizeof(KeyedItem), hipMemcpyHostToDevice, st));
        const uint32_t nscan = (uint32_t)plan.scan.size(), nseed = (uint32_t)plan.seed.size();
        RQC(qbf.ensure((uint64_t)std::max(plan.tiles, 1u) * 32 * idx->dim));
        RQC(qn2.ensure((uint64_t)std::max(plan.tiles, 1u) * 32));
        RQC(qsn.ensure((uint64_t)std::max(plan.tiles, 1u) * 32));

        KeyedArgs ka{};
        ka.base = idx->view(), ka.dim = idx->dim, ka.row_bytes = (uint32_t)idx->row_bytes();
        ka.post = post->pos.p, ka.allow = filter ? filter->pos_bits.p : nullptr;
        ka.order = order.p, ka.tiles = plan.tiles, ka.qpad = qp, ka.qbf = qbf.p, ka.qn2 = qn2.p, ka.qsn = qsn.p, ka.thr = thr.p, ka.cnt = cnt.p;
        ExactArgs ea{};  // the exact distances and the selection: the exact search's own launches, from per-query candidate positions
        ea.base = idx->view(), ea.dim = idx->dim, ea.n = (uint32_t)idx->n, ea.map_ids = idx->map_ids.p;
        ea.qpad = qp, ea.thr = thr.p, ea.nq = step, ea.topk = topk, ea.cnt = cnt.p;
        if (plan.any_matrix) launch_keyed_prep(ka, st);

        // scan (+ capacity check), exact distances and selection of one launch; *over: the scan's candidates did not fit (nothing else ran)
        const auto run = [&](const uint4 *its, uint32_t nitems, bool pre, uint32_t slots_q, bool counted, bool *over, uint64_t *total) -> rq_status {
            RQC(cand.ensure((uint64_t)step * slots_q));
            RQC(ekeys.ensure((uint64_t)step * slots_q));
            ka.items = its, ka.cap = slots_q, ka.cand = cand.p;
            ea.cap = slots_q, ea.cand = cand.p, ea.keys = ekeys.p;
            launch_keyed_clear(cnt.p, step, st);
            HIPC(hipEventRecord(g.ev[0], st));
            launch_keyed_scan(ka, nitems, idx->rows.kind(), pre, slabs, st);
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
            launch_exact_dist(ea, st);
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
            RQC(run(items.p + nscan, nseed, false, std::max(plan.largest_sample, 1u), false, &over, &total));
            stats.exact += total;
            launch_exact_thr(seed_dist.p, seed_n.p, step, topk, thr.p, nullptr, st);  // (a query outside the sample: seed_n = 0, f32::MAX)
        }
        ea.out_dist = d_out_dist + (uint64_t)g0 * topk, ea.out_id = d_out_id + (uint64_t)g0 * topk, ea.out_n = d_out_n + g0;
        bool replan = false;
        for (;;) {  // (2) again, and only (2), while a query's candidates do not fit its slots: the plan, the images and the bounds stay
            RQC(run(items.p, nscan, prefilter, cap, true, &over, &total));
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

static rq_status keyed_search_host(const rq_index *idx, const rq_postings *post, const rq_filter *filter, const float *queries, uint32_t nq,
                                   uint32_t len, const rq_attr_value_t *keys, uint32_t topk, const rq_exact_params_t *params, float *out_dist,
                                   uint32_t *out_id, uint32_t *out_n) {
    rq_exact_params_t prm{};
    RQC(keyed_validate(idx, post, !out_dist || !out_id || !out_n || (nq && (!queries || !keys)), len, topk, filter, params, &prm));
    const uint64_t cells = (uint64_t)nq * topk;
    DevBuf<float> dq, dd;
    DevBuf<uint32_t> di, dn;
    RQC(dq.upload(queries, (uint64_t)nq * len));
    RQC(dd.upload(out_dist, cells));  // the caller's arrays travel both ways: slots past out_n stay as they were
    RQC(di.upload(out_id, cells));
    RQC(dn.alloc(nq));
    RQC(keyed_search_device(idx, post, filter, dq.p, nq, len, keys, topk, params, dd.p, di.p, dn.p));
    if (cells) {
        HIPC(hipMemcpy(out_dist, dd.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out_id, di.p, cells * 4, hipMemcpyDeviceToHost));
    }
    if (nq) HIPC(hipMemcpy(out_n, dn.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}
