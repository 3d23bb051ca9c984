// host_exact.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  The exact search (rq_exact_search*, include/rabitq_hip.h; kernels: kernels_exact.h, compiled in
// inst_exact.hip): validation, the bound from a sample of the rows, the workspaces, the passes with their capacity re-runs, the stats, the host-pointer entry.
#pragma once
#include "kernels_exact.h"  // (the launch interface only: the kernels are inst_exact.hip's)

static thread_local rq_exact_stats_t g_exact_stats;  // the calling thread's last exact search (rq_last_exact_stats)

static rq_status exact_ensure_attributes() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] { err = exact_set_attributes(); });
    if (err != hipSuccess) return fail(RQ_ERR_HIP, std::string("hipFuncSetAttribute(exact_scan_kernel): ") + hipGetErrorString(err));
    return RQ_OK;
}

#define RQ_EXACT_CHUNK 65536u            // queries whose transformed rows and bounds are held at a time
#define RQ_EXACT_SLOT_BYTES 12ull        // a candidate slot: its position and its key
#define RQ_EXACT_SLOT_BUDGET (16ull << 30)  // bytes of candidate slots one launch may use at most (and a third of the free memory): fewer queries per launch beyond it

// The bound's sample: S stored rows, every stride-th position (cluster order: every list contributes its share).  The scan then
// keeps about n topk / S rows per query, so S ~ sqrt(n topk) balances the two steps' exact distances; at least 2 topk rows, at most
// all.  With a filter the stride shrinks by its density so that about S ADMITTED rows are sampled.  asked: rq_exact_params_t.seed_probe
// (sample rows per topk; 0 = automatic).
static uint32_t exact_sample_stride(uint64_t n, uint64_t admitted, uint32_t topk, uint32_t asked, uint32_t *sample_rows) {
    uint64_t S = asked ? (uint64_t)asked * topk : (uint64_t)std::ceil(std::sqrt((double)std::max<uint64_t>(admitted, 1) * topk));
    S = std::min<uint64_t>(std::max<uint64_t>(S, 2ull * topk), std::max<uint64_t>(admitted, 1));
    if (asked) S = std::min<uint64_t>((uint64_t)asked * topk, std::max<uint64_t>(admitted, 1));
    const uint64_t positions = std::min<uint64_t>(n, (S * n + std::max<uint64_t>(admitted, 1) - 1) / std::max<uint64_t>(admitted, 1));
    const uint64_t stride = std::max<uint64_t>(1, n / std::max<uint64_t>(positions, 1));
    *sample_rows = (uint32_t)((n + stride - 1) / stride);
    return (uint32_t)stride;
}

// The checks of both entries, before anything is allocated; *prm = the caller's parameters (zero = automatic where there are none).
static rq_status exact_validate(const rq_index *idx, bool args_null, uint32_t len, uint32_t topk, const rq_filter *filter,
                                const rq_exact_params_t *params, rq_exact_params_t *prm) {
    RQC(validate_call(idx, args_null, len, 1u, topk, filter));
    *prm = rq_exact_params_t{};
    if (params) {
        if (params->struct_size < 4) return fail(RQ_ERR_INVALID, "struct_size is not set (set it to sizeof(rq_exact_params_t) before the call)");
        memcpy(prm, params, std::min<size_t>(params->struct_size, sizeof *prm));
    }
    if (prm->flags & ~(RQ_EXACT_NO_SEED | RQ_EXACT_NO_PREFILTER)) return fail(RQ_ERR_INVALID, "unknown bit in rq_exact_params_t.flags");
    if (idx->base_host || idx->n_dev < idx->n)
        return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are tiered (HBM + pinned host memory): the exact search reads every row from HBM");
    if (idx->split_rows) return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are stored as split rows: the exact search reads plain rows");
    return RQ_OK;
}

static rq_status exact_search_device(const rq_index *idx, const rq_filter *filter, const float *d_q, uint32_t nq, uint32_t len, uint32_t topk,
                                     const rq_exact_params_t *params, float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n) {
    g_exact_stats = rq_exact_stats_t{};
    g_exact_stats.struct_size = sizeof(rq_exact_stats_t);
    rq_exact_params_t prm{};
    RQC(exact_validate(idx, !d_out_dist || !d_out_id || !d_out_n || (nq && !d_q), len, topk, filter, params, &prm));
    if (nq == 0) return RQ_OK;
    RQC(exact_ensure_attributes());
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
    if (idx->n == 0) {  // (nothing to scan: a launch of no blocks is not a launch)
        HIPC(hipMemsetAsync(d_out_n, 0, (size_t)nq * 4, st));
        HIPC(hipStreamSynchronize(st));
        return RQ_OK;
    }
    const bool prefilter = !(prm.flags & RQ_EXACT_NO_PREFILTER) && exact_scan_subtiles(idx->dim) != 0;
    const bool no_seed = (prm.flags & RQ_EXACT_NO_SEED) || !prefilter;  // (without the pre-filter a bound saves nothing: none is made)
    const uint64_t admitted = filter ? filter->rows : idx->n;
    uint32_t sample_rows = 0;
    const uint32_t stride = exact_sample_stride(idx->n, admitted, topk, prm.seed_probe, &sample_rows);
    const uint32_t cap_max = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(admitted, idx->n));  // (a query keeps at most every admitted row)
    // the capacity earlier calls on this index / filter learnt (as the query's survivor capacity is remembered); the test hook overrides it
    std::atomic<uint32_t> &cap_hint = filter ? const_cast<rq_filter *>(filter)->exact_cap_hint : const_cast<rq_index *>(idx)->exact_cap_hint;
    uint32_t cap = std::min<uint32_t>(cap_max, prm.cand_per_query ? prm.cand_per_query : std::max<uint32_t>(std::max<uint32_t>(4 * topk, 1024u), cap_hint.load()));
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const uint64_t slot_budget = std::max<uint64_t>(64ull << 20, std::min<uint64_t>(RQ_EXACT_SLOT_BUDGET, free_b / 3));
    rq_exact_stats_t &stats = g_exact_stats;
    stats.seed_probe = no_seed ? 0u : sample_rows;
    stats.scan_subtiles = prefilter ? exact_scan_subtiles(idx->dim) : 0u;  // (the decision launch_exact_scan takes for the counted launches)

    DevBuf<float> seed_dist, qscratch, thr, qn2, qsn;
    DevBuf<uint32_t> seed_id, seed_n, cand;
    DevBuf<unsigned int> cnt, unfilled;
    DevBuf<uint16_t> qbf;
    DevBuf<unsigned long long> keys;
    std::vector<unsigned int> h_cnt;
    RQC(unfilled.alloc(1));
    HIPC(hipMemsetAsync(unfilled.p, 0, 4, st));
    // scan (+ capacity check), exact distances and selection of one launch; *over: the scan's candidates did not fit (nothing else ran)
    auto run = [&](ExactArgs &a, bool pre, bool counted, bool *over, uint64_t *total) -> rq_status {
        RQC(cnt.ensure(a.nq));
        RQC(cand.ensure((uint64_t)a.nq * a.cap));
        RQC(keys.ensure((uint64_t)a.nq * a.cap));
        a.cand = cand.p, a.cnt = cnt.p, a.keys = keys.p;
        HIPC(hipMemsetAsync(cnt.p, 0, (size_t)a.nq * 4, st));
        HIPC(hipEventRecord(g.ev[0], st));
        launch_exact_scan(a, pre, st);
        HIPC(hipEventRecord(g.ev[1], st));
        h_cnt.resize(a.nq);
        HIPC(hipMemcpyAsync(h_cnt.data(), cnt.p, (size_t)a.nq * 4, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        HIPC(hipGetLastError());
        float ms = 0.0f;
        HIPC(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
        if (counted) stats.ms_scan += ms, stats.row_bytes_read += idx->n * idx->row_bytes(), stats.scan_launches += 1;
        else stats.ms_seed += ms;
        unsigned int most = 0;
        *total = 0;
        for (unsigned int c : h_cnt) *total += c, most = std::max(most, c);
        *over = most > a.cap;
        if (*over) {  // again, with the capacity the count has learnt
            cap = (uint32_t)std::min<uint64_t>(cap_max, ((uint64_t)most + most / 8 + 255) / 256 * 256);
            return RQ_OK;
        }
        HIPC(hipEventRecord(g.ev[0], st));
        launch_exact_dist(a, st);
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
    uint32_t bound_g0 = 0xFFFFFFFFu, bound_step = 0;  // the queries whose bounds thr holds (a repeated launch of the same queries keeps them)
    for (uint32_t q0 = 0; q0 < nq; q0 += RQ_EXACT_CHUNK) {
        const uint32_t m = std::min<uint32_t>(RQ_EXACT_CHUNK, nq - q0);
        bound_g0 = 0xFFFFFFFFu;
        const float *raw = d_q + (uint64_t)q0 * len;
        const float *qp = nullptr;  // q': transformed, padded
        RQC(transform_queries(idx, raw, m, len, /*want_padded=*/true, qscratch, st, &qp));
        RQC(thr.ensure(m));
        for (uint32_t g0 = 0; g0 < m;) {
            // the queries [g0, g0 + step): (1) the bound from the sample, (2) one scan launch, (3) the exact distances and the selection;
            // (2) is run again when a query's candidates did not fit its slots
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
            if (!no_seed && !have_bound) {  // (1): every sampled admitted row of every query, exactly; the topk-th smallest is the bound
                RQC(seed_dist.ensure((uint64_t)step * topk));
                RQC(seed_id.ensure((uint64_t)step * topk));
                RQC(seed_n.ensure(step));
                launch_exact_thr(nullptr, nullptr, step, topk, a.thr, nullptr, st);  // (the sample's own pass runs without a bound)
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

static rq_status exact_search_host(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len, uint32_t topk,
                                   const rq_exact_params_t *params, float *out_dist, uint32_t *out_id, uint32_t *out_n) {
    rq_exact_params_t prm{};
    RQC(exact_validate(idx, !out_dist || !out_id || !out_n || (nq && !queries), len, topk, filter, params, &prm));
    const uint64_t cells = (uint64_t)nq * topk;
    DevBuf<float> dq, dd;
    DevBuf<uint32_t> di, dn;
    RQC(dq.upload(queries, (uint64_t)nq * len));
    RQC(dd.upload(out_dist, cells));  // the caller's arrays travel both ways: slots past out_n stay as they were
    RQC(di.upload(out_id, cells));
    RQC(dn.alloc(nq));
    RQC(exact_search_device(idx, filter, dq.p, nq, len, topk, params, dd.p, di.p, dn.p));
    if (cells) {
        HIPC(hipMemcpy(out_dist, dd.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out_id, di.p, cells * 4, hipMemcpyDeviceToHost));
    }
    if (nq) HIPC(hipMemcpy(out_n, dn.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}
