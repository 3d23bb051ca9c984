// host_diverse.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  Diverse search (kernels_diverse.h): rq_query_batch_diverse, rq_exact_search_diverse
// and rq_diversify_results, all of them diverse_device -- group_device's pattern (host_group.h): the source call's driver at
// topk = fetch into workspace buffers, then one selection launch on the by-id call's stream; no result travels to the host in
// between.  Every entry reads the index and writes nothing of it.
#pragma once

static thread_local rq_diverse_stats_t g_diverse_stats;  // the calling thread's last diverse call (rq_last_diverse_stats)

// What a diverse call writes (fetched: nullable); what it reads is a GroupIn (host_group.h: the same three sources).
struct DiverseOut {
    float *dist = nullptr;
    uint32_t *id = nullptr;
    float *div = nullptr;
    uint32_t *n = nullptr, *fetched = nullptr;
};

// The checks that need no device, in the order the header gives: nulls, the struct, lambda, the limits.
static rq_status diverse_checks(const rq_index *idx, const GroupIn &in, uint32_t nq, const rq_diverse_params_t *dp, const DiverseOut &out) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    const bool src_null = in.src == GROUP_SRC_RESULTS ? (!in.dist || !in.id || !in.cnt) : !in.q;
    if (!dp || !out.dist || !out.id || !out.div || !out.n || (nq && src_null)) return fail(RQ_ERR_INVALID, "null argument");
    if (dp->struct_size != sizeof(rq_diverse_params_t))
        return fail(RQ_ERR_INVALID, "struct_size is not sizeof(rq_diverse_params_t) (set it before the call)");
    if (dp->flags) return fail(RQ_ERR_INVALID, "unknown bit in rq_diverse_params_t.flags");
    if (!(dp->lambda >= 0.0f && dp->lambda <= 1.0f)) return fail(RQ_ERR_INVALID, "lambda must be in [0, 1]");
    if (dp->topk == 0 || dp->topk > dp->fetch || dp->fetch > RQ_MAX_TOPK)
        return fail(RQ_ERR_UNSUPPORTED, "topk must be at least 1 and topk <= fetch <= 2048");
    return RQ_OK;
}

template <int MODE>
static void launch_diverse_mode(const DiverseArgs &da, hipStream_t st) {
    const size_t row = (size_t)da.dim * 4;
    if (da.fetch <= RQ_DIVERSE_WAVE_MAX) diverse_select_kernel<64, 64, MODE><<<da.nq, 64, row, st>>>(da);
    else if (da.fetch <= 256) diverse_select_kernel<256, 256, MODE><<<da.nq, 256, row, st>>>(da);
    else diverse_select_kernel<2048, 256, MODE><<<da.nq, 256, row, st>>>(da);
}
// (the row kind as launch_fetch picks the gather's mode)
static void launch_diverse_select(const rq_index *idx, const DiverseArgs &da, hipStream_t st) {
    if (idx->base_host != nullptr || idx->split_rows) launch_diverse_mode<FETCH_COLD>(da, st);
    else if (idx->rows.kind() == ROW_KIND_BYTE) launch_diverse_mode<FETCH_BYTE>(da, st);
    else if (idx->rows.kind() == ROW_KIND_HALF) launch_diverse_mode<FETCH_HALF>(da, st);
    else launch_diverse_mode<FETCH_F32>(da, st);
}

static rq_status diverse_device(const rq_index *idx, const GroupIn &in, uint32_t nq, const rq_diverse_params_t *dp, const DiverseOut &out) {
    RQC(diverse_checks(idx, in, nq, dp, out));
    const uint32_t fetch = dp->fetch;
    const rq_filter *filter = in.src == GROUP_SRC_RESULTS ? nullptr : live_or(idx, in.filter);
    // the source call's refusals at topk = fetch, before anything is made (the source checks them again)
    if (in.src == GROUP_SRC_EXACT) {
        rq_exact_params_t prm{};
        RQC(exact_validate(idx, false, in.len, fetch, filter, in.exact, &prm));
    } else if (in.src == GROUP_SRC_QUERY) {
        RQC(validate_call(idx, false, in.len, in.probe, fetch, filter));
    }
    if (idx->dim > RQ_DIVERSE_MAX_DIM) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
    if (nq >= (1u << 31)) return fail(RQ_ERR_UNSUPPORTED, "nq must be below 2^31");
    ByIdCall c;
    RQC(c.begin(idx));
    g_diverse_stats = rq_diverse_stats_t{};
    g_diverse_stats.struct_size = sizeof(rq_diverse_stats_t);
    g_diverse_stats.fetch = fetch, g_diverse_stats.directory_built = g_by_id_stats.built;
    if (nq == 0) return RQ_OK;
    Workspace &ws = *c.ws;
    DiverseArgs da{};
    rq_status qs = RQ_OK;
    if (in.src == GROUP_SRC_RESULTS) {
        da.dist = in.dist, da.id = in.id, da.cnt = in.cnt;
    } else {
        RQC(ws.id_res_dist.ensure((uint64_t)nq * fetch));
        RQC(ws.id_res_id.ensure((uint64_t)nq * fetch));
        RQC(ws.id_res_n.ensure(nq));
        PhaseClock clk;  // (the drivers run on streams of their own and return with their outputs complete)
        if (in.src == GROUP_SRC_EXACT)
            qs = exact_search_device(idx, filter, in.q, nq, in.len, fetch, in.exact, ws.id_res_dist.p, ws.id_res_id.p, ws.id_res_n.p);
        else
            qs = query_device(QueryCall{c.idx, filter, in.len, in.probe, fetch, in.heuristic != 0, QueryIO{in.q, ws.id_res_dist.p, ws.id_res_id.p, ws.id_res_n.p}},
                              nq, nullptr);
        if (qs != RQ_OK && qs != RQ_ERR_EMPTY) return qs;
        g_diverse_stats.ms_source = clk.lap();
        da.dist = ws.id_res_dist.p, da.id = ws.id_res_id.p, da.cnt = ws.id_res_n.p;
    }
    da.nq = nq, da.fetch = fetch, da.topk = dp->topk, da.dim = idx->dim;
    da.lambda = dp->lambda, da.mu = 1.0f - dp->lambda;
    da.dir.rows = idx->n, da.dir.top = c.dir->top;
    da.dir.dense = c.dir->hashed ? nullptr : c.dir->dense.p, da.dir.slots = c.dir->slots.p, da.dir.bits = c.dir->bits;
    da.dir.live = idx->live ? idx->live->pos_bits.p : nullptr;  // (read at call time, as ByIdCall::lookup does)
    da.base = idx->view();
    da.out_dist = out.dist, da.out_id = out.id, da.out_div = out.div;
    da.out_n = out.n, da.out_fetched = in.src == GROUP_SRC_RESULTS ? nullptr : out.fetched;
    RQC(ws.id_found.ensure(5));
    da.stats = ws.id_found.p;
    HIPC(hipMemsetAsync(ws.id_found.p, 0, 40, c.st));
    HIPC(hipEventRecord(c.ev[0], c.st));
    launch_diverse_select(idx, da, c.st);
    HIPC(hipEventRecord(c.ev[1], c.st));
    HIPC(hipMemcpyAsync(ws.h_totals, ws.id_found.p, 40, hipMemcpyDeviceToHost, c.st));
    HIPC(hipStreamSynchronize(c.st));
    HIPC(hipGetLastError());
    (void)hipEventElapsedTime(&g_diverse_stats.ms_select, c.ev[0], c.ev[1]);
    g_diverse_stats.candidates = ws.h_totals[0], g_diverse_stats.absent = ws.h_totals[1], g_diverse_stats.skipped = ws.h_totals[2];
    g_diverse_stats.taken = ws.h_totals[3], g_diverse_stats.pair_distances = ws.h_totals[4];
    return qs;
}

// The host-pointer forms: the inputs go up, diverse_device runs, the outputs come down.
static rq_status diverse_host(const rq_index *idx, const GroupIn &in, uint32_t nq, const rq_diverse_params_t *dp, const DiverseOut &out) {
    RQC(diverse_checks(idx, in, nq, dp, out));
    RQC(ensure_device());
    const uint64_t cells = (uint64_t)nq * dp->topk, src_cells = (uint64_t)nq * dp->fetch;
    DevBuf<float> d_q, d_sd, d_od, d_ov;
    DevBuf<uint32_t> d_si, d_sn, d_oi, d_n, d_f;
    GroupIn din = in;
    if (in.src == GROUP_SRC_RESULTS) {
        RQC(d_sd.upload(in.dist, src_cells));
        RQC(d_si.upload(in.id, src_cells));
        RQC(d_sn.upload(in.cnt, nq));
        din.dist = d_sd.p, din.id = d_si.p, din.cnt = d_sn.p;
    } else {
        RQC(d_q.upload(in.q, (uint64_t)nq * in.len));
        din.q = d_q.p;
    }
    RQC(d_od.alloc(cells));
    RQC(d_oi.alloc(cells));
    RQC(d_ov.alloc(cells));
    RQC(d_n.alloc(nq));
    RQC(d_f.alloc(nq));
    const rq_status s = diverse_device(idx, din, nq, dp, DiverseOut{d_od.p, d_oi.p, d_ov.p, d_n.p, d_f.p});
    if (s != RQ_OK && s != RQ_ERR_EMPTY) return s;
    if (nq) {
        HIPC(hipMemcpy(out.dist, d_od.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.id, d_oi.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.div, d_ov.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.n, d_n.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
        if (out.fetched && in.src != GROUP_SRC_RESULTS) HIPC(hipMemcpy(out.fetched, d_f.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    }
    return s;
}
