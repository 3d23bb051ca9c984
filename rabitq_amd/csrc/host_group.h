// host_group.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  Grouped search (kernels_group.h): rq_query_batch_grouped, rq_exact_search_grouped
// and rq_group_results, all of them group_device -- the source call's driver at topk = fetch into workspace buffers, then one
// selection launch on the by-id call's stream, in neighbours_device's pattern (host_directory.h): no result travels to the host in
// between.  Every entry reads the index and writes nothing of it.
#pragma once

static thread_local rq_group_stats_t g_group_stats;  // the calling thread's last grouped call (rq_last_group_stats)

enum { GROUP_SRC_QUERY = 0, GROUP_SRC_EXACT = 1, GROUP_SRC_RESULTS = 2 };
// What a grouped call reads besides the index (src decides which fields) ...
struct GroupIn {
    int src = GROUP_SRC_RESULTS;
    const rq_filter *filter = nullptr;  // QUERY, EXACT (nullable)
    const float *q = nullptr;           // QUERY, EXACT: nq x len
    uint32_t len = 0, probe = 1;
    int heuristic = 0;
    const rq_exact_params_t *exact = nullptr;  // EXACT (nullable)
    const float *dist = nullptr;               // RESULTS: the caller's rows, nq x fetch
    const uint32_t *id = nullptr, *cnt = nullptr;
};
// ... and what it writes (fetched: nullable)
struct GroupOut {
    float *dist = nullptr;
    uint32_t *id = nullptr;
    uint64_t *key = nullptr;
    uint32_t *group_n = nullptr, *n = nullptr, *fetched = nullptr;
};

// The checks that need no device, in the order the header gives: nulls, the struct, the limits, the column.
static rq_status group_checks(const rq_index *idx, const GroupIn &in, uint32_t nq, const char *column, const rq_group_params_t *gp, const GroupOut &out,
                              AttrColumn **col) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    const bool src_null = in.src == GROUP_SRC_RESULTS ? (!in.dist || !in.id || !in.cnt) : !in.q;
    if (!column || !gp || !out.dist || !out.id || !out.key || !out.group_n || !out.n || (nq && src_null)) return fail(RQ_ERR_INVALID, "null argument");
    if (gp->struct_size != sizeof(rq_group_params_t))
        return fail(RQ_ERR_INVALID, "struct_size is not sizeof(rq_group_params_t) (set it before the call)");
    if (gp->flags) return fail(RQ_ERR_INVALID, "unknown bit in rq_group_params_t.flags");
    if (gp->topk == 0 || gp->group_size == 0 || gp->fetch > RQ_MAX_TOPK || (uint64_t)gp->topk * gp->group_size > gp->fetch)
        return fail(RQ_ERR_UNSUPPORTED, "topk and group_size must be at least 1 and topk * group_size <= fetch <= 2048");
    RQC(attr_named(idx, column, false, col));
    if ((*col)->type == RQ_ATTR_F32)
        return fail(RQ_ERR_INVALID, std::string("grouping is for integer columns (column ") + column + " is f32: -0 / +0 and NaNs have no agreed equality)");
    return RQ_OK;
}

static void launch_group_select(const GroupArgs &ga, hipStream_t st) {
    if (ga.fetch <= RQ_GROUP_WAVE_MAX) group_select_wave_kernel<<<ceil_div(ga.nq, 4), 256, 0, st>>>(ga);
    else if (ga.fetch <= 256) group_select_block_kernel<256><<<ga.nq, 256, 0, st>>>(ga);
    else group_select_block_kernel<2048><<<ga.nq, 256, 0, st>>>(ga);
}

static rq_status group_device(const rq_index *idx, const GroupIn &in, uint32_t nq, const char *column, const rq_group_params_t *gp, const GroupOut &out) {
    AttrColumn *col = nullptr;
    RQC(group_checks(idx, in, nq, column, gp, out, &col));
    const uint32_t fetch = gp->fetch;
    const rq_filter *filter = in.src == GROUP_SRC_RESULTS ? nullptr : live_or(idx, in.filter);
    // the source call's refusals at topk = fetch, before anything is made (the source checks them again)
    if (in.src == GROUP_SRC_EXACT) {
        rq_exact_params_t prm{};
        RQC(exact_validate(idx, false, in.len, fetch, filter, in.exact, &prm));
    } else if (in.src == GROUP_SRC_QUERY) {
        RQC(validate_call(idx, false, in.len, in.probe, fetch, filter));
    }
    if (nq >= (1u << 31)) return fail(RQ_ERR_UNSUPPORTED, "nq must be below 2^31");
    ByIdCall c;
    RQC(c.begin(idx));
    g_group_stats = rq_group_stats_t{};
    g_group_stats.struct_size = sizeof(rq_group_stats_t);
    g_group_stats.fetch = fetch, g_group_stats.directory_built = g_by_id_stats.built;
    if (nq == 0) return RQ_OK;
    Workspace &ws = *c.ws;
    GroupArgs ga{};
    rq_status qs = RQ_OK;
    if (in.src == GROUP_SRC_RESULTS) {
        ga.dist = in.dist, ga.id = in.id, ga.cnt = in.cnt;
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
        g_group_stats.ms_source = clk.lap();
        ga.dist = ws.id_res_dist.p, ga.id = ws.id_res_id.p, ga.cnt = ws.id_res_n.p;
    }
    ga.nq = nq, ga.fetch = fetch, ga.topk = gp->topk, ga.gsize = gp->group_size;
    ga.rows = idx->n, ga.top = c.dir->top;
    ga.dense = c.dir->hashed ? nullptr : c.dir->dense.p, ga.slots = c.dir->slots.p, ga.bits = c.dir->bits;
    ga.wide = attr_elem(col->type) == 8 ? 1u : 0u;
    ga.live = idx->live ? idx->live->pos_bits.p : nullptr;  // (read at call time, as ByIdCall::lookup does)
    ga.col = reinterpret_cast<const uint32_t *>(col->data.p);
    ga.out_dist = out.dist, ga.out_id = out.id, ga.out_key = reinterpret_cast<unsigned long long *>(out.key);
    ga.out_group_n = out.group_n, ga.out_n = out.n, ga.out_fetched = in.src == GROUP_SRC_RESULTS ? nullptr : out.fetched;
    RQC(ws.id_found.ensure(4));
    ga.stats = ws.id_found.p;
    HIPC(hipMemsetAsync(ws.id_found.p, 0, 32, c.st));
    HIPC(hipEventRecord(c.ev[0], c.st));
    launch_group_select(ga, c.st);
    HIPC(hipEventRecord(c.ev[1], c.st));
    HIPC(hipMemcpyAsync(ws.h_totals, ws.id_found.p, 32, hipMemcpyDeviceToHost, c.st));
    HIPC(hipStreamSynchronize(c.st));
    HIPC(hipGetLastError());
    (void)hipEventElapsedTime(&g_group_stats.ms_group, c.ev[0], c.ev[1]);
    g_group_stats.candidates = ws.h_totals[0], g_group_stats.absent = ws.h_totals[1];
    g_group_stats.kept = ws.h_totals[2], g_group_stats.groups = ws.h_totals[3];
    return qs;
}

// The host-pointer forms: the inputs go up, group_device runs, the outputs come down.
static rq_status group_host(const rq_index *idx, const GroupIn &in, uint32_t nq, const char *column, const rq_group_params_t *gp, const GroupOut &out) {
    AttrColumn *col = nullptr;
    RQC(group_checks(idx, in, nq, column, gp, out, &col));
    RQC(ensure_device());
    const uint64_t groups = (uint64_t)nq * gp->topk, cells = groups * gp->group_size, src_cells = (uint64_t)nq * gp->fetch;
    DevBuf<float> d_q, d_sd, d_od;
    DevBuf<uint32_t> d_si, d_sn, d_oi, d_gn, d_n, d_f;
    DevBuf<uint64_t> d_key;
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
    RQC(d_key.alloc(groups));
    RQC(d_gn.alloc(groups));
    RQC(d_n.alloc(nq));
    RQC(d_f.alloc(nq));
    const rq_status s = group_device(idx, din, nq, column, gp, GroupOut{d_od.p, d_oi.p, d_key.p, d_gn.p, d_n.p, d_f.p});
    if (s != RQ_OK && s != RQ_ERR_EMPTY) return s;
    if (nq) {
        HIPC(hipMemcpy(out.dist, d_od.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.id, d_oi.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.key, d_key.p, groups * 8, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.group_n, d_gn.p, groups * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.n, d_n.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
        if (out.fetched && in.src != GROUP_SRC_RESULTS) HIPC(hipMemcpy(out.fetched, d_f.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    }
    return s;
}
