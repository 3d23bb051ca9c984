// host_directory.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  Rows by id (kernels_directory.h): the id directory of an index and the entries on
// top of it -- rq_locate, rq_fetch_rows, rq_fetch_stored, rq_pair_distances, rq_neighbours_of[_exact], rq_last_by_id_stats.  Every
// entry reads the index and writes nothing of it: the directory (under its own mutex) and the buffers of a pooled workspace are all
// that a call touches.
#pragma once

static thread_local rq_by_id_stats_t g_by_id_stats;  // the calling thread's last by-id call (rq_last_by_id_stats)

// ---- the directory -------------------------------------------------------------------------------------------------------------------
// The rule between the two forms, and the hash table's capacity: functions of (top, n) alone (tests/by_id_model.py restates both).
static bool directory_is_dense(uint64_t top, uint64_t n) { return top <= 4 * n + 65536; }
static uint32_t directory_hash_bits(uint64_t n) {  // log2 of the power of two >= max(2 n, 16); the hash form has n < 2^30
    uint32_t bits = 4;
    while ((1ull << bits) < 2 * n) ++bits;
    return bits;
}

// The directory of idx's current layout: the one it has, or a new one (one scan of the ids for `top`, one pass that fills the form the
// rule picks).  *built (nullable): this call made it.
static rq_status ensure_directory(const rq_index *cidx, const IdDirectory **out, bool *built) {
    rq_index *idx = const_cast<rq_index *>(cidx);
    std::lock_guard<std::mutex> g(idx->dir_mu);
    if (built) *built = false;
    if (idx->dir && idx->dir->generation == idx->generation) {
        *out = idx->dir.get();
        return RQ_OK;
    }
    idx->dir.reset();
    PhaseClock clk;
    std::unique_ptr<IdDirectory> d(new IdDirectory());
    const uint64_t n = idx->n;
    uint64_t hits = 0;
    RQC(scan_ids(idx, nullptr, 0, &d->top, &hits));
    d->generation = idx->generation;
    d->hashed = !directory_is_dense(d->top, n);
    DevBuf<unsigned int> counters;  // {longest chain, rows that found no slot}
    RQC(counters.alloc(2));
    HIPC(hipMemset(counters.p, 0, 8));
    if (d->hashed) {
        d->bits = directory_hash_bits(n);
        if (d->bits > 31) return fail(RQ_ERR_UNSUPPORTED, "internal: id directory of more than 2^31 slots");
        RQC(d->slots.alloc((size_t)1 << d->bits));
        d->bytes = (uint64_t)8 << d->bits;
        HIPC(hipMemset(d->slots.p, 0xFF, d->bytes));
    } else {
        RQC(d->dense.alloc(d->top));
        d->bytes = d->top * 4;
        if (d->top) HIPC(hipMemset(d->dense.p, 0xFF, d->bytes));
    }
    if (n)
        directory_build_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(n, 256), 4096), 256>>>(idx->map_ids.p, n, d->hashed ? nullptr : d->dense.p,
                                                                                               d->slots.p, d->bits, counters.p, counters.p + 1);
    unsigned int h[2] = {0, 0};
    HIPC(hipMemcpy(h, counters.p, 8, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    if (h[1]) return fail(RQ_ERR_HIP, "internal: " + std::to_string(h[1]) + " rows found no slot in the id directory");
    d->longest_chain = h[0];
    d->ms_build = clk.lap();
    if (built) *built = true;
    idx->dir = std::move(d);
    *out = idx->dir.get();
    return RQ_OK;
}

// ---- what every by-id call starts with -----------------------------------------------------------------------------------------------
// A pooled workspace (its stream, its id_* buffers), the directory, and a pair of events each around the lookup and the gather.
struct ByIdCall {
    rq_index *idx = nullptr;
    const IdDirectory *dir = nullptr;
    Workspace *ws = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // lookup begin / end, gather begin / end
    ByIdCall() = default;
    ByIdCall(const ByIdCall &) = delete;
    ByIdCall &operator=(const ByIdCall &) = delete;
    ~ByIdCall() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (ws) ws_release(idx, ws);
    }
    rq_status begin(const rq_index *cidx) {
        RQC(ensure_device());
        idx = const_cast<rq_index *>(cidx);
        bool built = false;
        RQC(ensure_directory(idx, &dir, &built));
        g_by_id_stats = rq_by_id_stats_t{};
        g_by_id_stats.struct_size = sizeof(rq_by_id_stats_t);
        g_by_id_stats.form = dir->hashed ? RQ_DIRECTORY_HASH : RQ_DIRECTORY_DENSE;
        g_by_id_stats.directory_bytes = dir->bytes, g_by_id_stats.ms_build = dir->ms_build, g_by_id_stats.longest_chain = dir->longest_chain;
        g_by_id_stats.built = built ? 1u : 0u;
        ws = ws_acquire(idx);
        RQC(ws_ensure_stream(*ws));
        st = ws->stream;
        for (hipEvent_t &e : ev) HIPC(hipEventCreate(&e));
        return RQ_OK;
    }
    // ids (device, m) -> pos (device, m); the call's found / absent counts arrive with finish()
    rq_status lookup(const uint32_t *d_ids, uint64_t m, uint32_t *d_pos) {
        RQC(ws->id_found.ensure(1));
        HIPC(hipMemsetAsync(ws->id_found.p, 0, 8, st));
        HIPC(hipEventRecord(ev[0], st));
        const uint32_t *live = idx->live ? idx->live->pos_bits.p : nullptr;  // (read at call time: the removal epoch is not part of the directory)
        directory_lookup_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(m, 256), 8192), 256, 0, st>>>(
            d_ids, m, dir->top, dir->hashed ? nullptr : dir->dense.p, dir->slots.p, dir->bits, live, d_pos, ws->id_found.p);
        HIPC(hipEventRecord(ev[1], st));
        HIPC(hipMemcpyAsync(ws->h_totals, ws->id_found.p, 8, hipMemcpyDeviceToHost, st));
        asked = m;
        return RQ_OK;
    }
    // waits for the stream and completes the stats
    rq_status finish() {
        HIPC(hipStreamSynchronize(st));
        HIPC(hipGetLastError());
        if (asked) {
            g_by_id_stats.found = ws->h_totals[0], g_by_id_stats.absent = asked - ws->h_totals[0];
            (void)hipEventElapsedTime(&g_by_id_stats.ms_lookup, ev[0], ev[1]);
        }
        if (gathered) {
            (void)hipEventElapsedTime(&g_by_id_stats.ms_gather, ev[2], ev[3]);
            // as rq_mutate_stats_t.gather_bytes counts: every moved row read once and written once, and the map (here: the positions);
            // an absent id's destination is written, and its stand-in read is of one cached row
            g_by_id_stats.gather_bytes = g_by_id_stats.found * gather_src_bytes + gathered * (gather_dst_bytes + 4);
        }
        return RQ_OK;
    }
    uint64_t asked = 0, gathered = 0, gather_src_bytes = 0, gather_dst_bytes = 0;
};

// ---- the gather's launch -------------------------------------------------------------------------------------------------------------
template <int MODE, int R>
static void launch_fetch_mode(const uint32_t *d_pos, uint64_t m, const rq_index *idx, uint32_t LP, bool absent_row0, void *d_out, uint32_t *d_found,
                              hipStream_t st) {
    const uint32_t G = LP <= 4 ? 4u : LP <= 8 ? 8u : LP <= 16 ? 16u : LP <= 32 ? 32u : 64u;
    const uint32_t rows_per_block = 4 * R * (64 / G);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ceil_div(m, rows_per_block), 1u << 20);
    const BaseView bv = idx->view();
    uint4 *out = static_cast<uint4 *>(d_out);
    const uint32_t a0 = absent_row0 ? 1u : 0u;
    if constexpr (MODE == FETCH_RAW) {  // (a widened row has at least 16 pieces: only the raw copy meets the narrow sub-groups)
        if (G == 4) return (void)fetch_gather_kernel<MODE, 4, R><<<grid, 256, 0, st>>>(d_pos, m, bv, idx->dim, LP, a0, out, d_found);
        if (G == 8) return (void)fetch_gather_kernel<MODE, 8, R><<<grid, 256, 0, st>>>(d_pos, m, bv, idx->dim, LP, a0, out, d_found);
    }
    if (G <= 16) fetch_gather_kernel<MODE, 16, R><<<grid, 256, 0, st>>>(d_pos, m, bv, idx->dim, LP, a0, out, d_found);
    else if (G == 32) fetch_gather_kernel<MODE, 32, R><<<grid, 256, 0, st>>>(d_pos, m, bv, idx->dim, LP, a0, out, d_found);
    else fetch_gather_kernel<MODE, 64, R><<<grid, 256, 0, st>>>(d_pos, m, bv, idx->dim, LP, a0, out, d_found);
}
// Rows at d_pos[0 .. m) -> d_out: widened to dim f32 (stored == false) or as stored.  The index has at least one row.  Rows in flight
// per sub-group: 4 of 16-byte loads (merge_gather_kernel's), 8 where a typed row's loads are 8 or 4 bytes.
static void launch_fetch(ByIdCall &c, const uint32_t *d_pos, uint64_t m, bool stored, bool absent_row0, void *d_out, uint32_t *d_found) {
    const rq_index *idx = c.idx;
    const uint32_t dim = idx->dim;
    const bool cold = idx->base_host != nullptr || idx->split_rows;
    const uint32_t LP = stored ? (uint32_t)(idx->row_bytes() / 16) : dim / 4;
    (void)hipEventRecord(c.ev[2], c.st);
    if (stored) launch_fetch_mode<FETCH_RAW, 4>(d_pos, m, idx, LP, absent_row0, d_out, d_found, c.st);
    else if (cold) launch_fetch_mode<FETCH_COLD, 4>(d_pos, m, idx, LP, absent_row0, d_out, d_found, c.st);
    else if (idx->rows.kind() == ROW_KIND_BYTE) launch_fetch_mode<FETCH_BYTE, 8>(d_pos, m, idx, LP, absent_row0, d_out, d_found, c.st);
    else if (idx->rows.kind() == ROW_KIND_HALF) launch_fetch_mode<FETCH_HALF, 8>(d_pos, m, idx, LP, absent_row0, d_out, d_found, c.st);
    else launch_fetch_mode<FETCH_F32, 4>(d_pos, m, idx, LP, absent_row0, d_out, d_found, c.st);
    (void)hipEventRecord(c.ev[3], c.st);
    c.gathered = m, c.gather_src_bytes = idx->row_bytes(), c.gather_dst_bytes = (uint64_t)LP * 16;
}

static rq_status by_id_args(const rq_index *idx, bool args_null) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    if (args_null) return fail(RQ_ERR_INVALID, "null argument");
    return RQ_OK;
}
static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- rq_locate -----------------------------------------------------------------------------------------------------------------------
static rq_status locate_device(const rq_index *idx, const uint32_t *d_ids, uint64_t m, uint32_t *d_out_pos) {
    RQC(by_id_args(idx, m && (!d_ids || !d_out_pos)));
    ByIdCall c;
    RQC(c.begin(idx));
    if (m == 0) return RQ_OK;
    RQC(c.lookup(d_ids, m, d_out_pos));
    return c.finish();
}
static rq_status locate_host(const rq_index *idx, const uint32_t *ids, uint64_t m, uint32_t *out_pos) {
    RQC(by_id_args(idx, m && (!ids || !out_pos)));
    RQC(ensure_device());
    DevBuf<uint32_t> d_ids, d_pos;
    RQC(d_ids.upload(ids, m));
    RQC(d_pos.alloc(m));
    RQC(locate_device(idx, d_ids.p, m, d_pos.p));
    if (m) HIPC(hipMemcpy(out_pos, d_pos.p, m * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

// ---- rq_fetch_rows / rq_fetch_stored ---------------------------------------------------------------------------------------------------
static rq_status fetch_checks(const rq_index *idx, bool stored) {
    if (stored && !idx->rows.typed()) return fail(RQ_ERR_INVALID, "rq_fetch_stored: this index stores f32 rows (rq_fetch_rows)");
    return RQ_OK;
}
static rq_status fetch_device(const rq_index *idx, const uint32_t *d_ids, uint64_t m, bool stored, void *d_out_rows, uint32_t *d_out_found) {
    RQC(by_id_args(idx, m && (!d_ids || !d_out_rows)));
    RQC(fetch_checks(idx, stored));
    if (!aligned16(d_out_rows)) return fail(RQ_ERR_INVALID, "the row output must be 16-byte aligned");
    ByIdCall c;
    RQC(c.begin(idx));
    if (m == 0) return RQ_OK;
    if (idx->n == 0) {  // every id is absent, and there is no row to stand in for a load
        HIPC(hipMemsetAsync(d_out_rows, 0, m * (stored ? idx->row_bytes() : (size_t)idx->dim * 4), c.st));
        if (d_out_found) HIPC(hipMemsetAsync(d_out_found, 0, m * 4, c.st));
        g_by_id_stats.absent = m;
        HIPC(hipStreamSynchronize(c.st));
        return RQ_OK;
    }
    RQC(c.ws->id_pos.ensure(m));
    RQC(c.lookup(d_ids, m, c.ws->id_pos.p));
    launch_fetch(c, c.ws->id_pos.p, m, stored, false, d_out_rows, d_out_found);
    return c.finish();
}
static rq_status fetch_host(const rq_index *idx, const uint32_t *ids, uint64_t m, bool stored, void *out_rows, uint32_t *out_found) {
    RQC(by_id_args(idx, m && (!ids || !out_rows)));
    RQC(fetch_checks(idx, stored));
    RQC(ensure_device());
    const size_t row = stored ? idx->row_bytes() : (size_t)idx->dim * 4;
    DevBuf<uint32_t> d_ids, d_found;
    DevBuf<uint8_t> d_rows;
    RQC(d_ids.upload(ids, m));
    RQC(d_found.alloc(m));
    RQC(d_rows.alloc(m * row));
    RQC(fetch_device(idx, d_ids.p, m, stored, d_rows.p, d_found.p));
    if (m) HIPC(hipMemcpy(out_rows, d_rows.p, m * row, hipMemcpyDeviceToHost));
    if (m && out_found) HIPC(hipMemcpy(out_found, d_found.p, m * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

// ---- rq_pair_distances ---------------------------------------------------------------------------------------------------------------
static rq_status pair_distances_device(const rq_index *idx, const float *d_q, uint32_t nq, uint32_t len, const uint32_t *d_ids, uint32_t c_ids,
                                       float *d_out) {
    const uint64_t cells = (uint64_t)nq * c_ids;
    RQC(by_id_args(idx, cells && (!d_q || !d_ids || !d_out)));
    RQC(raw_len_check(idx, "query", len));
    if (idx->dim > 4096) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
    ByIdCall c;
    RQC(c.begin(idx));
    if (cells == 0) return RQ_OK;
    if (idx->n == 0) {
        fill_f32_kernel<<<ceil_div(cells, 256), 256, 0, c.st>>>(d_out, __builtin_inff(), cells);
        g_by_id_stats.absent = cells;
        HIPC(hipStreamSynchronize(c.st));
        return RQ_OK;
    }
    RQC(c.ws->id_pos.ensure(cells));
    RQC(c.lookup(d_ids, cells, c.ws->id_pos.p));
    const float *qp;  // the prepared queries: transformed and padded, as the rerank of a pass sees them
    RQC(transform_queries(idx, d_q, nq, len, /*want_padded=*/true, c.ws->qpad, c.st, &qp));
    pair_distance_kernel<<<nq, 256, (size_t)idx->dim * 4, c.st>>>(qp, c.ws->id_pos.p, c_ids, idx->view(), idx->dim, d_out);
    return c.finish();
}
static rq_status pair_distances_host(const rq_index *idx, const float *q, uint32_t nq, uint32_t len, const uint32_t *ids, uint32_t c_ids, float *out) {
    const uint64_t cells = (uint64_t)nq * c_ids;
    RQC(by_id_args(idx, cells && (!q || !ids || !out)));
    RQC(ensure_device());
    DevBuf<float> d_q, d_out;
    DevBuf<uint32_t> d_ids;
    RQC(d_q.upload(q, cells ? (uint64_t)nq * len : 0));
    RQC(d_ids.upload(ids, cells));
    RQC(d_out.alloc(cells));
    RQC(pair_distances_device(idx, d_q.p, nq, len, d_ids.p, c_ids, d_out.p));
    if (cells) HIPC(hipMemcpy(out, d_out.p, cells * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

// ---- rq_neighbours_of / rq_neighbours_of_exact -------------------------------------------------------------------------------------------
// lookup -> gather into the query buffer -> the plain entry's driver at topk + 1 -> drop_self_kernel; no data comes back to the host
// in between (one wait for the gather's stream: the drivers run on streams of their own).  exact: rq_exact_search's driver in place
// of the approximate one.
static rq_status neighbours_device(const rq_index *idx, const uint32_t *d_ids, uint32_t m, bool exact, uint32_t probe, uint32_t topk, int heuristic,
                                   const rq_filter *filter, const rq_exact_params_t *params, float *d_out_dist, uint32_t *d_out_ids,
                                   uint32_t *d_out_found) {
    RQC(by_id_args(idx, m && (!d_ids || !d_out_dist || !d_out_ids || !d_out_found)));
    const uint32_t dim = idx->dim, L = idx->metric.id == RQ_METRIC_IP ? idx->metric.d : dim, w = topk + 1;
    filter = live_or(idx, filter);
    // the plain entry's refusals at topk + 1, before anything is made (the plain call below checks them again)
    if (topk == 0 || topk == 0xFFFFFFFFu) return fail(RQ_ERR_UNSUPPORTED, "topk must be in [1, 2047] (the plain call runs at topk + 1)");
    if (exact) {
        rq_exact_params_t prm{};
        RQC(exact_validate(idx, false, L, w, filter, params, &prm));
    } else {
        RQC(validate_call(idx, false, L, probe, w, filter));
    }
    ByIdCall c;
    RQC(c.begin(idx));
    if (m == 0) return RQ_OK;
    Workspace &ws = *c.ws;
    RQC(ws.id_pos.ensure(m));
    RQC(ws.id_rows.ensure((uint64_t)m * dim));
    RQC(ws.id_res_dist.ensure((uint64_t)m * w));
    RQC(ws.id_res_id.ensure((uint64_t)m * w));
    RQC(ws.id_res_n.ensure(m));
    rq_status qs = RQ_OK;
    if (idx->n == 0) {  // nothing stored: every id is absent
        HIPC(hipMemsetAsync(ws.id_pos.p, 0xFF, (size_t)m * 4, c.st));
        HIPC(hipMemsetAsync(ws.id_res_n.p, 0, (size_t)m * 4, c.st));
        g_by_id_stats.absent = m;
    } else {
        RQC(c.lookup(d_ids, m, ws.id_pos.p));
        launch_fetch(c, ws.id_pos.p, m, false, /*absent_row0=*/true, ws.id_rows.p, nullptr);
        const float *d_q = ws.id_rows.p;
        if (L != dim) {  // an inner-product index's queries have its d floats: the augmented coordinate and the padding are cut off
            RQC(ws.id_rows_raw.ensure((uint64_t)m * L));
            unpad_rows_kernel<<<ceil_div((uint64_t)m * L, 256), 256, 0, c.st>>>(ws.id_rows.p, ws.id_rows_raw.p, m, dim, L);
            d_q = ws.id_rows_raw.p;
        }
        RQC(c.finish());  // (the drivers run on streams of their own)
        if (exact) qs = exact_search_device(idx, filter, d_q, m, L, w, params, ws.id_res_dist.p, ws.id_res_id.p, ws.id_res_n.p);
        else
            qs = query_device(QueryCall{c.idx, filter, L, probe, w, heuristic != 0, QueryIO{d_q, ws.id_res_dist.p, ws.id_res_id.p, ws.id_res_n.p}}, m, nullptr);
        if (qs != RQ_OK && qs != RQ_ERR_EMPTY) return qs;
    }
    drop_self_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(m, 4), 1u << 16), 256, 0, c.st>>>(d_ids, ws.id_pos.p, m, topk, ws.id_res_dist.p, ws.id_res_id.p,
                                                                                           ws.id_res_n.p, d_out_dist, d_out_ids, d_out_found);
    HIPC(hipStreamSynchronize(c.st));
    HIPC(hipGetLastError());
    return qs;
}
static rq_status neighbours_host(const rq_index *idx, const uint32_t *ids, uint32_t m, bool exact, uint32_t probe, uint32_t topk, int heuristic,
                                 const rq_filter *filter, const rq_exact_params_t *params, float *out_dist, uint32_t *out_ids, uint32_t *out_found) {
    RQC(by_id_args(idx, m && (!ids || !out_dist || !out_ids || !out_found)));
    RQC(ensure_device());
    const uint64_t cells = (uint64_t)m * topk;
    DevBuf<uint32_t> d_ids, d_oid, d_found;
    DevBuf<float> d_od;
    RQC(d_ids.upload(ids, m));
    RQC(d_od.alloc(cells));
    RQC(d_oid.alloc(cells));
    RQC(d_found.alloc(m));
    const rq_status s = neighbours_device(idx, d_ids.p, m, exact, probe, topk, heuristic, filter, params, d_od.p, d_oid.p, d_found.p);
    if (s != RQ_OK && s != RQ_ERR_EMPTY) return s;
    if (cells) {
        HIPC(hipMemcpy(out_dist, d_od.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out_ids, d_oid.p, cells * 4, hipMemcpyDeviceToHost));
    }
    if (m) HIPC(hipMemcpy(out_found, d_found.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    return s;
}
