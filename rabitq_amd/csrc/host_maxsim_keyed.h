// host_maxsim_keyed.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in
// order; they are not stand-alone headers; this one needs host_maxsim.h and host_keyed.h).  Multi-vector search over documents named
// by a column (kernels: kernels_maxsim.h, compiled in inst_maxsim.hip): rq_maxsim_scores_keyed* and
// rq_query_batch_maxsim_keyed*, all four of them maxsim_keyed_device -- maxsim_device's shape (host_maxsim.h) with a postings object
// in the place of the document stride.  Every entry reads the index and the postings and writes nothing of the index.
#pragma once

// What a keyed call reads and writes besides MaxsimIn / MaxsimOut (out.u: the scoring's rows; unused end to end).
struct MaxsimKeyedIn {
    const rq_postings *post = nullptr;
    const rq_attr_value_t *keys = nullptr;  // scores: nq x ncand keys in device memory (the host form: in host memory, for the checks only)
    const uint32_t *segs = nullptr;         // scores, host form: their segments, searched on the host (keyed_segments) and uploaded
    rq_attr_value_t *out_keys = nullptr;    // end to end: nq x topk
};

// The checks that need no device: nulls and the parameters before anything of the index or the postings is read.
static rq_status maxsim_keyed_checks(const rq_index *idx, const MaxsimIn &in, const MaxsimKeyedIn &kin, uint32_t nq, const rq_maxsim_params_t *mp,
                                     const MaxsimOut &out) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    const bool cells = nq && (in.query || in.ncand);
    if (!kin.post || !mp || (cells && (!out.a || (in.query ? !kin.out_keys : !out.u))) || (in.query && !out.n) ||
        (cells && (!in.tokens || (!in.query && !kin.keys && !kin.segs))))
        return fail(RQ_ERR_INVALID, "null argument");
    if (mp->struct_size != sizeof(rq_maxsim_params_t))
        return fail(RQ_ERR_INVALID, "struct_size is not sizeof(rq_maxsim_params_t) (set it before the call)");
    if (mp->flags & ~RQ_MAXSIM_NO_PREFILTER) return fail(RQ_ERR_INVALID, "unknown bit in rq_maxsim_params_t.flags");
    if (mp->doc_stride != 0) return fail(RQ_ERR_INVALID, "doc_stride must be 0 where the postings name the documents");
    if (mp->tokens == 0 || mp->tokens > RQ_MAXSIM_MAX_TOKENS) return fail(RQ_ERR_INVALID, "tokens must be in [1, 256]");
    if (in.query) {
        if ((uint64_t)mp->tokens * mp->fetch > RQ_MAXSIM_MAX_SOURCE || mp->fetch == 0)
            return fail(RQ_ERR_UNSUPPORTED, "fetch must be at least 1 and tokens * fetch <= 2048");
        if (mp->topk == 0 || mp->topk > RQ_MAX_TOPK) return fail(RQ_ERR_UNSUPPORTED, "topk must be in [1, 2048]");
    }
    if ((uint64_t)nq * mp->tokens >= (1ull << 31)) return fail(RQ_ERR_UNSUPPORTED, "nq * tokens must be below 2^31");
    if (kin.post->idx != idx) return fail(RQ_ERR_INVALID, "the postings were made for another index");
    RQC(postings_current(kin.post));
    if (idx->base_host || idx->n_dev < idx->n)
        return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are tiered (HBM + pinned host memory): multi-vector search reads every row from HBM");
    if (idx->split_rows) return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are stored as split rows: multi-vector search reads plain rows");
    if (idx->is_shard) return fail(RQ_ERR_UNSUPPORTED, "a shard holds part of every document: multi-vector search runs on whole indexes");
    if (idx->dim > 4096) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
    return RQ_OK;
}

// The sorted values and the segment starts in device memory: made by the first call, kept on the postings object.
static rq_status postings_device_copy(const rq_postings *cp) {
    rq_postings *p = const_cast<rq_postings *>(cp);
    std::lock_guard<std::mutex> lock(p->dev_mu);
    if (p->dev_ready) return RQ_OK;
    const std::vector<uint32_t> starts(p->starts.begin(), p->starts.end());  // (a position is a u32, so is a count of them)
    RQC(p->d_values.upload(p->values.data(), p->values.size()));
    RQC(p->d_starts.upload(starts.data(), starts.size()));
    p->dev_ready = true;
    return RQ_OK;
}

static rq_status maxsim_keyed_device(const rq_index *idx, const MaxsimIn &in, const MaxsimKeyedIn &kin, uint32_t nq, const rq_maxsim_params_t *mp,
                                     const MaxsimOut &out) {
    RQC(maxsim_keyed_checks(idx, in, kin, nq, mp, out));
    const rq_postings *post = kin.post;
    const uint32_t T = mp->tokens, fetch = mp->fetch, rows_q = nq * T;
    const rq_filter *filter = in.query ? live_or(idx, in.filter) : nullptr;
    const AttrColumn *col = nullptr;
    if (in.query) {
        RQC(validate_call(idx, false, in.len, in.probe, fetch, filter));  // the source's refusals at topk = fetch, before anything is made
        const int ci = attr_find(idx, post->column);  // (step 2 reads the column as it is now)
        if (ci < 0 || idx->attrs[(size_t)ci]->type != post->type)
            return fail(RQ_ERR_INVALID, "the index no longer has the postings' column " + post->column + " in the type they were made from");
        col = idx->attrs[(size_t)ci].get();
    } else {
        RQC(ensure_device());
        RQC(raw_len_check(idx, "token", in.len));
    }
    RQC(maxsim_ensure_attributes());
    ByIdCall c;
    RQC(c.begin(idx));
    g_maxsim_stats = rq_maxsim_stats_t{};
    g_maxsim_stats.struct_size = sizeof(rq_maxsim_stats_t);
    g_maxsim_stats.directory_built = g_by_id_stats.built;
    const uint32_t ncand = in.query ? T * fetch : in.ncand;
    if (nq == 0 || ncand == 0) return RQ_OK;
    RQC(postings_device_copy(post));
    Workspace &ws = *c.ws;
    MaxsimKeyedArgs ka{};
    MaxsimArgs &ma = ka.m;
    rq_status qs = RQ_OK;
    ka.post = post->pos.p, ka.starts = post->d_starts.p, ka.values = reinterpret_cast<const unsigned long long *>(post->d_values.p);
    ka.nv = (uint32_t)post->values.size(), ka.is_signed = post->is_signed() ? 1u : 0u, ka.wide = post->wide() ? 1u : 0u;
    ka.out_keys = reinterpret_cast<unsigned long long *>(kin.out_keys);
    ma.nq = nq, ma.T = T, ma.dim = idx->dim, ma.ncand = ncand, ma.n_tokens = in.n_tokens;
    const uint64_t cells = (uint64_t)nq * ncand;
    if (in.query) {
        RQC(ws.id_res_dist.ensure((uint64_t)rows_q * fetch));
        RQC(ws.id_res_id.ensure((uint64_t)rows_q * fetch));
        RQC(ws.id_res_n.ensure(rows_q));
        PhaseClock clk;  // (the driver runs on streams of its own and returns with its outputs complete)
        qs = query_device(QueryCall{c.idx, filter, in.len, in.probe, fetch, in.heuristic != 0, QueryIO{in.tokens, ws.id_res_dist.p, ws.id_res_id.p, ws.id_res_n.p}},
                          rows_q, nullptr);
        if (qs != RQ_OK && qs != RQ_ERR_EMPTY) return qs;
        g_maxsim_stats.ms_source = clk.lap();
        // the candidate segments, their row counts and the unique counts in id_pos; the scores in id_rows
        RQC(ws.id_pos.ensure(2 * cells + nq));
        RQC(ws.id_rows.ensure(cells));
        ma.src_id = ws.id_res_id.p, ma.src_n = ws.id_res_n.p, ma.fetch = fetch, ma.topk = mp->topk;
        ma.cand_out = ws.id_pos.p, ma.cand_n_out = ws.id_pos.p + 2 * cells;
        ma.cand = ma.cand_out, ma.cand_n = ma.cand_n_out, ma.rows = ws.id_pos.p + cells, ma.score = ws.id_rows.p;
        ma.out_dist = out.a, ma.out_n = out.n, ma.out_cand = out.candidates ? out.candidates : ma.cand_n_out;
        // id -> position -> the column's value: the directory and the column as 32-bit words (the walk reads neither)
        ma.dir.rows = idx->n, ma.dir.top = c.dir->top;
        ma.dir.dense = c.dir->hashed ? nullptr : c.dir->dense.p, ma.dir.slots = c.dir->slots.p, ma.dir.bits = c.dir->bits;
        ma.dir.col = reinterpret_cast<const uint32_t *>(col->data.p), ma.dir.wide = ka.wide;
    } else {
        ma.cand = kin.segs, ma.cand_n = in.cand_n, ma.score = out.a, ma.rows = out.u;
        if (!kin.segs) {  // keys in device memory: their segments by keyed_lookup_kernel
            RQC(ws.id_pos.ensure(cells));
            ma.cand = ws.id_pos.p;
        }
    }
    RQC(transform_queries(idx, in.tokens, rows_q, in.len, /*want_padded=*/true, ws.qpad, c.st, &ma.tok));
    ma.base = idx->view();
    bool pre = false;
    size_t lds = 0;
    maxsim_plan(idx->dim, mp->flags, ma, &pre, &lds);
    // (rq_keyed_tuning's slabs = 1 asks for one slab here as in the keyed scan: a measurement knob, results never depend on it)
    const uint32_t slabs = pre && g_keyed_slabs.load() != 1 ? maxsim_keyed_slabs(idx->dim, T, ma.tok_lds != 0, ma.list_cap) : 1u;
    lds = maxsim_lds(idx->dim, T, pre, ma.tok_lds != 0, ma.list_cap, slabs).total;
    g_maxsim_stats.prefilter = pre ? 1u : 0u, g_maxsim_stats.lds_bytes = (uint32_t)lds, g_maxsim_stats.tokens_in_lds = ma.tok_lds;
    RQC(ws.id_found.ensure(5));
    ma.stats = ws.id_found.p;
    HIPC(hipMemsetAsync(ws.id_found.p, 0, 40, c.st));
    if (in.query) launch_maxsim_candidates_keyed(ka, c.st);
    else if (!kin.segs) launch_keyed_lookup(reinterpret_cast<const unsigned long long *>(kin.keys), cells, ka, ws.id_pos.p, c.st);
    HIPC(hipEventRecord(c.ev[0], c.st));
    launch_maxsim_score_keyed(ka, idx->rows.kind(), pre, slabs, lds, c.st);
    HIPC(hipEventRecord(c.ev[1], c.st));
    if (in.query) launch_maxsim_select_keyed(ka, c.st);
    HIPC(hipMemcpyAsync(ws.h_totals, ws.id_found.p, 40, hipMemcpyDeviceToHost, c.st));
    HIPC(hipStreamSynchronize(c.st));
    HIPC(hipGetLastError());
    (void)hipEventElapsedTime(&g_maxsim_stats.ms_score, c.ev[0], c.ev[1]);
    g_maxsim_stats.rows_gathered = ws.h_totals[0], g_maxsim_stats.pairs = ws.h_totals[1];
    g_maxsim_stats.exact_distances = ws.h_totals[2], g_maxsim_stats.list_overflows = ws.h_totals[3], g_maxsim_stats.candidates = ws.h_totals[4];
    return qs;
}

// The host-pointer forms: the inputs go up (the scoring's keys as segments, searched here), maxsim_keyed_device runs, the outputs come down.
static rq_status maxsim_keyed_host(const rq_index *idx, const MaxsimIn &in, const MaxsimKeyedIn &kin, uint32_t nq, const rq_maxsim_params_t *mp,
                                   const MaxsimOut &out) {
    RQC(maxsim_keyed_checks(idx, in, kin, nq, mp, out));
    RQC(ensure_device());
    const uint64_t cells = (uint64_t)nq * (in.query ? mp->topk : in.ncand);
    DevBuf<float> d_tok, d_a;
    DevBuf<uint32_t> d_nt, d_seg, d_cn, d_u, d_n, d_c;
    DevBuf<uint64_t> d_keys;
    MaxsimIn din = in;
    MaxsimKeyedIn dkin = kin;
    if (cells) {
        RQC(d_tok.upload(in.tokens, (uint64_t)nq * mp->tokens * in.len));
        din.tokens = d_tok.p;
    }
    if (in.n_tokens && nq) {
        RQC(d_nt.upload(in.n_tokens, nq));
        din.n_tokens = d_nt.p;
    }
    if (!in.query && cells) {
        std::vector<uint32_t> segs(cells);
        keyed_segments(kin.post->values.data(), (uint32_t)kin.post->values.size(), kin.post->is_signed(), kin.post->wide(),
                       reinterpret_cast<const uint64_t *>(kin.keys), cells, segs.data());
        RQC(d_seg.upload(segs.data(), cells));
        dkin.segs = d_seg.p, dkin.keys = nullptr;
        if (in.cand_n) {
            RQC(d_cn.upload(in.cand_n, nq));
            din.cand_n = d_cn.p;
        }
    }
    RQC(d_a.alloc(cells));
    if (in.query) RQC(d_keys.alloc(cells));
    else RQC(d_u.alloc(cells));
    RQC(d_n.alloc(nq));
    RQC(d_c.alloc(nq));
    dkin.out_keys = reinterpret_cast<rq_attr_value_t *>(d_keys.p);
    const rq_status s = maxsim_keyed_device(idx, din, dkin, nq, mp, MaxsimOut{d_a.p, d_u.p, d_n.p, d_c.p});
    if (s != RQ_OK && s != RQ_ERR_EMPTY) return s;
    if (cells) {
        HIPC(hipMemcpy(out.a, d_a.p, cells * 4, hipMemcpyDeviceToHost));
        if (in.query) HIPC(hipMemcpy(kin.out_keys, d_keys.p, cells * 8, hipMemcpyDeviceToHost));
        else HIPC(hipMemcpy(out.u, d_u.p, cells * 4, hipMemcpyDeviceToHost));
    }
    if (in.query && nq) {
        HIPC(hipMemcpy(out.n, d_n.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
        if (out.candidates) HIPC(hipMemcpy(out.candidates, d_c.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    }
    return s;
}
