// host_maxsim.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  Multi-vector search (kernels: kernels_maxsim.h, compiled in inst_maxsim.hip):
// rq_maxsim_scores and rq_query_batch_maxsim, both of them maxsim_device -- group_device's pattern (host_group.h): the plain query
// driver on the token rows at topk = fetch into workspace buffers, then the candidates, scoring and selection launches on the by-id
// call's stream; no result travels to the host in between.  Every entry reads the index and writes nothing of it.
#pragma once
#include "kernels_maxsim.h"  // (the launch interface only: the kernels are inst_maxsim.hip's)

static thread_local rq_maxsim_stats_t g_maxsim_stats;  // the calling thread's last multi-vector call (rq_last_maxsim_stats)

static rq_status maxsim_ensure_attributes() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] { err = maxsim_set_attributes(); });
    if (err != hipSuccess) return fail(RQ_ERR_HIP, std::string("hipFuncSetAttribute(maxsim_score_kernel): ") + hipGetErrorString(err));
    return RQ_OK;
}

// What a call reads besides the index and its params (query: the end-to-end entry) ...
struct MaxsimIn {
    bool query = false;
    const rq_filter *filter = nullptr;
    const float *tokens = nullptr;       // nq x T x len
    const uint32_t *n_tokens = nullptr;  // nq, nullable
    uint32_t len = 0, probe = 1;
    int heuristic = 0;
    const uint32_t *cand = nullptr, *cand_n = nullptr;  // scores: nq x ncand, nq (nullable)
    uint32_t ncand = 0;
};
// ... and what it writes: scores -> a = score, u = rows; query -> a = dist, u = docs, n, candidates (nullable)
struct MaxsimOut {
    float *a = nullptr;
    uint32_t *u = nullptr, *n = nullptr, *candidates = nullptr;
};

// The checks that need no device, in the order the header gives.
static rq_status maxsim_checks(const rq_index *idx, const MaxsimIn &in, uint32_t nq, const rq_maxsim_params_t *mp, const MaxsimOut &out) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    const bool cells = nq && (in.query || in.ncand);
    if (!mp || (cells && (!out.a || !out.u)) || (in.query && !out.n) || (cells && (!in.tokens || (!in.query && !in.cand))))
        return fail(RQ_ERR_INVALID, "null argument");
    if (mp->struct_size != sizeof(rq_maxsim_params_t))
        return fail(RQ_ERR_INVALID, "struct_size is not sizeof(rq_maxsim_params_t) (set it before the call)");
    if (mp->flags & ~RQ_MAXSIM_NO_PREFILTER) return fail(RQ_ERR_INVALID, "unknown bit in rq_maxsim_params_t.flags");
    if (mp->doc_stride == 0 || mp->doc_stride > RQ_MAXSIM_MAX_STRIDE) return fail(RQ_ERR_INVALID, "doc_stride must be in [1, 4096]");
    if (mp->tokens == 0 || mp->tokens > RQ_MAXSIM_MAX_TOKENS) return fail(RQ_ERR_INVALID, "tokens must be in [1, 256]");
    if (idx->base_host || idx->n_dev < idx->n)
        return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are tiered (HBM + pinned host memory): multi-vector search reads every row from HBM");
    if (idx->split_rows) return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are stored as split rows: multi-vector search reads plain rows");
    if (idx->is_shard) return fail(RQ_ERR_UNSUPPORTED, "a shard holds part of every document: multi-vector search runs on whole indexes");
    if (idx->dim > 4096) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
    if (in.query) {
        if ((uint64_t)mp->tokens * mp->fetch > RQ_MAXSIM_MAX_SOURCE || mp->fetch == 0)
            return fail(RQ_ERR_UNSUPPORTED, "fetch must be at least 1 and tokens * fetch <= 2048");
        if (mp->topk == 0 || mp->topk > RQ_MAX_TOPK) return fail(RQ_ERR_UNSUPPORTED, "topk must be in [1, 2048]");
    }
    if ((uint64_t)nq * mp->tokens >= (1ull << 31)) return fail(RQ_ERR_UNSUPPORTED, "nq * tokens must be below 2^31");
    return RQ_OK;
}

// The form and the launch shape of the scoring: the matrix-core pass where its tiles fit in a CU's LDS (two blocks per CU wanted,
// the f32 tokens staged beside them where that still fits), and a group size that fills the machine at small nq and lets a block
// amortise staging its tokens at large ncand.
static void maxsim_plan(uint32_t dim, uint32_t flags, MaxsimArgs &ma, bool *pre, size_t *lds) {
    ma.list_cap = maxsim_list_cap(ma.T);
    *pre = !(flags & RQ_MAXSIM_NO_PREFILTER) && maxsim_lds(dim, ma.T, true, false, ma.list_cap).total <= RQ_MAXSIM_LDS_MAX;
    const uint32_t with_tok = maxsim_lds(dim, ma.T, *pre, true, ma.list_cap).total;
    ma.tok_lds = with_tok <= RQ_MAXSIM_LDS_TWO || (with_tok <= RQ_MAXSIM_LDS_MAX && maxsim_lds(dim, ma.T, *pre, false, ma.list_cap).total > RQ_MAXSIM_LDS_TWO) ? 1u : 0u;
    *lds = maxsim_lds(dim, ma.T, *pre, ma.tok_lds != 0, ma.list_cap).total;
    const uint64_t slots = (uint64_t)ma.nq * ma.ncand;
    uint32_t g = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(4, (slots / 2048 + 3) & ~3ull));
    while ((uint64_t)ma.nq * ceil_div(ma.ncand, g) >= (1ull << 31)) g *= 2;
    ma.group = g, ma.chunks = std::max<uint32_t>(ceil_div(ma.ncand, g), 1u);
}

static rq_status maxsim_device(const rq_index *idx, const MaxsimIn &in, uint32_t nq, const rq_maxsim_params_t *mp, const MaxsimOut &out) {
    RQC(maxsim_checks(idx, in, nq, mp, out));
    const uint32_t T = mp->tokens, fetch = mp->fetch, rows_q = nq * T;
    const rq_filter *filter = in.query ? live_or(idx, in.filter) : nullptr;
    if (in.query) RQC(validate_call(idx, false, in.len, in.probe, fetch, filter));  // the source's refusals at topk = fetch, before anything is made
    else {
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
    Workspace &ws = *c.ws;
    MaxsimArgs ma{};
    rq_status qs = RQ_OK;
    ma.nq = nq, ma.T = T, ma.dim = idx->dim, ma.ncand = ncand, ma.S = mp->doc_stride, ma.n_tokens = in.n_tokens;
    if (in.query) {
        RQC(ws.id_res_dist.ensure((uint64_t)rows_q * fetch));
        RQC(ws.id_res_id.ensure((uint64_t)rows_q * fetch));
        RQC(ws.id_res_n.ensure(rows_q));
        PhaseClock clk;  // (the driver runs on streams of its own and returns with its outputs complete)
        qs = query_device(QueryCall{c.idx, filter, in.len, in.probe, fetch, in.heuristic != 0, QueryIO{in.tokens, ws.id_res_dist.p, ws.id_res_id.p, ws.id_res_n.p}},
                          rows_q, nullptr);
        if (qs != RQ_OK && qs != RQ_ERR_EMPTY) return qs;
        g_maxsim_stats.ms_source = clk.lap();
        // the candidates, their row counts and the unique counts in id_pos; the scores in id_rows
        const uint64_t cells = (uint64_t)nq * ncand;
        RQC(ws.id_pos.ensure(2 * cells + nq));
        RQC(ws.id_rows.ensure(cells));
        ma.src_id = ws.id_res_id.p, ma.src_n = ws.id_res_n.p, ma.fetch = fetch, ma.topk = mp->topk;
        ma.cand_out = ws.id_pos.p, ma.cand_n_out = ws.id_pos.p + 2 * cells;
        ma.cand = ma.cand_out, ma.cand_n = ma.cand_n_out, ma.rows = ws.id_pos.p + cells, ma.score = ws.id_rows.p;
        ma.out_dist = out.a, ma.out_docs = out.u, ma.out_n = out.n, ma.out_cand = out.candidates ? out.candidates : ma.cand_n_out;
    } else {
        ma.cand = in.cand, ma.cand_n = in.cand_n, ma.score = out.a, ma.rows = out.u;
    }
    RQC(transform_queries(idx, in.tokens, rows_q, in.len, /*want_padded=*/true, ws.qpad, c.st, &ma.tok));
    ma.dir.rows = idx->n, ma.dir.top = c.dir->top;
    ma.dir.dense = c.dir->hashed ? nullptr : c.dir->dense.p, ma.dir.slots = c.dir->slots.p, ma.dir.bits = c.dir->bits;
    ma.dir.live = idx->live ? idx->live->pos_bits.p : nullptr;  // (read at call time, as ByIdCall::lookup does)
    ma.base = idx->view();
    bool pre = false;
    size_t lds = 0;
    maxsim_plan(idx->dim, mp->flags, ma, &pre, &lds);
    g_maxsim_stats.prefilter = pre ? 1u : 0u, g_maxsim_stats.lds_bytes = (uint32_t)lds, g_maxsim_stats.tokens_in_lds = ma.tok_lds;
    RQC(ws.id_found.ensure(5));
    ma.stats = ws.id_found.p;
    HIPC(hipMemsetAsync(ws.id_found.p, 0, 40, c.st));
    if (in.query) launch_maxsim_candidates(ma, c.st);
    HIPC(hipEventRecord(c.ev[0], c.st));
    launch_maxsim_score(ma, idx->rows.kind(), pre, lds, c.st);
    HIPC(hipEventRecord(c.ev[1], c.st));
    if (in.query) launch_maxsim_select(ma, c.st);
    HIPC(hipMemcpyAsync(ws.h_totals, ws.id_found.p, 40, hipMemcpyDeviceToHost, c.st));
    HIPC(hipStreamSynchronize(c.st));
    HIPC(hipGetLastError());
    (void)hipEventElapsedTime(&g_maxsim_stats.ms_score, c.ev[0], c.ev[1]);
    g_maxsim_stats.rows_gathered = ws.h_totals[0], g_maxsim_stats.pairs = ws.h_totals[1];
    g_maxsim_stats.exact_distances = ws.h_totals[2], g_maxsim_stats.list_overflows = ws.h_totals[3], g_maxsim_stats.candidates = ws.h_totals[4];
    return qs;
}

// The host-pointer forms: the inputs go up, maxsim_device runs, the outputs come down.
static rq_status maxsim_host(const rq_index *idx, const MaxsimIn &in, uint32_t nq, const rq_maxsim_params_t *mp, const MaxsimOut &out) {
    RQC(maxsim_checks(idx, in, nq, mp, out));
    RQC(ensure_device());
    const uint64_t cells = (uint64_t)nq * (in.query ? mp->topk : in.ncand);
    DevBuf<float> d_tok, d_a;
    DevBuf<uint32_t> d_nt, d_cand, d_cn, d_u, d_n, d_c;
    MaxsimIn din = in;
    if (cells) {
        RQC(d_tok.upload(in.tokens, (uint64_t)nq * mp->tokens * in.len));
        din.tokens = d_tok.p;
    }
    if (in.n_tokens && nq) {
        RQC(d_nt.upload(in.n_tokens, nq));
        din.n_tokens = d_nt.p;
    }
    if (!in.query && cells) {
        RQC(d_cand.upload(in.cand, cells));
        din.cand = d_cand.p;
        if (in.cand_n) {
            RQC(d_cn.upload(in.cand_n, nq));
            din.cand_n = d_cn.p;
        }
    }
    RQC(d_a.alloc(cells));
    RQC(d_u.alloc(cells));
    RQC(d_n.alloc(nq));
    RQC(d_c.alloc(nq));
    const rq_status s = maxsim_device(idx, din, nq, mp, MaxsimOut{d_a.p, d_u.p, d_n.p, d_c.p});
    if (s != RQ_OK && s != RQ_ERR_EMPTY) return s;
    if (cells) {
        HIPC(hipMemcpy(out.a, d_a.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out.u, d_u.p, cells * 4, hipMemcpyDeviceToHost));
    }
    if (in.query && nq) {
        HIPC(hipMemcpy(out.n, d_n.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
        if (out.candidates) HIPC(hipMemcpy(out.candidates, d_c.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    }
    return s;
}
