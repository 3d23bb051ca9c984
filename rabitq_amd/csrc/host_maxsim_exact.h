// host_maxsim_exact.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in
// order; they are not stand-alone headers; this one needs host_maxsim_keyed.h).  Exact multi-vector search (kernels:
// kernels_maxsim_exact.h, compiled in inst_maxsim_exact.hip; the scoring kernel is inst_maxsim.hip's): rq_exact_search_maxsim*, both
// of them maxsim_exact_device -- maxsim_keyed_device's shape with the bound pass in the place of the source call.  Every entry reads
// the index and the postings and writes nothing of the index.
#pragma once
#include <chrono>
#include "kernels_maxsim_exact.h"  // (the launch interface only: the kernels are inst_maxsim_exact.hip's)

static thread_local rq_maxsim_exact_stats_t g_maxsim_exact_stats;  // the calling thread's last call (rq_last_maxsim_exact_stats)

static rq_status maxsim_exact_ensure_attributes() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] { err = maxsim_exact_set_attributes(); });
    if (err != hipSuccess) return fail(RQ_ERR_HIP, std::string("hipFuncSetAttribute(maxsim_bound_kernel): ") + hipGetErrorString(err));
    return RQ_OK;
}

struct MaxsimExactIO {
    const rq_postings *post = nullptr;
    const float *tokens = nullptr;       // nq x T x len
    const uint32_t *n_tokens = nullptr;  // nq, nullable
    uint32_t len = 0;
    float *dist = nullptr;               // nq x topk
    rq_attr_value_t *keys = nullptr;     // nq x topk
    uint32_t *n = nullptr;               // nq
};

// The checks that need no device, maxsim_keyed_checks' in its words and its order: nulls and the parameters before anything of the
// index or the postings is read.
static rq_status maxsim_exact_checks(const rq_index *idx, const MaxsimExactIO &io, uint32_t nq, const rq_maxsim_params_t *mp) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    if (!io.post || !mp || (nq && (!io.tokens || !io.dist || !io.keys || !io.n))) return fail(RQ_ERR_INVALID, "null argument");
    if (mp->struct_size != sizeof(rq_maxsim_params_t))
        return fail(RQ_ERR_INVALID, "struct_size is not sizeof(rq_maxsim_params_t) (set it before the call)");
    if (mp->flags & ~RQ_MAXSIM_NO_PREFILTER) return fail(RQ_ERR_INVALID, "unknown bit in rq_maxsim_params_t.flags");
    if (mp->doc_stride != 0) return fail(RQ_ERR_INVALID, "doc_stride must be 0 where the postings name the documents");
    if (mp->fetch != 0) return fail(RQ_ERR_INVALID, "fetch must be 0: the exact search reads every document");
    if (mp->tokens == 0 || mp->tokens > RQ_MAXSIM_MAX_TOKENS) return fail(RQ_ERR_INVALID, "tokens must be in [1, 256]");
    if (mp->topk == 0 || mp->topk > RQ_MAX_TOPK) return fail(RQ_ERR_UNSUPPORTED, "topk must be in [1, 2048]");
    if ((uint64_t)nq * mp->tokens >= (1ull << 31)) return fail(RQ_ERR_UNSUPPORTED, "nq * tokens must be below 2^31");
    if (io.post->idx != idx) return fail(RQ_ERR_INVALID, "the postings were made for another index");
    RQC(postings_current(io.post));
    if (idx->base_host || idx->n_dev < idx->n)
        return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are tiered (HBM + pinned host memory): multi-vector search reads every row from HBM");
    if (idx->split_rows) return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are stored as split rows: multi-vector search reads plain rows");
    if (idx->is_shard) return fail(RQ_ERR_UNSUPPORTED, "a shard holds part of every document: multi-vector search runs on whole indexes");
    if (idx->dim > 4096) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
    return RQ_OK;
}

static rq_status maxsim_exact_device(const rq_index *idx, const MaxsimExactIO &io, uint32_t nq, const rq_maxsim_params_t *mp) {
    RQC(maxsim_exact_checks(idx, io, nq, mp));
    const auto wall0 = std::chrono::steady_clock::now();
    RQC(ensure_device());
    RQC(raw_len_check(idx, "token", io.len));
    RQC(maxsim_ensure_attributes());
    RQC(maxsim_exact_ensure_attributes());
    ByIdCall c;
    RQC(c.begin(idx));
    rq_maxsim_exact_stats_t &stats = g_maxsim_exact_stats;
    stats = rq_maxsim_exact_stats_t{};
    stats.struct_size = sizeof(rq_maxsim_exact_stats_t);
    if (nq == 0) return RQ_OK;
    const rq_postings *post = io.post;
    RQC(postings_device_copy(post));
    Workspace &ws = *c.ws;
    const uint32_t T = mp->tokens, topk = mp->topk, dim = idx->dim, nv = (uint32_t)post->values.size();
    const uint64_t postings = post->starts.empty() ? 0 : post->starts.back();
    uint32_t Bc = 0, img_lds = 0, bslabs = 1, blds = 0;
    const bool bound = maxsim_bound_plan(dim, T, &Bc, &img_lds, &bslabs, &blds) && !(mp->flags & RQ_MAXSIM_NO_PREFILTER) && nv != 0;
    const MaxsimExactCut cut = maxsim_exact_cut(nq, nv, postings, bound ? Bc : 0u);
    const uint32_t P = cut.pass_queries, S = std::min<uint32_t>(RQ_MSX_ROUND_SLOTS, std::max(nv, 1u)), t32 = (T + 31u) & ~31u, rowb = dim * 2 + 16;
    stats.prefilter = bound ? 1u : 0u, stats.documents = nv;
    if (bound) stats.chunk_queries = Bc, stats.lds_bytes = blds, stats.image_in_lds = img_lds;

    const float *tok = nullptr;
    RQC(transform_queries(idx, io.tokens, nq * T, io.len, /*want_padded=*/true, ws.qpad, c.st, &tok));
    // the pass's work memory, carved from the by-id buffers of the workspace:
    //   id_rows      L, U                         2 P nv floats
    //   id_pos       survivors, their counts; a round's candidates, counts and rows      P nv + P + P S + P + P S
    //   id_res_dist  a round's scores, tau        P S + P
    //   id_res_id    the running topk keys (u64) and their counts     2 P topk + P
    //   id_rows_raw  the token image and the norms                    P T32 (rowb / 4 + 2)
    const uint64_t Pnv = (uint64_t)P * nv, PS = (uint64_t)P * S;
    RQC(ws.id_rows.ensure(bound ? 2 * Pnv : 1));
    RQC(ws.id_pos.ensure(Pnv + 2 * PS + 2 * (uint64_t)P));
    RQC(ws.id_res_dist.ensure(PS + P));
    RQC(ws.id_res_id.ensure(2 * (uint64_t)P * topk + P));
    RQC(ws.id_rows_raw.ensure(bound ? (uint64_t)P * t32 * (rowb / 4 + 2) : 1));
    RQC(ws.id_found.ensure(16));
    HIPC(hipMemsetAsync(ws.id_found.p, 0, 16 * 8, c.st));

    MaxsimBoundArgs ba{};
    ba.T = T, ba.dim = dim, ba.Bc = bound ? Bc : 1u, ba.img_lds = img_lds;
    ba.img = reinterpret_cast<unsigned char *>(ws.id_rows_raw.p);
    ba.qn2 = ws.id_rows_raw.p + (uint64_t)P * t32 * (rowb / 4), ba.qsn = ba.qn2 + (uint64_t)P * t32;
    ba.post = post->pos.p, ba.starts = post->d_starts.p, ba.nv = nv, ba.unit_rows = cut.unit_rows;
    ba.base = idx->view();
    ba.L = ws.id_rows.p, ba.U = ws.id_rows.p + (bound ? Pnv : 0);
    ba.topk = topk, ba.all = bound ? 0u : 1u;
    ba.tau = ws.id_res_dist.p + PS;
    ba.surv = ws.id_pos.p, ba.surv_n = ws.id_pos.p + Pnv;
    uint32_t *cand = ba.surv_n + P, *cand_n = cand + PS, *rows = cand_n + P;
    unsigned long long *run = reinterpret_cast<unsigned long long *>(ws.id_res_id.p);
    uint32_t *run_n = ws.id_res_id.p + 2 * (uint64_t)P * topk;

    MaxsimKeyedArgs ka{};
    MaxsimArgs &ma = ka.m;
    ka.post = post->pos.p, ka.starts = post->d_starts.p, ka.values = reinterpret_cast<const unsigned long long *>(post->d_values.p);
    ka.nv = nv, ka.is_signed = post->is_signed() ? 1u : 0u, ka.wide = post->wide() ? 1u : 0u;
    ma.T = T, ma.dim = dim, ma.topk = topk, ma.base = idx->view();
    ma.cand = cand, ma.cand_n = cand_n, ma.rows = rows, ma.score = ws.id_res_dist.p;
    ma.stats = ws.id_found.p;  // (the scoring kernel's five totals; slots 8 and 9 are the compaction's)

    for (uint32_t q0 = 0; q0 < nq; q0 += P) {
        const uint32_t np = std::min(P, nq - q0);
        ba.tok = tok + (uint64_t)q0 * T * dim, ba.n_tokens = io.n_tokens ? io.n_tokens + q0 : nullptr, ba.nq = np;
        ba.totals = ws.id_found.p + 8;
        HIPC(hipMemsetAsync(ba.totals, 0, 16, c.st));
        HIPC(hipEventRecord(c.ev[0], c.st));
        if (bound) {
            launch_maxsim_bound_prep(ba, c.st);
            if (cut.units) launch_maxsim_bound(ba, idx->rows.kind(), bslabs, cut.units, blds, c.st);
            launch_maxsim_bound_threshold(ba, c.st);
            stats.query_chunks += ceil_div(np, Bc), stats.postings_walked += postings * ceil_div(np, Bc);
        }
        launch_maxsim_bound_compact(ba, c.st);
        HIPC(hipEventRecord(c.ev[1], c.st));
        HIPC(hipMemcpyAsync(ws.h_totals + 8, ba.totals, 16, hipMemcpyDeviceToHost, c.st));
        HIPC(hipStreamSynchronize(c.st));  // the survivors' largest count sizes the rounds
        HIPC(hipGetLastError());
        const uint32_t most = (uint32_t)ws.h_totals[8];
        stats.survivors += ws.h_totals[9];
        const uint32_t rounds = std::max<uint32_t>(ceil_div(most, S), 1u);
        ka.out_keys = reinterpret_cast<unsigned long long *>(io.keys) + (uint64_t)q0 * topk;
        ma.out_dist = io.dist + (uint64_t)q0 * topk, ma.out_n = io.n + q0;
        ma.nq = np, ma.tok = ba.tok, ma.n_tokens = ba.n_tokens;
        HIPC(hipEventRecord(c.ev[2], c.st));
        for (uint32_t r = 0; r < rounds; ++r) {  // a round: the survivors [r S, r S + S) of every query; no document is ever dropped
            const uint32_t first = r * S, slots = std::max<uint32_t>(std::min<uint32_t>(S, most - std::min(most, first)), 1u);
            ma.ncand = slots;
            launch_maxsim_exact_round(ba, first, slots, cand, cand_n, c.st);
            bool pre = false;
            size_t lds = 0;
            maxsim_plan(dim, mp->flags, ma, &pre, &lds);
            const uint32_t slabs = pre && g_keyed_slabs.load() != 1 ? maxsim_keyed_slabs(dim, T, ma.tok_lds != 0, ma.list_cap) : 1u;
            lds = maxsim_lds(dim, T, pre, ma.tok_lds != 0, ma.list_cap, slabs).total;
            launch_maxsim_score_keyed(ka, idx->rows.kind(), pre, slabs, lds, c.st);
            launch_maxsim_exact_merge(ka, run, run_n, r == 0, r + 1 == rounds, c.st);
        }
        HIPC(hipEventRecord(c.ev[3], c.st));
        HIPC(hipMemcpyAsync(ws.h_totals, ws.id_found.p, 40, hipMemcpyDeviceToHost, c.st));
        HIPC(hipStreamSynchronize(c.st));
        HIPC(hipGetLastError());
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, c.ev[0], c.ev[1]);
        stats.ms_bound += ms;
        (void)hipEventElapsedTime(&ms, c.ev[2], c.ev[3]);
        stats.ms_score += ms;
        stats.rounds += rounds, stats.passes += 1;
        stats.pairs = ws.h_totals[1];  // (the scoring kernel adds across rounds and passes)
    }
    stats.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return RQ_OK;
}

// The host-pointer form: the tokens go up, maxsim_exact_device runs, the outputs come down.
static rq_status maxsim_exact_host(const rq_index *idx, const MaxsimExactIO &io, uint32_t nq, const rq_maxsim_params_t *mp) {
    RQC(maxsim_exact_checks(idx, io, nq, mp));
    RQC(ensure_device());
    const uint64_t cells = (uint64_t)nq * mp->topk;
    DevBuf<float> d_tok, d_dist;
    DevBuf<uint32_t> d_nt, d_n;
    DevBuf<uint64_t> d_keys;
    MaxsimExactIO dio = io;
    if (nq) {
        RQC(d_tok.upload(io.tokens, (uint64_t)nq * mp->tokens * io.len));
        dio.tokens = d_tok.p;
        if (io.n_tokens) {
            RQC(d_nt.upload(io.n_tokens, nq));
            dio.n_tokens = d_nt.p;
        }
    }
    RQC(d_dist.alloc(cells));
    RQC(d_keys.alloc(cells));
    RQC(d_n.alloc(nq));
    dio.dist = d_dist.p, dio.keys = reinterpret_cast<rq_attr_value_t *>(d_keys.p), dio.n = d_n.p;
    RQC(maxsim_exact_device(idx, dio, nq, mp));
    if (nq) {
        HIPC(hipMemcpy(io.dist, d_dist.p, cells * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(io.keys, d_keys.p, cells * 8, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(io.n, d_n.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    }
    return RQ_OK;
}
