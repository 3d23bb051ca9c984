// host_query.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  The query pipeline: RaBitQ::query (src/rabitq.rs:268-333) as staged passes -- a pass's workspace, its phases, run_pass and finish_pass (what turns a call into passes: host_call.h).
#pragma once
// ------------------------------------------------------------------------------------------------
// the query pipeline
// ------------------------------------------------------------------------------------------------
static rq_status ws_prepare(const rq_index *idx, Workspace &ws, const QueryParams &qp) {
    const uint32_t nprobe = std::min(qp.probe, idx->k);
    const uint64_t nq = qp.nq, npairs = nq * nprobe;
    RQC(ws_ensure_stream(ws));
    RQC(ws.qpad.ensure(nq * idx->dim));
    RQC(ws.y.ensure(nq * idx->dim));
    if (!qp.ext_lists) RQC(ws.dist.ensure(nq * idx->k));
    RQC(ws.probe_dist.ensure(npairs));
    RQC(ws.probe_cluster.ensure(npairs));
    RQC(ws.scal.ensure(npairs));
    if (!scan_is_fused(idx->W)) RQC(ws.planes.ensure(npairs * 4 * idx->W));  // bit planes: only the generic-W scan reads them
    RQC(ws.qnib.ensure(npairs * 8 * idx->W));
    RQC(ws.qf6.ensure(npairs * 12 * idx->W));
    RQC(ws.rough_cnt.ensure(nq));
    RQC(ws.totals.ensure(16));  // [0..7] the pass's totals, [12] rows of the pre-filtered coarse ranking that fell back to exact order
    RQC(ws.stat.ensure(256));
    // record-major (8W + tail per pair) or tile images (pairs padded to 32 per list, 12W + 2 + tail per slot)
    RQC(ws.recs.ensure((npairs + 32ull * idx->k + 32) * (12ull * idx->W + 2 + RQ_REC_TAIL)));
    RQC(ws.grp_cnt.ensure(idx->k + 4));
    RQC(ws.grp_start.ensure(idx->k + 1));
    RQC(ws.q_hist.ensure(idx->k + 2));
    RQC(ws.q_start.ensure(idx->k + 2));
    RQC(ws.q_order.ensure(nq));
    RQC(ws.thr.ensure(nq));
    RQC(ws.surv.ensure(nq * qp.cap));
    RQC(ws.runs.ensure(nq * qp.cap));
    // second run directory, through which long directories (> 512 runs) are ordered: only once the index has shown
    // that it produces them (or with enlarged buffers); until then a stray long directory is bitonic-sorted in place
    ws.use_runs_tmp = qp.cap > RQ_DEFAULT_CAP || qp.seg_final || hints_of(idx, qp.filter).big_dirs.load() > 0;
    if (ws.use_runs_tmp) RQC(ws.runs_tmp.ensure(nq * qp.cap));
    RQC(ws.surv_cnt.ensure(nq));
    RQC(ws.heap_len.ensure(nq));
    RQC(ws.heap_key.ensure(nq * qp.topk));
    RQC(ws.heap_id.ensure(nq * qp.topk));
    RQC(ws.precise.ensure(nq));
    RQC(ws.need.ensure(nq));
    RQC(ws.ovf.ensure(nq));
    RQC(ws.q_cap.ensure(nq));
    RQC(ws.q_base.ensure(nq));
    RQC(ws.nsurv.ensure(nq));
    RQC(ws.nshadow.ensure(nq));
    RQC(ws.recent.ensure(nq));
    RQC(ws.win_count.ensure(nq));
    RQC(ws.arr_len.ensure(nq));
    RQC(ws.row_map.ensure(nq));
    RQC(ws.big_list.ensure(nq + 3));  // [nq] = entries, [nq + 1] = blocks done, [nq + 2] = most entries of any stage of the pass
    if (qp.heuristic) RQC(ws.arr.ensure(nq * qp.hcap));
    if (qp.range) RQC(ws.range_hits.ensure(nq));
    return RQ_OK;
}

struct PassResult {
    uint64_t rough = 0, precise = 0, overflowed = 0, max_need = 0;
};

// Second half of a pass: wait for the stream, read the totals, collect the profile.
static rq_status finish_pass(const rq_index *idx, Workspace &ws, PassResult *res, rq_profile_t *prof_acc) {
    Prof &pf = ws.prof;
    const uint32_t nq = ws.pend.nq, dim = idx->dim;
    HIPC(hipStreamSynchronize(ws.stream));
    HIPC(hipGetLastError());
    res->rough = ws.h_totals[0];
    res->precise = ws.h_totals[1];
    res->overflowed = ws.h_totals[2];
    res->max_need = ws.h_totals[4];
    if (ws.pend.large && !ws.pend.range) hints_of(idx, ws.pend.filter).big_dirs.store((uint32_t)ws.h_totals[7]);
    // The additive gate is a looser test than the rank-5 threshold it replaces: an index / workload on which it sends more than
    // 3 % of the sub-tile steps down the exact path (each costs ~10 plain steps) goes back to the bf16 threshold MFMA for good
    // (results do not depend on the choice; option scan_gate pins it)
    // (a range pass does not feed the decision: its one stage covers the nearest list too and its radii may admit everything, which
    // says nothing about the final stages of the top-k passes the flag steers)
    if (ws.pend.additive && !ws.pend.range && ws.h_totals[8] >= 4096 && ws.h_totals[9] * 32 > ws.h_totals[8])
        const_cast<rq_index *>(idx)->additive_loose.store(1);
    if (prof_acc) prof_acc->matrix_subtile_steps += ws.h_totals[8], prof_acc->matrix_exact_steps += ws.h_totals[9];
    if (prof_acc) prof_acc->coarse_fallback_rows += (uint32_t)std::min<unsigned long long>(ws.h_totals[10], 0xFFFFFFFFull);
    if (pf.on && prof_acc) {
        float ms[PF_N] = {0};
        pf.collect(ms);
        prof_acc->ms_rotate += ms[PF_ROTATE], prof_acc->ms_coarse += ms[PF_COARSE];
        prof_acc->ms_select += ms[PF_SELECT], prof_acc->ms_prep += ms[PF_PREP], prof_acc->ms_group += ms[PF_GROUP];
        prof_acc->ms_scan += ms[PF_SCAN] + ms[PF_SCAN_MATRIX], prof_acc->ms_scan_matrix += ms[PF_SCAN_MATRIX];
        prof_acc->ms_rerank += ms[PF_RERANK], prof_acc->ms_sort += ms[PF_SORT];
        if (ws.pend.n_matrix_ranges) {  // pairs scored by those launches: per query, its stream length clipped to the range
            std::vector<unsigned long long> len(nq);
            HIPC(hipMemcpy(len.data(), ws.pend.filter ? ws.stream_len.p : ws.rough_cnt.p, (size_t)nq * 8, hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < ws.pend.n_matrix_ranges; ++i) {
                const StreamRange r = ws.pend.matrix_ranges[i];
                for (uint32_t b = 0; b < nq; ++b)
                    prof_acc->matrix_pairs += std::min<unsigned long long>(len[b], r.s_hi) - std::min<unsigned long long>(len[b], r.s_lo);
            }
        }
        prof_acc->ms_replay += ms[PF_REPLAY], prof_acc->ms_total += ms[PF_TOTAL], prof_acc->ms_early += ms[PF_EARLY];
    }
    if (prof_acc) {
        const uint64_t slots = std::max<uint64_t>((uint64_t)nq * ws.pend.cap, ws.pend.seg_slots);
        prof_acc->survivor_workspace_bytes = std::max<uint64_t>(prof_acc->survivor_workspace_bytes,
            ws.pend.seg_slots ? (ws.surv.count + ws.runs.count + ws.runs_tmp.count + ws.arena_recs.count + ws.arena_runs.count) * 16ull
                              : slots * (ws.use_runs_tmp ? 48ull : 32ull));
        prof_acc->segmented_passes += ws.pend.seg_slots ? 1u : 0u;
        prof_acc->scan_candidates += res->rough;
        prof_acc->scan_bytes += res->rough * (uint64_t)(dim / 8 + 16);
        prof_acc->rerank_candidates += ws.h_totals[3];
        prof_acc->rerank_shadow_rejects += ws.h_totals[5];
        if (g_scan_dbg.load() & 256) {  // developer hook: where the matrix-core scan's waves spend their cycles
            unsigned long long ht[12];
            HIPC(hipMemcpy(ht, ws.stat.p + 128, sizeof ht, hipMemcpyDeviceToHost));
            if (ht[3])
                fprintf(stderr, "[rabitq_hip] scan_mfma exact path (wave 0 of every block): %.0f cycles per block inside it (of which flushes %.0f), "
                        "%.1f flagged registers, %.1f with survivors and %.2f flushes per block\n", (double)ht[5] / ht[3], (double)ht[6] / ht[3],
                        (double)ht[9] / ht[3], (double)ht[7] / ht[3], (double)ht[8] / ht[3]);
            if (ht[3])
                fprintf(stderr, "[rabitq_hip] scan_mfma timing: %llu blocks, %.1f tiles/block; per block cycles: start-up %.0f, "
                        "tile-loop waits %.0f, tile bodies %.0f (per tile: wait %.0f, body %.0f)\n", ht[3], (double)ht[4] / ht[3],
                        (double)ht[0] / ht[3], (double)ht[1] / ht[3], (double)ht[2] / ht[3], (double)ht[1] / std::max(1ull, ht[4]),
                        (double)ht[2] / std::max(1ull, ht[4]));
        }
        if ((g_scan_dbg.load() & 4096) && nq <= RQ_SB_MAX_NQ) {  // developer hook: phase boundaries of sb_query_kernel's block 0
            unsigned long long hs[32];
            HIPC(hipMemcpy(hs, ws.stat.p, sizeof hs, hipMemcpyDeviceToHost));
            std::string line = "[rabitq_hip] sb_query_kernel phases (us since entry):";
            for (unsigned long long i = 1; i < std::min<unsigned long long>(hs[0], 30); ++i) line += " " + std::to_string((hs[1 + i] - hs[1]) / 100.0).substr(0, 6);
            fprintf(stderr, "%s\n", line.c_str());
        }
    }
    return RQ_OK;
}

// sb_query_kernel<W, mode, filtered>: one block per query (the filtered instantiations: inst_small_filt.hip)
template <int W>
static void launch_sb_query_w(int mode, uint32_t nq, size_t dyn, hipStream_t st, const SbArgs &sa) {
    if (mode == 2) sb_query_kernel<W, 2, false><<<nq, 1024, dyn, st>>>(sa);
    else if (mode == 1) sb_query_kernel<W, 1, false><<<nq, 1024, dyn, st>>>(sa);
    else sb_query_kernel<W, 0, false><<<nq, 1024, dyn, st>>>(sa);
}
static void launch_sb_query(uint32_t W, int mode, bool filtered, uint32_t nq, size_t dyn, hipStream_t st, const SbArgs &sa) {
    if (filtered) return launch_sb_query_filtered(W, mode, nq, dyn, st, sa);
#define RQ_SBQ(WW) case WW: launch_sb_query_w<WW>(mode, nq, dyn, st, sa); break;
    switch (W) {
        RQ_SMALL_BATCH_WIDTHS(RQ_SBQ)
        default: break;  // (not reached: plan_pass takes the path for small_batch_has(W) only, which is made from the same list)
    }
#undef RQ_SBQ
}

// ------------------------------------------------------------------------------------------------
// one pass: the plan (host_plan.h) executed as phases
// ------------------------------------------------------------------------------------------------
// One stage on its way through group + fill, scan and finish.
struct StageRun {
    const StagePlan &s;
    uint32_t no;
    ScanArgs a{};
    ScanPtrs sp{};
    QSeg seg{};                // the survivors' geometry: uniform, or per-query segments behind an arena stage
    bool runs_in_tmp = false;  // (arena stage) the ordering pass writes the directory
};
// One pass: its arguments, its plan, what the front phases resolve, and the phases themselves (run_pass calls them in order).
struct Pass {
    const rq_index *idx;
    Workspace &ws;
    const QueryParams &qp;
    const PassPlan &pl;
    Prof &pf;
    hipStream_t st;
    const uint32_t dim, k, W, nq, topk, nprobe, npairs;
    const QueryIO &io;  // the pass's arrays
    const uint32_t *d_row_map;
    rq_profile_t *prof_acc;
    const float *qpad;              // the queries, padded to dim (io.d_q itself when nothing was padded)
    const uint32_t *probe_cluster;  // the probe lists: ranked here, or the caller's
    const float *probe_dist;
    ReplayState rs;
    const uint32_t *rerank_order = nullptr;
    uint32_t nlive = 0;            // listed pass: the pairs whose list has members here (ws.live_list)
    bool sb_results_done = false;  // results and totals were written by the small-batch kernels (heap ranker)
    PendingPass pend;              // what finish_pass will want to know (assigned to the workspace once, by results())

    // small batches: coarse distances, then the early stages (or the whole stream) inside one block per query
    rq_status small_front() {
        SbArgs sa{};
        sa.nstages = pl.sb_nstages;
        for (uint32_t i = 0; i < sa.nstages; ++i) sa.s_lo[i] = pl.sb_lo[i], sa.s_hi[i] = pl.sb_hi[i];
        sa.finalize = pl.sb_whole ? 1u : 0u, sa.fill_final = pl.sb_fill_final ? 1u : 0u, sa.final_lo = pl.sb_final_lo;
        sa.codes = reinterpret_cast<const uint32_t *>(idx->codes.p), sa.factors = idx->factors.p, sa.centroids = idx->centroids.p;
        sa.offsets = idx->offsets.p, sa.map_ids = idx->map_ids.p, sa.base = idx->view();
        sa.dist = ws.dist.p, sa.y = ws.y.p, sa.qpad = ws.qpad.p, sa.probe_cluster = ws.probe_cluster.p, sa.probe_dist = ws.probe_dist.p;
        sa.qf6 = pl.write_q6 ? ws.qf6.p : nullptr;
        sa.scal = ws.scal.p, sa.qnib = ws.qnib.p, sa.rough_cnt = ws.rough_cnt.p, sa.surv_cnt = ws.surv_cnt.p, sa.totals = ws.totals.p;
        sa.rs = rs, sa.out_dist = io.out_dist, sa.out_id = io.out_id, sa.out_n = io.out_n, sa.recs = ws.recs.p, sa.fs = idx->fstats;
        sa.k = k, sa.dim = dim, sa.nprobe = nprobe, sa.topk = topk, sa.cap = qp.cap, sa.hcap = qp.hcap;
        const rq_filter *filt = qp.filter;
        if (filt) {
            RQC(ws.stream_len.ensure(nq));
            sa.pos_bits = filt->pos_bits.p, sa.sub_off = filt->sub_off.p, sa.stream_len = ws.stream_len.p;
        }
        sa.stamps = (pl.dbg & 4096) ? ws.stat.p : nullptr;
        if (sa.stamps) HIPC(hipMemsetAsync(ws.stat.p, 0, 8, st));
        else HIPC(hipMemsetAsync(ws.stat.p, 0, 256 * sizeof(unsigned long long), st));  // (the counters of a final matrix-core stage, if any)
        pf.begin(PF_COARSE);
        const float *sb_q;  // (cosine: N(q), padded -- what the front kernel rotates and hands on as qpad; else the raw queries: it pads them itself)
        uint32_t sb_len;
        RQC(transform_queries(idx, io.d_q, nq, qp.len, /*want_padded=*/false, ws.qnorm, st, &sb_q, &sb_len));
        sb_front_kernel<<<dim3(ceil_div(k, RQ_SB_LISTS), ceil_div(nq, RQ_SB_QT)), 256, (size_t)2 * RQ_SB_QT * dim * sizeof(float), st>>>(
            sb_q, sb_len, idx->P.p, idx->centroids.p, ws.y.p, ws.qpad.p, ws.dist.p, k, dim, nq, ws.totals.p, ws.big_list.p + nq);
        pf.end();
        pf.begin(PF_EARLY);
        const size_t dyn = (size_t)RQ_SB_CAP * sizeof(SurvRec) + (size_t)dim * 4 + (size_t)topk * 16;
        const int mode = qp.heuristic ? 2 : (topk < 64 ? 1 : 0);
        launch_sb_query(W, mode, filt != nullptr, nq, dyn, st, sa);
        pf.end();
        qpad = ws.qpad.p;
        sb_results_done = pl.sb_whole && !qp.heuristic;
        if (prof_acc) prof_acc->small_batch_passes++;
        return RQ_OK;
    }

    // 1. pad (rabitq.rs:277-280) + rotate (:282); 2. coarse distances + probe selection (:283-297), unless the caller supplied the lists
    rq_status rotate_coarse() {
        pf.begin(PF_ROTATE);
        RQC(transform_queries(idx, io.d_q, nq, qp.len, /*want_padded=*/true, ws.qpad, st, &qpad));
        launch_rotate(qpad, idx->P.p, ws.y.p, nq, dim, nq >= 32, st);
        pf.end();
        if (io.ext_cluster) {
            probe_cluster = io.ext_cluster, probe_dist = io.ext_dist;
        } else if (coarse_prefilter_applies(idx, nq, nprobe)) {
            pf.begin(PF_COARSE);
            HIPC(hipMemsetAsync(ws.totals.p + 12, 0, 8, st));
            RQC(ws.coarse_redo.ensure(nq));
            RQC(ws.qf6.ensure((size_t)nq * dim / 2 + 16));  // (room for the pre-rounded query rows of the wide instantiation)
            launch_coarse_prefiltered(idx, ws.y.p, ws.dist.p, nq, nprobe, ws.probe_cluster.p, ws.probe_dist.p, nprobe, ws.totals.p + 12, ws.coarse_redo.p, st,
                                      reinterpret_cast<uint16_t *>(ws.qf6.p));  // (the fp6 images are written later: prep)
            pend.prefiltered = true;
            pf.end();
        } else {
            pf.begin(PF_COARSE);
            launch_coarse(idx->cent_t.p, ws.y.p, ws.dist.p, k, dim, nq, k, st);
            pf.end();
            pf.begin(PF_SELECT);
            launch_select(ws.dist.p, k, nprobe, ws.probe_cluster.p, ws.probe_dist.p, 0, nprobe, nq, st);
            pf.end();
        }
        // adaptive probing: cut the ranked rows in place, whichever form filled them (the pre-filtered form's fallback rows are
        // finished inside its launches); on the pass's stream, no host wait
        if (qp.rule.on() && !io.ext_cluster) {
            pf.begin(PF_SELECT);
            RQC(ws.probe_n.ensure(nq));
            probe_cut_kernel<<<ceil_div(nq, 4), 256, 0, st>>>(ws.probe_cluster.p, ws.probe_dist.p, nprobe, nq, qp.rule.ratio, qp.rule.min_probe,
                                                              qp.rule.caps, ws.probe_n.p, qp.rule.out_nprobe);
            pf.end();
        }
        return RQ_OK;
    }

    // the final stage grouped ahead of the quantisation (PassPlan::placed): stream positions, places, the images' layout
    rq_status place_final() {
        const StagePlan &fin = pl.st[pl.nstages - 1];
        const uint32_t nblk = ceil_div(npairs, RQ_RANK_ITEMS);
        RQC(ws.img_final.ensure(((size_t)npairs + 32ull * k + 32) * (12ull * W + 2 + RQ_REC_TAIL)));  // (as ws.recs)
        RQC(ws.pair_begin.ensure(npairs));
        RQC(ws.fin_rank.ensure(npairs));
        RQC(ws.fin_rank_base.ensure((size_t)nblk * k));
        RQC(ws.fin_grp_cnt.ensure(k + 4));
        RQC(ws.fin_grp_start.ensure(k + 1));
        if (pl.fin_additive) RQC(ws.grp_vref.ensure(2 * (size_t)k));
        pf.begin(PF_GROUP);
        {  // every word the pass wants zeroed, in one launch
            ClearSpans cs{};
            cs.p[0] = reinterpret_cast<uint32_t *>(ws.totals.p), cs.n[0] = 16;   // the pass's totals [0..7]
            cs.p[1] = reinterpret_cast<uint32_t *>(ws.stat.p), cs.n[1] = 512;    // the matrix-core scan's step counters (+ developer hooks)
            cs.p[2] = ws.big_list.p + nq, cs.n[2] = 3;
            cs.p[3] = ws.fin_grp_cnt.p, cs.n[3] = k + 4;
            if (pl.large) cs.p[4] = ws.q_hist.p, cs.n[4] = k + 2;
            clear_words_kernel<<<std::max(2u, ceil_div(k + 4, 256)), 256, 0, st>>>(cs);
        }
        pair_prefix_lens_kernel<<<ceil_div(nq, 4), 256, 0, st>>>(idx->offsets.p, probe_cluster, k, nq, nprobe, ws.rough_cnt.p, ws.pair_begin.p, ws.scal.p);
        group_rank_kernel<<<nblk, 1024, (size_t)k * 4, st>>>(nullptr, probe_cluster, npairs, nprobe, nprobe, fin.s_lo, fin.s_hi, k, ws.fin_grp_cnt.p,
                                                            ws.fin_rank.p, ws.fin_rank_base.p, ws.pair_begin.p, idx->offsets.p);
        group_scan_kernel<<<1, 1024, 0, st>>>(ws.fin_grp_cnt.p, k, ws.fin_grp_start.p, 1u | 2u | (pl.fin_additive ? 4u : 0u), ws.img_final.p, 12 * W);
        pf.end();
        return RQ_OK;
    }

    // 3. per-pair query quantisation (:304-317), behind the listed split where the plan wants one, and the queries' stream lengths
    rq_status quantise() {
        const rq_filter *filt = qp.filter;
        uint32_t *qn = pl.write_qn ? ws.qnib.p : nullptr;
        uint32_t *q6 = pl.write_q6 ? ws.qf6.p : nullptr;
        if (pl.will_list) {
            RQC(ws.live_list.ensure((size_t)npairs + 1));
            HIPC(hipMemsetAsync(ws.live_list.p + npairs, 0, 4, st));
            // (filtered: the split reads list lengths from the sub-index's offsets -- a list that admits nothing is an empty one)
            pair_split_kernel<<<ceil_div(npairs, 4096), 1024, 0, st>>>(filt ? filt->sub_off.p : idx->offsets.p, probe_cluster, probe_dist, npairs,
                                                                       nprobe, k, ws.scal.p, ws.live_list.p, ws.live_list.p + npairs);
            // the launches over the listed pairs are sized by their number: one small copy and a wait (tens of microseconds against
            // the milliseconds that 7 of 8 idle lane groups cost)
            // (into the workspace's pinned block, not a pageable stack word; the wait is the price of sizing the launches below by the
            // count -- rq_query_batch_device_begin on a shard-like index therefore returns only once rotate, coarse ranking and this
            // split have run: include/rabitq_hip.h says so)
            unsigned long long *h_live = ws.h_totals + 15;
            *h_live = 0;
            HIPC(hipMemcpyAsync(h_live, ws.live_list.p + npairs, 4, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            nlive = (uint32_t)*h_live;
        }
        PrepPlace pp{};
        if (pl.placed) {
            const StagePlan &fin = pl.st[pl.nstages - 1];
            pp.stream_begin = ws.pair_begin.p, pp.rank = ws.fin_rank.p, pp.blk_base = ws.fin_rank_base.p, pp.grp_start = ws.fin_grp_start.p;
            pp.img = ws.img_final.p, pp.s_lo = fin.s_lo, pp.s_hi = fin.s_hi, pp.tile_images = pl.fin_additive ? 2u : 1u;
        }
        const uint32_t per_block = pl.prep_ppb * pl.prep_pp;
#define RQ_PREP_SMALL(LP, R, PP) \
    do { \
        if (pl.placed) \
            prep_small_placed_kernel<LP, R, PP><<<ceil_div(npairs, per_block), 256, 0, st>>>(ws.y.p, idx->centroids.p, idx->offsets.p, probe_cluster, \
                                                                    probe_dist, npairs, nprobe, ws.scal.p, qn, k, idx->nonempty_lists * 2 < k ? 2u : 1u, pl.qn_slots, pp); \
        else if (pl.will_list) \
            prep_small_listed_kernel<LP, R, PP><<<std::max(1u, ceil_div(nlive, per_block)), 256, 0, st>>>(ws.y.p, idx->centroids.p, idx->offsets.p, probe_cluster, \
                                                                    probe_dist, ws.live_list.p, nlive, nprobe, ws.scal.p, qn, q6, k); \
        else \
            prep_small_kernel<LP, R, PP><<<ceil_div(npairs, per_block), 256, 0, st>>>(ws.y.p, idx->centroids.p, idx->offsets.p, probe_cluster, \
                                                                    probe_dist, npairs, nprobe, ws.scal.p, qn, q6, k, idx->nonempty_lists * 2 < k ? 2u : 1u, pl.qn_slots); \
    } while (0)
#define RQ_X(D, LP, R, PPB, PP) \
    if (dim == D) RQ_PREP_SMALL(LP, R, PP); \
    else
        RQ_PREP_SHAPES(RQ_X)
#undef RQ_X
#undef RQ_PREP_SMALL
            prep_kernel<<<ceil_div(npairs, 4), 256, 0, st>>>(ws.y.p, idx->centroids.p, idx->offsets.p, probe_cluster, probe_dist,
                                                             npairs, nprobe, dim, ws.scal.p,
                                                             scan_is_fused(W) ? nullptr : ws.planes.p,   // only the generic-W scan reads bit planes
                                                             qn, q6, nullptr, k, 1u);
        if (filt) {  // (the rough counter: the admitted rows of the probed lists; the stream lengths go to stream_len)
            RQC(ws.stream_len.ensure(nq));
            pair_prefix_filtered_kernel<<<ceil_div(nq, 4), 256, 0, st>>>(ws.scal.p, nq, nprobe, ws.rough_cnt.p, probe_cluster, filt->sub_off.p, k,
                                                                         ws.stream_len.p);
        } else if (!pl.placed)  // (placed: the stream positions were needed ahead of the quantisation, which has copied them into the scalars)
            pair_prefix_kernel<<<ceil_div(nq, 4), 256, 0, st>>>(ws.scal.p, nq, nprobe, ws.rough_cnt.p);
        return RQ_OK;
    }

    // the rerank order of a large batch; 4. ranker state (rerank.rs:70-77, :129-139) and per-query counters
    rq_status orders_state() {
        if (pl.large) {  // large batch: rerank queries of the same nearest list back to back (cache locality of the row gather)
            if (!pl.placed) HIPC(hipMemsetAsync(ws.q_hist.p, 0, (size_t)(k + 2) * 4, st));
            order_count_kernel<<<ceil_div(nq, 256), 256, 0, st>>>(probe_cluster, nprobe, nq, k, ws.q_hist.p);
            group_scan_kernel<<<1, 1024, 0, st>>>(ws.q_hist.p, k + 1, ws.q_start.p, 0u, nullptr, 0u);  // also zeroes the histogram: cursor
            order_scatter_kernel<<<ceil_div(nq, 256), 256, 0, st>>>(probe_cluster, nprobe, nq, k, ws.q_start.p, ws.q_hist.p,
                                                                    ws.q_order.p);
            rerank_order = ws.q_order.p;
        }
        init_state_kernel<<<ceil_div(nq, 256), 256, 0, st>>>(rs, ws.surv_cnt.p, nq, qp.thr_init, d_row_map);
        if (!pl.placed) {  // (placed: cleared by the pass's one clearing launch)
            HIPC(hipMemsetAsync(ws.totals.p, 0, 8 * sizeof(unsigned long long), st));
            HIPC(hipMemsetAsync(ws.big_list.p + nq, 0, 12, st));
            HIPC(hipMemsetAsync(ws.stat.p, 0, 256 * sizeof(unsigned long long), st));  // the matrix-core scan's step counters (+ developer hooks)
        }
        return RQ_OK;
    }

    // a stage's grouping and its work records (query operand + scalars + current threshold + local range)
    rq_status stage_group_fill(StageRun &r) {
        const StagePlan &s = r.s;
        ScanArgs &a = r.a;
        pf.begin(PF_GROUP);
        a.cluster_major = s.cluster_major ? 1u : 0u;
        if (s.placed) {
            // grouped and filled already, but for what hangs on the thresholds: the tails' threshold part and, additive gate, C_q and
            // the lists' v' ranges
            stage_tail_kernel<<<k, 256, 0, st>>>(ws.img_final.p, ws.fin_grp_start.p, ws.fin_grp_cnt.p, ws.thr.p, 12 * W, idx->fstats,
                                                 s.additive ? 2u : 1u, idx->list_uref.p, ws.grp_vref.p);
            a.ngroups = k;
        } else if (s.cluster_major) {
            HIPC(hipMemsetAsync(ws.grp_cnt.p, 0, (size_t)((k + 4) & ~3u) * 4, st));  // 16-byte multiple: one fill kernel
            if (s.ranked) {
                const uint32_t nblk = ceil_div(s.stage_pairs, RQ_RANK_ITEMS);
                RQC(ws.pair_rank.ensure(s.stage_pairs));
                RQC(ws.rank_base.ensure((size_t)nblk * k));
                group_rank_kernel<<<nblk, 1024, (size_t)k * 4, st>>>(ws.scal.p, probe_cluster, s.stage_pairs, nprobe, s.slot_hi, s.s_lo,
                                                                    s.s_hi, k, ws.grp_cnt.p, ws.pair_rank.p, ws.rank_base.p);
            } else
                group_count_kernel<<<ceil_div(s.stage_pairs, 256), 256, 0, st>>>(ws.scal.p, probe_cluster, s.stage_pairs, nprobe,
                                                                               s.slot_hi, s.s_lo, s.s_hi, ws.grp_cnt.p);
            group_scan_kernel<<<1, 1024, 0, st>>>(ws.grp_cnt.p, k, ws.grp_start.p, (s.matrix ? 1u : 0u) | (s.ranked ? 2u : 0u) | (s.additive ? 4u : 0u), ws.recs.p, 12 * W);
            a.ngroups = k;
        } else
            a.ngroups = npairs;
        const uint32_t *operand = s.matrix ? ws.qf6.p : (scan_is_fused(W) ? ws.qnib.p : reinterpret_cast<const uint32_t *>(ws.planes.p));
        if (!(pl.sb_fill_final && !s.cluster_major) && !s.placed) {  // (the small-batch kernel has written a pair-major final stage's records already)
            // a sharded pass visits only the listed pairs when the stage's work items ARE the pairs (every slot can be in the stage)
            const bool fill_listed = pl.will_list && s.ranked && s.slot_hi == nprobe;
            const uint32_t fill_items = fill_listed ? nlive : s.stage_pairs;
            // eight lanes per pair (16-byte copies) wherever the operand rows are 16-byte aligned: record-major records and the additive
            // tile images (the bf16-form images keep rows of opdw + 2 dwords: 8-byte aligned, sixteen lanes); final stage of the
            // headline step 0.75 -> 0.45 ms
            const bool fill8 = !s.matrix || s.additive;
            auto fill = fill8 ? stage_fill_kernel<8> : stage_fill_kernel<16>;
            if (fill_items)
                fill<<<ceil_div(fill_items, fill8 ? 32 : 16), 256, 0, st>>>(ws.scal.p, probe_cluster, operand, ws.thr.p, fill_items, nprobe, s.slot_hi,
                                                                           s.matrix ? 12 * W : 8 * W, s.s_lo, s.s_hi, a.cluster_major, ws.grp_start.p, ws.grp_cnt.p,
                                                                           ws.recs.p, idx->fstats, s.matrix ? (s.additive ? 2u : 1u) : 0u,
                                                                           s.ranked ? ws.pair_rank.p : nullptr, ws.rank_base.p, k, idx->list_uref.p,
                                                                           fill_listed ? ws.live_list.p : nullptr);
        }
        if (s.additive && !s.placed) {  // the stage's v' ranges per list (the candidates' side of the additive bound is built from them in the scan)
            RQC(ws.grp_vref.ensure(2 * (size_t)k));
            group_vrange_kernel<<<k, 256, 0, st>>>(ws.recs.p, ws.grp_start.p, ws.grp_cnt.p, 12 * W, ws.grp_vref.p);
        }
        if (s.additive) pend.additive = true;
        pf.end();
        return RQ_OK;
    }

    void stage_launch_scan(StageRun &r) {
        pf.begin(r.s.matrix ? PF_SCAN_MATRIX : PF_SCAN);
        if (r.s.matrix) launch_scan_mfma(r.sp, r.a, idx->W, st, r.s.additive);  // (the kernel must match the record format stage_fill_kernel wrote)
        else launch_scan(r.sp, r.a, idx->W, st);
        pf.end();
    }

    // Arena stage (large batches of an index whose survivor counts are very unequal -- hard distribution, final stage:
    // median 12 survivors per query, mean 2 800, maximum beyond 100 000): every stage that CAN exceed the uniform capacity
    // (span > capacity) appends its survivors to one arena shared by all queries while counting them per query; the
    // exact counts size a segment per query (prefix sum), the host makes room for their sum, and a scatter pass moves
    // every run to its query's segment.  The workspace follows the SUM of the survivors, not nq x the worst query, and
    // no query can overflow.
    rq_status stage_scan_arena(StageRun &r) {
        const rq_filter *filt = qp.filter;
        ScanArgs &a = r.a;
        // capacity: what earlier batches needed (+ headroom), at least half the uniform buffers' worth; a shard holds
        // 1 / RQ_ARENA_SHARDS of it
        // (the hint is read here, not by the planner: an earlier arena stage of this pass may just have raised it)
        uint64_t want = std::max<uint64_t>(hints_of(idx, filt).arena.load(), (uint64_t)nq * qp.cap / 2);
        unsigned long long total_slots = 0;
        uint32_t arena_rsub = 0;
        bool arena_retried = false;
        ws.arena_failed = true;  // (until the stage has its arena: an allocation failure or a give-up below returns from inside the loop)
#ifdef RQ_DEV_ABLATIONS
        if (g_seg_opt.load() == 3) {  // developer build only (make dev): the arena cannot be had -- through a REAL failing allocation (1 PiB), sticky error and all
            DevBuf<SurvRec> never;
            RQC(never.alloc(1ull << 46));
            return fail(RQ_ERR_OOM, "survivor arena: injected failure (developer hook survivor_segments = 3)");
        }
#endif
        for (int attempt = 0;; ++attempt) {
            want = std::min<uint64_t>(want, 0xFFFF0000ull);
            RQC(ws.arena_recs.ensure(want));
            RQC(ws.arena_runs.ensure(want));
            RQC(ws.arena_cur.ensure(RQ_ARENA_SHARDS + 4));
            RQC(ws.arena_fail.ensure(RQ_ARENA_SHARDS));
            HIPC(hipMemsetAsync(ws.arena_cur.p, 0, (RQ_ARENA_SHARDS + 4) * 8, st));
            HIPC(hipMemsetAsync(ws.arena_fail.p, 0xFF, RQ_ARENA_SHARDS * 4, st));
            ScanExtra hx{};
            RQC(ws.arena_places.ensure(want));
            hx.arena_places = ws.arena_places.p, hx.allow = filt ? filt->pos_bits.p : nullptr;
            hx.arena_recs = ws.arena_recs.p, hx.arena_runs = reinterpret_cast<uint4 *>(ws.arena_runs.p), hx.arena_cur = ws.arena_cur.p;
            hx.arena_fail = ws.arena_fail.p;
            {  // seven eighths of the arena in shards, the rest as the common area (what a full shard turns away: few, heavy blocks)
                const uint64_t have = std::min<uint64_t>(ws.arena_recs.count, ws.arena_runs.count);
                hx.arena_sub = hx.arena_rsub = (uint32_t)(have * 7 / 8 / RQ_ARENA_SHARDS);
                hx.arena_common = (uint32_t)std::min<uint64_t>(have - (uint64_t)hx.arena_sub * RQ_ARENA_SHARDS, 0xFFFFFF00ull);
            }
            arena_rsub = hx.arena_rsub;
            RQC(ws.scan_extra.ensure(1));
            HIPC(hipMemcpyAsync(ws.scan_extra.p, &hx, sizeof hx, hipMemcpyHostToDevice, st));
            a.x = ws.scan_extra.p;
            a.dense_dir = 0u;
            stage_launch_scan(r);
            pf.begin(PF_GROUP);
            // sizes from the exact counts, one round trip for the shard-overflow flag and the sum of the segments
            seg_exact_kernel<<<ceil_div(nq, 256), 256, 0, st>>>(ws.surv_cnt.p, nq, 64u, ws.q_cap.p);
            seg_scan_kernel<<<1, 1024, 0, st>>>(ws.q_cap.p, nq, ws.q_base.p, ws.arena_cur.p + RQ_ARENA_SHARDS + 1);
            unsigned long long tail[2] = {0, 0};
            HIPC(hipMemcpyAsync(tail, ws.arena_cur.p + RQ_ARENA_SHARDS, 16, hipMemcpyDeviceToHost, st));
            HIPC(hipStreamSynchronize(st));
            total_slots = tail[1];
            if (!(uint32_t)tail[0]) break;
            pf.end();
            if (attempt >= 6 || want >= 0xFFFF0000ull) return fail(RQ_ERR_OOM, "survivor arena kept overflowing");
            // A shard AND the common area ran full: the stage again (its per-query counters start from zero again) with a
            // larger arena: the exact counts are known now.  A grid of at least 2048 blocks spreads over all the shards: twice
            // the arena, at least the survivors + a quarter.  A SMALL grid uses only a few of the 2048 shards, so doubling
            // alone could stay short for ever (found by the fuzz driver: 700 queries whose every candidate survives, on a
            // 130-block grid): there the common area (an eighth of the arena) is made to hold ALL of the stage's survivors,
            // which takes whatever the shards turn away
            const uint64_t nblocks = a.use_table ? a.ngroups : (uint64_t)a.ngroups * a.tiles_per_group;
            HIPC(hipMemsetAsync(ws.surv_cnt.p, 0, (size_t)nq * sizeof(unsigned long long), st));
            want = std::max<uint64_t>(want * 2, 1u << 20);
            if (nblocks < RQ_ARENA_SHARDS) want = std::max<uint64_t>(want, 8 * total_slots + (1u << 16)), arena_retried = true;
            else want = std::max<uint64_t>(want, total_slots + total_slots / 4);
        }
        ws.arena_failed = false;
        {  // remember what this stage needed
            std::atomic<uint64_t> &arena_hint = hints_of(idx, filt).arena;
            uint64_t cur = arena_hint.load();
            const uint64_t learnt = std::max<uint64_t>(total_slots + total_slots * 3 / 5, arena_retried ? std::min<uint64_t>(want, 0xFFFF0000ull) : 0ull);
            while (cur < learnt && !arena_hint.compare_exchange_weak(cur, learnt)) {}
        }
        if (total_slots > ws.surv.count || total_slots > ws.runs.count || total_slots > ws.runs_tmp.count) {
            const uint64_t grow = total_slots + total_slots / 8;
            RQC(ws.surv.ensure(grow));
            RQC(ws.runs.ensure(grow));
            RQC(ws.runs_tmp.ensure(grow));
        }
        r.sp.surv = ws.surv.p, r.sp.runs = ws.runs.p;
        arena_scatter_kernel<<<dim3(RQ_ARENA_SHARDS + RQ_ARENA_COMMON_BLOCKS, 2), 256, 0, st>>>(ws.arena_recs.p, reinterpret_cast<const uint4 *>(ws.arena_runs.p), ws.arena_cur.p,
                                                                          ws.arena_fail.p, arena_rsub, ws.q_base.p, ws.arena_places.p, ws.surv.p, ws.runs_tmp.p);
        r.runs_in_tmp = true;
        pf.end();
        r.seg = QSeg{ws.q_base.p, ws.q_cap.p, qp.cap};
        pend.seg_slots = std::max<uint64_t>(pend.seg_slots, total_slots);
        return RQ_OK;
    }

    // a stage's scan: its arguments, the grid (plain or through the tile table), then the launch -- inside the arena loop for an arena stage
    rq_status stage_scan(StageRun &r) {
        const StagePlan &s = r.s;
        ScanArgs &a = r.a;
        ScanPtrs &sp = r.sp;
        sp.codes = reinterpret_cast<const uint32_t *>(idx->codes.p), sp.factors = idx->factors.p, sp.offsets = idx->offsets.p;
        sp.grp_start = s.placed ? ws.fin_grp_start.p : ws.grp_start.p;
        sp.grp_cnt = s.placed ? ws.fin_grp_cnt.p : ws.grp_cnt.p;
        sp.recs = s.placed ? ws.img_final.p : ws.recs.p;
        sp.surv = ws.surv.p, sp.runs = ws.runs.p, sp.surv_cnt = ws.surv_cnt.p;
        sp.stat = ws.stat.p;  // 64 x {sub-tile steps, exact-path steps} of the matrix-core scan
        sp.list_uref = idx->list_uref.p, sp.grp_vref = ws.grp_vref.p;
        sp.arena = s.arena_stage, sp.filtered = qp.filter != nullptr;
        a.x = qp.filter ? qp.filter->extra.p : nullptr;  // (an arena stage points it at its own ScanExtra, the filter's bitmap included)
        a.cap = qp.cap, a.dbg = pl.dbg;
        a.tiles_per_group = s.tiles_per_group;
        sp.tile_table = nullptr;
        if (s.want_table) {
            uint32_t count = 0;
            sp.tile_table = get_tile_table(idx, s.tile, &count);
            if (sp.tile_table) a.use_table = 1u, a.ngroups = count, a.tiles_per_group = 1u;
        }
        a.dense_dir = s.dense_cells ? 1u : 0u;
        r.seg = QSeg{nullptr, nullptr, qp.cap};  // uniform geometry: every stage but a segmented one
        if (s.arena_stage) {
            RQC(stage_scan_arena(r));
        } else {
            if (s.dense_cells) {
                pf.begin(PF_SORT);
                clear_dir_kernel<<<ceil_div((uint64_t)qp.nq * s.dense_cells, 256), 256, 0, st>>>(ws.runs.p, qp.nq, r.seg, s.dense_cells);
                pf.end();
            }
            stage_launch_scan(r);
        }
        if (s.matrix) pend.matrix_stages++;
        // (launches, not stages: a grid beyond the launch bound -- or option max_scan_blocks -- is issued in chunks; an empty grid still
        // counts as the stage's one)
        const uint32_t launches = std::max(1u, scan_chunk_count(a));
        if (prof_acc && s.additive) prof_acc->matrix_additive_launches += launches;
        if (prof_acc) prof_acc->scan_launches += launches;
        if (prof_acc && s.matrix) {
            prof_acc->matrix_launches += launches;
            pend.matrix_ranges[pend.n_matrix_ranges++] = {s.s_lo, s.s_hi};
        }
        return RQ_OK;
    }

    // sort_runs_mid_kernel's bitmap words; scan_debug bit 2048 (test hook): none, so long directories take the fall-back orderings
    uint32_t mid_lds_words() const { return (pl.dbg & 2048) ? 0u : RQ_SORT_MID_LDS_WORDS; }

    // the exact rerank of every survivor by the whole chip (grid (gx, nq)), reading the index's rows as they are stored
    void launch_accurate(uint32_t gx, const QSeg &seg, const uint32_t *order) {
        with_row_kind(idx->rows.kind(), [&](auto row_kind) {
            accurate_kernel<decltype(row_kind)::value><<<dim3(gx, nq), 256, (size_t)dim * sizeof(float), st>>>(ws.surv.p, ws.surv_cnt.p, seg, idx->view(), qpad, dim,
                                                                                                            order, probe_cluster, nprobe);
        });
    }

    // small batch: one fused launch per stage (launch-bound regime)
    void stage_finish_small(StageRun &r) {
        const QSeg &seg = r.seg;
        pf.begin(PF_RERANK);
        const uint32_t fin_threads = nq <= 16 ? 1024u : 256u;  // a handful of queries: more lanes on each one's rerank
        // survivor buffers beyond the default mean this index / these queries leave long run directories (overflow
        // re-runs, loose thresholds): those are ordered by the slot-bucketed kernel first; the fused kernel then sorts
        // only what fits its LDS
        uint32_t flags = qp.cap > RQ_DEFAULT_CAP && nprobe <= 1024 ? 1u : 0u;  // bit 0: the directories are presorted, bit 1: the rows are gathered
        if (flags) {
            sort_runs_kernel<<<nq, 64, 0, st>>>(ws.runs.p, ws.surv_cnt.p, seg, ws.big_list.p, ws.big_list.p + nq, RQ_SORT_LDS_RECS, nullptr);
            sort_runs_mid_kernel<<<std::min(nq, 256u), 256, RQ_SORT_MID_LDS_WORDS * 8, st>>>(ws.runs.p, ws.use_runs_tmp ? ws.runs_tmp.p : nullptr, ws.surv_cnt.p,
                                                                                          seg, ws.big_list.p, ws.big_list.p + nq, nprobe, 0u,
                                                                                          mid_lds_words());
        }
        if (pl.small && !qp.heuristic) {  // small-batch path, heap ranker: the stage's finish also writes the results and the totals
            // a handful of queries: their final-stage survivors (~1000 rows each) are gathered by the whole chip -- one block
            // per query would pull them through a single CU's memory pipeline (~30 GB/s)
            if (nq <= 32) {
                launch_accurate(std::max(1u, std::min(16u, 256u / nq)), seg, nullptr);
                flags |= 2u;
            }
            with_row_kind(idx->rows.kind(), [&](auto row_kind) {  // the kernels whose rerank reads the index's rows (kernels_rerank.h: accurate_rows<KIND>)
                constexpr int K = decltype(row_kind)::value;
                auto finish = topk < 64 ? sb_finish_kernel<true, K> : sb_finish_kernel<false, K>;
                finish<<<nq, fin_threads, (size_t)dim * sizeof(float) + (2 * RQ_SBF_RUNS + RQ_SBF_RECS) * 16, st>>>(
                    ws.surv.p, ws.runs.p, ws.surv_cnt.p, seg, idx->view(), qpad, dim, topk, rs, probe_cluster, nprobe, flags,
                    idx->map_ids.p, io.out_dist, io.out_id, io.out_n, ws.rough_cnt.p, ws.totals.p);
            });
            sb_results_done = true;
        } else {
            with_row_kind(idx->rows.kind(), [&](auto row_kind) {
                constexpr int K = decltype(row_kind)::value;
                auto finish = qp.heuristic ? stage_finish_kernel<true, K> : stage_finish_kernel<false, K>;
                finish<<<nq, fin_threads, (size_t)dim * sizeof(float), st>>>(ws.surv.p, ws.runs.p, ws.surv_cnt.p, seg, idx->view(), qpad, dim, topk, rs,
                                                                             probe_cluster, nprobe, flags);
            });
        }
        pf.end();
    }

    // the 8-bit pre-filter with its rows through the LDS ring (plan: rerank_ring_rule; dim = 16 NPC)
    template <int NPC>
    void launch_ring8(uint32_t gx, const QSeg &seg) {
        accurate_ring8_kernel<RQ_RING_V, NPC><<<dim3(gx, nq), 256, rerank_ring_lds(dim, nprobe), st>>>(
            ws.surv.p, ws.surv_cnt.p, seg, idx->base.p, idx->base_q8.p, idx->list_q8.p, qpad, rerank_order, ws.thr.p, probe_cluster, nprobe,
            ws.nshadow.p, k);
    }

    // large batch: full-chip rerank, then run-directory sort, then one replay wave per query
    void stage_finish_large(StageRun &r) {
        const uint32_t dense_cells = r.s.dense_cells;
        const QSeg &seg = r.seg;
        pf.begin(PF_RERANK);
        const uint32_t gx = std::max(1u, std::min(16u, 4096u / std::max(nq, 1u)));
        // past the first stage the thresholds are finite: survivors go through the shadow rows first (the plan's rule, and its route)
        const bool prefilter = r.s.prefilter;
        if (r.s.rerank_ring) {
#define RQ_RING8(NPC) case NPC: launch_ring8<NPC>(gx, seg); break;
            switch (dim / 16) {
                RQ_RING8_NPC(RQ_RING8)
                default: break;  // (not reached: rerank_ring_rule admits the dimensions of the same list only)
            }
#undef RQ_RING8
        } else if (r.s.rerank_q8)
            accurate_filtered8_kernel<<<dim3(gx, nq), 256, (size_t)dim * sizeof(float) + (nprobe <= RQ_ACC8_LDS_PROBES ? (size_t)nprobe * 16 : 0), st>>>(
                ws.surv.p, ws.surv_cnt.p, seg, idx->base.p, idx->base_q8.p, idx->list_q8.p, qpad, dim, rerank_order, ws.thr.p,
                probe_cluster, nprobe, ws.nshadow.p, k);
        else if (idx->base_h.p && prefilter)
            accurate_filtered_kernel<<<dim3(gx, nq), 256, (size_t)dim * sizeof(float), st>>>(
                ws.surv.p, ws.surv_cnt.p, seg, idx->base.p, idx->base_h.p, qpad, dim, rerank_order, ws.thr.p,
                ws.nshadow.p);
        else if (idx->split_rows && prefilter)  // tiered: the rows' own first plane is the pre-filter
            accurate_split_kernel<<<dim3(gx, nq), 256, (size_t)dim * sizeof(float) + (nprobe <= RQ_ACC8_LDS_PROBES ? (size_t)nprobe * 16 : 0), st>>>(
                ws.surv.p, ws.surv_cnt.p, seg, idx->view(), qpad, dim, rerank_order, ws.thr.p, probe_cluster, nprobe, ws.nshadow.p);
        else  // every survivor reads its row: 4*dim bytes, or the 2*dim / dim bytes of a half-precision / byte row (no shadow rows, no first plane)
            launch_accurate(gx, seg, rerank_order);
        if (qp.range)  // every survivor has its exact distance (or +inf: proven outside the radius): count the hits, nothing to order
            range_count_kernel<<<ceil_div(nq, 4), 256, 0, st>>>(ws.surv.p, ws.surv_cnt.p, qp.cap, ws.thr.p, nq, ws.range_hits.p, ws.need.p,
                                                                ws.ovf.p, ws.precise.p, ws.nsurv.p);
        pf.end();
        if (qp.range) return;
        if (!dense_cells) {
            pf.begin(PF_SORT);
            sort_runs_kernel<<<nq, 64, 0, st>>>(ws.runs.p, ws.surv_cnt.p, seg, ws.big_list.p, ws.big_list.p + nq, 512u,
                                                r.runs_in_tmp ? ws.runs_tmp.p : nullptr);
            // queries with long run directories (loose thresholds, very unequal lists): cell-bitmap ordering, persistent blocks walking the list
            sort_runs_mid_kernel<<<pl.mid_blocks, 256, RQ_SORT_MID_LDS_WORDS * 8, st>>>(ws.runs.p, (ws.use_runs_tmp || r.runs_in_tmp) ? ws.runs_tmp.p : nullptr,
                                                                                       ws.surv_cnt.p, seg, ws.big_list.p, ws.big_list.p + nq, nprobe,
                                                                                       r.runs_in_tmp ? 1u : 0u, mid_lds_words());
            pf.end();
        }
        pf.begin(PF_REPLAY);
        if (qp.heuristic)
            replay_kernel<true><<<nq, 64, 16, st>>>(ws.surv.p, ws.runs.p, ws.surv_cnt.p, seg, topk, rs, dense_cells);
        else if (topk < 64)  // the heap in registers, one element per lane (a push before a pop holds topk + 1 elements)
            replay_kernel<false, true><<<nq, 64, 16, st>>>(ws.surv.p, ws.runs.p, ws.surv_cnt.p, seg, topk, rs, dense_cells);
        else
            replay_kernel<false><<<nq, 64, (size_t)topk * 8, st>>>(ws.surv.p, ws.runs.p, ws.surv_cnt.p, seg, topk, rs, dense_cells);
        pf.end();
    }

    // 6. results, the totals' way back to the host, and what finish_pass needs to know
    rq_status results(size_t total_span) {
        pf.begin(PF_REPLAY);
        if (!sb_results_done) {  // (else: written by sb_query_kernel / sb_finish_kernel together with the totals)
            // (a range pass writes no rows: the hits stay in the survivor buffers, the caller sizes the result from their counts and emits their keys)
            if (qp.heuristic && !qp.range) {
                sort_survivors_kernel<<<nq, 256, 0, st>>>(ws.arr.p, ws.arr_len.p, qp.hcap);
                finalize_heuristic_kernel<<<ceil_div((uint64_t)nq * topk, 256), 256, 0, st>>>(rs, nq, topk, d_row_map, idx->map_ids.p,
                                                                                               io.out_dist, io.out_id, io.out_n);
            } else if (!qp.range) {
                finalize_heap_kernel<<<ceil_div((uint64_t)nq * topk, 256), 256, 0, st>>>(rs, nq, topk, d_row_map, idx->map_ids.p, io.out_dist,
                                                                                          io.out_id, io.out_n);
            }
            metrics_sum_kernel<<<std::min(256u, ceil_div(nq, 256)), 256, 0, st>>>(
                ws.rough_cnt.p, ws.precise.p, ws.need.p, qp.heuristic ? ws.arr_len.p : nullptr, ws.nsurv.p, ws.nshadow.p, nq, ws.ovf.p, qp.hcap,
                ws.totals.p);
        }
        pf.end();
        if (pf.on) (void)hipEventRecord(pf.spans[total_span].b, st);
        HIPC(hipMemcpyAsync(ws.h_totals, ws.totals.p, 7 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        ws.h_totals[7] = 0, ws.h_totals[8] = 0, ws.h_totals[9] = 0, ws.h_totals[10] = 0;
        if (pend.prefiltered) HIPC(hipMemcpyAsync(ws.h_totals + 10, ws.totals.p + 12, 8, hipMemcpyDeviceToHost, st));
        if (pend.matrix_stages) {  // sub-tile steps of the matrix-core stages and how many of them took the exact path
            stat_fold_kernel<<<1, 64, 0, st>>>(ws.stat.p, ws.stat.p + 200);
            HIPC(hipMemcpyAsync(ws.h_totals + 8, ws.stat.p + 200, 16, hipMemcpyDeviceToHost, st));
        }
        if (pl.large)  // (the long-directory hint only sizes launches of large batches: a small batch saves the copy's round trip)
            HIPC(hipMemcpyAsync(ws.h_totals + 7, ws.big_list.p + nq + 2, 4, hipMemcpyDeviceToHost, st));
        ws.pend = pend;
        return RQ_OK;
    }
};

// Runs one pass of `call` (already advanced to the pass's first query) over qp.nq queries.  Results go to row row_map[b] (or b) of
// the call's output arrays.  On return the stream is synchronised, unless `defer`: the caller then finishes the pass (finish_pass).
static rq_status run_pass(Workspace &ws, const QueryCall &call, const QueryParams &qp, const uint32_t *d_row_map, PassResult *res,
                          rq_profile_t *prof_acc, bool defer) {
    const rq_index *idx = call.idx;
    const QueryIO &io = call.io;
    PassPlan pl;
    plan_pass(idx, qp, d_row_map != nullptr, io.ext_cluster != nullptr, pl);
    Pass c{idx, ws, qp, pl, ws.prof, ws.stream, idx->dim, idx->k, idx->W, qp.nq, qp.topk, pl.nprobe, pl.npairs, io, d_row_map,
           prof_acc, io.d_q, ws.probe_cluster.p, ws.probe_dist.p};
    c.rs.thr = ws.thr.p, c.rs.heap_len = ws.heap_len.p, c.rs.heap_key = ws.heap_key.p, c.rs.heap_id = ws.heap_id.p;
    c.rs.precise = ws.precise.p, c.rs.need = ws.need.p, c.rs.nsurv = ws.nsurv.p, c.rs.nshadow = ws.nshadow.p, c.rs.recent_max = ws.recent.p, c.rs.win_count = ws.win_count.p;
    c.rs.arr_len = ws.arr_len.p, c.rs.arr = ws.arr.p, c.rs.hcap = qp.hcap, c.rs.ovf = ws.ovf.p;
    c.pend.nq = qp.nq, c.pend.cap = qp.cap, c.pend.filter = qp.filter, c.pend.range = qp.range, c.pend.large = pl.large;
    Prof &pf = ws.prof;
    pf.reset(g_profiling.load(), ws.stream);
    pf.begin(PF_TOTAL);
    const size_t total_span = pf.spans.size() ? pf.spans.size() - 1 : 0;
    if (pl.small) {
        RQC(c.small_front());
    } else {
        RQC(c.rotate_coarse());
        if (pl.placed) RQC(c.place_final());
        pf.begin(PF_PREP);
        RQC(c.quantise());
        RQC(c.orders_state());
        pf.end();
    }
    for (uint32_t i = 0; i < pl.nstages; ++i) {
        StageRun r{pl.st[i], i};
        RQC(c.stage_group_fill(r));
        RQC(c.stage_scan(r));
        if (finish_large(pl, qp)) c.stage_finish_large(r);  // (host_plan.h: also a small batch whose survivor buffers are large)
        else c.stage_finish_small(r);
    }
    RQC(c.results(total_span));
    if (defer) return RQ_OK;
    return finish_pass(idx, ws, res, prof_acc);
}
