// host_plan.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  What one query pass will do, decided ONCE before anything is enqueued: plan_pass reads the index,
// the pass's parameters and one snapshot of the options and hints; it makes no HIP call, launches nothing and reads no workspace
// buffer.  host_query.h (run_pass) executes the plan; host_call.h decides which passes a call runs.
#pragma once
struct QueryParams {
    uint32_t nq, len, probe, topk;
    bool heuristic;
    uint32_t cap, hcap;  // survivor / heuristic-array capacity per query (powers of two)
    // Seeded pass (rq_query_batch_device_seeded): per-query initial thresholds (device; f32::MAX = none).  A first pass
    // runs the whole stream as ONE stage under them; an overflow re-run (row map given) starts from them and stages as usual.
    const float *thr_init = nullptr;
    // Segmented pass: `cap` bounds the stages whose span fits it; a stage that can exceed it appends to the shared arena and
    // its survivors are scattered into per-query segments sized by their exact counts (the workspace then scales with the
    // sum of the survivors instead of nq x the worst query)
    bool seg_final = false;
    bool ext_lists = false;  // the probe lists come from the caller: no coarse ranking in the pass (and no nq x k distance matrix)
    // Filtered pass (rq_query_batch*_filtered): only the filter's rows can survive the scan, the pairs whose list admits nothing
    // are settled before the quantisation, and the rough counter counts admitted rows.  Every pass of the call carries it (overlapped
    // passes, overflow re-runs, arena repeats).
    const rq_filter *filter = nullptr;
    // Range pass (host_range.h): thr_init holds the radii, the whole stream runs as ONE stage under them (re-runs too: a fixed
    // threshold has nothing to learn), and behind the exact distances the pass only counts each query's hits (ws.range_hits) --
    // no run ordering, no replay, no result rows; topk is 1 (the ranker state is allocated, not used).
    bool range = false;
    // Adaptive probing (rq_probe_rule_t; kernels_coarse.h: probe_cut_kernel): the pass cuts every query's ranked probe row at the end of
    // rotate_coarse and is planned like a pass over caller-supplied lists (plan_pass).  Overflow re-runs carry no rule:
    // they take the pass's cut rows as their probe lists.
    ProbeRule rule;
};

// The device arrays of a query call, or of one pass of it (QueryCall::at).
struct QueryIO {
    const float *d_q = nullptr;  // nq x len
    float *out_dist = nullptr;   // nq x topk (a range call has no result rows: null)
    uint32_t *out_id = nullptr, *out_n = nullptr;
    // nq x min(probe, k): if given, the probe lists are taken from there (visiting order as supplied; id 0xFFFFFFFF = no list)
    // instead of being ranked here
    const uint32_t *ext_cluster = nullptr;
    const float *ext_dist = nullptr;
    const float *thr_init = nullptr;  // nq: a seeded call's initial thresholds, a range call's radii (QueryParams::thr_init)
};
// One query call as every layer below the C entries sees it.  Overflow re-runs address a pass's arrays through a row map, so they take
// the pass's QueryCall as it is.
struct QueryCall {
    rq_index *idx = nullptr;
    const rq_filter *filter = nullptr;
    uint32_t len = 0, probe = 0, topk = 0;
    bool heuristic = false;
    QueryIO io;
    ProbeRule rule;  // adaptive probing (rule.on()): caps and the nprobe output advance with the pass
    uint32_t npb() const { return std::min(probe, idx->k); }  // columns of the probe lists
    // The call of a pass that starts at query q0: the one place that knows the arrays' strides.
    QueryCall at(uint64_t q0) const {
        QueryCall c = *this;
        c.io.d_q = io.d_q + q0 * len;
        c.io.out_dist = io.out_dist ? io.out_dist + q0 * topk : nullptr;
        c.io.out_id = io.out_id ? io.out_id + q0 * topk : nullptr;
        c.io.out_n = io.out_n ? io.out_n + q0 : nullptr;
        c.io.ext_cluster = io.ext_cluster ? io.ext_cluster + q0 * npb() : nullptr;
        c.io.ext_dist = io.ext_dist ? io.ext_dist + q0 * npb() : nullptr;
        c.io.thr_init = io.thr_init ? io.thr_init + q0 : nullptr;
        c.rule.caps = rule.caps ? rule.caps + q0 : nullptr;
        c.rule.out_nprobe = rule.out_nprobe ? rule.out_nprobe + q0 : nullptr;
        return c;
    }
};
// The parameters of a pass of `c` over nq queries with the given capacities (what the call decides; the caller adds seg_final / ext_lists / range).
static QueryParams pass_params(const QueryCall &c, uint32_t nq, uint32_t cap, uint32_t hcap) {
    QueryParams qp{nq, c.len, c.probe, c.topk, c.heuristic, cap, hcap};
    qp.thr_init = c.io.thr_init, qp.filter = c.filter, qp.rule = c.rule;
    return qp;
}

#define RQ_DEFAULT_CAP 4096u
#define RQ_MAX_CAP_HINT 32768u
#define RQ_MAX_NQ_PER_PASS 65536u
#define RQ_MAX_PROBE 16384u
#define RQ_SB_FILT_REACH 65536u  // stored stream positions a query's block scans at most on a filtered small-batch pass

// The dimensions with a lane-group quantisation kernel and its shape: X(dim, lanes per pair, rounds, pairs per block and round, pairs
// in flight per lane group).  Every other dimension takes the generic prep_kernel (and neither a listed nor a placed pass).
// dim 128: 16 lanes per pair, two rounds of 64 dimensions, two pairs per lane group in flight (round 4: 32 lanes, one round, four
// pairs: the min / max / sum reductions over the pair's lanes are half of the kernel's vector work, and half the lanes do a
// quarter less of it: 0.96 -> 0.66 ms per 4.2 M pairs)
// dim 768: 1.61 -> 1.34 ms per 2.1 M pairs against 64 lanes x 3 rounds x 2 pairs
#define RQ_PREP_SHAPES(X) X(128, 16, 2, 16, 2) X(64, 16, 1, 16, 4) X(256, 32, 2, 8, 2) X(512, 32, 4, 8, 1) X(768, 32, 6, 8, 1) X(1024, 32, 8, 8, 1)

// One stage of a pass.  The reference visits a query's candidates as ONE stream: probed lists nearest-first,
// members in stored order.  A stage covers stream positions [s_lo, s_hi) (of every query) and is
// scanned with the threshold each query's ranker holds at the start of the stage -- an upper
// bound of the reference's threshold everywhere in the stage, since it never rises -- then the
// survivors are replayed in the reference's order.  Stage 0 = the first topk candidates
// (threshold f32::MAX), later stages grow geometrically.
struct StagePlan {
    uint32_t s_lo, s_hi;
    uint64_t span, est_pairs;
    bool matrix;         // scanned on the matrix cores (else the VALU kernel)
    bool cluster_major;  // list-major work records (else one per pair)
    bool ranked;         // places inside the groups come out of the counting pass (group_rank_kernel)
    bool additive;       // matrix-core scan with the additive gate (else the bf16 threshold form)
    bool arena_stage;    // can exceed the uniform survivor capacity: appends to the shared arena
    bool placed;         // grouped before the quantisation, which wrote its operand rows in place
    bool want_table;     // one block per existing (list, tile), if the index has the table
    bool prefilter;      // stage_finish_large: the thresholds are finite, the survivors go through the index's shadow rows first ...
    bool rerank_q8;      // ... the 8-bit ones ...
    bool rerank_ring;    // ... which travel through the LDS ring (accurate_ring8_kernel; else accurate_filtered8_kernel's registers)
    uint32_t slot_hi, stage_pairs;  // probe slots the stage can touch, and its work items
    uint32_t dense_cells;           // cells of the dense run directory (0: runs are appended and sorted)
    uint32_t tile, tiles_per_group;
};

struct PassPlan {
    uint32_t nprobe, npairs;
    uint32_t dbg;   // option scan_debug, one snapshot for the whole pass (as of every other option the plan reads)
    bool large;     // the large-batch form of the stages (option large_batch_from, read once: whatever executes the pass asks the plan)
    bool small;     // few, fat launches (kernels_small.h): the early stages run inside one block per query
    uint32_t sb_nstages, sb_lo[RQ_SB_MAX_STAGES], sb_hi[RQ_SB_MAX_STAGES], sb_final_lo;
    bool sb_whole, sb_fill_final;
    bool will_list;     // the pairs whose list has (admitted) members are listed, the quantisation runs over those
    bool placed;        // the final stage is placed before the quantisation ...
    bool fin_additive;  // ... and the gate its images are laid out for
    bool write_qn, write_q6;  // operands the quantisation writes: 4-bit (VALU scans), fp6 (matrix-core scans)
    uint32_t qn_slots;        // probe slots whose pairs get the 4-bit operand
    uint32_t prep_lp, prep_r, prep_ppb, prep_pp;  // the quantisation kernel's shape (prep_lp == 0: the generic kernel)
    uint32_t mid_blocks;      // persistent blocks of the long-directory ordering
    uint32_t nstages;         // the stages the host launches (small: only what the block per query leaves)
    StagePlan st[RQ_MAX_STAGES];
};

// first_hi: end of the first stage; settle_cap: where the early stages must end at the latest; settle_pct: option stage_settle_pct as
// plan_pass read it (pl.large: the batch form it decided on)
static void plan_stages(const rq_index *idx, uint32_t nprobe, uint64_t first_hi, uint64_t growth, uint64_t settle_cap, uint64_t settle_pct, PassPlan &pl) {
    pl.nstages = 0;
    const uint64_t total_max = std::min<uint64_t>((uint64_t)nprobe * idx->max_list_len, idx->n);
    uint64_t lo = 0, hi = first_hi;
    const uint64_t avg = std::max<uint64_t>(1, idx->n / std::max<uint32_t>(idx->nonempty_lists, 1));  // (over the lists that exist here: a shard owns k / world of them)
    // the threshold has settled once a query has seen its whole nearest list; with unbalanced lists (Zipf sizes) the
    // nearest list of many queries is one of the long ones, so the bar is the LONGEST list (capped: a single
    // monster list must not push the whole batch through many thin stages)
    uint64_t settle = std::min(settle_cap, std::max<uint64_t>(avg, std::min<uint64_t>(idx->max_list_len, 16 * avg)));
    if (pl.large) settle = std::max<uint64_t>(1, settle * settle_pct / 100);
    while (lo < total_max) {
        // past the first two lists' worth of candidates the threshold is already tight: scan the rest of
        // the stream as ONE stage (every list then meets all its queries at once: full 32-query tiles)
        // (RQ_MAX_STAGES: out of reach for a geometric schedule over 32-bit stream positions; the rest would go into the final stage)
        const bool last = hi >= total_max || lo >= settle || pl.nstages + 1 == RQ_MAX_STAGES;
        pl.st[pl.nstages++] = StagePlan{(uint32_t)lo, last ? 0xFFFFFFFFu : (uint32_t)hi};
        if (last) break;
        lo = hi;
        hi = std::min<uint64_t>(hi * growth, 0xFFFFFFF0ull);
        // the geometric step must not carry an early (VALU) stage over many lists when lists are short:
        // past two lists' worth the rest belongs to the final stage
        // (a step that ends within a factor two BELOW that mark is carried up to it: the hard distribution ran a thin matrix-core
        // stage [40960, 48828) behind [5120, 40960) -- 4.5 ms of launches for 8 000 stream positions)
        if (lo < 2 * avg && 2 * hi > 2 * avg) hi = 2 * avg;
        // ... and the last early stage ends exactly where the threshold has settled: everything beyond belongs to the
        // final (matrix-core) stage, where a list meets all its queries at once
        if (lo < settle && hi > settle) hi = settle;
    }
}

// The rerank pre-filter's route for the 8-bit shadow rows (kernels_rerank.h): true = accurate_ring8_kernel, false =
// accurate_filtered8_kernel.  The ring is instantiated for the dimensions whose rows are 4 .. 16 pieces of 16 bytes (dim 64, 128, 192,
// 256); beside the query and the probed lists' maps (at most RQ_ACC8_LDS_PROBES of them: the ring kernel reads the maps from LDS only)
// its two slots take at most 1 + 16 + 64 KB there, inside the 156 KB the kernels are registered with (ensure_kernel_attributes).
// scan_debug bit 32768 (measurements, tests) keeps the register kernel.
static inline uint32_t rerank_ring_lds(uint32_t dim, uint32_t nprobe) { return dim * 4u + nprobe * 16u + q8_ring_bytes(RQ_RING_V, dim); }
static inline bool rerank_ring_has(uint32_t dim) {  // (dim is a multiple of 64)
    switch (dim / 16) { RQ_RING8_NPC(RQ_SHAPE_CASE) return true; default: return false; }
}
static inline bool rerank_ring_rule(uint32_t dim, uint32_t nprobe, uint32_t dbg) {
    return !(dbg & 32768u) && rerank_ring_has(dim) && nprobe <= RQ_ACC8_LDS_PROBES;
}
// whether a pass's stages finish with the full-chip kernels (stage_finish_large: rerank, run-directory sort, replay) -- large batches,
// range calls, and small batches whose survivor buffers are large (queries re-run after an overflow: tens of thousands of survivors
// each, which one block per query would rerank and order alone)
static inline bool finish_large(const PassPlan &pl, const QueryParams &qp) { return qp.range || pl.large || qp.cap > 4 * RQ_DEFAULT_CAP; }

// the widths with a small-batch path (sb_query_kernel: host_query.h launches it, inst_small_filt.hip its filtered instantiations)
static inline bool small_batch_has(uint32_t W) {
    switch (W) { RQ_SMALL_BATCH_WIDTHS(RQ_SHAPE_CASE) return true; default: return false; }
}

// has_row_map: the pass re-runs overflowed queries of an earlier one; caller_lists: the probe lists come from the caller.
// A cut pass (qp.rule.on(): adaptive probing) is planned as a pass over caller-supplied lists: its rows hold "no list" slots like a
// shard's, so it never takes the small-batch path (sb_query_kernel selects its lists itself) and gives up the placed final stage
// and the slot_hi / qn_slots reach bounds.  (The bounds would still hold for a prefix cut -- the slots that remain keep their
// stream positions -- and only the placed stage's kernels would need reading; neither has been measured on a cut pass yet.)
static void plan_pass(const rq_index *idx, const QueryParams &qp, bool has_row_map, bool caller_lists, PassPlan &pl) {
    const bool ext_lists = caller_lists || qp.rule.on();
    const uint32_t dim = idx->dim, k = idx->k, W = idx->W;
    const uint32_t nq = qp.nq, nprobe = std::min(qp.probe, k), topk = qp.topk;
    const uint32_t npairs = nq * nprobe;
    const rq_filter *filt = qp.filter;
    const bool large = rq_large_batch(nq), fused = scan_is_fused(W);
    pl = PassPlan{};
    pl.nprobe = nprobe, pl.npairs = npairs, pl.large = large;
    // shortest list of the pass: a filtered pass settles the pairs whose list admits nothing as empty ones, so no slot bound can be
    // derived from stream positions (as on a shard)
    const uint32_t min_len = filt ? 0u : idx->min_list_len;
    const int impl = g_scan_impl.load();
    pl.dbg = (uint32_t)g_scan_dbg.load();
    const int gate_opt = g_scan_gate.load(), rank_opt = g_group_rank.load(), tt_opt = g_scan_tile_table.load(), gopt = g_stage_growth.load();
    const bool dense_opt = g_dense_dir.load() != 0, additive_loose = idx->additive_loose.load() != 0;
    const uint64_t settle_pct = (uint64_t)g_stage_settle_pct.load();
    const uint32_t cm_div = (uint32_t)g_cluster_major_div.load();
    const uint64_t avg_len = std::max<uint64_t>(1, idx->n / std::max<uint32_t>(idx->nonempty_lists, 1));
    const uint64_t total_max = std::min<uint64_t>((uint64_t)nprobe * idx->max_list_len, idx->n);
    const bool one_stage = qp.range || (qp.thr_init != nullptr && !has_row_map);  // thresholds are already tight: nothing to learn in early stages

    // ---- the stage list ---------------------------------------------------------------------------------------------
    // small batches: few, fat launches (kernels_small.h)
    const bool sb_w = small_batch_has(W);
    pl.small = g_small_batch.load() == 0 && nq <= RQ_SB_MAX_NQ && !ext_lists && !has_row_map && !qp.thr_init && sb_w &&
               k <= RQ_SB_MAX_K && nprobe <= 64 && topk <= RQ_SB_MAX_TOPK && qp.cap <= 4 * RQ_DEFAULT_CAP;
    // A filtered pass (option small_batch_filtered: 0 never, 1 automatic, 2 whenever the shape allows): the block's stage boundaries
    // are stretched by 1 / density, the filter's density inside the lists that admit anything (lists that admit nothing take no stream
    // positions), so that the ranker sees as many ADMITTED candidates per stage as an unfiltered pass sees candidates -- but a
    // query's block never scans more than RQ_SB_FILT_REACH stored positions.  Automatic: the path is taken when the first stage
    // (16 x topk admitted candidates, which fill the heap) fits that reach; a sparser filter would hand the final stage a threshold
    // that is still f32::MAX, and every admitted row of the probed lists would survive it: such passes stay on the staged launches.
    uint64_t sb_first = 16ull * std::max<uint32_t>(topk, 1), sb_span = (uint64_t)std::max(1, g_sb_span.load());
    if (pl.small && filt) {
        const int fopt = g_sb_filtered.load();
        const double dens = filt->live_rows ? (double)filt->rows / (double)filt->live_rows : 0.0;
        const double first_f = dens > 0.0 ? (double)sb_first / dens : 2.0 * RQ_SB_FILT_REACH;
        pl.small = fopt == 2 || (fopt == 1 && first_f <= (double)RQ_SB_FILT_REACH);
        sb_span = dens > 0.0 ? (uint64_t)std::min<double>((double)sb_span / dens, (double)RQ_SB_FILT_REACH) : RQ_SB_FILT_REACH;
        sb_first = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::min<double>(first_f, (double)RQ_SB_FILT_REACH), sb_span));
    }
    if (pl.small) {
        // the early stages run inside one block per query: the first one takes what would be two (16 x topk candidates
        // under threshold f32::MAX cost one gather round), and the in-block part ends after 64 K candidates at the latest
        plan_stages(idx, nprobe, sb_first, gopt >= 2 ? (uint64_t)gopt : 8, sb_span, settle_pct, pl);
        if (pl.nstages > RQ_SB_MAX_STAGES) pl.small = false;
    }
    if (pl.small) {
        // a short remainder (small indexes, few probes) is scanned in the block as well: no further launch
        // (filtered: only within the block's reach; and a stream that the stretched first stage covers alone stays in the block --
        // handed on, its one stage would run under threshold f32::MAX)
        const bool fits = pl.nstages == 0 || (total_max - pl.st[pl.nstages - 1].s_lo) * (uint64_t)(dim / 8 + 16) <= (1ull << 20);
        const bool whole = pl.sb_whole = filt ? pl.nstages == 0 || ((fits || pl.nstages == 1) && total_max <= RQ_SB_FILT_REACH) : fits;
        pl.sb_nstages = whole ? pl.nstages : pl.nstages - 1;
        for (uint32_t i = 0; i < pl.sb_nstages; ++i) pl.sb_lo[i] = pl.st[i].s_lo, pl.sb_hi[i] = pl.st[i].s_hi;
        const StagePlan fin = whole ? StagePlan{} : pl.st[pl.nstages - 1];
        // whether sb_query_kernel writes the final stage's pair-major records: the kernels decide with the rule of a VALU stage over
        // every probe slot (a final stage that turns out list-major after all is filled by stage_fill_kernel like any other)
        pl.sb_fill_final = !whole && !(npairs >= k / 2 && npairs > 64);
        pl.sb_final_lo = fin.s_lo;
        pl.nstages = 0;
        if (!whole) pl.st[pl.nstages++] = fin;
    } else if (one_stage) {
        pl.nstages = 1;
        pl.st[0] = StagePlan{0u, 0xFFFFFFFFu};
    } else {
        // geometric growth of the early stages: 16 (coarser stages: a stage of launches less) below 32 768 queries, 8 (tighter
        // thresholds: ~9 % fewer exact distances) from there on.  Up to round 4 the step to 8 came at 256 queries; re-swept on the
        // round-5 kernels: 512 queries 1.70 -> 1.54 ms per call with 16, 2048 2.32 -> 2.23, 8192 3.83 -> 3.74, 16 384 5.64 -> 5.57,
        // 65 536 17.05 -> 17.12
        const uint64_t growth = gopt >= 2 ? (uint64_t)gopt : (nq >= 32768 ? 8 : 16);
        // the first stage runs with threshold f32::MAX (everything survives) until the ranker's heap is full; in a large
        // batch it also takes what would be the next stage (whose threshold -- the worst of the first topk -- lets most
        // of it through anyway): one stage of launches less for ~1 % more exact distances
        plan_stages(idx, nprobe, (uint64_t)std::max<uint32_t>(topk, 1) * (large ? growth : 1), growth, ~0ull, settle_pct, pl);
    }

    // ---- every stage's engine, grouping, gate and geometry --------------------------------------------------------------
    for (uint32_t i = 0; i < pl.nstages; ++i) {
        StagePlan &s = pl.st[i];
        s.span = (uint64_t)std::min<uint64_t>(s.s_hi, (uint64_t)nprobe * idx->max_list_len) - s.s_lo;
        s.est_pairs = (uint64_t)nq * std::min<uint64_t>(nprobe, s.span / avg_len + 2);
        // matrix cores pay once many queries share each list AND survivors are rare, i.e. past the nearest list
        // (stages inside it leave hundreds of survivors per query: the exact path dominates there and the VALU
        // kernel wins, measured at any batch size)
        s.matrix = scan_has_mfma(W) && impl != 1 &&
                   (impl == 2 || (s.est_pairs >= 8ull * k && (s.s_lo >= avg_len * settle_pct / 100 || one_stage)));
        // list-major once the stage's pairs reach k / 32 (k / 2 up to round 4, and still on the small-batch path, whose kernels decide with
        // that rule): a pair-major EARLY stage launches a block for every (query, probe slot, tile) although only the first slots are in
        // it -- at 512 queries the early stages took 1.06 ms pair-major against 0.3 list-major (batch 256: 1.43 -> 1.12 ms per call,
        // 512: 2.42 -> 1.62)
        s.cluster_major = s.matrix || (s.est_pairs >= k / (pl.small ? 2u : cm_div) && s.est_pairs > 64);
        // an arena stage: a stage that can exceed the uniform survivor capacity; its scan instantiation has its own tile
        s.arena_stage = qp.seg_final && s.span > qp.cap && fused && large;
        // (filtered stages run the bf16 threshold form: the filtered instantiations exist for that gate only)
        s.additive = s.matrix && !s.arena_stage && !filt && scan_has_additive(W) && idx->list_uref.p != nullptr && gate_opt != 1 &&
                     (gate_opt == 2 || !additive_loose);
        // slots a stage can touch: slot s starts at stream position >= s * (shortest list), so only the first few
        // slots of every query need to be looked at in the early stages (not derivable when lists may be empty,
        // e.g. a shard that does not own every probed list)
        s.slot_hi = nprobe;
        if (s.cluster_major && min_len > 0 && !ext_lists && s.s_hi != 0xFFFFFFFFu)
            s.slot_hi = (uint32_t)std::min<uint64_t>(nprobe, (uint64_t)(s.s_hi - 1) / min_len + 1);
        s.stage_pairs = nq * s.slot_hi;
        // big stages: places inside the groups come out of the counting pass (LDS histogram per block)
        // (option group_rank: 0 never, 1 auto, 2 whenever the histogram fits LDS (tests))
        s.ranked = s.cluster_major && k <= 32768 &&
                   (rank_opt == 2 || (rank_opt == 1 && s.stage_pairs >= 16 * RQ_RANK_ITEMS && s.stage_pairs / RQ_RANK_ITEMS >= k / 256));
        s.tile = s.matrix ? scan_mfma_tile(W, s.arena_stage, s.additive) : scan_tile(W);
        s.tiles_per_group = ceil_div(std::min<uint64_t>(idx->max_list_len, s.s_hi), s.tile);
        // the stage reaches every position of the lists and the lists are very unequal (one block per existing
        // (list, tile) instead of k x the longest list's tiles; measured neutral-to-slower for moderately unequal
        // lists, where the empty blocks of the plain grid cost less than the table's dependent load)
        // (option scan_tile_table: 0 = never, 1 = when the plain grid is mostly empty blocks, 2 = always)
        const uint64_t grid_blocks = (uint64_t)k * s.tiles_per_group, real_tiles = idx->n / s.tile + k;
        s.want_table = s.cluster_major && fused && s.s_hi >= idx->max_list_len && (tt_opt == 2 || (tt_opt == 1 && grid_blocks > 4 * real_tiles));
        // large batches, VALU-kernel stages: the run descriptors go into a dense directory indexed by stream position
        // (stage_fill_kernel: RQ_REC_CELL0), so the stage needs no sort of its run directory
        // (an arena stage appends its runs: they are placed by the scatter pass)
        if (large && !s.matrix && fused && dense_opt && s.s_hi != 0xFFFFFFFFu && !(qp.seg_final && s.span > qp.cap)) {
            const uint64_t cells = (uint64_t)((s.s_hi - 1) >> 6) - (s.s_lo >> 6) + 2ull * s.slot_hi + 2;
            if (cells <= qp.cap) s.dense_cells = (uint32_t)cells;
        }
        // past the first stage the thresholds are finite: survivors go through the shadow rows first (stage_finish_large)
        s.prefilter = (i > 0 || qp.thr_init) && !(pl.dbg & 512);
        s.rerank_q8 = s.prefilter && idx->base_q8.p != nullptr;
        s.rerank_ring = s.rerank_q8 && rerank_ring_rule(dim, nprobe, pl.dbg);
    }

    // ---- the quantisation ---------------------------------------------------------------------------------------------
#define RQ_X(D, LP, R, PPB, PP) \
    if (dim == D) pl.prep_lp = LP, pl.prep_r = R, pl.prep_ppb = PPB, pl.prep_pp = PP;
    RQ_PREP_SHAPES(RQ_X)
#undef RQ_X
    const bool prep_dim = pl.prep_lp != 0;
    // an index most of whose lists are empty (a shard of a multi-GPU deployment: the probe lists name the lists of every shard):
    // the pairs with nothing to scan are settled by one thread each, the quantisation runs over the listed others
    // -- and a filtered pass, whose pairs with nothing admitted are settled the same way (a filter correlated with the clustering: a
    // tenant, a region, leaves most probed lists empty)
    pl.will_list = !pl.small && (filt || (idx->nonempty_lists * 2 < k && npairs >= 65536)) && g_pair_split.load() != 0 && prep_dim;
    // Final stage placed ahead of the quantisation (option prep_placement).  Its grouping depends on the
    // probe lists, the list lengths and the stage boundaries only, all known before it: the stream positions come from the index's offsets,
    // the places from group_rank_kernel / group_scan_kernel, and the quantisation then writes every pair's fp6 operand row and the
    // threshold-free part of its tail straight into the stage's tile images -- no pair-major copy of the operand, no copy pass, and
    // the tails are completed (with the lists' v' ranges on the way) by stage_tail_kernel once the early stages have set the
    // thresholds.  The images live in a buffer of their own: the early stages' records go through ws.recs in between.
    // Passes that keep the older kernels: small-batch, filtered, listed (shard-like), arena (seg_final), seeded and re-run passes,
    // caller-supplied probe lists, a final stage placed by atomics (small stages), dimensions without a lane-group quantisation kernel.
    if (g_prep_placement.load() != 0 && !pl.small && !filt && !ext_lists && !has_row_map && !qp.thr_init && !qp.seg_final && !pl.will_list &&
        prep_dim && fused && pl.nstages) {
        StagePlan &fin = pl.st[pl.nstages - 1];
        pl.placed = fin.s_hi == 0xFFFFFFFFu && fin.matrix && fin.ranked;
        for (uint32_t i = 0; i + 1 < pl.nstages; ++i) pl.placed = pl.placed && !pl.st[i].matrix;
        fin.placed = pl.placed;
        pl.fin_additive = pl.placed && fin.additive;
    }
    pl.write_qn = fused;
    pl.write_q6 = scan_has_mfma(W) && impl != 1;  // (a final stage over few lists may run on the matrix cores)
    // The 4-bit operand (64 of a pair's ~210 bytes at dim 128) is read by the VALU scans only, and a VALU stage that ends at stream
    // position s_hi cannot reach probe slot s_hi / (shortest list) or beyond: the matrix-core stages' pairs are written without it.
    pl.qn_slots = nprobe;
    if (pl.write_qn && pl.write_q6 && !ext_lists && min_len > 0) {
        uint32_t reach = 0;
        for (uint32_t i = 0; i < pl.nstages; ++i)
            if (!pl.st[i].matrix)
                reach = std::max<uint32_t>(reach, pl.st[i].s_hi == 0xFFFFFFFFu ? nprobe : (uint32_t)std::min<uint64_t>(nprobe, (uint64_t)(pl.st[i].s_hi - 1) / min_len + 1));
        pl.qn_slots = reach;
    }
    // persistent blocks of the long-directory ordering: sized by how many such directories recent passes produced
    const uint32_t big_hint = hints_of(idx, filt).big_dirs.load();
    pl.mid_blocks = big_hint == 0 ? 64u : std::min(4096u, std::max(256u, big_hint / 4));

    if (pl.dbg & 16384) {  // developer hook: the pass's stage list, and the plan as key=value tokens (one line per pass, one per stage)
        fprintf(stderr, "[rabitq_hip] plan: pass nq=%u nprobe=%u large=%d small=%d will_list=%d placed=%d fin_additive=%d qn_slots=%u nstages=%u seg_final=%d sb_nstages=%u sb_whole=%d\n",
                nq, nprobe, (int)pl.large, (int)pl.small, (int)pl.will_list, (int)pl.placed, (int)pl.fin_additive, pl.qn_slots, pl.nstages, (int)qp.seg_final,
                pl.small ? pl.sb_nstages : 0u, (int)(pl.small && pl.sb_whole));
        for (uint32_t i = 0; pl.small && i < pl.sb_nstages; ++i)  // (the stages a small batch runs inside its block per query)
            fprintf(stderr, "[rabitq_hip] plan: sb_stage=%u lo=%u hi=%u\n", i, pl.sb_lo[i], pl.sb_hi[i]);
        for (uint32_t i = 0; i < pl.nstages; ++i) {
            const StagePlan &s = pl.st[i];
            fprintf(stderr, "[rabitq_hip] stage %u: [%u, %u) span %llu est_pairs %llu %s\n", i, s.s_lo, s.s_hi, (unsigned long long)s.span,
                    (unsigned long long)s.est_pairs, s.matrix ? "matrix cores" : (s.cluster_major ? "VALU, list-major" : "VALU, pair-major"));
            if (s.placed) fprintf(stderr, "[rabitq_hip] stage %u: placed ahead of the quantisation (%s gate)\n", i, pl.fin_additive ? "additive" : "bf16");
            fprintf(stderr, "[rabitq_hip] plan: stage=%u lo=%u hi=%u matrix=%d cluster_major=%d ranked=%d additive=%d arena=%d placed=%d table=%d dense_cells=%u slot_hi=%u\n",
                    i, s.s_lo, s.s_hi, (int)s.matrix, (int)s.cluster_major, (int)s.ranked, (int)s.additive, (int)s.arena_stage, (int)s.placed, (int)s.want_table,
                    s.dense_cells, s.slot_hi);
            // (outside the `plan:` lines, whose token set is fixed)
            if (s.rerank_q8 && finish_large(pl, qp)) fprintf(stderr, "[rabitq_hip] stage %u: rerank=%s\n", i, s.rerank_ring ? "ring" : "regs");
        }
    }
}
