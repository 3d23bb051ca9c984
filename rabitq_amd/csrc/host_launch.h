// host_launch.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  The kernel launch dispatch: coarse ranking, probe selection, rotation, the VALU and matrix-core
// scans with their geometry, and the dynamic-LDS attributes.  Which width has which instantiation comes from the lists of
// kernel_shapes.h: every switch, predicate and attribute line over a family's widths here is generated from its list.
#pragma once
// The bf16 tile kernels (assign_approx_kernel in host_build.h, coarse_approx_kernel below) exist for these widths.
static bool bf16_tile_has(uint32_t W) {
    switch (W) { RQ_BF16_TILE_SHAPES(RQ_SHAPE_CASE) return true; default: return false; }
}
template <int W, int NT>
static constexpr size_t assign_lds_bytes() { return 2 * (32 * (64 * W * 2 + 16) + 128); }  // assign_approx_kernel: two centroid-tile images

// the probe selection runs one wave per query (row in registers) for these shapes, one block per query otherwise.
// Up to 4096 lists only: select_probe_wave_kernel<128> (4097 .. 8192 lists; 256 VGPRs, 91 AGPRs and 325 spilled SGPRs) returned lists
// beyond the true nprobe-th at 8000 and 8192 lists -- on ~2000 of 2048 mixture rows, against a float64 model and against the
// block-per-query selection of the same rows (7000 and fewer were right) -- so those rows go to the block-per-query selection until
// that instantiation is understood.  select_refine_wave_kernel<128> still calls it for its fall-back rows (coarse_impl 3 / dim > 512).
static bool select_is_wave(uint32_t k, uint32_t nprobe, uint32_t nq) { return nprobe <= 64 && k <= 4096 && nq >= 8; }
// coarse ranking distances (src/rabitq.rs:283-287), every query against the lists [first, first + k) of cent_t
static void launch_coarse(const float *cent_t, const float *y, float *dist, uint32_t k, uint32_t dim, uint32_t nq,
                          uint32_t kstride, hipStream_t st) {
    const int impl = g_coarse_impl.load();
    const bool sreg = (impl == 2 || (impl == 0 && nq >= 2048)) && nq > 0;
    if (g_scan_dbg.load() & 16384)  // developer hook: the exact-order distance kernel of this ranking
        fprintf(stderr, "[rabitq_hip] plan: coarse=exact kernel=%s nq=%u k=%u\n", sreg ? "sreg" : (nq >= 64 && dim <= 2048 ? "lds8" : "lds4"), nq, k);
    if (sreg)  // many queries per list: query side in SGPRs
        coarse_dist_sreg_kernel<8><<<dim3(ceil_div(nq, 8), ceil_div(k, 256)), 256, 0, st>>>(cent_t, y, dist, k, dim, nq, kstride);
    else if (nq >= 64 && dim <= 2048)  // 8 queries per thread: 8 packed VALU ops per centroid element loaded
        coarse_dist_kernel<8><<<dim3(ceil_div(nq, 8), ceil_div(k, 256)), 256, 8 * dim * sizeof(float), st>>>(cent_t, y, dist, k, dim, nq,
                                                                                                    kstride);
    else
        coarse_dist_kernel<4><<<dim3(ceil_div(nq, 4), ceil_div(k, 256)), 256, 4 * dim * sizeof(float), st>>>(cent_t, y, dist, k, dim, nq,
                                                                                                    kstride);
}

// registers per lane of the wave-per-query selections (the row of k <= 8192 distances in registers): f(integral_constant<int, KPL>)
template <typename F>
static void with_row_kpl(uint32_t k, F f) {
    if (k <= 1024) f(std::integral_constant<int, 16>{});
    else if (k <= 4096) f(std::integral_constant<int, 64>{});
    else f(std::integral_constant<int, 128>{});
}
// probe selection: one wave per query when the row fits in registers and nprobe <= 64, else one block per query
static void launch_select(const float *dist, uint32_t k, uint32_t nprobe, uint32_t *out_cluster, float *out_dist,
                          uint32_t id_offset, uint32_t out_stride, uint32_t nq, hipStream_t st) {
    if (select_is_wave(k, nprobe, nq)) {
        with_row_kpl(k, [&](auto kpl) {
            select_probe_wave_kernel<decltype(kpl)::value><<<ceil_div(nq, 4), 256, 0, st>>>(dist, k, nprobe, out_cluster, out_dist, id_offset, out_stride, nq);
        });
        return;
    }
    select_probe_kernel<<<nq, 256, (size_t)nprobe * 8, st>>>(dist, k, nprobe, out_cluster, out_dist, id_offset, out_stride);
}

// Coarse ranking of nq rotated queries against ALL k lists: the matrix-core pre-filter + exact-order refinement where it applies
// (coarse_impl 3, or -- once measured faster -- auto for big batches), else the exact-order distance kernels + selection.
// (more lists than one wave holds in registers -- the ranking of a multi-GPU deployment is over the lists of ALL shards -- go through
// the tile-minima selection, select_refine_tiled_kernel)
static bool coarse_prefilter_applies(const rq_index *idx, uint32_t nq, uint32_t nprobe) {
    const int impl = g_coarse_impl.load();
    return (impl == 3 || impl == 4 || (impl == 0 && nq >= 2048)) && bf16_tile_has(idx->W) && std::isfinite(idx->cent_norm_max) &&
           idx->cent_bf.p != nullptr && nprobe <= 64 && nq >= 8 && idx->k >= 64 && nprobe >= 1 && idx->k <= 65536;
}
// coarse_candidates_kernel: the two centroid-tile images, then 4 waves x NT x 32 queries x ntile tile keys
template <int W, int NT>
static size_t coarse_candidates_lds_bytes(uint32_t ntile) { return assign_lds_bytes<W, NT>() + (size_t)4 * NT * 32 * ntile * 4; }
#define RQ_LDS_PER_BLOCK (160u * 1024u)
// the widths coarse_candidates_kernel is instantiated for (dim <= 256)
static bool coarse_candidates_has(uint32_t W) {
#define RQ_CCK_W(WW, NT) || W == WW
    return false RQ_COARSE_CAND_SHAPES(RQ_CCK_W);
#undef RQ_CCK_W
}
// The route without the nq x k matrix (coarse_candidates_kernel + refine_candidates_kernel): the automatic rule only, from 4096 lists
// (below, rows of the matrix are short and the kernels that read them are not where the time goes) to 8192 (the tile keys of 128
// queries stay in LDS), dim <= 256 (wider margins overflow the candidate slots, and this route has no second collect), and
// only where the tile keys fit beside the centroid images (dim 256 stops at 7936 lists).  scan_debug bit 65536 keeps the two-kernel route.
static bool coarse_fused_applies(const rq_index *idx, uint32_t nprobe, bool have_redo) {
    const uint32_t k = idx->k, ntile = ceil_div(k, 32u);
    if (g_coarse_impl.load() != 0 || (g_scan_dbg.load() & 65536) || !have_redo || k < 4096 || k > 8192 || !coarse_candidates_has(idx->W) || ntile < nprobe) return false;
    const size_t images = 2 * (32 * ((size_t)idx->dim * 2 + 16) + 128);
    return images + (size_t)4 * 32 * ntile * 4 <= RQ_LDS_PER_BLOCK;
}
// redo: nq words (the tiled selection's flags; the matrix-free route's candidate counts, then its flags); null: rows in registers only
// y_bf: room for nq x dim bf16 (the query rows pre-rounded for the wide instantiation; any workspace buffer that is free at this point)
static void launch_coarse_prefiltered(const rq_index *idx, const float *y, float *dist, uint32_t nq, uint32_t nprobe, uint32_t *out_cluster,
                                      float *out_dist, uint32_t out_stride, unsigned long long *fallback_rows, uint32_t *redo, hipStream_t st,
                                      uint16_t *y_bf) {
    const uint32_t k = idx->k, dim = idx->dim;
    if (coarse_fused_applies(idx, nprobe, redo != nullptr)) {
        const uint32_t ntile = ceil_div(k, 32u);
        if (g_scan_dbg.load() & 16384) fprintf(stderr, "[rabitq_hip] plan: coarse=prefilter_fused nq=%u k=%u nprobe=%u\n", nq, k, nprobe);
        // two query tiles per wave where their tile keys fit (dim <= 128 up to 4544 lists), else one: the first shape of the width, in
        // the list's order, whose keys fit.  (No else: coarse_fused_applies above holds only for a width of the same list whose
        // one-tile shape fits, so a shape is always found.)
#define RQ_CCK(WW, NT)                                                                                                                   \
    else if (idx->W == WW && coarse_candidates_lds_bytes<WW, NT>(ntile) <= RQ_LDS_PER_BLOCK)                                             \
        coarse_candidates_kernel<WW, NT><<<ceil_div(nq, 128 * NT), 256, coarse_candidates_lds_bytes<WW, NT>(ntile), st>>>(               \
            y, idx->cent_bf.p, idx->cent_sqnorm.p, idx->cent_norm_max, nq, k, nprobe, dist, redo);
        if (false) {}
        RQ_COARSE_CAND_SHAPES(RQ_CCK)
#undef RQ_CCK
        refine_candidates_kernel<<<ceil_div(nq, 4), 256, 0, st>>>(dist, y, idx->centroids.p, k, dim, nprobe, out_cluster, out_dist, out_stride, nq, redo,
                                                                  fallback_rows);
        // rows that overflowed the slots hold exact-order distances now: the block-per-query selection takes them (it exits at once for the others)
        select_probe_kernel<<<nq, 256, (size_t)nprobe * 8, st>>>(dist, k, nprobe, out_cluster, out_dist, 0u, out_stride, redo);
        return;
    }
    if (idx->W > 8) to_bf16_kernel<<<ceil_div((uint64_t)nq * dim / 8, 256), 256, 0, st>>>(y, (uint64_t)nq * dim, y_bf);
#define RQ_CAP(WW, NT)                                                                                                      \
    case WW:                                                                                                                \
        coarse_approx_kernel<WW, NT><<<ceil_div(nq, 128 * NT), 256, assign_lds_bytes<WW, NT>(), st>>>(y, idx->cent_bf.p, idx->cent_sqnorm.p, \
                                                                                                      nq, k, dist, y_bf);  \
        break;
    switch (idx->W) {
        RQ_BF16_TILE_SHAPES(RQ_CAP)
        default: break;  // (not reached: coarse_prefilter_applies asks bf16_tile_has, which is made from the same list)
    }
#undef RQ_CAP
    const dim3 g(ceil_div(nq, 4)), b(256);
    // the selection: tile minima (select_refine_tiled_kernel) wherever a row has at least nprobe tiles of 32 lists -- measured faster than
    // the register-resident row from 4096 lists up, and the only form beyond 8192 --, else the row in registers
    const uint32_t ntile = ceil_div(k, 32u);
    const int impl = g_coarse_impl.load();
    // (dim 768 and beyond stay on the row in registers below 8192 lists: 2.45 against 2.77 ms per 32 768 queries on the 100M x 768 index --
    // the margin of the pre-filter grows with the dimension, so more tiles are read again.  Round 4 saw 22 ms here: the time sat between
    // the launches behind coarse_approx_kernel<12,1>, which then spilled 142 registers -- a dispatch that needs more scratch than the queue
    // holds is set up and torn down around the launch -- and needs no scratch any more.)
    const bool tiled = redo != nullptr && ntile >= nprobe &&
                       (k > 8192 || impl == 4 || (impl != 3 && k >= (uint32_t)g_coarse_tiled_from.load() && idx->W <= 8));
    if (g_scan_dbg.load() & 16384)  // developer hook: which selection the pre-filtered ranking takes
        fprintf(stderr, "[rabitq_hip] plan: coarse=%s nq=%u k=%u nprobe=%u\n", tiled ? "prefilter_tiled" : "prefilter_regs", nq, k, nprobe);
    if (tiled) {
#define RQ_TILED(TPL)                                                                                                             \
    select_refine_tiled_kernel<TPL><<<g, b, 4 * 64 * (TPL) * 4, st>>>(dist, y, idx->centroids.p, idx->cent_norm_max, k, dim, nprobe, out_cluster, \
                                                                    out_dist, out_stride, nq, redo, fallback_rows)
        if (ntile <= 128) RQ_TILED(2);
        else if (ntile <= 256) RQ_TILED(4);
        else if (ntile <= 512) RQ_TILED(8);
        else if (ntile <= 1024) RQ_TILED(16);
        else RQ_TILED(32);
#undef RQ_TILED
        // rows the tiled kernel could not handle hold exact-order distances now: the block-per-query selection takes them (it exits at once for the others)
        select_probe_kernel<<<nq, 256, (size_t)nprobe * 8, st>>>(dist, k, nprobe, out_cluster, out_dist, 0u, out_stride, redo);
    } else {
        with_row_kpl(k, [&](auto kpl) {
            select_refine_wave_kernel<decltype(kpl)::value><<<g, b, 0, st>>>(dist, y, idx->centroids.p, idx->cent_norm_max, k, dim, nprobe, out_cluster, out_dist,
                                                                             out_stride, nq, fallback_rows);
        });
    }
}

// ------------------------------------------------------------------------------------------------
// rotation launcher (MFMA kernel for bulk, VALU kernel for a handful of rows; bit-identical)
// ------------------------------------------------------------------------------------------------
static void launch_rotate(const float *x, const float *P, float *out, uint64_t n, uint32_t dim, bool mfma,
                          hipStream_t st) {
    const uint64_t rows_per_launch = mfma ? (1ull << 40) : (uint64_t)RQ_MAX_BLOCKS_256 * 4;
    for (uint64_t r0 = 0; r0 < n; r0 += rows_per_launch) {
        const uint64_t m = std::min(rows_per_launch, n - r0);
        const float *xs = x + r0 * dim;
        float *os = out + r0 * dim;
        if (mfma) {
            // persistent: 2 blocks per CU x 256 CUs, split between the column tiles
            const uint32_t ncol = dim / ROT_BN;
            const uint64_t nrow_tiles = ceil_div(m, ROT_BM);
            const uint32_t groups = (uint32_t)std::min<uint64_t>(nrow_tiles, std::max<uint32_t>(1, 512 / ncol));
            rotate_mfma_kernel<<<dim3(groups * ncol), dim3(256), 0, st>>>(xs, P, os, m, dim, groups);
        } else {
            rotate_valu_kernel<<<dim3(ceil_div(m, 4), dim / 64), dim3(64, 4), 0, st>>>(xs, P, os, m, dim);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// scan dispatch on W = dim / 64
// ------------------------------------------------------------------------------------------------
// The tile table of `tile` positions per block (see ScanArgs::use_table); nullptr on failure (the caller then uses the
// plain grid).  Built once per (index, tile size).
static const uint4 *get_tile_table(const rq_index *cidx, uint32_t tile, uint32_t *count) {
    rq_index *idx = const_cast<rq_index *>(cidx);
    std::lock_guard<std::mutex> lk(idx->tt_mu);
    auto it = idx->tile_tables.find(tile);
    if (it == idx->tile_tables.end()) {
        std::vector<uint4> h;
        h.reserve(idx->n / tile + idx->k + 1);
        for (uint32_t c = 0; c < idx->k; ++c) {
            const uint32_t b = idx->h_offsets[c], len = idx->h_offsets[c + 1] - b;
            for (uint32_t f = 0; f < len; f += tile) h.push_back(make_uint4(c, f, b, len));
        }
        std::unique_ptr<DevBuf<uint4>> buf(new DevBuf<uint4>());
        if (buf->alloc(h.size()) != RQ_OK) return nullptr;
        if (!h.empty() && hipMemcpy(buf->p, h.data(), h.size() * sizeof(uint4), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        buf->count = h.size();
        it = idx->tile_tables.emplace(tile, std::move(buf)).first;
    }
    *count = (uint32_t)it->second->count;
    return it->second->p;
}

// A stage's grid is ngroups x tiles_per_group blocks.  Shapes whose grid exceeds the launch bound (few huge lists
// x many pairs, ~1e9 vectors with skewed lists) are issued as several launches over (group, tile) sub-ranges; the
// survivors of one stage are unordered until the run directory is sorted, so the split changes nothing.  (Tests lower the bound:
// option "max_scan_blocks".)
template <typename F>
static void launch_scan_chunks(const ScanArgs &a, F &&launch) {
    if (a.ngroups == 0 || a.tiles_per_group == 0) return;
    const uint32_t maxb = std::max(1u, g_max_scan_blocks.load());
    const uint32_t tchunk = std::min(a.tiles_per_group, maxb);
    const uint32_t gchunk = std::max(1u, maxb / tchunk);
    for (uint32_t t0 = 0; t0 < a.tiles_per_group; t0 += tchunk)
        for (uint32_t g0 = 0; g0 < a.ngroups; g0 += gchunk) {
            ScanArgs c = a;
            c.tile_base = t0, c.group_base = g0;
            c.tiles_per_group = std::min(tchunk, a.tiles_per_group - t0);
            c.ngroups = std::min(gchunk, a.ngroups - g0);
            launch(c, dim3(c.ngroups * c.tiles_per_group));
        }
}

// launches launch_scan_chunks issues for these arguments (rq_profile_t::scan_launches counts them, not the stages)
static uint32_t scan_chunk_count(const ScanArgs &a) {
    if (a.ngroups == 0 || a.tiles_per_group == 0) return 0;
    const uint32_t maxb = std::max(1u, g_max_scan_blocks.load());
    const uint32_t tchunk = std::min(a.tiles_per_group, maxb);
    const uint32_t gchunk = std::max(1u, maxb / tchunk);
    return ceil_div(a.tiles_per_group, tchunk) * ceil_div(a.ngroups, gchunk);
}

#define SCAN_ARGS p.codes, p.factors, p.offsets, p.grp_start, p.recs, p.surv, p.runs, p.surv_cnt, p.tile_table, a
template <bool ARENA, bool FILT>
static void launch_scan_t(const ScanPtrs &p, const ScanArgs &args, uint32_t W, hipStream_t st) {
    launch_scan_chunks(args, [&](const ScanArgs &a, dim3 g) {
        const dim3 b(256);
#define RQ_SCAN_K(WW, CPL)                                                                        \
    case WW:                                                                                      \
        if constexpr (FILT) scan_kernel<WW, CPL, ARENA, true><<<g, b, 0, st>>>(SCAN_ARGS);         \
        else scan_kernel<WW, CPL, ARENA><<<g, b, 0, st>>>(SCAN_ARGS);                             \
        break;
        switch (W) {
            RQ_SCAN_VALU_SHAPES(RQ_SCAN_K)
            default:  // the widths without a fused kernel (arena stages exist for the fused dims only)
                if constexpr (!ARENA && FILT) scan_generic_filtered_kernel<<<g, b, 0, st>>>(SCAN_ARGS, W);
                else if constexpr (!ARENA) scan_generic_kernel<<<g, b, 0, st>>>(SCAN_ARGS, W);
                break;
        }
#undef RQ_SCAN_K
    });
}
// p.arena: the arena instantiations (the stage appends to the shared arena, ScanExtra); p.filtered: the filtered ones (args.x
// holds the filter's position bitmap, together with the arena's fields in an arena stage)
static void launch_scan(const ScanPtrs &p, const ScanArgs &args, uint32_t W, hipStream_t st) {
    if (p.filtered) {
        if (p.arena) launch_scan_t<true, true>(p, args, W, st);
        else launch_scan_t<false, true>(p, args, W, st);
    } else if (p.arena) launch_scan_t<true, false>(p, args, W, st);
    else launch_scan_t<false, false>(p, args, W, st);
}

// matrix-core scan instantiations: W = dim/64, NT = 32-candidate sub-tiles per wave (resident operand registers
// 6*W*NT), blocks per CU per scan_mfma_blocks_per_cu<W>()
static bool scan_has_mfma(uint32_t W) {
    switch (W) { RQ_SCAN_MFMA_SHAPES(RQ_SHAPE_CASE) return true; default: return false; }
}
// the additive-gate instantiations (dim 64 / 128, uniform survivor buffers)
static bool scan_has_additive(uint32_t W) {
    switch (W) { RQ_SCAN_MFMA_ADD_SHAPES(RQ_SHAPE_CASE) return true; default: return false; }
}
#define RQ_SHAPE_SECOND(WW, N) case WW: return N;
static uint32_t scan_mfma_nt(uint32_t W, bool additive = false) {  // 0: no such instantiation (callers ask scan_has_mfma / scan_has_additive first)
    if (additive) switch (W) { RQ_SCAN_MFMA_ADD_SHAPES(RQ_SHAPE_SECOND) default: return 0; }
    switch (W) { RQ_SCAN_MFMA_SHAPES(RQ_SHAPE_SECOND) default: return 0; }
}
#undef RQ_SHAPE_SECOND
static uint32_t scan_mfma_nw(uint32_t W, bool arena) { return W == 2 && !arena ? 8u : 4u; }  // scan_mfma_waves<W, ARENA>()
static uint32_t scan_mfma_tile(uint32_t W, bool arena, bool additive = false) { return 32 * scan_mfma_nw(W, arena) * scan_mfma_nt(W, additive && !arena); }
static size_t scan_mfma_ring_bytes(uint32_t W, bool arena = false) {  // scan_mfma_ring_slots<W, ARENA>() tile images
    (void)arena;
    const uint64_t slots = W <= 2 ? 4ull : (W >= 16 ? 5ull : 3ull);
    return slots * (32 * (12 * W + 2) + RQ_REC_TAIL * 32) * 4;
}
template <int W, int NT, bool ARENA, bool ADD = false, bool FILT = false>
static void launch_scan_mfma_t(const ScanPtrs &p, const ScanArgs &a, dim3 g, hipStream_t st) {
    scan_mfma_kernel<W, NT, ARENA, ADD, FILT><<<g, dim3(64 * scan_mfma_waves<W, ARENA>()), scan_mfma_ring_bytes(W, ARENA), st>>>(p.codes, p.factors, p.offsets, p.grp_start, p.grp_cnt,
                                                                                    p.recs, p.surv, p.runs, p.surv_cnt, p.stat, p.tile_table, p.list_uref, p.grp_vref, a);
}
// the additive-gate instantiations: callers check scan_has_additive(W) first
static void launch_scan_mfma_add(const ScanPtrs &p, const ScanArgs &args, uint32_t W, hipStream_t st) {
    launch_scan_chunks(args, [&](const ScanArgs &a, dim3 g) {
#define RQ_SCAN_M(WW, NT) case WW: launch_scan_mfma_t<WW, NT, false, true>(p, a, g, st); break;
        switch (W) { RQ_SCAN_MFMA_ADD_SHAPES(RQ_SCAN_M) default: break; }
#undef RQ_SCAN_M
    });
}
// callers check scan_has_mfma(W) first; p.arena: the arena instantiations, p.filtered: the filtered ones (bf16 gate)
template <bool ARENA, bool FILT = false>
static void launch_scan_mfma_a(const ScanPtrs &p, const ScanArgs &args, uint32_t W, hipStream_t st) {
    launch_scan_chunks(args, [&](const ScanArgs &a, dim3 g) {
#define RQ_SCAN_M(WW, NT) case WW: launch_scan_mfma_t<WW, NT, ARENA, false, FILT>(p, a, g, st); break;
        switch (W) { RQ_SCAN_MFMA_SHAPES(RQ_SCAN_M) default: break; }
#undef RQ_SCAN_M
    });
}
static void launch_scan_mfma(const ScanPtrs &p, const ScanArgs &args, uint32_t W, hipStream_t st, bool additive = false) {
    if (p.filtered) {  // (filtered stages never take the additive gate: run_pass)
        if (p.arena) launch_scan_mfma_a<true, true>(p, args, W, st);
        else launch_scan_mfma_a<false, true>(p, args, W, st);
    } else if (p.arena) launch_scan_mfma_a<true>(p, args, W, st);
    else if (additive) launch_scan_mfma_add(p, args, W, st);
    else launch_scan_mfma_a<false>(p, args, W, st);
}

// the widths with a fused VALU kernel (the others: scan_generic_kernel), and the candidates a block of the VALU scan covers
static bool scan_is_fused(uint32_t W) {
    switch (W) { RQ_SCAN_VALU_SHAPES(RQ_SHAPE_CASE) return true; default: return false; }
}
static uint32_t scan_tile(uint32_t W) {
#define RQ_SCAN_TILE(WW, CPL) case WW: return 256 * CPL;
    switch (W) { RQ_SCAN_VALU_SHAPES(RQ_SCAN_TILE) default: return 256; }
#undef RQ_SCAN_TILE
}

// the filtered instantiations of sb_query_kernel live in a translation unit of their own (inst_small_filt.hip)
void launch_sb_query_filtered(uint32_t W, int mode, uint32_t nq, size_t dyn, hipStream_t st, const SbArgs &sa);
hipError_t sb_query_filtered_set_attributes(int bytes);
// f(integral_constant<KIND>): the run-time row kind (RowSpec::kind) as the constant the rerank kernels are instantiated on
template <typename F>
static void with_row_kind(int kind, F &&f) {
    switch (kind) {
        case ROW_KIND_BYTE: f(std::integral_constant<int, ROW_KIND_BYTE>{}); break;
        case ROW_KIND_HALF: f(std::integral_constant<int, ROW_KIND_HALF>{}); break;
        default: f(std::integral_constant<int, ROW_KIND_F32>{}); break;
    }
}

// ------------------------------------------------------------------------------------------------
// Kernels whose dynamic LDS can exceed the 64 KiB default: the attribute is set once per process, before the
// first launch of any of them (every entry point that can reach such a launch calls this first), and a refusal
// is reported instead of surfacing later as a failed launch.
// ------------------------------------------------------------------------------------------------
static rq_status ensure_kernel_attributes() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    static const char *what = "";
    std::call_once(once, [] {
        auto set = [&](const void *fn, int bytes, const char *name) {
            if (err != hipSuccess) return;
            err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
            if (err != hipSuccess) what = name;
        };
        set(reinterpret_cast<const void *>(select_probe_kernel), 140 * 1024, "select_probe_kernel");
        set(reinterpret_cast<const void *>(coarse_dist_kernel<4>), 140 * 1024, "coarse_dist_kernel<4>");
        set(reinterpret_cast<const void *>(coarse_dist_kernel<8>), 140 * 1024, "coarse_dist_kernel<8>");
        set(reinterpret_cast<const void *>(assign_generic_kernel<8>), 140 * 1024, "assign_generic_kernel<8>");
        set(reinterpret_cast<const void *>(merge_smallest_u64_kernel), 16384 * 8, "merge_smallest_u64_kernel");
        set(reinterpret_cast<const void *>(group_rank_kernel), 32768 * 4, "group_rank_kernel");
        set(reinterpret_cast<const void *>(sb_front_kernel), 140 * 1024, "sb_front_kernel");
#define RQ_ATTR(NPC) set(reinterpret_cast<const void *>(accurate_ring8_kernel<RQ_RING_V, NPC>), 156 * 1024, "accurate_ring8_kernel<" #NPC ">");
        RQ_RING8_NPC(RQ_ATTR)
#undef RQ_ATTR
        set(reinterpret_cast<const void *>(sort_runs_mid_kernel), RQ_SORT_MID_LDS_WORDS * 8, "sort_runs_mid_kernel");  // (+ 34 KiB of static LDS)
        set(reinterpret_cast<const void *>(range_sort_block_kernel<1024, RQ_RANGE_TILE>), RQ_RANGE_TILE * 8, "range_sort_block_kernel");
        set(reinterpret_cast<const void *>(range_sort_tile_kernel), RQ_RANGE_TILE * 8, "range_sort_tile_kernel");
        // the bf16 tile kernels: the shapes whose two images pass 48 KiB (W >= 6)
#define RQ_ATTR(KERNEL, WW, NT) \
    if constexpr (assign_lds_bytes<WW, NT>() > 48 * 1024) set(reinterpret_cast<const void *>(KERNEL<WW, NT>), (int)assign_lds_bytes<WW, NT>(), #KERNEL "<" #WW "," #NT ">");
#define RQ_ATTR_ASG(WW, NT) RQ_ATTR(assign_approx_kernel, WW, NT)
#define RQ_ATTR_CAP(WW, NT) RQ_ATTR(coarse_approx_kernel, WW, NT)
        RQ_BF16_TILE_SHAPES(RQ_ATTR_ASG)
        RQ_BF16_TILE_SHAPES(RQ_ATTR_CAP)
#undef RQ_ATTR_ASG
#undef RQ_ATTR_CAP
#undef RQ_ATTR
#define RQ_ATTR(WW, NT) set(reinterpret_cast<const void *>(coarse_candidates_kernel<WW, NT>), (int)RQ_LDS_PER_BLOCK, "coarse_candidates_kernel<" #WW "," #NT ">");
        RQ_COARSE_CAND_SHAPES(RQ_ATTR)
#undef RQ_ATTR
        for (int kind : {ROW_KIND_F32, ROW_KIND_HALF, ROW_KIND_BYTE})
            with_row_kind(kind, [&](auto row_kind) {
                constexpr int K = decltype(row_kind)::value;
                set(reinterpret_cast<const void *>(sb_finish_kernel<true, K>), 104 * 1024, "sb_finish_kernel");   // (+ 33 KiB of static LDS)
                set(reinterpret_cast<const void *>(sb_finish_kernel<false, K>), 104 * 1024, "sb_finish_kernel");  // (+ 49 KiB of static LDS)
            });
#define RQ_ATTR(WW)                                                                                      \
    set(reinterpret_cast<const void *>(sb_query_kernel<WW, 0, false>), 120 * 1024, "sb_query_kernel");   \
    set(reinterpret_cast<const void *>(sb_query_kernel<WW, 1, false>), 120 * 1024, "sb_query_kernel");   \
    set(reinterpret_cast<const void *>(sb_query_kernel<WW, 2, false>), 120 * 1024, "sb_query_kernel");
        RQ_SMALL_BATCH_WIDTHS(RQ_ATTR)
#undef RQ_ATTR
        if (err == hipSuccess && (err = sb_query_filtered_set_attributes(120 * 1024)) != hipSuccess) what = "sb_query_kernel (filtered)";
        // the matrix-core scan: the uniform, arena, filtered and filtered arena instantiations (bf16 gate) of every shape, then the
        // additive ones, all with the ring of their width.  In the error text an NT that is a tuning constant (RQ_NT_W2, ...) reads
        // "NT", as it always has: RQ_ATTR stringizes its own arguments (#NT there is the list's token, not the constant's value) and
        // hands the strings to RQ_MFMA_NAME.
#define RQ_MFMA_NAME(WS, NS) (NS[0] <= '9' ? "scan_mfma_kernel<" WS "," NS ">" : "scan_mfma_kernel<" WS ",NT>")
#define RQ_ATTR(WW, NT)                                                                                                                          \
    set(reinterpret_cast<const void *>(scan_mfma_kernel<WW, NT, false>), (int)scan_mfma_ring_bytes(WW), RQ_MFMA_NAME(#WW, #NT));                 \
    set(reinterpret_cast<const void *>(scan_mfma_kernel<WW, NT, true>), (int)scan_mfma_ring_bytes(WW), RQ_MFMA_NAME(#WW, #NT));                  \
    set(reinterpret_cast<const void *>(scan_mfma_kernel<WW, NT, false, false, true>), (int)scan_mfma_ring_bytes(WW), RQ_MFMA_NAME(#WW, #NT));    \
    set(reinterpret_cast<const void *>(scan_mfma_kernel<WW, NT, true, false, true>), (int)scan_mfma_ring_bytes(WW), RQ_MFMA_NAME(#WW, #NT));
        RQ_SCAN_MFMA_SHAPES(RQ_ATTR)
#undef RQ_ATTR
#define RQ_ATTR(WW, NT) set(reinterpret_cast<const void *>(scan_mfma_kernel<WW, NT, false, true>), (int)scan_mfma_ring_bytes(WW), RQ_MFMA_NAME(#WW, #NT));
        RQ_SCAN_MFMA_ADD_SHAPES(RQ_ATTR)
#undef RQ_ATTR
#undef RQ_MFMA_NAME
    });
    if (err != hipSuccess)
        return fail(RQ_ERR_HIP, std::string("hipFuncSetAttribute(") + what + "): " + hipGetErrorString(err));
    return RQ_OK;
}

