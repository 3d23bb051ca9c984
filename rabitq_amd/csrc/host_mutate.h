// host_mutate.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  In-place mutation (rq_add / rq_remove): one relayout from (index, rows to drop, new rows)
// to the index a fresh build of the live rows would produce, bit for bit.  Lazy removal (rq_remove_lazy / rq_compact,
// DESIGN §4.18): rows marked dead in a filter the index owns, dropped by the next relayout; and what a filter derives from its
// position bitmap (filter_finish), shared with rq_filter_create.
#pragma once

// The key word of every stored row (row_key), once per index: the stored rows are the build's zero-padded input, so rotating
// them again (same kernel, same P) and taking the distance to their own list's centroid in the assignment's lane order gives
// back the build's key bit for bit.
static thread_local rq_mutate_stats_t g_mutate_stats;  // the calling thread's last rq_add / rq_remove / rq_merge_from / rq_extract (rq_last_mutate_stats)
struct PhaseClock {  // wall time of a phase; every phase ends in a device synchronisation, so it covers the device work too
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    float lap() {
        const auto now = std::chrono::steady_clock::now();
        const float ms = std::chrono::duration<float, std::milli>(now - t).count();
        t = now;
        return ms;
    }
};

static rq_status ensure_row_keys(rq_index *idx) {
    if (idx->row_key_valid) return RQ_OK;
    PhaseClock clk;
    const uint64_t n = idx->n;
    const uint32_t dim = idx->dim;
    DevBuf<uint32_t> rk;
    RQC(rk.alloc(n));
    if (n) {
        const uint64_t chunk = std::min<uint64_t>(n, std::max<uint64_t>(64, (256ull << 20) / ((uint64_t)dim * 4)));
        DevBuf<float> xrot;
        RQC(xrot.alloc(chunk * dim));
        for (uint64_t r0 = 0; r0 < n; r0 += chunk) {
            const uint64_t mm = std::min(chunk, n - r0);
            launch_rotate(idx->base.p + r0 * dim, idx->P.p, xrot.p, mm, dim, true, nullptr);
            row_key_kernel<<<ceil_div(2 * mm, 256), 256>>>(xrot.p, r0, mm, dim, idx->centroids.p, idx->offsets.p, idx->k, rk.p);
        }
    }
    // the merge places rows by binary search over each list's keys: it needs every list strictly ascending, as the build leaves it
    DevBuf<unsigned int> bad;
    RQC(bad.alloc(1));
    HIPC(hipMemset(bad.p, 0, 4));
    if (n && idx->k) list_order_kernel<<<idx->k, 256>>>(idx->offsets.p, rk.p, idx->map_ids.p, bad.p);
    unsigned int h_bad = 0;
    HIPC(hipMemcpy(&h_bad, bad.p, 4, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    std::swap(idx->row_key.p, rk.p);
    std::swap(idx->row_key.count, rk.count);
    idx->row_key_valid = true;
    idx->row_order_ok = h_bad == 0;
    g_mutate_stats.ms_keys = clk.lap();
    return RQ_OK;
}

// what rq_add and rq_merge_from answer where ensure_row_keys found a list out of order
static const char *const kOrderRefusal =
    "a list of this index is not in the build's order (distance to its centroid, then id): rows can be "
    "removed from it, but not added (an index from rq_from_arrays / rq_load_dir whose ids were remapped?)";

static rq_status mutate_refusals(const rq_index *idx) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    if (idx->base_host) return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are tiered (HBM + pinned host memory): it cannot be mutated");
    if (idx->split_rows) return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are stored as split rows: it cannot be mutated");
    if (idx->rows.typed()) return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are half-precision or byte rows: it cannot be mutated");
    if (idx->is_shard) return fail(RQ_ERR_UNSUPPORTED, "a shard made by rq_shard_index cannot be mutated (its ids are global)");
    if (idx->dim > 4096) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
    if (idx->open_tickets.load()) return fail(RQ_ERR_INVALID, "a rq_query_batch_device_begin ticket of this index has not ended");
    return RQ_OK;
}

template <typename T>
static void swap_buf(DevBuf<T> &a, DevBuf<T> &b) {
    std::swap(a.p, b.p);
    std::swap(a.count, b.count);
}

// The new rows of a relayout, after pass 1 and the per-list sort (device memory).
struct NewRows {
    uint64_t m = 0;
    uint32_t d = 0;
    const float *rows = nullptr;         // m x d, device
    DevBuf<uint32_t> off;                // k + 1: sorted new rows of list c = [off[c], off[c + 1])
    DevBuf<unsigned long long> keys;     // m: ord32_biased(dist) << 32 | batch rank of the row's id
    DevBuf<uint32_t> ids;                // m: ids in ascending order (empty: id0 + rank)
    DevBuf<uint32_t> src;                // m: input row of batch rank r (empty: r)
    uint32_t id0 = 0;
    std::unique_ptr<rq_builder> b;       // pass-1 state: codes_tmp / factors_tmp by input row
};

// Pass 1 of the build on the new rows (rotate, nearest list, sign-pack + factors) with the index's own rotation and centroids,
// then the build's grouping by list and per-list sort.  ranks (nullable, device): the rank of row i's id within the batch.
static rq_status new_rows_prepare(const rq_index *idx, const float *d_rows, uint64_t m, uint32_t d, const uint32_t *ranks, NewRows &nr) {
    const uint32_t k = idx->k, dim = idx->dim;
    PhaseClock clk;
    nr.m = m, nr.d = d, nr.rows = d_rows;
    nr.b.reset(new rq_builder());
    rq_builder *b = nr.b.get();
    b->idx.reset(new rq_index());
    rq_index *bx = b->idx.get();
    bx->dim = dim, bx->k = k, bx->n = m, bx->W = idx->W;
    b->d = d;
    RQC(bx->P.alloc((size_t)dim * dim));
    RQC(bx->centroids.alloc((size_t)k * dim));
    RQC(bx->cent_t.alloc((size_t)dim * k));
    HIPC(hipMemcpy(bx->P.p, idx->P.p, (size_t)dim * dim * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(bx->centroids.p, idx->centroids.p, (size_t)k * dim * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(bx->cent_t.p, idx->cent_t.p, (size_t)k * dim * 4, hipMemcpyDeviceToDevice));
    RQC(builder_alloc_pass1(b));
    RQC(builder_assign(b, RowsIn::plain(d_rows), 0, m));
    b->xpad.release();
    b->xrot.release();
    DevBuf<uint32_t> cnt;
    RQC(cnt.alloc((size_t)k + 1));
    RQC(nr.off.alloc((size_t)k + 1));
    RQC(nr.keys.alloc(m));
    HIPC(hipMemset(cnt.p, 0, ((size_t)k + 1) * 4));
    label_hist_kernel<<<ceil_div(m, 256), 256>>>(b->label.p, m, cnt.p);
    group_scan_kernel<<<1, 1024>>>(cnt.p, k, nr.off.p, 0u, nullptr, 0u);  // also zeroes cnt -> cursor
    label_scatter_kernel<<<ceil_div(m, 256), 256>>>(b->label.p, b->mind.p, m, 0, nr.off.p, cnt.p, nr.keys.p, ranks);
    list_sort_kernel<<<k, 1024>>>(nr.keys.p, nr.off.p);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    b->label.release();
    b->mind.release();
    g_mutate_stats.ms_assign = clk.lap();
    return RQ_OK;
}

// The commit of a relayout (rq_add / rq_remove; rq_merge_from, host_merge.h): the new layout's arrays and derived state move into
// *idx, the old ones leave with nx; the generation is bumped, workspaces and tile tables go, the learnt hints stay.
static rq_status commit_layout(rq_index *idx, std::unique_ptr<rq_index> &nx, PhaseClock &clk) {
    rq_mutate_stats_t &st = g_mutate_stats;
    swap_buf(idx->base, nx->base), swap_buf(idx->P, nx->P), swap_buf(idx->centroids, nx->centroids), swap_buf(idx->cent_t, nx->cent_t);
    swap_buf(idx->base_h, nx->base_h), swap_buf(idx->base_q8, nx->base_q8), swap_buf(idx->list_q8, nx->list_q8);
    swap_buf(idx->offsets, nx->offsets), swap_buf(idx->map_ids, nx->map_ids), swap_buf(idx->codes, nx->codes);
    swap_buf(idx->factors, nx->factors), swap_buf(idx->list_uref, nx->list_uref), swap_buf(idx->cent_bf, nx->cent_bf);
    swap_buf(idx->cent_sqnorm, nx->cent_sqnorm), swap_buf(idx->row_key, nx->row_key);
    idx->n = nx->n, idx->n_dev = nx->n_dev, idx->max_list_len = nx->max_list_len, idx->min_list_len = nx->min_list_len;
    idx->cent_norm_max = nx->cent_norm_max, idx->nonempty_lists = nx->nonempty_lists, idx->fstats = nx->fstats;
    idx->pass_budget = nx->pass_budget;
    idx->h_offsets.swap(nx->h_offsets);
    idx->row_key_valid = true;
    delete idx->live;  // the pending removals went with the old layout (every relayout of a pending index drops them)
    idx->live = nullptr;
    {  // workspaces and tile tables describe the old layout (no query runs during a mutation; the learnt hints stay)
        std::lock_guard<std::mutex> g(idx->tt_mu);
        idx->tile_tables.clear();
    }
    {
        std::lock_guard<std::mutex> g(idx->ws_mu);
        idx->ws_pool.clear();
    }
    ++idx->generation;
    nx.reset();  // the old layout's arrays
    HIPC(hipDeviceSynchronize());
    st.ms_free = clk.lap();
    // The derived state was chosen while the old layout still held its HBM: a shadow that did not fit then, and the pass budget,
    // are decided again now, as a fresh build would decide them.
    // (Both are optional refinements of a committed index: a failure here leaves the shadow out, it does not fail the call.)
    if (!idx->base_q8.p && !idx->base_h.p) (void)derive_shadow_rows(idx);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        idx->pass_budget = std::min<uint64_t>(std::max<uint64_t>(free_b / 3, 4ull << 30), 96ull << 30);
    (void)hipGetLastError();
    st.ms_derive += clk.lap();
    return RQ_OK;
}

// The relayout: a fresh index with the kept old rows and the new rows in the build's order, its derived state recomputed, moved
// into *idx only when everything has succeeded.  drop_bits (device, position bitmap) and nr are never both given.
static rq_status relayout(rq_index *idx, const uint32_t *drop_bits, const std::vector<uint32_t> &dropped_per_list, NewRows *nr) {
    const uint32_t k = idx->k, dim = idx->dim, W = idx->W;
    const uint64_t n_old = idx->n;
    std::vector<uint32_t> h_new((size_t)k + 1, 0), h_out((size_t)k + 1, 0);
    if (nr) HIPC(hipMemcpy(h_new.data(), nr->off.p, ((size_t)k + 1) * 4, hipMemcpyDeviceToHost));
    uint64_t n = 0;
    for (uint32_t c = 0; c < k; ++c) {
        h_out[c] = (uint32_t)n;
        n += (uint64_t)idx->h_offsets[c + 1] - idx->h_offsets[c] - (dropped_per_list.empty() ? 0u : dropped_per_list[c]);
        n += h_new[c + 1] - h_new[c];
    }
    h_out[k] = (uint32_t)n;
    rq_mutate_stats_t &st = g_mutate_stats;
    PhaseClock clk;
    std::unique_ptr<rq_index> nx(new rq_index());
    nx->dim = dim, nx->k = k, nx->W = W, nx->n = n, nx->n_dev = n;
    RQC(nx->P.alloc((size_t)dim * dim));
    RQC(nx->centroids.alloc((size_t)k * dim));
    RQC(nx->offsets.alloc((size_t)k + 1));
    RQC(nx->base.alloc(n * dim));
    RQC(nx->codes.alloc(n * W));
    RQC(nx->factors.alloc(n));
    RQC(nx->map_ids.alloc(n));
    RQC(nx->row_key.alloc(n));
    DevBuf<uint32_t> src_of_dst, empty_off;
    DevBuf<unsigned int> holes;
    RQC(src_of_dst.alloc(n));
    RQC(holes.alloc(1));
    HIPC(hipMemset(holes.p, 0, 4));
    HIPC(hipMemset(src_of_dst.p, 0xFF, n * 4));  // (a destination the merge left unset is skipped by the gather, never read through)
    HIPC(hipMemcpy(nx->P.p, idx->P.p, (size_t)dim * dim * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(nx->centroids.p, idx->centroids.p, (size_t)k * dim * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(nx->offsets.p, h_out.data(), ((size_t)k + 1) * 4, hipMemcpyHostToDevice));
    const uint32_t *new_off = nullptr;
    if (nr) {
        new_off = nr->off.p;
    } else {  // no new rows: every list's range is empty
        RQC(empty_off.alloc((size_t)k + 1));
        HIPC(hipMemset(empty_off.p, 0, ((size_t)k + 1) * 4));
        new_off = empty_off.p;
    }
    HIPC(hipDeviceSynchronize());
    st.ms_alloc = clk.lap();
    const unsigned long long *nkeys = nr ? nr->keys.p : nullptr;
    const uint32_t *nids = nr && nr->ids.p ? nr->ids.p : nullptr, *nsrc = nr && nr->src.p ? nr->src.p : nullptr;
    const uint32_t id0 = nr ? nr->id0 : 0u;
    if (k)
        mutate_merge_kernel<<<k, 256>>>(idx->offsets.p, idx->row_key.p, idx->map_ids.p, drop_bits, new_off, nkeys, nids, id0,
                                        nx->offsets.p, (uint32_t)n_old, src_of_dst.p);
    HIPC(hipDeviceSynchronize());
    st.ms_merge = clk.lap();
    if (n)
        mutate_gather_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(n, 4), 1u << 20), 256>>>(
            src_of_dst.p, n, (uint32_t)n_old, nr ? (uint32_t)nr->m : 0u, dim, W, idx->base.p, idx->codes.p, idx->factors.p, idx->map_ids.p, idx->row_key.p,
            nkeys, nids, id0, nsrc, nr ? nr->rows : nullptr, nr ? nr->d : dim, nr ? nr->b->codes_tmp.p : nullptr,
            nr ? nr->b->factors_tmp.p : nullptr, nx->base.p, nx->codes.p, nx->factors.p, nx->map_ids.p, nx->row_key.p, holes.p);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    st.ms_gather = clk.lap();
    // bytes the gather moves: every destination row read once and written once (raw vector, codes, factors, id, key)
    st.gather_bytes = 2 * n * ((uint64_t)dim * 4 + (uint64_t)W * 8 + 16 + 4 + 4) + n * 4;
    unsigned int h_holes = 0;
    HIPC(hipMemcpy(&h_holes, holes.p, 4, hipMemcpyDeviceToHost));
    if (h_holes)  // (cannot happen on lists in the build's order, which rq_add checks; refused rather than committed)
        return fail(RQ_ERR_HIP, "internal: the merge left " + std::to_string(h_holes) + " rows of the new layout unset");
    src_of_dst.release();
    if (nr) nr->b.reset();  // pass-1 buffers, before the derived state takes its room
    RQC(finish_index(nx.get()));
    nx->row_key_valid = true;
    st.ms_derive = clk.lap();

    return commit_layout(idx, nx, clk);
}

// 1 + the largest id the index holds (0 if empty), and how many of its ids are among the m ascending ids `sorted` (device; nullable)
static rq_status scan_ids(const rq_index *idx, const uint32_t *sorted, uint64_t m, uint64_t *top, uint64_t *hits) {
    DevBuf<unsigned long long> out;
    RQC(out.alloc(2));
    HIPC(hipMemset(out.p, 0, 16));
    if (idx->n)
        id_scan_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(idx->n, 256), 4096), 256>>>(idx->map_ids.p, idx->n, sorted, (uint32_t)m, out.p);
    unsigned long long h[2];
    HIPC(hipMemcpy(h, out.p, 16, hipMemcpyDeviceToHost));
    *top = h[0], *hits = h[1];
    return RQ_OK;
}

static void mutate_stats_begin(const rq_index *idx) {
    g_mutate_stats = rq_mutate_stats_t{};
    g_mutate_stats.struct_size = sizeof(rq_mutate_stats_t);
    g_mutate_stats.rows_before = g_mutate_stats.rows_after = idx ? idx->n : 0;
}

// ---- filters and lazy removal -----------------------------------------------------------------------------------
// What follows from a filter's position bitmap (f->pos_bits, filled by work already enqueued on `st`, in idx's layout): the admitted
// rows per list, their prefix sums (the sub-index's offsets, device and host), the ScanExtra and the row counts.  The caller's
// filters (rq_filter_create) and the index's live filter (rq_remove_lazy) are finished here.
static rq_status filter_finish(const rq_index *idx, rq_filter *f, hipStream_t st) {
    const uint32_t k = idx->k;
    DevBuf<uint32_t> counts;
    RQC(counts.alloc(std::max<uint32_t>(k, 1)));
    RQC(f->sub_off.alloc((size_t)k + 1));
    RQC(f->extra.alloc(1));
    if (k) filter_lists_kernel<<<k, 256, 0, st>>>(f->pos_bits.p, idx->offsets.p, counts.p);
    std::vector<uint32_t> h_cnt(k);
    std::vector<uint32_t> &h_off = f->h_sub_off;
    h_off.assign((size_t)k + 1, 0);
    if (k) HIPC(hipMemcpyAsync(h_cnt.data(), counts.p, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    for (uint32_t c = 0; c < k; ++c) h_off[c + 1] = h_off[c] + h_cnt[c];  // the sub-index's offsets (<= n < 2^32)
    HIPC(hipMemcpy(f->sub_off.p, h_off.data(), h_off.size() * 4, hipMemcpyHostToDevice));
    ScanExtra hx{};
    hx.allow = f->pos_bits.p;
    HIPC(hipMemcpy(f->extra.p, &hx, sizeof hx, hipMemcpyHostToDevice));
    f->rows = h_off[k];
    f->live_rows = 0;
    if (idx->h_offsets.size() == (size_t)k + 1) {
        for (uint32_t c = 0; c < k; ++c) f->live_rows += h_cnt[c] ? idx->h_offsets[c + 1] - idx->h_offsets[c] : 0u;
    } else
        f->live_rows = idx->n;
    f->idx = idx;
    f->generation = idx->generation;
    f->removal_epoch = idx->removal_epoch;
    return RQ_OK;
}

// words of a position bitmap over n positions: whole 64-position waves, and never empty
static uint64_t pos_bitmap_words(uint64_t n) { return (n + 63) / 64 * 2 + 2; }
static uint32_t bitmap_grid(uint64_t nwords) { return (uint32_t)std::min<uint64_t>(ceil_div(nwords, 256), 4096); }

// rq_remove_lazy: the rows whose id bit is set leave the live filter; nothing of the index's arrays moves.  The new bitmap and
// what follows from it are made beside the old ones and swapped in only when everything has succeeded.
static rq_status index_remove_lazy(rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, uint64_t *out_marked) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");  // (before the device is looked for, as rq_merge_from)
    RQC(ensure_device());
    if (out_marked) *out_marked = 0;
    if (idx->is_shard) return fail(RQ_ERR_UNSUPPORTED, "a shard made by rq_shard_index cannot be mutated (its ids are global)");
    if (nbits > (1ull << 32)) return fail(RQ_ERR_INVALID, "nbits > 2^32 (ids are u32)");
    if (!id_bits && nbits > 0) return fail(RQ_ERR_INVALID, "null bitmap with nbits > 0");
    if (idx->open_tickets.load()) return fail(RQ_ERR_INVALID, "a rq_query_batch_device_begin ticket of this index has not ended");
    const uint64_t n = idx->n, nwords = pos_bitmap_words(n), in_words = (nbits + 31) / 32;
    if (n == 0 || nbits == 0) return RQ_OK;
    DevBuf<uint32_t> staged;
    const uint32_t *d_bits = id_bits;
    if (!bits_on_device) {
        RQC(staged.upload(id_bits, in_words));
        d_bits = staged.p;
    }
    std::unique_ptr<rq_filter> nf(new rq_filter());
    DevBuf<unsigned long long> marked;
    RQC(nf->pos_bits.alloc(nwords));
    RQC(marked.alloc(1));
    HIPC(hipMemset(nf->pos_bits.p, 0, nwords * 4));
    HIPC(hipMemset(marked.p, 0, 8));
    tombstone_positions_kernel<<<(uint32_t)((n + 255) / 256), 256>>>(idx->map_ids.p, n, d_bits, nbits, idx->live ? idx->live->pos_bits.p : nullptr,
                                                                     nf->pos_bits.p, nwords, marked.p);
    unsigned long long h_marked = 0;
    HIPC(hipMemcpy(&h_marked, marked.p, 8, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    if (h_marked == 0) return RQ_OK;  // nothing changed: the epoch stays, earlier filters stay valid
    RQC(filter_finish(idx, nf.get(), nullptr));
    if (!idx->live) {
        idx->live = nf.release();
    } else {  // in place: the filter object and the hints its passes learnt stay
        rq_filter *L = idx->live;
        swap_buf(L->pos_bits, nf->pos_bits), swap_buf(L->sub_off, nf->sub_off), swap_buf(L->extra, nf->extra);
        L->h_sub_off.swap(nf->h_sub_off);
        L->rows = nf->rows, L->live_rows = nf->live_rows;
    }
    idx->live->removal_epoch = ++idx->removal_epoch;
    if (out_marked) *out_marked = h_marked;
    return RQ_OK;
}

// The relayout that drops the pending removals (the index has some, and mutate_refusals has passed): rq_remove of the dead rows.
static rq_status compact_relayout(rq_index *idx) {
    const uint64_t k = idx->k, nwords = pos_bitmap_words(idx->n);
    DevBuf<uint32_t> drop;
    RQC(drop.alloc(nwords));
    HIPC(hipMemset(drop.p, 0, nwords * 4));
    bitmap_or_not_kernel<<<bitmap_grid(nwords), 256>>>(drop.p, idx->live->pos_bits.p, nwords);
    HIPC(hipGetLastError());
    std::vector<uint32_t> dropped(k);
    const std::vector<uint32_t> &so = idx->live->h_sub_off;
    for (uint32_t c = 0; c < k; ++c) dropped[c] = idx->h_offsets[c + 1] - idx->h_offsets[c] - (so[c + 1] - so[c]);
    RQC(ensure_row_keys(idx));
    return relayout(idx, drop.p, dropped, nullptr);
}

// rq_add / rq_merge_from on an index with pending removals compact it first: one more relayout, whose phases are added to the
// call's own when it ends (rows_before stays the stored row count the call found).
struct CompactFirst {
    rq_mutate_stats_t pre{};
    bool on = false;
    rq_status run(rq_index *idx) {
        if (!idx->live) return RQ_OK;
        RQC(compact_relayout(idx));
        pre = g_mutate_stats, on = true;
        const uint64_t rows_before = pre.rows_before;
        mutate_stats_begin(idx);
        g_mutate_stats.rows_before = rows_before;
        return RQ_OK;
    }
    ~CompactFirst() {
        if (!on) return;
        rq_mutate_stats_t &st = g_mutate_stats;
        st.ms_keys += pre.ms_keys, st.ms_assign += pre.ms_assign, st.ms_alloc += pre.ms_alloc, st.ms_merge += pre.ms_merge;
        st.ms_gather += pre.ms_gather, st.ms_derive += pre.ms_derive, st.ms_free += pre.ms_free, st.gather_bytes += pre.gather_bytes;
    }
};

static rq_status index_compact(rq_index *idx, uint64_t *out_removed) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");  // (before the device is looked for)
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    mutate_stats_begin(idx);
    if (out_removed) *out_removed = 0;
    if (!idx->live) return RQ_OK;  // nothing pending: nothing changes, the generation stays
    RQC(mutate_refusals(idx));
    const uint64_t total = idx->pending();
    RQC(compact_relayout(idx));
    if (out_removed) *out_removed = total;
    return RQ_OK;
}

static rq_status index_add(rq_index *idx, const float *rows, uint64_t m, uint32_t d, const uint32_t *ids, int rows_on_device,
                           uint32_t *out_first_id) {
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    mutate_stats_begin(idx);
    RQC(mutate_refusals(idx));
    if (m && !rows) return fail(RQ_ERR_INVALID, "null rows with m > 0");
    RQC(raw_len_check(idx, "row", d));
    if (m >= 0xFFFFFFFFull || idx->n + m >= 0xFFFFFFFFull) return fail(RQ_ERR_UNSUPPORTED, "n must fit u32 ids (rabitq.rs:64-65)");
    CompactFirst pending;  // (before the ids are looked at: a dead row's id is free again)
    RQC(pending.run(idx));
    uint64_t top = 0, hits = 0;
    NewRows nr;
    std::vector<uint32_t> h_ids;
    DevBuf<uint32_t> ranks;
    if (ids) {  // explicit ids: unique in the batch, absent from the index
        h_ids.resize(m);
        if (m && rows_on_device) HIPC(hipMemcpy(h_ids.data(), ids, m * 4, hipMemcpyDeviceToHost));
        else if (m) memcpy(h_ids.data(), ids, m * 4);
        std::vector<uint32_t> order(m);
        for (uint64_t i = 0; i < m; ++i) order[i] = (uint32_t)i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return h_ids[a] < h_ids[b]; });
        std::vector<uint32_t> sorted(m), rank(m);
        for (uint64_t r = 0; r < m; ++r) sorted[r] = h_ids[order[r]], rank[order[r]] = (uint32_t)r;
        for (uint64_t r = 1; r < m; ++r)
            if (sorted[r] == sorted[r - 1]) return fail(RQ_ERR_INVALID, "id " + std::to_string(sorted[r]) + " appears twice in the batch");
        if (m == 0) {
            if (out_first_id) *out_first_id = 0;
            return RQ_OK;
        }
        RQC(nr.ids.upload(sorted.data(), m));
        RQC(scan_ids(idx, nr.ids.p, m, &top, &hits));
        if (hits) return fail(RQ_ERR_INVALID, std::to_string(hits) + " of the ids are already in the index");
        RQC(nr.src.upload(order.data(), m));
        RQC(ranks.upload(rank.data(), m));
        if (out_first_id) *out_first_id = sorted[0];
    } else {  // the next ids: 1 + the largest id the index holds
        RQC(scan_ids(idx, nullptr, 0, &top, &hits));
        if (top + m > (1ull << 32)) return fail(RQ_ERR_UNSUPPORTED, "the next ids would pass 2^32 - 1 (ids are u32)");
        nr.id0 = (uint32_t)top;
        if (out_first_id) *out_first_id = (uint32_t)top;
        if (m == 0) return RQ_OK;
    }
    DevBuf<float> staged;  // host rows are copied once
    const float *d_rows = rows;
    if (!rows_on_device) {
        RQC(staged.upload(rows, m * d));
        d_rows = staged.p;
    }
    RQC(ensure_row_keys(idx));
    if (!idx->row_order_ok) return fail(RQ_ERR_UNSUPPORTED, kOrderRefusal);
    if (idx->metric.id != RQ_METRIC_L2) {  // N(row) / A(row; the index's S), padded: pass 1 and the gather then take the rows as an L2 build of them does
        DevBuf<float> stored;
        DevBuf<uint32_t> bad;
        RQC(stored.alloc(m * idx->dim));
        const bool refuses = metric_refuses_rows(idx->metric);
        if (refuses) RQC(bad.alloc(1));
        RQC(transform_rows(idx->metric, idx->dim, d_rows, m, d, 0, stored.p, nullptr, BaseView{}, nullptr, bad.p));
        HIPC(hipDeviceSynchronize());
        HIPC(hipGetLastError());
        if (refuses) RQC(bad_row_check(bad.p, " of the batch:", "the index's sq_bound"));  // refused before anything of the index is touched
        staged.take(stored);  // (the raw copy is released)
        d_rows = staged.p, d = idx->dim;
    }
    RQC(new_rows_prepare(idx, d_rows, m, d, ranks.p, nr));
    ranks.release();
    return relayout(idx, nullptr, {}, &nr);
}

static rq_status index_remove(rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, uint64_t *out_removed) {
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    mutate_stats_begin(idx);
    RQC(mutate_refusals(idx));
    if (nbits > (1ull << 32)) return fail(RQ_ERR_INVALID, "nbits > 2^32 (ids are u32)");
    if (!id_bits && nbits > 0) return fail(RQ_ERR_INVALID, "null bitmap with nbits > 0");
    if (out_removed) *out_removed = 0;
    const uint64_t n = idx->n, k = idx->k, nwords = (n + 63) / 64 * 2 + 2, in_words = (nbits + 31) / 32;
    const uint64_t pending = idx->pending();  // rows marked dead by rq_remove_lazy: this relayout drops them with the requested ones
    if (n == 0 || (nbits == 0 && !pending)) return RQ_OK;
    DevBuf<uint32_t> staged, pos_bits, counts;
    const uint32_t *d_bits = id_bits;
    if (!bits_on_device && in_words) {
        RQC(staged.upload(id_bits, in_words));
        d_bits = staged.p;
    }
    RQC(pos_bits.alloc(nwords));
    RQC(counts.alloc(std::max<uint64_t>(k, 1)));
    HIPC(hipMemset(pos_bits.p, 0, nwords * 4));
    if (nbits) filter_positions_kernel<<<(uint32_t)((n + 255) / 256), 256>>>(idx->map_ids.p, n, d_bits, nbits, pos_bits.p, nwords);
    if (pending) bitmap_or_not_kernel<<<bitmap_grid(nwords), 256>>>(pos_bits.p, idx->live->pos_bits.p, nwords);
    if (k) filter_lists_kernel<<<(uint32_t)k, 256>>>(pos_bits.p, idx->offsets.p, counts.p);
    std::vector<uint32_t> dropped(k);
    if (k) HIPC(hipMemcpy(dropped.data(), counts.p, k * 4, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    uint64_t total = 0;
    for (uint32_t v : dropped) total += v;
    if (total == 0) return RQ_OK;
    staged.release();
    counts.release();
    RQC(ensure_row_keys(idx));
    RQC(relayout(idx, pos_bits.p, dropped, nullptr));
    if (out_removed) *out_removed = total - pending;  // (rows that were live; the pending ones were counted when they were marked)
    return RQ_OK;
}
