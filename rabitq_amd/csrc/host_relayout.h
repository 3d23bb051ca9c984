// host_relayout.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  The relayout core behind rq_add / rq_remove / rq_compact / rq_merge_from / rq_extract
// (entries: host_mutate.h): two sides A and B over the same rotation and centroids, plus an optional
// keep-bitmap on A -> merge_lists_kernel -> merge_gather_kernel -> finish_index -> commit_layout, or a hand-out for rq_extract.
// Also what the entries share before it: the key cache, the refusals, the id-bitmap prologue, and what a filter derives from its
// position bitmap (filter_finish, shared by rq_filter_create and rq_remove_lazy).
#pragma once

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

static void mutate_stats_begin(const rq_index *idx) {
    g_mutate_stats = rq_mutate_stats_t{};
    g_mutate_stats.struct_size = sizeof(rq_mutate_stats_t);
    g_mutate_stats.rows_before = g_mutate_stats.rows_after = idx ? idx->n : 0;
}

// The key word of every stored row (row_key), once per index: the stored rows are the build's zero-padded input, so rotating
// them again (same kernel, same P) and taking the distance to their own list's centroid in the assignment's lane order gives
// back the build's key bit for bit.
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

// ---- position bitmaps -------------------------------------------------------------------------------------------
// words of a position bitmap over n positions: whole 64-position waves, and never empty
static uint64_t pos_bitmap_words(uint64_t n) { return (n + 63) / 64 * 2 + 2; }
static uint32_t bitmap_grid(uint64_t nwords) { return (uint32_t)std::min<uint64_t>(ceil_div(nwords, 256), 4096); }

// what every entry that takes an id bitmap refuses
static rq_status id_bits_check(const uint32_t *id_bits, uint64_t nbits) {
    if (nbits > (1ull << 32)) return fail(RQ_ERR_INVALID, "nbits > 2^32 (ids are u32)");
    if (!id_bits && nbits > 0) return fail(RQ_ERR_INVALID, "null bitmap with nbits > 0");
    return RQ_OK;
}

// The id bitmap of a call where the kernels can read it: a host bitmap is copied into `staged`, which then has to outlive them.
static rq_status stage_id_bits(const uint32_t *id_bits, uint64_t nbits, int bits_on_device, DevBuf<uint32_t> &staged, const uint32_t **d_bits) {
    *d_bits = id_bits;
    if (bits_on_device || nbits == 0) return RQ_OK;
    RQC(staged.upload(id_bits, (nbits + 31) / 32));
    *d_bits = staged.p;
    return RQ_OK;
}

// The rows of each list whose bit is set in a position bitmap of idx's layout (enqueued on `st`, which is waited for), as prefix
// sums: h_off (k + 1) holds the list offsets of the sub-index those rows form (<= n < 2^32).
static rq_status list_prefix_sums(const rq_index *idx, const uint32_t *pos_bits, hipStream_t st, std::vector<uint32_t> &h_off) {
    const uint32_t k = idx->k;
    DevBuf<uint32_t> counts;
    RQC(counts.alloc(std::max<uint32_t>(k, 1)));
    if (k) filter_lists_kernel<<<k, 256, 0, st>>>(pos_bits, idx->offsets.p, counts.p);  // (masks each list's first and last word)
    std::vector<uint32_t> h_cnt(k);
    if (k) HIPC(hipMemcpyAsync(h_cnt.data(), counts.p, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    h_off.assign((size_t)k + 1, 0);
    for (uint32_t c = 0; c < k; ++c) h_off[c + 1] = h_off[c] + h_cnt[c];
    return RQ_OK;
}

// The prologue of every entry that takes ids as a bitmap (rq_filter_create, rq_remove, rq_extract): id bitmap (nbits bits, host or
// device; every_id: no bitmap, every id is set) -> the bitmap by position in idx's layout (filter_positions_kernel), complemented
// for flip == ~0u, ANDed with the live bitmap where removals are pending -> the selected rows per list as prefix sums (h_off).
// Runs on `st` and returns when it is done.  Bits past the last position are not defined (see bitmap_and_live_kernel).
static rq_status position_bits(const rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, bool every_id, uint32_t flip,
                               hipStream_t st, DevBuf<uint32_t> &pos_bits, std::vector<uint32_t> &h_off) {
    const uint64_t n = idx->n, nwords = pos_bitmap_words(n);
    DevBuf<uint32_t> staged;
    const uint32_t *d_bits = nullptr;
    if (!every_id) RQC(stage_id_bits(id_bits, nbits, bits_on_device, staged, &d_bits));
    RQC(pos_bits.alloc(nwords));
    HIPC(hipMemsetAsync(pos_bits.p, every_id ? 0xFF : 0, nwords * 4, st));
    if (n && nbits && !every_id) filter_positions_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, st>>>(idx->map_ids.p, n, d_bits, nbits, pos_bits.p, nwords);
    if (idx->live || flip)
        bitmap_and_live_kernel<<<bitmap_grid(nwords), 256, 0, st>>>(pos_bits.p, flip, idx->live ? idx->live->pos_bits.p : nullptr, nwords);
    return list_prefix_sums(idx, pos_bits.p, st, h_off);
}

// What follows from a filter's position bitmap and the prefix sums of its rows per list (f->pos_bits, f->h_sub_off: position_bits
// or list_prefix_sums, in idx's layout): the sub-index's offsets on the device, the ScanExtra and the row counts.  The caller's
// filters (rq_filter_create) and the index's live filter (rq_remove_lazy) are finished here.
static rq_status filter_finish(const rq_index *idx, rq_filter *f) {
    const uint32_t k = idx->k;
    const std::vector<uint32_t> &h_off = f->h_sub_off;
    RQC(f->sub_off.upload(h_off.data(), h_off.size()));
    RQC(f->extra.alloc(1));
    ScanExtra hx{};
    hx.allow = f->pos_bits.p;
    HIPC(hipMemcpy(f->extra.p, &hx, sizeof hx, hipMemcpyHostToDevice));
    f->rows = h_off[k];
    f->live_rows = 0;
    if (idx->h_offsets.size() == (size_t)k + 1) {
        for (uint32_t c = 0; c < k; ++c) f->live_rows += h_off[c + 1] > h_off[c] ? idx->h_offsets[c + 1] - idx->h_offsets[c] : 0u;
    } else
        f->live_rows = idx->n;
    f->idx = idx;
    f->generation = idx->generation;
    f->removal_epoch = idx->removal_epoch;
    return RQ_OK;
}

// ---- the core ------------------------------------------------------------------------------------------------------------------------
// (host_attr.h) every attribute column of a follows the layout's destination-to-source map into nx; *bytes += what that moves
static rq_status columns_follow(const rq_index *a, const rq_index *b, const uint32_t *src_of_dst, uint64_t n, rq_index *nx, uint64_t *bytes);

static MergeSide merge_side(const rq_index *idx, bool keys) {
    if (!idx) return MergeSide{nullptr, nullptr, nullptr, nullptr, nullptr};
    return MergeSide{reinterpret_cast<const float4 *>(idx->base.p), idx->codes.p, idx->factors.p, idx->map_ids.p, keys ? idx->row_key.p : nullptr};
}

// Sub-group width and rows in flight by row length (kernels_relayout.h): dim / 4 lanes of 16 B, at least 16, at most 64.
static void launch_merge_gather(const uint32_t *src_of_dst, uint64_t n, const rq_index *a, const rq_index *b, uint32_t shift_b, bool keys,
                                rq_index *out, unsigned int *holes) {
    constexpr int R = 4;
    const uint32_t dim = a->dim, W = a->W, n_a = (uint32_t)a->n, n_b = b ? (uint32_t)b->n : 0u;
    const MergeSide sa = merge_side(a, keys), sb = merge_side(b, keys);
    float4 *base_o = reinterpret_cast<float4 *>(out->base.p);
    uint32_t *key_o = keys ? out->row_key.p : nullptr;
    const uint32_t G = dim <= 64 ? 16u : (dim <= 128 ? 32u : 64u);
    const uint32_t rows_per_block = 4 * R * (64 / G);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ceil_div(n, rows_per_block), 1u << 20);
    if (G == 16)
        merge_gather_kernel<16, R><<<grid, 256>>>(src_of_dst, n, n_a, n_b, dim, W, sa, sb, shift_b, base_o, out->codes.p, out->factors.p, out->map_ids.p, key_o, holes);
    else if (G == 32)
        merge_gather_kernel<32, R><<<grid, 256>>>(src_of_dst, n, n_a, n_b, dim, W, sa, sb, shift_b, base_o, out->codes.p, out->factors.p, out->map_ids.p, key_o, holes);
    else
        merge_gather_kernel<64, R><<<grid, 256>>>(src_of_dst, n, n_a, n_b, dim, W, sa, sb, shift_b, base_o, out->codes.p, out->factors.p, out->map_ids.p, key_o, holes);
}

// The new layout beside its sources: arrays, merge, gather, derived state.  a: an index.  b (nullable): the other side, an index or
// the batch of an rq_add in an index's shape (offsets, row_key, map_ids, base, codes, factors, n, h_offsets; add_side, host_mutate.h),
// its ids counting with shift_b added.  keep_bits (nullable, never with b): the rows of a that stay, as a position bitmap.
// h_out: the new list offsets (k + 1).  keys: the key cache travels (a, and b, have one).  Nothing of a or b is written.
static rq_status build_layout(const rq_index *a, const rq_index *b, uint32_t shift_b, const uint32_t *keep_bits, bool keys,
                              const std::vector<uint32_t> &h_out, std::unique_ptr<rq_index> &nx, PhaseClock &clk) {
    rq_mutate_stats_t &st = g_mutate_stats;
    const uint32_t k = a->k, dim = a->dim, W = a->W;
    const uint64_t n = h_out[k];
    nx.reset(new rq_index());
    nx->dim = dim, nx->k = k, nx->W = W, nx->n = n, nx->n_dev = n, nx->metric = a->metric, nx->rows = a->rows;
    RQC(nx->P.alloc((size_t)dim * dim));
    RQC(nx->centroids.alloc((size_t)k * dim));
    RQC(nx->offsets.alloc((size_t)k + 1));
    RQC(nx->base.alloc(n * dim));
    RQC(nx->codes.alloc(n * W));
    RQC(nx->factors.alloc(n));
    RQC(nx->map_ids.alloc(n));
    if (keys) RQC(nx->row_key.alloc(n));
    DevBuf<uint32_t> src_of_dst;
    DevBuf<unsigned int> holes;
    RQC(src_of_dst.alloc(n));
    RQC(holes.alloc(1));
    HIPC(hipMemset(holes.p, 0, 4));
    HIPC(hipMemset(src_of_dst.p, 0xFF, n * 4));  // (a destination the merge left unset is skipped by the gather, never read through)
    HIPC(hipMemcpy(nx->P.p, a->P.p, (size_t)dim * dim * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(nx->centroids.p, a->centroids.p, (size_t)k * dim * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(nx->offsets.p, h_out.data(), ((size_t)k + 1) * 4, hipMemcpyHostToDevice));
    HIPC(hipDeviceSynchronize());
    st.ms_alloc = clk.lap();
    if (k)
        merge_lists_kernel<<<k, 256>>>(a->offsets.p, a->row_key.p, a->map_ids.p, keep_bits, b ? b->offsets.p : nullptr, b ? b->row_key.p : nullptr,
                                       b ? b->map_ids.p : nullptr, shift_b, nx->offsets.p, (uint32_t)a->n, src_of_dst.p);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    st.ms_merge = clk.lap();
    if (n) launch_merge_gather(src_of_dst.p, n, a, b, shift_b, keys, nx.get(), holes.p);
    uint64_t column_bytes = 0;  // the attribute columns of a, by the same map (none: nothing is allocated or launched)
    RQC(columns_follow(a, b, src_of_dst.p, n, nx.get(), &column_bytes));
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    st.ms_gather = clk.lap();
    // bytes the gather moves: every destination row read once and written once (raw vector, codes, factors, id, key), and the map
    st.gather_bytes = 2 * n * ((uint64_t)dim * 4 + (uint64_t)W * 8 + 16 + 4 + (keys ? 4 : 0)) + n * 4 + column_bytes;
    unsigned int h_holes = 0;
    HIPC(hipMemcpy(&h_holes, holes.p, 4, hipMemcpyDeviceToHost));
    if (h_holes)  // (cannot happen on lists in the build's order with unique ids, which the caller checks; refused rather than committed)
        return fail(RQ_ERR_HIP, "internal: the merge left " + std::to_string(h_holes) + " rows of the new layout unset");
    src_of_dst.release();
    RQC(finish_index(nx.get()));
    nx->row_key_valid = keys;
    st.ms_derive = clk.lap();
    return RQ_OK;
}

// The commit of a relayout: the new layout's arrays and derived state move into *idx, the old ones leave with nx; the generation
// is bumped, workspaces and tile tables go, the learnt hints stay.
static rq_status commit_layout(rq_index *idx, std::unique_ptr<rq_index> &nx, PhaseClock &clk) {
    rq_mutate_stats_t &st = g_mutate_stats;
    swap_buf(idx->base, nx->base), swap_buf(idx->P, nx->P), swap_buf(idx->centroids, nx->centroids), swap_buf(idx->cent_t, nx->cent_t);
    swap_buf(idx->base_h, nx->base_h), swap_buf(idx->base_q8, nx->base_q8), swap_buf(idx->list_q8, nx->list_q8);
    swap_buf(idx->offsets, nx->offsets), swap_buf(idx->map_ids, nx->map_ids), swap_buf(idx->codes, nx->codes);
    swap_buf(idx->factors, nx->factors), swap_buf(idx->list_uref, nx->list_uref), swap_buf(idx->cent_bf, nx->cent_bf);
    swap_buf(idx->cent_sqnorm, nx->cent_sqnorm), swap_buf(idx->row_key, nx->row_key);
    idx->attrs.swap(nx->attrs);
    idx->n = nx->n, idx->n_dev = nx->n_dev, idx->max_list_len = nx->max_list_len, idx->min_list_len = nx->min_list_len;
    idx->cent_norm_max = nx->cent_norm_max, idx->nonempty_lists = nx->nonempty_lists, idx->fstats = nx->fstats;
    idx->pass_budget = nx->pass_budget;
    idx->h_offsets.swap(nx->h_offsets);
    idx->row_key_valid = true;
    delete idx->live;  // the pending removals went with the old layout (every relayout of a pending index drops them)
    idx->live = nullptr;
    {  // the id directory names positions of the old layout (made again by the next by-id call: host_directory.h)
        std::lock_guard<std::mutex> g(idx->dir_mu);
        idx->dir.reset();
    }
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

// The two relayouts of *idx in place.  relayout_with: side b merged in (rq_add, rq_merge_from; both key caches are there, every
// list of both in the build's order, no id on both sides).  relayout_keeping: only the rows of keep_bits stay (rq_remove,
// rq_compact; h_out: their prefix sums per list).
static rq_status relayout_with(rq_index *idx, const rq_index *b, uint32_t shift_b) {
    const uint32_t k = idx->k;
    std::vector<uint32_t> h_out((size_t)k + 1, 0);
    uint64_t n = 0;
    for (uint32_t c = 0; c < k; ++c) {
        h_out[c] = (uint32_t)n;
        n += (uint64_t)idx->h_offsets[c + 1] - idx->h_offsets[c] + b->h_offsets[c + 1] - b->h_offsets[c];
    }
    h_out[k] = (uint32_t)n;
    PhaseClock clk;
    std::unique_ptr<rq_index> nx;
    RQC(build_layout(idx, b, shift_b, nullptr, true, h_out, nx, clk));
    return commit_layout(idx, nx, clk);
}
static rq_status relayout_keeping(rq_index *idx, const uint32_t *keep_bits, const std::vector<uint32_t> &h_out) {
    RQC(ensure_row_keys(idx));  // (the keep branch reads no keys; the cache is made so that it travels, and stays valid afterwards)
    PhaseClock clk;
    std::unique_ptr<rq_index> nx;
    RQC(build_layout(idx, nullptr, 0u, keep_bits, true, h_out, nx, clk));
    return commit_layout(idx, nx, clk);
}
