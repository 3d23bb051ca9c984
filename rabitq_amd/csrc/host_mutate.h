// host_mutate.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  The entries that change an index's rows, each one relayout through the core of
// host_relayout.h to the index a fresh build of the live rows would produce, bit for bit: rq_add / rq_remove,
// rq_merge_from / rq_extract (§4.17: two indexes over the same rotation and centroids merged list by list, and a sub-index copied
// out of one, without pass 1), and lazy removal (rq_remove_lazy / rq_compact, §4.18): rows marked dead in a filter the index
// owns, dropped by the next relayout.
#pragma once

// ---- lazy removal ------------------------------------------------------------------------------------------------------------------
// rq_remove_lazy: the rows whose id bit is set leave the live filter; nothing of the index's arrays moves.  The new bitmap and
// what follows from it are made beside the old ones and swapped in only when everything has succeeded.
static rq_status index_remove_lazy(rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, uint64_t *out_marked) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");  // (before the device is looked for, as rq_merge_from)
    RQC(ensure_device());
    if (out_marked) *out_marked = 0;
    if (idx->is_shard) return fail(RQ_ERR_UNSUPPORTED, "a shard made by rq_shard_index cannot be mutated (its ids are global)");
    RQC(id_bits_check(id_bits, nbits));
    if (idx->open_tickets.load()) return fail(RQ_ERR_INVALID, "a rq_query_batch_device_begin ticket of this index has not ended");
    const uint64_t n = idx->n, nwords = pos_bitmap_words(n);
    if (n == 0 || nbits == 0) return RQ_OK;
    DevBuf<uint32_t> staged;
    const uint32_t *d_bits = nullptr;
    RQC(stage_id_bits(id_bits, nbits, bits_on_device, staged, &d_bits));
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
    RQC(list_prefix_sums(idx, nf->pos_bits.p, nullptr, nf->h_sub_off));
    RQC(filter_finish(idx, nf.get()));
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

// The relayout that drops the pending removals (the index has some, and mutate_refusals has passed): the live bitmap is the keep
// bitmap, and the live filter's offsets are the new layout's.
static rq_status compact_relayout(rq_index *idx) { return relayout_keeping(idx, idx->live->pos_bits.p, idx->live->h_sub_off); }

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

// ---- rq_remove -----------------------------------------------------------------------------------------------------------------------
static rq_status index_remove(rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, uint64_t *out_removed) {
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    mutate_stats_begin(idx);
    RQC(mutate_refusals(idx));
    RQC(id_bits_check(id_bits, nbits));
    if (out_removed) *out_removed = 0;
    const uint64_t pending = idx->pending();  // rows marked dead by rq_remove_lazy: this relayout drops them with the requested ones
    if (idx->n == 0 || (nbits == 0 && !pending)) return RQ_OK;
    DevBuf<uint32_t> keep;  // NOT requested AND live
    std::vector<uint32_t> h_out;
    RQC(position_bits(idx, id_bits, nbits, bits_on_device, false, ~0u, nullptr, keep, h_out));
    const uint64_t total = idx->n - h_out[idx->k];
    if (total == 0) return RQ_OK;
    RQC(relayout_keeping(idx, keep.p, h_out));
    if (out_removed) *out_removed = total - pending;  // (rows that were live; the pending ones were counted when they were marked)
    return RQ_OK;
}

// ---- rq_add --------------------------------------------------------------------------------------------------------------------------
// The batch of an rq_add as side B of the merge, an index's arrays in device memory (build_layout): pass 1 of the build on the new
// rows (rotate, nearest list, sign-pack + factors) with the index's own rotation and centroids, the build's grouping by list and
// per-list sort, and then the rows, codes, factors, ids and key words put into that order (batch_side_kernel).  ranks (nullable,
// device): the rank of row i's id within the batch, the low word of its sort key; ids (nullable: id0 + rank): the ids ascending;
// src (nullable: rank): the input row of a rank.  The whole of it counts as the call's ms_assign.
static rq_status add_side(const rq_index *idx, const float *d_rows, uint64_t m, uint32_t d, const uint32_t *ranks, const uint32_t *ids,
                          uint32_t id0, const uint32_t *src, std::unique_ptr<rq_index> &side) {
    const uint32_t k = idx->k, dim = idx->dim;
    PhaseClock clk;
    rq_builder b;
    b.idx.reset(new rq_index());
    rq_index *bx = b.idx.get();
    bx->dim = dim, bx->k = k, bx->n = m, bx->n_dev = m, bx->W = idx->W;
    b.d = d;
    RQC(bx->P.alloc((size_t)dim * dim));
    RQC(bx->centroids.alloc((size_t)k * dim));
    RQC(bx->cent_t.alloc((size_t)dim * k));
    HIPC(hipMemcpy(bx->P.p, idx->P.p, (size_t)dim * dim * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(bx->centroids.p, idx->centroids.p, (size_t)k * dim * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(bx->cent_t.p, idx->cent_t.p, (size_t)k * dim * 4, hipMemcpyDeviceToDevice));
    RQC(builder_alloc_pass1(&b));
    RQC(builder_assign(&b, RowsIn::plain(d_rows), 0, m));
    b.xpad.release();
    b.xrot.release();
    DevBuf<uint32_t> cnt;
    DevBuf<unsigned long long> keys;  // m: ord32_biased(dist) << 32 | batch rank of the row's id, grouped by list
    RQC(cnt.alloc((size_t)k + 1));
    RQC(bx->offsets.alloc((size_t)k + 1));
    RQC(keys.alloc(m));
    HIPC(hipMemset(cnt.p, 0, ((size_t)k + 1) * 4));
    label_hist_kernel<<<ceil_div(m, 256), 256>>>(b.label.p, m, cnt.p);
    group_scan_kernel<<<1, 1024>>>(cnt.p, k, bx->offsets.p, 0u, nullptr, 0u);  // also zeroes cnt -> cursor
    label_scatter_kernel<<<ceil_div(m, 256), 256>>>(b.label.p, b.mind.p, m, 0, bx->offsets.p, cnt.p, keys.p, ranks);
    list_sort_kernel<<<k, 1024>>>(keys.p, bx->offsets.p);
    bx->h_offsets.resize((size_t)k + 1);
    HIPC(hipMemcpy(bx->h_offsets.data(), bx->offsets.p, ((size_t)k + 1) * 4, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    b.label.release();
    b.mind.release();
    RQC(bx->base.alloc(m * dim));
    RQC(bx->codes.alloc(m * bx->W));
    RQC(bx->factors.alloc(m));
    RQC(bx->map_ids.alloc(m));
    RQC(bx->row_key.alloc(m));
    batch_side_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(m, 4), 1u << 20), 256>>>(keys.p, m, dim, bx->W, ids, id0, src, d_rows, d, b.codes_tmp.p,
                                                                                       b.factors_tmp.p, bx->base.p, bx->codes.p, bx->factors.p,
                                                                                       bx->map_ids.p, bx->row_key.p);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    bx->P.release(), bx->centroids.release(), bx->cent_t.release();
    side = std::move(b.idx);  // (the rest of pass 1 -- codes and factors by input row -- goes with the builder, before the gather)
    g_mutate_stats.ms_assign = clk.lap();
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
    uint32_t id0 = 0;
    DevBuf<uint32_t> sorted_ids, src, ranks;  // explicit ids: the ids ascending, the input row of each rank, the rank of each input row
    if (ids) {  // explicit ids: unique in the batch, absent from the index
        std::vector<uint32_t> h_ids(m);
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
        RQC(sorted_ids.upload(sorted.data(), m));
        RQC(scan_ids(idx, sorted_ids.p, m, &top, &hits));
        if (hits) return fail(RQ_ERR_INVALID, std::to_string(hits) + " of the ids are already in the index");
        RQC(src.upload(order.data(), m));
        RQC(ranks.upload(rank.data(), m));
        if (out_first_id) *out_first_id = sorted[0];
    } else {  // the next ids: 1 + the largest id the index holds
        RQC(scan_ids(idx, nullptr, 0, &top, &hits));
        if (top + m > (1ull << 32)) return fail(RQ_ERR_UNSUPPORTED, "the next ids would pass 2^32 - 1 (ids are u32)");
        id0 = (uint32_t)top;
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
    if (idx->metric.id != RQ_METRIC_L2) {  // N(row) / A(row; the index's S), padded: pass 1 and the side then take the rows as an L2 build of them does
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
    std::unique_ptr<rq_index> side;
    RQC(add_side(idx, d_rows, m, d, ranks.p, sorted_ids.p, id0, src.p, side));
    staged.release(), ranks.release(), sorted_ids.release(), src.release();
    return relayout_with(idx, side.get(), 0u);  // the call rq_merge_from makes
}

// ---- rq_merge_from / rq_extract --------------------------------------------------------------------------------------------------
// (host_attr.h) a column of the same name in both indexes has the same type, else RQ_ERR_INVALID
static rq_status attr_merge_check(const rq_index *dst, const rq_index *src);

// `what` of the two indexes equal bit for bit (device arrays of `count` 32-bit words), else RQ_ERR_INVALID naming the first difference
static rq_status same_bits_check(const char *what, const float *a, const float *b, uint64_t count) {
    DevBuf<unsigned long long> first;
    RQC(first.alloc(1));
    HIPC(hipMemset(first.p, 0xFF, 8));
    if (count)
        bits_differ_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(count, 256), 4096), 256>>>(
            reinterpret_cast<const uint32_t *>(a), reinterpret_cast<const uint32_t *>(b), count, first.p);
    unsigned long long h = 0;
    HIPC(hipMemcpy(&h, first.p, 8, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    if (h != ~0ull) return fail(RQ_ERR_INVALID, std::string("the two indexes differ in ") + what + ": first at element " + std::to_string(h));
    return RQ_OK;
}

// The rows of src whose id + shift is an id of dst (a device pass over both id arrays through a bitmap of dst's ids; top_dst,
// top_src: 1 + the largest id of each, and no shifted id passes 2^32 - 1).
static rq_status count_id_collisions(const rq_index *dst, const rq_index *src, uint32_t shift, uint64_t top_dst, uint64_t top_src,
                                     uint64_t *hits) {
    *hits = 0;
    const uint64_t nbits = std::min<uint64_t>(top_dst, top_src + shift);  // ids at or past either top cannot collide
    if (nbits == 0 || !dst->n || !src->n) return RQ_OK;
    const uint64_t nwords = (nbits + 31) / 32;
    DevBuf<uint32_t> bits;
    DevBuf<unsigned long long> out;
    RQC(bits.alloc(nwords));
    RQC(out.alloc(1));
    HIPC(hipMemset(bits.p, 0, nwords * 4));
    HIPC(hipMemset(out.p, 0, 8));
    id_bitmap_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(dst->n, 256), 4096), 256>>>(dst->map_ids.p, dst->n, nbits, bits.p);
    id_hits_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(src->n, 256), 4096), 256>>>(src->map_ids.p, src->n, shift, nbits, bits.p, out.p);
    unsigned long long h = 0;
    HIPC(hipMemcpy(&h, out.p, 8, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    *hits = h;
    return RQ_OK;
}

static rq_status index_merge_from(rq_index *dst, rq_index *src, uint32_t id_mode, uint32_t id_shift, uint32_t *out_shift) {
    mutate_stats_begin(dst);
    if (!dst || !src) return fail(RQ_ERR_INVALID, "null index");
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    if (dst == src) return fail(RQ_ERR_INVALID, "an index cannot be merged into itself (dst == src)");
    if (id_mode > RQ_MERGE_IDS_APPEND) return fail(RQ_ERR_INVALID, "unknown id_mode " + std::to_string(id_mode) + " (RQ_MERGE_IDS_KEEP, _SHIFT or _APPEND)");
    RQC(mutate_refusals(dst));
    RQC(mutate_refusals(src));
    if (src->live)  // (src is never written: the caller compacts it, or extracts its live rows, first)
        return fail(RQ_ERR_UNSUPPORTED, "src has pending removals (rq_remove_lazy): rq_compact it, or rq_extract its live rows, first");
    if (dst->dim != src->dim) return fail(RQ_ERR_INVALID, "the two indexes differ in dim: " + std::to_string(dst->dim) + " and " + std::to_string(src->dim));
    if (dst->k != src->k) return fail(RQ_ERR_INVALID, "the two indexes differ in k: " + std::to_string(dst->k) + " and " + std::to_string(src->k));
    if (dst->metric.id != src->metric.id) return fail(RQ_ERR_INVALID, "the two indexes differ in metric");
    if (dst->metric.d != src->metric.d) return fail(RQ_ERR_INVALID, "the two inner-product indexes differ in the row length d");
    if (memcmp(&dst->metric.S, &src->metric.S, 4) != 0) return fail(RQ_ERR_INVALID, "the two inner-product indexes differ in sq_bound (S)");
    RQC(attr_merge_check(dst, src));
    RQC(same_bits_check("the rotation P", dst->P.p, src->P.p, (uint64_t)dst->dim * dst->dim));
    RQC(same_bits_check("the rotated centroids", dst->centroids.p, src->centroids.p, (uint64_t)dst->k * dst->dim));
    if (dst->n + src->n >= 0xFFFFFFFFull) return fail(RQ_ERR_UNSUPPORTED, "n must fit u32 ids (rabitq.rs:64-65)");
    CompactFirst pending;  // a dst with pending removals is compacted before its ids are looked at (a dead row's id is free again)
    RQC(pending.run(dst));
    uint64_t top_dst = 0, top_src = 0, hits = 0;
    RQC(scan_ids(dst, nullptr, 0, &top_dst, &hits));
    RQC(scan_ids(src, nullptr, 0, &top_src, &hits));
    uint64_t shift = id_mode == RQ_MERGE_IDS_KEEP ? 0 : (id_mode == RQ_MERGE_IDS_SHIFT ? id_shift : top_dst);
    if (src->n == 0 && shift > 0xFFFFFFFFull) shift = 0;  // (APPEND of nothing to an index that holds id 2^32 - 1)
    if (src->n && top_src - 1 + shift > 0xFFFFFFFFull) return fail(RQ_ERR_UNSUPPORTED, "the shifted ids would pass 2^32 - 1 (ids are u32)");
    if (out_shift) *out_shift = (uint32_t)shift;
    if (src->n == 0) return RQ_OK;  // as an empty add: nothing changes, the generation stays
    if (id_mode != RQ_MERGE_IDS_APPEND) {  // (appended ids start past every id of dst)
        RQC(count_id_collisions(dst, src, (uint32_t)shift, top_dst, top_src, &hits));
        if (hits) return fail(RQ_ERR_INVALID, std::to_string(hits) + " of the ids of src are already in dst");
    }
    RQC(ensure_row_keys(dst));
    const float ms_keys_dst = g_mutate_stats.ms_keys;  // (ensure_row_keys sets the phase where it derives anything: the two add up)
    g_mutate_stats.ms_keys = 0.0f;
    RQC(ensure_row_keys(src));
    g_mutate_stats.ms_keys += ms_keys_dst;
    if (!dst->row_order_ok || !src->row_order_ok) return fail(RQ_ERR_UNSUPPORTED, kOrderRefusal);
    return relayout_with(dst, src, (uint32_t)shift);
}

static rq_status index_extract(rq_index *src, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, rq_index **out) {
    mutate_stats_begin(src);
    if (out) *out = nullptr;
    if (!src || !out) return fail(RQ_ERR_INVALID, "null argument");
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    RQC(mutate_refusals(src));
    const bool every_id = !id_bits && nbits == RQ_EXTRACT_ALL_IDS;  // a copy: no bitmap is made or read
    if (!every_id) RQC(id_bits_check(id_bits, nbits));
    DevBuf<uint32_t> keep;  // requested AND live
    std::vector<uint32_t> h_out;
    RQC(position_bits(src, id_bits, nbits, bits_on_device, every_id, 0u, nullptr, keep, h_out));
    PhaseClock clk;
    std::unique_ptr<rq_index> nx;
    // (the lists keep their order whatever it is, and the ranks need no keys: the key cache travels only where src has one)
    RQC(build_layout(src, nullptr, 0u, keep.p, src->row_key_valid, h_out, nx, clk));
    nx->row_order_ok = src->row_order_ok;
    g_mutate_stats.rows_after = nx->n;
    *out = nx.release();
    return RQ_OK;
}
