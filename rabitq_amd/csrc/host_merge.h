// host_merge.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  rq_merge_from / rq_extract: two indexes over the same rotation and centroids
// merged list by list, and a sub-index copied out of one, without pass 1 -- rows, codes and factors move as they stand.
#pragma once

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

static MergeSide merge_side(const rq_index *idx, bool keys) {
    if (!idx) return MergeSide{nullptr, nullptr, nullptr, nullptr, nullptr};
    return MergeSide{reinterpret_cast<const float4 *>(idx->base.p), idx->codes.p, idx->factors.p, idx->map_ids.p, keys ? idx->row_key.p : nullptr};
}

// Sub-group width and rows in flight by row length (kernels_merge.h): dim / 4 lanes of 16 B, at least 16, at most 64.
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

// The new layout of a merge (b != nullptr) or an extraction (keep_bits, b == nullptr) beside the sources: arrays, merge, gather,
// derived state.  h_out: the new list offsets (k + 1).  Nothing of a or b is written.
static rq_status merged_layout(const rq_index *a, const rq_index *b, uint32_t shift_b, const uint32_t *keep_bits, bool keys,
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
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    st.ms_gather = clk.lap();
    // bytes the gather moves: every destination row read once and written once (raw vector, codes, factors, id, key), and the map
    st.gather_bytes = 2 * n * ((uint64_t)dim * 4 + (uint64_t)W * 8 + 16 + 4 + (keys ? 4 : 0)) + n * 4;
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
    const uint32_t k = dst->k;
    std::vector<uint32_t> h_out((size_t)k + 1, 0);
    uint64_t n = 0;
    for (uint32_t c = 0; c < k; ++c) {
        h_out[c] = (uint32_t)n;
        n += (uint64_t)dst->h_offsets[c + 1] - dst->h_offsets[c] + src->h_offsets[c + 1] - src->h_offsets[c];
    }
    h_out[k] = (uint32_t)n;
    PhaseClock clk;
    std::unique_ptr<rq_index> nx;
    RQC(merged_layout(dst, src, (uint32_t)shift, nullptr, true, h_out, nx, clk));
    return commit_layout(dst, nx, clk);
}

static rq_status index_extract(rq_index *src, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, rq_index **out) {
    mutate_stats_begin(src);
    if (out) *out = nullptr;
    if (!src || !out) return fail(RQ_ERR_INVALID, "null argument");
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    RQC(mutate_refusals(src));
    const bool every_id = !id_bits && nbits == RQ_EXTRACT_ALL_IDS;  // a copy: no bitmap is made or read
    if (!every_id && nbits > (1ull << 32)) return fail(RQ_ERR_INVALID, "nbits > 2^32 (ids are u32)");
    if (!every_id && !id_bits && nbits > 0) return fail(RQ_ERR_INVALID, "null bitmap with nbits > 0");
    const uint64_t n = src->n, k = src->k, nwords = (n + 63) / 64 * 2 + 2, in_words = every_id ? 0 : (nbits + 31) / 32;
    DevBuf<uint32_t> staged, pos_bits, counts;
    const uint32_t *d_bits = id_bits;
    if (!bits_on_device && in_words) {
        RQC(staged.upload(id_bits, in_words));
        d_bits = staged.p;
    }
    RQC(pos_bits.alloc(nwords));
    RQC(counts.alloc(std::max<uint64_t>(k, 1)));
    HIPC(hipMemset(pos_bits.p, every_id ? 0xFF : 0, nwords * 4));
    if (n && !every_id) filter_positions_kernel<<<(uint32_t)((n + 255) / 256), 256>>>(src->map_ids.p, n, d_bits, nbits, pos_bits.p, nwords);
    if (src->live) bitmap_and_kernel<<<bitmap_grid(nwords), 256>>>(pos_bits.p, src->live->pos_bits.p, nwords);  // keep = requested AND live
    if (k) filter_lists_kernel<<<(uint32_t)k, 256>>>(pos_bits.p, src->offsets.p, counts.p);  // (masks each list's first and last word)
    std::vector<uint32_t> kept(k), h_out(k + 1, 0);
    if (k) HIPC(hipMemcpy(kept.data(), counts.p, k * 4, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    staged.release();
    counts.release();
    uint64_t total = 0;
    for (uint32_t c = 0; c < k; ++c) h_out[c] = (uint32_t)total, total += kept[c];
    h_out[k] = (uint32_t)total;
    PhaseClock clk;
    std::unique_ptr<rq_index> nx;
    // (the lists keep their order whatever it is, and the ranks need no keys: the key cache travels only where src has one)
    RQC(merged_layout(src, nullptr, 0u, pos_bits.p, src->row_key_valid, h_out, nx, clk));
    nx->row_order_ok = src->row_order_ok;
    g_mutate_stats.rows_after = nx->n;
    *out = nx.release();
    return RQ_OK;
}
