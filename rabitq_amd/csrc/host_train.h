// host_train.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  The centroid trainer behind rq_train_centroids* (contract: include/rabitq_hip.h, "centroid
// training with a contract", and DESIGN.md section 4.16; kernels: kernels_train.h).  Nothing here touches rq_kmeans_device.
#pragma once

struct TrainSpec {
    uint64_t n;
    uint32_t d, k, iters, ppc;
    uint64_t seed;
    MetricSpec metric;  // RQ_METRIC_IP: d and S filled (S may still be NaN: automatic)
    RowSpec rows;
    uint32_t cols() const { return d + (metric.id == RQ_METRIC_IP ? 1u : 0u); }
    uint32_t dim() const { return ceil64(cols()); }
    uint64_t ns() const { return std::min<uint64_t>(n, (uint64_t)std::max(ppc, 1u) * k); }
};

// everything an entry refuses before it touches the device (params: as the caller passed them)
static rq_status train_spec(uint64_t n, uint32_t d, uint32_t k, const rq_train_params_t *p, const void *rows, const void *out, TrainSpec *ts) {
    if (!p || !rows || !out) return fail(RQ_ERR_INVALID, "null argument");
    if (p->struct_size != sizeof(rq_train_params_t)) return fail(RQ_ERR_INVALID, "rq_train_params_t.struct_size is not sizeof(rq_train_params_t)");
    if (p->metric != RQ_METRIC_IP) RQC(metric_entry_check(p->metric));
    RQC(row_type_check(RowSpec{p->row_type}, MetricSpec{p->metric}));
    if (d == 0 || k == 0) return fail(RQ_ERR_INVALID, "d == 0 or k == 0");
    if (n < k) return fail(RQ_ERR_INVALID, "fewer rows (" + std::to_string(n) + ") than centroids (" + std::to_string(k) + ")");
    if (n >= 0xFFFFFFFFull) return fail(RQ_ERR_UNSUPPORTED, "n must fit u32 ids (rabitq.rs:64-65)");
    *ts = TrainSpec{n, d, k, p->iters, p->points_per_centroid, p->seed, MetricSpec{p->metric}, RowSpec{p->row_type}};
    if (p->metric == RQ_METRIC_IP) {
        RQC(ip_d_check(d));
        if (p->sq_bound == p->sq_bound && !ip_bound_ok(p->sq_bound))
            return fail(RQ_ERR_INVALID, "sq_bound must be finite and >= 0, or NaN for the largest squared norm of the input");
        ts->metric = metric_ip(d, p->sq_bound);
    }
    if (ts->dim() > 4096) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 (an inner-product index: d > 4095) not supported");
    if (ts->ns() * ts->dim() > (1ull << 31)) return fail(RQ_ERR_UNSUPPORTED, "training sample too large (sample rows x dim > 2^31)");
    return RQ_OK;
}

// steps 1 and 2: ns sample rows of d_rows (n x d elements of ts.rows, device) gathered as stored, widened, transformed -> xs (ns x dim)
static rq_status train_sample(const TrainSpec &ts, const void *d_rows, DevBuf<float> &xs) {
    const uint64_t ns = ts.ns();
    const uint32_t d = ts.d, dim = ts.dim();
    DevBuf<uint8_t> typed;
    DevBuf<float> wide;
    DevBuf<uint32_t> bad;
    const uint32_t none = RQ_NO_BAD_ROW;
    RQC(bad.upload(&none, 1));
    RQC(wide.alloc(ns * d));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ceil_div(ns, 4), 1u << 20);
    if (!ts.rows.typed()) {
        train_gather_kernel<<<grid, 256>>>(static_cast<const float *>(d_rows), ts.n, d, ns, ts.seed, ts.rows.id, wide.p, bad.p);
    } else {
        RQC(typed.alloc(ns * ts.rows.row_bytes(d)));
        if (ts.rows.bytes()) train_gather_kernel<<<grid, 256>>>(static_cast<const uint8_t *>(d_rows), ts.n, d, ns, ts.seed, ts.rows.id, typed.p, bad.p);
        else train_gather_kernel<<<grid, 256>>>(static_cast<const uint16_t *>(d_rows), ts.n, d, ns, ts.seed, ts.rows.id, reinterpret_cast<uint16_t *>(typed.p), bad.p);
    }
    uint32_t h_bad = RQ_NO_BAD_ROW;
    HIPC(hipMemcpy(&h_bad, bad.p, 4, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    if (h_bad != RQ_NO_BAD_ROW)  // (before anything computes with the rows)
        return fail(RQ_ERR_INVALID, "row " + std::to_string(rq_train_sample_pos(h_bad, ts.n, ns, ts.seed)) + " (sample position " + std::to_string(h_bad) + ") holds a non-finite element");
    if (ts.rows.typed()) launch_widen(typed.p, ts.rows, ns * d, wide.p);
    if (ts.metric.id == RQ_METRIC_L2 && d == dim) {  // (an L2 row of dim floats is its own transform)
        xs.take(wide);
        return RQ_OK;
    }
    RQC(xs.alloc(ns * dim));
    RQC(transform_rows(ts.metric, dim, wide.p, ns, d, 0, xs.p, nullptr, BaseView{}, nullptr, bad.p));
    if (metric_refuses_rows(ts.metric)) RQC(bad_row_check(bad.p, " of the sample:", "sq_bound"));
    return RQ_OK;
}

// steps 3 to 5 on the transformed sample xs (ns x dim, device): k x cols centroids into d_out (device); objective (host, nullable)
static rq_status train_core(const TrainSpec &ts, const float *xs, float *d_out, double *objective, rq_train_stats_t *stats) {
    const uint64_t ns = ts.ns();
    const uint32_t k = ts.k, dim = ts.dim();
    rq_index tmp;  // only its centroid buffers are used (launch_assign_prefiltered)
    tmp.dim = dim, tmp.k = k, tmp.W = dim / 64;
    RQC(tmp.centroids.alloc((size_t)k * dim));
    RQC(tmp.cent_t.alloc((size_t)k * dim));
    DevBuf<uint32_t> label, prev, cnt, offsets, changed, ops;
    DevBuf<float> dist;
    DevBuf<unsigned long long> keys;
    DevBuf<double> partial;
    RQC(label.alloc(ns));
    RQC(prev.alloc(ns));
    RQC(dist.alloc(ns));
    RQC(keys.alloc(ns));
    RQC(cnt.alloc((size_t)k + 1));
    RQC(offsets.alloc((size_t)k + 1));
    RQC(changed.alloc(1));
    RQC(partial.alloc(k));
    HIPC(hipMemset(prev.p, 0xFF, ns * 4));
    train_start_kernel<<<ceil_div((uint64_t)k * dim, 256), 256>>>(xs, ns, k, dim, tmp.centroids.p);
    const uint64_t chunk = std::min<uint64_t>(ns, RQ_BUILD_CHUNK);
    AssignAux ax;  // the build's assignment path: matrix-core pre-filter + exact refinement (option assign_impl); refreshed per iteration
    const bool prefilter = bf16_tile_has(tmp.W) && g_assign_impl.load() != 1;
    std::vector<uint32_t> h_off((size_t)k + 1), h_cnt(k), h_ops;
    std::vector<double> h_partial(k);
    uint32_t iters_run = ts.iters, splits = 0;
    for (uint32_t t = 0; t < ts.iters; ++t) {
        transpose_kernel<<<dim3(ceil_div(dim, 32), ceil_div(k, 32)), dim3(32, 8)>>>(tmp.centroids.p, tmp.cent_t.p, k, dim);
        if (prefilter) RQC(t == 0 ? assign_aux_init(&tmp, ax, chunk) : assign_aux_refresh(&tmp, ax));
        for (uint64_t i0 = 0; i0 < ns; i0 += chunk)
            RQC(launch_assign_prefiltered(xs + i0 * dim, &tmp, ax, std::min(chunk, ns - i0), label.p + i0, dist.p + i0));
        // stop test
        HIPC(hipMemset(changed.p, 0, 4));
        train_changed_kernel<<<ceil_div(ns, 256), 256>>>(label.p, prev.p, ns, changed.p);
        uint32_t h_changed = 0;
        HIPC(hipMemcpy(&h_changed, changed.p, 4, hipMemcpyDeviceToHost));
        if (t > 0 && h_changed == 0) {
            iters_run = t;
            break;
        }
        // stable grouping of the sample by label: counts, exclusive scan, bucket, sort each bucket by label << 32 | position
        HIPC(hipMemset(cnt.p, 0, ((size_t)k + 1) * 4));
        label_hist_kernel<<<ceil_div(ns, 256), 256>>>(label.p, ns, cnt.p);
        group_scan_kernel<<<1, 1024>>>(cnt.p, k, offsets.p, 0u, nullptr, 0u);  // also zeroes cnt -> cursor
        train_scatter_kernel<<<ceil_div(ns, 256), 256>>>(label.p, ns, offsets.p, cnt.p, keys.p);
        list_sort_kernel<<<k, 1024>>>(keys.p, offsets.p);
        // centroid sums and objective partials
        train_reduce_kernel<<<ceil_div((uint64_t)k * tmp.W, 4), 256>>>(xs, dist.p, keys.p, offsets.p, k, dim, tmp.centroids.p, partial.p);
        HIPC(hipMemcpy(h_off.data(), offsets.p, ((size_t)k + 1) * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(h_partial.data(), partial.p, (size_t)k * 8, hipMemcpyDeviceToHost));
        HIPC(hipGetLastError());
        double obj = 0.0;
        for (uint32_t j = 0; j < k; ++j) obj = obj + h_partial[j], h_cnt[j] = h_off[j + 1] - h_off[j];
        if (objective) objective[t] = obj;
        // empty clusters: the plan is made on the k counts here, the columns are scaled on the device
        h_ops.clear();
        for (uint32_t e = 0; e < k; ++e) {
            if (h_cnt[e]) continue;
            uint32_t donor = 0;
            for (uint32_t j = 1; j < k; ++j)
                if (h_cnt[j] > h_cnt[donor]) donor = j;
            if (h_cnt[donor] < 2) continue;
            h_cnt[e] = h_cnt[donor] / 2, h_cnt[donor] -= h_cnt[e];
            h_ops.push_back(e), h_ops.push_back(donor);
        }
        if (!h_ops.empty()) {
            splits += (uint32_t)(h_ops.size() / 2);
            RQC(ops.ensure(h_ops.size()));
            HIPC(hipMemcpy(ops.p, h_ops.data(), h_ops.size() * 4, hipMemcpyHostToDevice));
            train_split_kernel<<<1, 256>>>(ops.p, (uint32_t)(h_ops.size() / 2), dim, tmp.centroids.p);
        }
    }
    unpad_rows_kernel<<<ceil_div((uint64_t)k * ts.cols(), 256), 256>>>(tmp.centroids.p, d_out, k, dim, ts.cols());
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    if (stats) {
        rq_train_stats_t full{};
        full.iters_run = iters_run, full.sample_rows = (uint32_t)ns, full.splits = splits;
        RQC(copy_out_sized(stats, full));
    }
    return RQ_OK;
}

static rq_status train_device(const void *d_rows, uint64_t n, uint32_t d, uint32_t k, const rq_train_params_t *params, float *d_out,
                              double *objective, rq_train_stats_t *stats) {
    TrainSpec ts;
    RQC(train_spec(n, d, k, params, d_rows, d_out, &ts));
    if (stats && stats->struct_size < 8) return fail(RQ_ERR_INVALID, "struct_size is not set (set it to sizeof(the struct) before the call)");
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    if (ts.metric.id == RQ_METRIC_IP && ts.metric.S != ts.metric.S)  // automatic: over all n rows, as rq_row_sqnorm_max_device computes it
        RQC(rq_row_sqnorm_max_device(static_cast<const float *>(d_rows), n, d, &ts.metric.S));
    DevBuf<float> xs, out;  // (the centroids land in the caller's buffer only once nothing can be refused any more)
    RQC(train_sample(ts, d_rows, xs));
    RQC(out.alloc((size_t)k * ts.cols()));
    RQC(train_core(ts, xs.p, out.p, objective, stats));
    HIPC(hipMemcpy(d_out, out.p, (size_t)k * ts.cols() * 4, hipMemcpyDeviceToDevice));
    return RQ_OK;
}

// rows in host memory: the sample positions are computed here, the ns rows gathered here and uploaded; then the same core on the
// identity sample (n = ns).  The automatic bound of an inner-product run is rq_row_sqnorm_max's, over all n rows.
static rq_status train_host(const void *rows, uint64_t n, uint32_t d, uint32_t k, const rq_train_params_t *params, float *out,
                            double *objective, rq_train_stats_t *stats) {
    TrainSpec ts;
    RQC(train_spec(n, d, k, params, rows, out, &ts));
    RQC(ensure_device());
    rq_train_params_t p = *params;
    if (ts.metric.id == RQ_METRIC_IP && p.sq_bound != p.sq_bound) RQC(rq_row_sqnorm_max(static_cast<const float *>(rows), n, d, &p.sq_bound));
    const uint64_t ns = ts.ns();
    const size_t rb = ts.rows.row_bytes(d);
    std::vector<uint8_t> sample(ns * rb);
    for (uint64_t r = 0; r < ns; ++r)
        memcpy(sample.data() + r * rb, static_cast<const uint8_t *>(rows) + rq_train_sample_pos(r, n, ns, ts.seed) * rb, rb);
    DevBuf<uint8_t> ds;
    DevBuf<float> dout;
    RQC(ds.upload(sample.data(), sample.size()));
    RQC(dout.alloc((size_t)k * ts.cols()));
    RQC(train_device(ds.p, ns, d, k, &p, dout.p, objective, stats));
    HIPC(hipMemcpy(out, dout.p, (size_t)k * ts.cols() * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}
