// rabitq_hip.hip -- host side of librabitq_hip.so: index state, build / query orchestration,
// persistence and the extern "C" boundary declared in include/rabitq_hip.h.
//
// There is NO CPU fallback anywhere in this file: every arithmetic step of the path runs in the
// gfx950 kernels of kernels_query.h / kernels_build.h, and every entry point fails with
// RQ_ERR_NO_DEVICE / RQ_ERR_HIP when no device is usable.
#include "../../include/rabitq_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <charconv>
#include <chrono>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include <sys/stat.h>
#include <dlfcn.h>
#include <queue>
#include <map>

#include "common.h"
#include "kernels_build.h"
#include "kernels_query.h"
#include "kernels_range.h"
#include "kernels_small.h"
#include "kernels_train.h"
#include "kernels_relayout.h"
#include "kernels_directory.h"
#include "kernels_attr.h"
#include "kernels_group.h"
#include "kernels_diverse.h"

#include "kernel_shapes.h"
#include "host_state.h"
#include "host_options.h"
#include "host_launch.h"
#include "host_metric.h"
#include "host_plan.h"
#include "host_query.h"
#include "host_call.h"
#include "host_range.h"
#include "host_build.h"
#include "host_relayout.h"
#include "host_mutate.h"
#include "host_exact.h"
#include "host_exact_range.h"
#include "host_train.h"
#include "host_directory.h"
#include "host_attr.h"
#include "host_group.h"
#include "host_diverse.h"

// ------------------------------------------------------------------------------------------------
// extern "C"
// ------------------------------------------------------------------------------------------------
extern "C" {

const char *rq_version(void) { return "rabitq_hip 0.7.0 (gfx950, abi 4)"; }
uint32_t rq_abi_version(void) { return RQ_ABI_VERSION; }
const char *rq_last_error(void) { return g_err.c_str(); }

rq_status rq_init(int device) {
    RQC(ensure_device());
    HIPC(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPC(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(RQ_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is gfx950-only");
    return RQ_OK;
}

rq_status rq_kmeans_device(const float *d_base, uint64_t n, uint32_t d, uint32_t k, uint32_t iters,
                           uint32_t points_per_centroid, uint64_t seed, float *d_centroids_out) {
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    if (!d_base || !d_centroids_out || n == 0 || d == 0 || k == 0) return fail(RQ_ERR_INVALID, "bad k-means arguments");
    const uint32_t dim = (d + 63) / 64 * 64;
    if (dim > 4096) return fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
    const uint64_t ns = std::max<uint64_t>(k, std::min<uint64_t>(n, (uint64_t)std::max(points_per_centroid, 1u) * k));
    if (ns * dim > (1ull << 31)) return fail(RQ_ERR_UNSUPPORTED, "k-means sample too large");
    rq_index tmp;  // only its centroid buffers are used (launch_assign)
    tmp.dim = dim, tmp.k = k, tmp.W = dim / 64;
    DevBuf<float> xs, sums;
    DevBuf<uint32_t> label, counts;
    DevBuf<float> dist;
    RQC(xs.alloc(ns * dim));
    RQC(tmp.centroids.alloc((size_t)k * dim));
    RQC(tmp.cent_t.alloc((size_t)k * dim));
    RQC(sums.alloc((size_t)k * dim));
    RQC(label.alloc(ns));
    RQC(dist.alloc(ns));
    RQC(counts.alloc(k));
    kmeans_sample_kernel<<<ceil_div(ns * dim, 256), 256>>>(d_base, n, d, dim, seed, ns, xs.p);
    HIPC(hipMemcpy(tmp.centroids.p, xs.p, (size_t)k * dim * 4, hipMemcpyDeviceToDevice));  // init: first k sample rows
    for (uint32_t it = 0; it < iters; ++it) {
        transpose_kernel<<<dim3(ceil_div(dim, 32), ceil_div(k, 32)), dim3(32, 8)>>>(tmp.centroids.p, tmp.cent_t.p, k, dim);
        for (uint64_t i0 = 0; i0 < ns; i0 += (1ull << 20)) {
            const uint64_t m = std::min<uint64_t>(1ull << 20, ns - i0);
            launch_assign(xs.p + i0 * dim, &tmp, m, label.p + i0, dist.p + i0, nullptr);
        }
        HIPC(hipMemset(sums.p, 0, (size_t)k * dim * 4));
        HIPC(hipMemset(counts.p, 0, (size_t)k * 4));
        kmeans_accumulate_kernel<<<ceil_div(ns * dim, 256), 256>>>(xs.p, label.p, ns, dim, sums.p, counts.p);
        kmeans_update_kernel<<<ceil_div((uint64_t)k * dim, 256), 256>>>(sums.p, counts.p, xs.p, ns, k, dim,
                                                                        seed + it + 1, tmp.centroids.p);
    }
    unpad_rows_kernel<<<ceil_div((uint64_t)k * d, 256), 256>>>(tmp.centroids.p, d_centroids_out, k, dim, d);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    return RQ_OK;
}

// ---- centroid training with a contract (host_train.h) ----
rq_status rq_train_centroids_device(const void *d_rows, uint64_t n, uint32_t d, uint32_t k, const rq_train_params_t *params,
                                    float *d_centroids_out, double *objective_out, rq_train_stats_t *stats_out) {
    return train_device(d_rows, n, d, k, params, d_centroids_out, objective_out, stats_out);
}
rq_status rq_train_centroids(const void *rows, uint64_t n, uint32_t d, uint32_t k, const rq_train_params_t *params, float *centroids_out,
                             double *objective_out, rq_train_stats_t *stats_out) {
    return train_host(rows, n, d, k, params, centroids_out, objective_out, stats_out);
}

// ---- the row transforms on their own (the builds, rq_add and every query pass run the same kernels) ----
static rq_status normalize_d_check(uint32_t d) {
    if (d == 0) return fail(RQ_ERR_INVALID, "d == 0");
    return d <= 4096 ? RQ_OK : fail(RQ_ERR_UNSUPPORTED, "dim > 4096 not supported");
}
rq_status rq_normalize_device(const float *d_x, uint64_t n, uint32_t d, float *d_out) {
    RQC(ensure_device());
    if (n && (!d_x || !d_out)) return fail(RQ_ERR_INVALID, "null argument");
    RQC(normalize_d_check(d));
    return transform_all_rows(MetricSpec{RQ_METRIC_COSINE}, ceil64(d), d_x, n, d, nullptr, nullptr, d_out);
}
rq_status rq_normalize(const float *x, uint64_t n, uint32_t d, float *out) {
    return with_staged_rows(x, n, d, out, ceil64(d), normalize_d_check(d), [&](const float *dx, float *dout) { return rq_normalize_device(dx, n, d, dout); });
}

// ---- inner-product metric: A(x; S), the largest s and the two conversions ----
rq_status rq_ip_params(const rq_index *idx, uint32_t *d, float *sq_bound) {
    if (!idx || !d || !sq_bound) return fail(RQ_ERR_INVALID, "null argument");
    if (idx->metric.id != RQ_METRIC_IP) return fail(RQ_ERR_INVALID, "not an inner-product index");
    *d = idx->metric.d, *sq_bound = idx->metric.S;
    return RQ_OK;
}
rq_status rq_row_sqnorm_max_device(const float *d_x, uint64_t n, uint32_t d, float *out_max) {
    RQC(ensure_device());
    if ((n && !d_x) || !out_max) return fail(RQ_ERR_INVALID, "null argument");
    if (d == 0 || d > 4096) return fail(d ? RQ_ERR_UNSUPPORTED : RQ_ERR_INVALID, "d must be in [1, 4096]");
    uint32_t bad = RQ_NO_BAD_ROW;
    RQC(row_sqnorms(d_x, n, d, ceil64(d), __builtin_inff(), nullptr, out_max, &bad));
    return bad_row_refusal(bad, ":", nullptr);
}
rq_status rq_row_sqnorm_max(const float *x, uint64_t n, uint32_t d, float *out_max) {
    return with_staged_rows(x, n, d, nullptr, 0, RQ_OK, [&](const float *dx, float *) { return rq_row_sqnorm_max_device(dx, n, d, out_max); });
}
rq_status rq_augment_device(const float *d_x, uint64_t n, uint32_t d, float sq_bound, float *d_out) {
    RQC(ensure_device());
    if (n && (!d_x || !d_out)) return fail(RQ_ERR_INVALID, "null argument");
    RQC(ip_d_check(d));
    DevBuf<float> s;
    DevBuf<uint32_t> bad;
    RQC(s.alloc(n));
    RQC(bad.alloc(1));
    RQC(ip_resolve_bound(d_x, n, d, &sq_bound, s.p));  // (every row is valid from here on)
    return transform_all_rows(metric_ip(d, sq_bound), ceil64(d + 1), d_x, n, d, s.p, bad.p, d_out);
}
rq_status rq_augment(const float *x, uint64_t n, uint32_t d, float sq_bound, float *out) {
    return with_staged_rows(x, n, d, out, ceil64(d + 1), ip_d_check(d), [&](const float *dx, float *dout) { return rq_augment_device(dx, n, d, sq_bound, dout); });
}
// s_q of the queries of an inner-product index (row_sqnorm_kernel over Q(q)), then one of the two conversions
static rq_status ip_convert(const rq_index *idx, const float *d_q, uint32_t nq, uint32_t len, const float *d_in, uint32_t topk,
                            const uint32_t *d_n, float *d_out, bool radius) {
    RQC(ensure_device());
    if (!idx || (nq && (!d_q || !d_in || !d_out))) return fail(RQ_ERR_INVALID, "null argument");
    if (idx->metric.id != RQ_METRIC_IP) return fail(RQ_ERR_INVALID, "not an inner-product index");
    RQC(raw_len_check(idx, "query", len));
    if (!radius && topk == 0) return fail(RQ_ERR_INVALID, "topk == 0");
    if (nq == 0) return RQ_OK;
    DevBuf<float> sq;
    DevBuf<uint32_t> stat;
    RQC(sq.alloc(nq));
    RQC(stat.upload(RQ_SQNORM_STAT_INIT, 3));
    launch_row_sqnorm(d_q, nq, len, idx->dim, __builtin_inff(), 0, sq.p, stat.p, nullptr);
    if (radius) ip_radius_kernel<<<ceil_div(nq, 256), 256>>>(d_in, sq.p, idx->metric.S, nq, d_out);
    else ip_from_dist_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div((uint64_t)nq * topk, 256), 1u << 20), 256>>>(d_in, sq.p, d_n, idx->metric.S, nq, topk, d_out);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    return RQ_OK;
}
static rq_status ip_convert_host(const rq_index *idx, const float *q, uint32_t nq, uint32_t len, const float *in, uint32_t topk,
                                 const uint32_t *n, float *out, bool radius) {
    RQC(ensure_device());
    if (!idx || (nq && (!q || !in || !out))) return fail(RQ_ERR_INVALID, "null argument");
    const uint64_t cells = radius ? nq : (uint64_t)nq * topk;
    DevBuf<float> dq, din, dout;
    DevBuf<uint32_t> dn;
    RQC(dq.upload(q, (uint64_t)nq * len));
    RQC(din.upload(in, cells));
    RQC(dout.alloc(cells));
    if (n) RQC(dn.upload(n, nq));
    RQC(ip_convert(idx, dq.p, nq, len, din.p, topk, n ? dn.p : nullptr, dout.p, radius));
    if (cells) HIPC(hipMemcpy(out, dout.p, cells * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}
rq_status rq_ip_from_dist_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len, const float *d_dist,
                                 uint32_t topk, const uint32_t *d_n, float *d_out_ip) {
    return ip_convert(idx, d_queries, nq, len, d_dist, topk, d_n, d_out_ip, false);
}
rq_status rq_ip_from_dist(const rq_index *idx, const float *queries, uint32_t nq, uint32_t len, const float *dist, uint32_t topk,
                          const uint32_t *n, float *out_ip) {
    return ip_convert_host(idx, queries, nq, len, dist, topk, n, out_ip, false);
}
rq_status rq_ip_radius_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len, const float *d_min_ip,
                              float *d_out_radius) {
    return ip_convert(idx, d_queries, nq, len, d_min_ip, 1, nullptr, d_out_radius, true);
}
rq_status rq_ip_radius(const rq_index *idx, const float *queries, uint32_t nq, uint32_t len, const float *min_ip, float *out_radius) {
    return ip_convert_host(idx, queries, nq, len, min_ip, 1, nullptr, out_radius, true);
}

// ---- the builds: every entry forwards to build_device / build_host / build_from_path / builder_create / from_arrays with its MetricSpec ----
// (the *_metric entries take no d / S: they refuse RQ_METRIC_IP, and any id they do not know, before anything else)
rq_status rq_build_device(const float *d_base, uint64_t n, uint32_t d, const float *d_centroids, uint32_t k,
                          const float *orthogonal_host, uint64_t seed, rq_index **out) {
    return build_device(RowsIn::plain(d_base), n, d, d_centroids, k, d, orthogonal_host, seed, MetricSpec{}, out);
}
rq_status rq_build_device_metric(const float *d_base, uint64_t n, uint32_t d, const float *d_centroids, uint32_t k,
                                 const float *orthogonal_host, uint64_t seed, uint32_t metric, rq_index **out) {
    RQC(metric_entry_check(metric));
    return build_device(RowsIn::plain(d_base), n, d, d_centroids, k, d, orthogonal_host, seed, MetricSpec{metric}, out);
}
rq_status rq_build_device_ip(const float *d_base, uint64_t n, uint32_t d, const float *d_centroids, uint32_t k,
                             const float *orthogonal_host, uint64_t seed, uint32_t centroid_cols, float sq_bound, rq_index **out) {
    return build_device(RowsIn::plain(d_base), n, d, d_centroids, k, centroid_cols, orthogonal_host, seed, metric_ip(d, sq_bound), out);
}

rq_status rq_builder_create(uint64_t n, uint32_t d, const float *d_centroids, uint32_t k, const float *orthogonal_host,
                            uint64_t seed, uint64_t max_device_base_bytes, rq_builder **out) {
    return builder_create(n, d, d_centroids, k, orthogonal_host, seed, max_device_base_bytes, MetricSpec{}, RowSpec{}, d, out);
}
rq_status rq_builder_create_metric(uint64_t n, uint32_t d, const float *d_centroids, uint32_t k, const float *orthogonal_host,
                                   uint64_t seed, uint64_t max_device_base_bytes, uint32_t metric, rq_builder **out) {
    RQC(metric_entry_check(metric));
    return builder_create(n, d, d_centroids, k, orthogonal_host, seed, max_device_base_bytes, MetricSpec{metric}, RowSpec{}, d, out);
}
rq_status rq_builder_create_ip(uint64_t n, uint32_t d, const float *d_centroids, uint32_t k, const float *orthogonal_host,
                               uint64_t seed, uint64_t max_device_base_bytes, uint32_t centroid_cols, float sq_bound,
                               rq_builder **out) {
    return builder_create(n, d, d_centroids, k, orthogonal_host, seed, max_device_base_bytes, metric_ip(d, sq_bound), RowSpec{}, centroid_cols, out);
}
// ---- typed rows: the twins of the builds above that take a row type ----
rq_status rq_build_device_rows(const void *d_base, uint64_t n, uint32_t d, const float *d_centroids, uint32_t k,
                               const float *orthogonal_host, uint64_t seed, uint32_t metric, uint32_t row_type, rq_index **out) {
    if (out) *out = nullptr;
    RQC(row_type_check(RowSpec{row_type}, MetricSpec{metric}));
    RQC(metric_entry_check(metric));
    return build_device(RowsIn::of(d_base, RowSpec{row_type}), n, d, d_centroids, k, d, orthogonal_host, seed, MetricSpec{metric}, out);
}
rq_status rq_build_rows(const void *base, uint64_t n, uint32_t d, const float *centroids, uint32_t k, const float *orthogonal,
                        uint64_t seed, uint32_t metric, uint32_t row_type, rq_index **out) {
    if (out) *out = nullptr;
    RQC(row_type_check(RowSpec{row_type}, MetricSpec{metric}));
    RQC(metric_entry_check(metric));
    return build_host(RowsIn::of(base, RowSpec{row_type}), n, d, centroids, k, d, orthogonal, seed, MetricSpec{metric}, out);
}
rq_status rq_builder_create_rows(uint64_t n, uint32_t d, const float *d_centroids, uint32_t k, const float *orthogonal_host,
                                 uint64_t seed, uint64_t max_device_base_bytes, uint32_t metric, uint32_t row_type, rq_builder **out) {
    if (out) *out = nullptr;
    RQC(row_type_check(RowSpec{row_type}, MetricSpec{metric}));
    RQC(metric_entry_check(metric));
    return builder_create(n, d, d_centroids, k, orthogonal_host, seed, max_device_base_bytes, MetricSpec{metric}, RowSpec{row_type}, d, out);
}
rq_status rq_builder_assign_chunk_rows(rq_builder *b, const void *d_rows, uint64_t i0, uint64_t m) { return builder_assign(b, RowsIn::chunk_rows(b, d_rows), i0, m); }
rq_status rq_builder_place_chunk_rows(rq_builder *b, const void *d_rows, uint64_t i0, uint64_t m) { return builder_place(b, RowsIn::chunk_rows(b, d_rows), i0, m); }
rq_status rq_from_arrays_rows(uint32_t dim, uint64_t n, uint32_t k, const void *base, const float *orthogonal, const float *centroids,
                              const uint32_t *offsets, const uint32_t *map_ids, const uint64_t *codes, const rq_factor_t *factors,
                              uint32_t metric, uint32_t row_type, rq_index **out) {
    if (out) *out = nullptr;
    RQC(row_type_check(RowSpec{row_type}, MetricSpec{metric}));
    RQC(metric_entry_check(metric));
    return from_arrays(dim, n, k, RowsIn::of(base, RowSpec{row_type}), orthogonal, centroids, offsets, map_ids, codes, factors, MetricSpec{metric}, out);
}
rq_status rq_row_type(const rq_index *idx, uint32_t *out) {
    if (!idx || !out) return fail(RQ_ERR_INVALID, "null argument");
    *out = idx->rows.id;
    return RQ_OK;
}
// the row types rq_widen* take: the typed ones
static rq_status widen_type_check(RowSpec rows) {
    if (rows.known() && rows.typed()) return RQ_OK;
    return fail(RQ_ERR_INVALID, "row_type must be RQ_ROWS_F16, RQ_ROWS_BF16, RQ_ROWS_U8 or RQ_ROWS_I8");
}
rq_status rq_widen_device(const void *d_x, uint32_t row_type, uint64_t count, float *d_out) {
    RQC(ensure_device());
    RQC(widen_type_check(RowSpec{row_type}));
    if (count && (!d_x || !d_out)) return fail(RQ_ERR_INVALID, "null argument");
    launch_widen(d_x, RowSpec{row_type}, count, d_out);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    return RQ_OK;
}
rq_status rq_widen(const void *x, uint32_t row_type, uint64_t count, float *out) {
    RQC(ensure_device());
    RQC(widen_type_check(RowSpec{row_type}));
    if (count && (!x || !out)) return fail(RQ_ERR_INVALID, "null argument");
    DevBuf<uint8_t> dx;
    DevBuf<float> dout;
    RQC(dx.upload(static_cast<const uint8_t *>(x), count * RowSpec{row_type}.elem_bytes()));
    RQC(dout.alloc(count));
    RQC(rq_widen_device(dx.p, row_type, count, dout.p));
    if (count) HIPC(hipMemcpy(out, dout.p, count * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

rq_status rq_builder_assign_chunk(rq_builder *b, const float *d_rows, uint64_t i0, uint64_t m) { return builder_assign(b, RowsIn::plain(d_rows), i0, m); }
rq_status rq_builder_order(rq_builder *b) { return builder_order(b); }
rq_status rq_builder_place_chunk(rq_builder *b, const float *d_rows, uint64_t i0, uint64_t m) { return builder_place(b, RowsIn::plain(d_rows), i0, m); }
rq_status rq_builder_finish(rq_builder *b, rq_index **out) { return builder_finish(b, out); }
void rq_builder_free(rq_builder *b) { delete b; }
rq_status rq_builder_stats(const rq_builder *b, rq_build_stats_t *out) {
    if (!b || !out) return fail(RQ_ERR_INVALID, "null argument");
    return copy_out_sized(out, b->stats);
}

rq_status rq_build(const float *base, uint64_t n, uint32_t d, const float *centroids, uint32_t k,
                   const float *orthogonal, uint64_t seed, rq_index **out) {
    return build_host(RowsIn::plain(base), n, d, centroids, k, d, orthogonal, seed, MetricSpec{}, out);
}
rq_status rq_build_metric(const float *base, uint64_t n, uint32_t d, const float *centroids, uint32_t k,
                          const float *orthogonal, uint64_t seed, uint32_t metric, rq_index **out) {
    RQC(metric_entry_check(metric));
    return build_host(RowsIn::plain(base), n, d, centroids, k, d, orthogonal, seed, MetricSpec{metric}, out);
}
rq_status rq_build_ip(const float *base, uint64_t n, uint32_t d, const float *centroids, uint32_t k, const float *orthogonal,
                      uint64_t seed, uint32_t centroid_cols, float sq_bound, rq_index **out) {
    return build_host(RowsIn::plain(base), n, d, centroids, k, centroid_cols, orthogonal, seed, metric_ip(d, sq_bound), out);
}

rq_status rq_build_from_path(const char *base_fvecs, const char *centroid_fvecs, const float *orthogonal,
                             uint64_t seed, rq_index **out) {
    return build_from_path(base_fvecs, centroid_fvecs, orthogonal, seed, MetricSpec{}, out);
}
rq_status rq_build_from_path_metric(const char *base_fvecs, const char *centroid_fvecs, const float *orthogonal,
                                    uint64_t seed, uint32_t metric, rq_index **out) {
    RQC(metric_entry_check(metric));
    return build_from_path(base_fvecs, centroid_fvecs, orthogonal, seed, MetricSpec{metric}, out);
}
rq_status rq_build_from_path_ip(const char *base_fvecs, const char *centroid_fvecs, const float *orthogonal, uint64_t seed,
                                float sq_bound, rq_index **out) {
    return build_from_path(base_fvecs, centroid_fvecs, orthogonal, seed, metric_ip(0, sq_bound), out);  // (d: the base file's record length)
}

rq_status rq_from_arrays(uint32_t dim, uint64_t n, uint32_t k, const float *base, const float *orthogonal,
                         const float *centroids, const uint32_t *offsets, const uint32_t *map_ids,
                         const uint64_t *codes, const rq_factor_t *factors, rq_index **out) {
    return from_arrays(dim, n, k, RowsIn::plain(base), orthogonal, centroids, offsets, map_ids, codes, factors, MetricSpec{}, out);
}
rq_status rq_from_arrays_metric(uint32_t dim, uint64_t n, uint32_t k, const float *base, const float *orthogonal,
                                const float *centroids, const uint32_t *offsets, const uint32_t *map_ids,
                                const uint64_t *codes, const rq_factor_t *factors, uint32_t metric, rq_index **out) {
    RQC(metric_entry_check(metric));
    return from_arrays(dim, n, k, RowsIn::plain(base), orthogonal, centroids, offsets, map_ids, codes, factors, MetricSpec{metric}, out);
}
rq_status rq_from_arrays_ip(uint32_t dim, uint64_t n, uint32_t k, const float *base, const float *orthogonal,
                            const float *centroids, const uint32_t *offsets, const uint32_t *map_ids,
                            const uint64_t *codes, const rq_factor_t *factors, uint32_t d, float sq_bound, rq_index **out) {
    return from_arrays(dim, n, k, RowsIn::plain(base), orthogonal, centroids, offsets, map_ids, codes, factors, metric_ip(d, sq_bound), out);
}

// rabitq.rs:84-125
rq_status rq_load_dir(const char *dir, rq_index **out) {
    if (!dir || !out) return fail(RQ_ERR_INVALID, "null argument");
    const std::string d(dir);
    VecsFile ortho, cent, oi, fac, bin, base;
    RQC(read_vecs_file(d + "/orthogonal.fvecs", 4, ortho));
    RQC(read_vecs_file(d + "/centroids.fvecs", 4, cent));
    RQC(read_vecs_file(d + "/offsets_ids.ivecs", 4, oi));
    RQC(read_vecs_file(d + "/factors.fvecs", 4, fac));
    RQC(read_vecs_file(d + "/x_binary_vec.u64vecs", 8, bin));
    RQC(read_vecs_file(d + "/base.fvecs", 4, base));
    MetricSpec metric;  // the sixth file of a cosine or inner-product index's dump
    if (FILE *mf = fopen((d + "/metric").c_str(), "rb")) {
        char buf[32] = {0};
        const size_t got = fread(buf, 1, sizeof buf - 1, mf);
        fclose(mf);
        if (!metric_from_file_text(std::string(buf, got), &metric)) return fail(RQ_ERR_IO, "metric: unknown or malformed content in " + d + "/metric");
    }
    RowSpec rows;  // the `rows` file of a half-precision or byte-row index's dump
    if (FILE *rf = fopen((d + "/rows").c_str(), "rb")) {
        char buf[16] = {0};
        const size_t got = fread(buf, 1, sizeof buf - 1, rf);
        fclose(rf);
        const std::string text(buf, got);
        if (text.empty() || text.back() != '\n' || !RowSpec::from_tag(text.data(), text.size() - 1, &rows))
            return fail(RQ_ERR_IO, "rows: unknown content in " + d + "/rows");
    }
    const uint32_t dim = (uint32_t)ortho.lens.size();  // :108 dim = orthogonal.nrows()
    if (dim == 0 || dim % 64 != 0) return fail(RQ_ERR_DIM_MISMATCH, "orthogonal.fvecs: dim % 64 != 0 (rabitq.rs:109)");
    if (metric.id == RQ_METRIC_IP && !(ip_d_ok(metric.d, dim) && ip_bound_ok(metric.S)))
        return fail(RQ_ERR_IO, "metric: no valid d and bound of an inner-product index of this dim in " + d + "/metric");
    if (cent.lens.size() != dim || oi.lens.size() != 2) return fail(RQ_ERR_IO, "malformed index directory");
    const uint32_t k = cent.lens[0];
    // every record length is checked before anything is indexed by it (the reference's matrix_from_fvecs panics on
    // ragged input, src/utils.rs:44-49)
    for (uint32_t l : ortho.lens)
        if (l != dim) return fail(RQ_ERR_IO, "orthogonal.fvecs is not dim x dim");
    for (uint32_t l : cent.lens)
        if (l != k) return fail(RQ_ERR_IO, "centroids.fvecs is not dim records of k values");
    for (uint32_t l : base.lens)
        if (l != dim) return fail(RQ_ERR_IO, "base.fvecs record length != dim");
    // centroids.fvecs holds the dim x k matrix row-wise: un-transpose to k x dim
    std::vector<float> c((size_t)k * dim);
    const float *ct = reinterpret_cast<const float *>(cent.data.data());
    for (uint32_t r = 0; r < dim; ++r)
        for (uint32_t j = 0; j < k; ++j) c[(size_t)j * dim + r] = ct[(size_t)r * k + j];
    const uint32_t *oip = reinterpret_cast<const uint32_t *>(oi.data.data());
    const uint32_t first = oi.lens.front(), last = oi.lens.back();
    size_t total = 0;
    for (uint32_t l : oi.lens) total += l;
    if (first != k + 1) return fail(RQ_ERR_IO, "offsets record length != k + 1");
    const uint64_t n = last;
    if (fac.data.size() != n * 16 || bin.data.size() != n * (dim / 64) * 8 || base.data.size() != n * dim * 4 ||
        base.lens.size() != n)
        return fail(RQ_ERR_IO, "index arrays disagree on n");
    if (oip[k] != n) return fail(RQ_ERR_IO, "offsets[k] != number of vectors");
    for (uint32_t j = 0; j < k; ++j)
        if (oip[j] > oip[j + 1]) return fail(RQ_ERR_IO, "offsets are not non-decreasing");
    if (!rows.allowed_with(metric.id))
        return fail(RQ_ERR_IO, "rows: an index of this metric has no rows of the announced type (" + d + ")");
    std::vector<uint8_t> typed;  // typed rows: every value of base.fvecs must be one of the type's
    if (rows.typed()) RQC(narrow_exact(reinterpret_cast<const float *>(base.data.data()), n * dim, rows, typed, d + "/base.fvecs"));
    RQC(from_arrays(dim, n, k, RowsIn::of(rows.typed() ? typed.data() : base.data.data(), rows),
                    reinterpret_cast<const float *>(ortho.data.data()), c.data(), oip, oip + (total - last),
                    reinterpret_cast<const uint64_t *>(bin.data.data()),
                    reinterpret_cast<const rq_factor_t *>(fac.data.data()), metric, out));
    const rq_status as = attr_load_dir(d, *out);  // the attribute columns of the dump, where it has an `attrs` file
    if (as != RQ_OK) {
        delete *out;
        *out = nullptr;
    }
    return as;
}

rq_status rq_get_array(const rq_index *idx, int which, void *dst, uint64_t dst_bytes);

// rabitq.rs:128-156
rq_status rq_dump_dir(const rq_index *idx, const char *dir) {
    if (!idx || !dir) return fail(RQ_ERR_INVALID, "null argument");
    if (idx->live) return fail(RQ_ERR_UNSUPPORTED, kPendingRefusal);
    mkdir(dir, 0777);
    const std::string d(dir);
    const uint32_t dim = idx->dim, k = idx->k;
    const uint64_t n = idx->n;
    if (4 * n > 0xFFFFFFFFull || n * (dim / 64) > 0xFFFFFFFFull)
        return fail(RQ_ERR_UNSUPPORTED, "single-record files need 4n and n*dim/64 to fit the u32 header (rabitq.rs:141-155)");
    auto open = [&](const char *name, FILE **f) -> rq_status {
        *f = fopen((d + "/" + name).c_str(), "wb");
        return *f ? RQ_OK : fail(RQ_ERR_IO, "cannot create " + d + "/" + name);
    };
    FILE *f;
    {  // base.fvecs: n records of dim (cluster order), streamed in chunks
        RQC(open("base.fvecs", &f));
        const uint64_t chunk = std::max<uint64_t>(1, (256ull << 20) / (dim * 4));
        std::vector<float> buf(std::min<uint64_t>(chunk, std::max<uint64_t>(n, 1)) * dim);
        for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
            uint64_t m = std::min(chunk, n - i0);
            if (copy_base_rows(idx, i0, m, buf.data(), false) != RQ_OK) {
                fclose(f);
                return RQ_ERR_HIP;
            }
            for (uint64_t i = 0; i < m; ++i) {
                rq_status s = write_record(f, buf.data() + i * dim, dim, 4, "base.fvecs");
                if (s != RQ_OK) {
                    fclose(f);
                    return s;
                }
            }
        }
        fclose(f);
    }
    std::vector<float> P((size_t)dim * dim), C((size_t)k * dim), row(std::max<uint32_t>(k, 1));
    std::vector<uint32_t> off((size_t)k + 1), ids(n);
    std::vector<float> fac(n * 4);
    std::vector<uint64_t> codes(n * (dim / 64));
    RQC(rq_get_array(idx, RQ_ARR_ORTHOGONAL, P.data(), P.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_CENTROIDS, C.data(), C.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_OFFSETS, off.data(), off.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_MAP_IDS, ids.data(), ids.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_FACTORS, fac.data(), fac.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_CODES, codes.data(), codes.size() * 8));
    rq_status s = RQ_OK;
    RQC(open("orthogonal.fvecs", &f));
    for (uint32_t r = 0; r < dim && s == RQ_OK; ++r) s = write_record(f, P.data() + (size_t)r * dim, dim, 4, "orthogonal.fvecs");
    fclose(f);
    RQC(s);
    RQC(open("centroids.fvecs", &f));  // dim records of k values (rotated, transposed)
    for (uint32_t r = 0; r < dim && s == RQ_OK; ++r) {
        for (uint32_t j = 0; j < k; ++j) row[j] = C[(size_t)j * dim + r];
        s = write_record(f, row.data(), k, 4, "centroids.fvecs");
    }
    fclose(f);
    RQC(s);
    RQC(open("offsets_ids.ivecs", &f));
    s = write_record(f, off.data(), k + 1, 4, "offsets_ids.ivecs");
    if (s == RQ_OK) s = write_record(f, ids.data(), (uint32_t)n, 4, "offsets_ids.ivecs");
    fclose(f);
    RQC(s);
    RQC(open("factors.fvecs", &f));
    s = write_record(f, fac.data(), (uint32_t)(4 * n), 4, "factors.fvecs");
    fclose(f);
    RQC(s);
    RQC(open("x_binary_vec.u64vecs", &f));
    s = write_record(f, codes.data(), (uint32_t)(n * (dim / 64)), 8, "x_binary_vec.u64vecs");
    fclose(f);
    RQC(s);
    const std::string tag = metric_file_text(idx->metric);
    if (!tag.empty()) {  // (an L2 dump stays the crate's five files)
        RQC(open("metric", &f));
        const bool ok = fputs(tag.c_str(), f) >= 0;
        if (fclose(f) != 0 || !ok) return fail(RQ_ERR_IO, "write error on " + d + "/metric");
    } else {
        remove((d + "/metric").c_str());  // (a directory that held a cosine dump before)
    }
    if (idx->rows.typed()) {  // base.fvecs above holds W(rows): the reference loads the directory and answers identically
        RQC(open("rows", &f));
        const bool ok = fputs(idx->rows.tag(), f) >= 0 && fputc('\n', f) >= 0;
        if (fclose(f) != 0 || !ok) return fail(RQ_ERR_IO, "write error on " + d + "/rows");
    } else {
        remove((d + "/rows").c_str());
    }
    return attr_dump_dir(idx, d);  // (an index without columns: nothing is written)
}

// ---- JSON persistence: load_from_json / dump_to_json, src/rabitq.rs:72-81 ------------------------------------
// serde_json of `RaBitQ` (src/rabitq.rs:56-68): {"dim", "base": Mat, "orthogonal": Mat, "centroids": Mat, "rand_bias",
// "offsets", "map_ids", "x_binary_vec", "factors": [{factor_ip, factor_ppc, error_bound, center_distance_square}]}.
// A faer 0.19 `Mat` serialises as {"nrows", "ncols", "data": row-major sequence}; base is dim x n (one vector per
// column, :188), centroids dim x k (:189).  faer's source is not in the reference tree, so the Mat layout is restated
// from its published serde impl (parity unpinned, like every faer call site: DESIGN.md section 2).  Numbers are
// written in shortest round-trip form; f32 non-finite values become null as serde_json writes them (and, as in
// serde_json, a null does not load).  rand_bias is not used by the AVX2 path (src/simd.rs:177): 0.5 per dimension.

rq_status rq_dump_json(const rq_index *idx, const char *path) {
    if (!idx || !path) return fail(RQ_ERR_INVALID, "null argument");
    if (idx->live) return fail(RQ_ERR_UNSUPPORTED, kPendingRefusal);
    if (!idx->attrs.empty()) return fail(RQ_ERR_UNSUPPORTED, "the JSON image has no attribute columns (rq_dump_dir writes them)");
    const uint64_t n = idx->n, dim = idx->dim, k = idx->k;
    std::vector<float> base(n * dim), P(dim * dim), C(k * dim), fac(n * 4);
    std::vector<uint32_t> off(k + 1), ids(n);
    std::vector<uint64_t> codes(n * idx->W);
    RQC(rq_get_array(idx, RQ_ARR_BASE, base.data(), base.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_ORTHOGONAL, P.data(), P.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_CENTROIDS, C.data(), C.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_OFFSETS, off.data(), off.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_MAP_IDS, ids.data(), ids.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_FACTORS, fac.data(), fac.size() * 4));
    RQC(rq_get_array(idx, RQ_ARR_CODES, codes.data(), codes.size() * 8));
    FILE *f = fopen(path, "wb");
    if (!f) return fail(RQ_ERR_IO, std::string("cannot create ") + path);
    JsonOut o{f};
    o.raw("{\"dim\":"), o.u64(dim);
    o.raw(",\"base\":"), o.mat(base.data(), dim, n, true);          // dim x n: column j = vector j
    o.raw(",\"orthogonal\":"), o.mat(P.data(), dim, dim, false);
    o.raw(",\"centroids\":"), o.mat(C.data(), dim, k, true);       // dim x k: column j = rotated centroid j
    o.raw(",\"rand_bias\":[");
    for (uint64_t i = 0; i < dim; ++i) o.raw(i ? ",0.5" : "0.5");
    o.raw("],\"offsets\":[");
    for (uint64_t i = 0; i <= k; ++i) o.raw(i ? "," : ""), o.u64(off[i]);
    o.raw("],\"map_ids\":[");
    for (uint64_t i = 0; i < n; ++i) o.raw(i ? "," : ""), o.u64(ids[i]);
    o.raw("],\"x_binary_vec\":[");
    for (uint64_t i = 0; i < codes.size(); ++i) o.raw(i ? "," : ""), o.u64(codes[i]);
    o.raw("],\"factors\":[");
    for (uint64_t i = 0; i < n; ++i) {
        o.raw(i ? ",{\"factor_ip\":" : "{\"factor_ip\":"), o.f32(fac[4 * i]);
        o.raw(",\"factor_ppc\":"), o.f32(fac[4 * i + 1]);
        o.raw(",\"error_bound\":"), o.f32(fac[4 * i + 2]);
        o.raw(",\"center_distance_square\":"), o.f32(fac[4 * i + 3]), o.raw("}");
    }
    o.raw("]");
    o.raw(metric_json_members(idx->metric).c_str());
    if (idx->rows.typed()) o.raw(",\"rows\":\""), o.raw(idx->rows.tag()), o.raw("\"");
    o.raw("}");
    const bool closed = fclose(f) == 0;
    if (!o.ok || !closed) return fail(RQ_ERR_IO, std::string("write error on ") + path);
    return RQ_OK;
}

rq_status rq_load_json(const char *path, rq_index **out) {
    if (!path || !out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) return fail(RQ_ERR_IO, std::string("cannot open ") + path);  // "open json error"
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::string text((size_t)std::max(sz, 0l), '\0');
    const bool read_ok = sz <= 0 || fread(&text[0], 1, (size_t)sz, f) == (size_t)sz;
    fclose(f);
    if (!read_ok) return fail(RQ_ERR_IO, std::string("short read on ") + path);
    JsonIn in{text.data(), text.data() + text.size(), {}};
    unsigned long long dim = 0, br = 0, bc = 0, pr = 0, pc = 0, cr = 0, cc = 0;
    std::vector<float> base, P, cent, bias;
    std::vector<unsigned long long> off, ids, codes;
    std::vector<rq_factor_t> fac;
    std::string metric_name, rows_name;
    unsigned long long ip_d = 1ull << 32, ip_bits = 1ull << 32;  // members of an inner-product index (the preset: absent)
    bool good = in.need('{');
    if (good && !in.lit('}')) {
        do {
            std::string k;
            if (!(good = in.key(k))) break;
            if (k == "dim") good = in.num_u64(dim);
            else if (k == "base") good = in.mat(base, br, bc);
            else if (k == "orthogonal") good = in.mat(P, pr, pc);
            else if (k == "centroids") good = in.mat(cent, cr, cc);
            else if (k == "rand_bias") good = in.array(bias, [&](float &v) { return in.num_f32(v); });
            else if (k == "offsets") good = in.array(off, [&](unsigned long long &v) { return in.num_u64(v); });
            else if (k == "map_ids") good = in.array(ids, [&](unsigned long long &v) { return in.num_u64(v); });
            else if (k == "x_binary_vec") good = in.array(codes, [&](unsigned long long &v) { return in.num_u64(v); });
            else if (k == "factors")
                good = in.array(fac, [&](rq_factor_t &fv) {
                    fv = rq_factor_t{0, 0, 0, 0};
                    if (!in.need('{')) return false;
                    do {
                        std::string fk;
                        if (!in.key(fk)) return false;
                        float *dst = fk == "factor_ip" ? &fv.factor_ip : fk == "factor_ppc" ? &fv.factor_ppc
                                   : fk == "error_bound" ? &fv.error_bound
                                   : fk == "center_distance_square" ? &fv.center_distance_square : nullptr;
                        if (dst ? !in.num_f32(*dst) : !in.skip()) return false;
                    } while (in.lit(','));
                    return in.need('}');
                });
            else if (k == "metric") {
                in.ws();
                const char *v0 = in.p;
                good = in.skip();
                if (good) metric_name.assign(v0, in.p);
            } else if (k == "rows") {
                in.ws();
                const char *v0 = in.p;
                good = in.skip();
                if (good) rows_name.assign(v0, in.p);
            } else if (k == "ip_d") good = in.num_u64(ip_d);
            else if (k == "ip_sq_bound_bits") good = in.num_u64(ip_bits);
            else good = in.skip();
        } while (good && in.lit(','));
        good = good && in.need('}');
    }
    if (!good) return fail(RQ_ERR_IO, std::string("deserialize error in ") + path + (in.err.empty() ? "" : ": " + in.err));
    MetricSpec metric;
    if (!metric_from_json(metric_name, ip_d, ip_bits, &metric))
        return fail(RQ_ERR_IO, std::string("unknown metric ") + metric_name + ", or an inner-product index without its ip_d / ip_sq_bound_bits, in " + path);
    const uint64_t n = ids.size(), k = off.empty() ? 0 : off.size() - 1;
    if (dim == 0 || dim % 64 || pr != dim || pc != dim || P.size() != dim * dim || br != dim || bc != n || base.size() != dim * n ||
        cr != dim || cc != k || cent.size() != dim * k || off.empty() || fac.size() != n || codes.size() != n * (dim / 64) ||
        off.back() != n)
        return fail(RQ_ERR_IO, std::string("inconsistent index in ") + path);
    if (metric.id == RQ_METRIC_IP && !(ip_d_ok(metric.d, (uint32_t)dim) && ip_bound_ok(metric.S)))
        return fail(RQ_ERR_IO, std::string("no valid ip_d / ip_sq_bound_bits of an inner-product index of this dim in ") + path);
    for (uint64_t j = 0; j + 1 < off.size(); ++j)
        if (off[j] > off[j + 1]) return fail(RQ_ERR_IO, "offsets are not non-decreasing");
    // Mat (dim x cols, row-major sequence) -> one vector per row
    std::vector<float> base_rows(n * dim), cent_rows(k * dim);
    for (uint64_t i = 0; i < dim; ++i) {
        for (uint64_t j = 0; j < n; ++j) base_rows[j * dim + i] = base[i * n + j];
        for (uint64_t j = 0; j < k; ++j) cent_rows[j * dim + i] = cent[i * k + j];
    }
    std::vector<uint32_t> off32(off.begin(), off.end()), ids32(ids.begin(), ids.end());
    std::vector<uint64_t> codes64(codes.begin(), codes.end());
    RowSpec rows;
    if (!rows_name.empty() && !(rows_name.size() > 2 && rows_name.front() == '"' && rows_name.back() == '"' &&
                                RowSpec::from_tag(rows_name.data() + 1, rows_name.size() - 2, &rows) && rows.allowed_with(metric.id)))
        return fail(RQ_ERR_IO, std::string("unknown \"rows\" member ") + rows_name + " in " + path);
    std::vector<uint8_t> typed;
    if (rows.typed()) RQC(narrow_exact(base_rows.data(), n * dim, rows, typed, path));
    return from_arrays((uint32_t)dim, n, (uint32_t)k, RowsIn::of(rows.typed() ? (const void *)typed.data() : base_rows.data(), rows), P.data(), cent_rows.data(), off32.data(), ids32.data(),
                       codes64.data(), fac.data(), metric, out);
}

void rq_free(rq_index *idx) { delete idx; }

rq_status rq_info(const rq_index *idx, rq_info_t *out) {
    if (!idx || !out) return fail(RQ_ERR_INVALID, "null argument");
    rq_info_t full{};
    full.dim = idx->dim, full.k = idx->k, full.n = idx->n, full.max_list_len = idx->max_list_len, full.n_hbm = idx->n_dev;
    full.split_rows = idx->split_rows ? 1u : 0u, full.metric = idx->metric.id;
    return copy_out_sized(out, full);
}

rq_status rq_get_device_ptr(const rq_index *idx, int which, const void **out_ptr, uint64_t *out_bytes) {
    if (!idx || !out_ptr || !out_bytes) return fail(RQ_ERR_INVALID, "null argument");
    switch (which) {
        case RQ_ARR_BASE:
            if (idx->n_dev < idx->n)  // tiered: the HBM tier holds packed list heads, not rows at their positions
                return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are tiered (HBM + pinned host memory): no single device array; use rq_get_array");
            if (idx->split_rows)  // (common.h) not an array of f32 rows
                return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are stored as split rows (two 16-bit planes per row): no f32 device array; use rq_get_array");
            if (idx->rows.typed())
                return fail(RQ_ERR_UNSUPPORTED, "the raw vectors of this index are half-precision or byte rows: no f32 device array; use rq_get_array, or RQ_ARR_BASE_ROWS for the stored rows");
            *out_ptr = idx->base.p, *out_bytes = idx->n_dev * idx->dim * 4;
            break;
        case RQ_ARR_ORTHOGONAL: *out_ptr = idx->P.p, *out_bytes = (uint64_t)idx->dim * idx->dim * 4; break;
        case RQ_ARR_CENTROIDS: *out_ptr = idx->centroids.p, *out_bytes = (uint64_t)idx->k * idx->dim * 4; break;
        case RQ_ARR_OFFSETS: *out_ptr = idx->offsets.p, *out_bytes = ((uint64_t)idx->k + 1) * 4; break;
        case RQ_ARR_MAP_IDS: *out_ptr = idx->map_ids.p, *out_bytes = idx->n * 4; break;
        case RQ_ARR_CODES: *out_ptr = idx->codes.p, *out_bytes = idx->n * idx->W * 8; break;
        case RQ_ARR_FACTORS: *out_ptr = idx->factors.p, *out_bytes = idx->n * 16; break;
        case RQ_ARR_BASE_ROWS:
            if (!idx->rows.typed()) return fail(RQ_ERR_INVALID, "RQ_ARR_BASE_ROWS: this index stores f32 rows (RQ_ARR_BASE)");
            *out_ptr = idx->base.p, *out_bytes = idx->n * idx->row_bytes();
            break;
        default: return fail(RQ_ERR_INVALID, "unknown array id");
    }
    return RQ_OK;
}

rq_status rq_get_array(const rq_index *idx, int which, void *dst, uint64_t dst_bytes) {
    const void *p;
    uint64_t bytes;
    if (idx && which == RQ_ARR_BASE && (idx->n_dev < idx->n || idx->split_rows || idx->rows.typed())) {  // both tiers / split rows / half rows (widened)
        if (!dst || dst_bytes < idx->n * idx->dim * 4) return fail(RQ_ERR_INVALID, "destination too small");
        return copy_base_rows(idx, 0, idx->n, static_cast<float *>(dst), false);
    }
    RQC(rq_get_device_ptr(idx, which, &p, &bytes));
    if (!dst || dst_bytes < bytes) return fail(RQ_ERR_INVALID, "destination too small");
    if (bytes) HIPC(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    return RQ_OK;
}

rq_status rq_coarse_topk_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len,
                                uint32_t list_lo, uint32_t list_hi, uint32_t probe, uint32_t *d_out_cluster,
                                float *d_out_dist) {
    RQC(ensure_device());
    if (!idx || !d_queries || !d_out_cluster || !d_out_dist) return fail(RQ_ERR_INVALID, "null argument");
    RQC(raw_len_check(idx, "query", len));
    if (probe == 0 || list_lo >= list_hi || list_hi > idx->k) return fail(RQ_ERR_INVALID, "bad list range / probe");
    if (probe > RQ_MAX_PROBE) return fail(RQ_ERR_UNSUPPORTED, "probe > 16384");
    if (nq == 0) return RQ_OK;
    const uint32_t dim = idx->dim, kc = list_hi - list_lo, np = std::min(probe, kc);
    // runs on a pooled workspace (its buffers and stream): this entry sits in the per-batch loop of sharded
    // deployments, so nothing may be allocated or freed per call
    rq_index *mi = const_cast<rq_index *>(idx);
    Workspace *ws = ws_acquire(mi);
    WsLease rel(mi, ws);
    if (!ws->stream) HIPC(hipStreamCreateWithFlags(&ws->stream, hipStreamNonBlocking));
    hipStream_t st = ws->stream;
    // the distance matrix is chunk x kc floats: queries go through in chunks of at most 2^31 cells (8 GiB), so that a
    // multi-GPU batch (65536 x N queries) against tens of thousands of lists does not ask for one 70 GB buffer
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(nq, std::max<uint64_t>(1024, (1ull << 31) / std::max(kc, idx->k)));
    RQC(ws->y.ensure((uint64_t)chunk * dim));
    RQC(ws->dist.ensure((uint64_t)chunk * std::max(kc, idx->k)));
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t m = std::min(chunk, nq - q0);
        const float *qp;  // (the first chunk is the largest: the scratch buffer is sized once)
        RQC(transform_queries(idx, d_queries + (uint64_t)q0 * len, m, len, /*want_padded=*/true, ws->qpad, st, &qp));
        launch_rotate(qp, idx->P.p, ws->y.p, m, dim, m >= 32, st);
        if (kc == idx->k && coarse_prefilter_applies(idx, m, np)) {
            RQC(ws->coarse_redo.ensure(m));
            RQC(ws->qf6.ensure((size_t)m * dim / 2 + 16));
            launch_coarse_prefiltered(idx, ws->y.p, ws->dist.p, m, np, d_out_cluster + (uint64_t)q0 * probe, d_out_dist + (uint64_t)q0 * probe, probe, nullptr,
                                      ws->coarse_redo.p, st, reinterpret_cast<uint16_t *>(ws->qf6.p));
            continue;
        }
        launch_coarse(idx->cent_t.p + list_lo, ws->y.p, ws->dist.p, kc, dim, m, idx->k, st);
        launch_select(ws->dist.p, kc, np, d_out_cluster + (uint64_t)q0 * probe, d_out_dist + (uint64_t)q0 * probe, list_lo, probe, m, st);
    }
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    return RQ_OK;
}

rq_status rq_merge_smallest_u64_device(const uint64_t *d_in, uint32_t world, uint32_t nq, uint32_t width, uint32_t m_out,
                                       uint64_t *d_out) {
    RQC(ensure_device());
    if (!d_in || !d_out) return fail(RQ_ERR_INVALID, "null argument");
    if (nq == 0 || m_out == 0) return RQ_OK;
    const uint64_t m = (uint64_t)world * width;
    if (m == 0 || m > 16384) return fail(RQ_ERR_UNSUPPORTED, "world * width must be in [1, 16384]");
    RQC(ensure_kernel_attributes());
    // on the legacy default stream, asynchronously: ordered with the caller's default-stream work (torch's
    // current stream is that stream unless the caller changed it), like a library call of its own framework
    merge_smallest_u64_kernel<<<nq, 256, (size_t)pow2_ceil((uint32_t)m) * 8, nullptr>>>(
        reinterpret_cast<const unsigned long long *>(d_in), world, nq, width, m_out, reinterpret_cast<unsigned long long *>(d_out),
        (uint64_t)nq * width);
    HIPC(hipGetLastError());
    return RQ_OK;
}

// The call description of a C entry (host_plan.h: QueryCall).  A call without a filter on an index with pending removals runs under
// the index's live filter (live_or): nothing behind this point knows the difference.
static QueryCall topk_call(const rq_index *idx, const rq_filter *filter, uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank, const QueryIO &io) {
    return QueryCall{const_cast<rq_index *>(idx), live_or(idx, filter), len, probe, topk, heuristic_rank != 0, io};
}

rq_status rq_query_batch_device_probed(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len,
                                       const uint32_t *d_probe_cluster, const float *d_probe_dist, uint32_t probe,
                                       uint32_t topk, int heuristic_rank, float *d_out_dist, uint32_t *d_out_id,
                                       uint32_t *d_out_n) {
    if (!d_probe_cluster || !d_probe_dist) return fail(RQ_ERR_INVALID, "null probe lists");
    if (idx && idx->live) return fail(RQ_ERR_UNSUPPORTED, kPendingRefusal);
    if (idx && probe > idx->k) return fail(RQ_ERR_INVALID, "probe lists must have min(probe, k) columns: pass probe <= k");
    return query_device(topk_call(idx, nullptr, len, probe, topk, heuristic_rank, {d_queries, d_out_dist, d_out_id, d_out_n, d_probe_cluster, d_probe_dist}), nq, nullptr);
}

rq_status rq_query_batch_device_seeded(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len,
                                       const uint32_t *d_probe_cluster, const float *d_probe_dist, uint32_t probe,
                                       uint32_t topk, int heuristic_rank, const float *d_thr_init, float *d_out_dist,
                                       uint32_t *d_out_id, uint32_t *d_out_n) {
    if (!d_probe_cluster || !d_probe_dist || !d_thr_init) return fail(RQ_ERR_INVALID, "null probe lists / thresholds");
    if (idx && idx->live) return fail(RQ_ERR_UNSUPPORTED, kPendingRefusal);
    if (idx && probe > idx->k) return fail(RQ_ERR_INVALID, "probe lists must have min(probe, k) columns: pass probe <= k");
    return query_device(topk_call(idx, nullptr, len, probe, topk, heuristic_rank, {d_queries, d_out_dist, d_out_id, d_out_n, d_probe_cluster, d_probe_dist, d_thr_init}),
                        nq, nullptr);
}

rq_status rq_query_batch_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len,
                                uint32_t probe, uint32_t topk, int heuristic_rank, float *d_out_dist,
                                uint32_t *d_out_id, uint32_t *d_out_n) {
    return query_device(topk_call(idx, nullptr, len, probe, topk, heuristic_rank, {d_queries, d_out_dist, d_out_id, d_out_n}), nq, nullptr);
}

rq_status rq_query_batch_device_filtered(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq,
                                         uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank, float *d_out_dist,
                                         uint32_t *d_out_id, uint32_t *d_out_n) {
    return query_device(topk_call(idx, filter, len, probe, topk, heuristic_rank, {d_queries, d_out_dist, d_out_id, d_out_n}), nq, nullptr);
}

rq_status rq_query_batch_device_begin(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len,
                                      uint32_t probe, uint32_t topk, int heuristic_rank, float *d_out_dist,
                                      uint32_t *d_out_id, uint32_t *d_out_n, rq_ticket **out_ticket) {
    return query_device_begin(topk_call(idx, nullptr, len, probe, topk, heuristic_rank, {d_queries, d_out_dist, d_out_id, d_out_n}), nq, out_ticket);
}
rq_status rq_query_batch_device_begin_filtered(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq,
                                               uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank, float *d_out_dist,
                                               uint32_t *d_out_id, uint32_t *d_out_n, rq_ticket **out_ticket) {
    return query_device_begin(topk_call(idx, filter, len, probe, topk, heuristic_rank, {d_queries, d_out_dist, d_out_id, d_out_n}), nq, out_ticket);
}
rq_status rq_query_batch_device_end(rq_ticket *ticket) { return query_device_end(ticket); }

// Device staging of the host-pointer entry points: grown on demand, kept per host thread so a
// per-vector `query()` loop does not pay hipMalloc/hipFree on every call (intentionally never freed).
struct HostStaging {
    void *p[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[4] = {0, 0, 0, 0};
    void *pin = nullptr;  // pinned, device-mapped host buffer for small calls (zero-copy in both directions)
    size_t pin_cap = 0;
    rq_status get(int i, size_t bytes, void **out) {
        if (bytes > cap[i]) {
            if (p[i]) (void)hipFree(p[i]);
            p[i] = nullptr, cap[i] = 0;
            size_t want = std::max<size_t>(bytes, 4096);
            hipError_t e = hipMalloc(&p[i], want);
            if (e != hipSuccess) return fail(RQ_ERR_OOM, std::string("staging hipMalloc failed: ") + hipGetErrorString(e));
            cap[i] = want;
        }
        *out = p[i];
        return RQ_OK;
    }
    rq_status get_pinned(size_t bytes, void **out) {
        if (bytes > pin_cap) {
            if (pin) (void)hipHostFree(pin);
            pin = nullptr, pin_cap = 0;
            size_t want = std::max<size_t>(bytes, 65536);
            hipError_t e = hipHostMalloc(&pin, want, hipHostMallocMapped | hipHostMallocCoherent);
            if (e != hipSuccess) return fail(RQ_ERR_OOM, std::string("pinned staging allocation failed: ") + hipGetErrorString(e));
            pin_cap = want;
        }
        *out = pin;
        return RQ_OK;
    }
};
static thread_local HostStaging g_staging;
#define RQ_ZERO_COPY_BYTES (1u << 20)

static rq_status query_batch_host(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                  uint32_t probe, uint32_t topk, int heuristic_rank, float *out_dist, uint32_t *out_id, uint32_t *out_n) {
    RQC(ensure_device());
    if (!idx || !queries || !out_dist || !out_id || !out_n) return fail(RQ_ERR_INVALID, "null argument");
    if (filter && filter->idx != idx) return fail(RQ_ERR_INVALID, "the filter was made for another index");
    if (nq == 0) return RQ_OK;
    if (topk == 0) return fail(RQ_ERR_UNSUPPORTED, "topk must be in [1, 2048]");
    const size_t qb = ((size_t)nq * len * 4 + 255) & ~(size_t)255, ob = ((size_t)nq * topk * 4 + 255) & ~(size_t)255;
    if (qb + 2 * ob + (size_t)nq * 4 <= RQ_ZERO_COPY_BYTES) {
        // small call (the reference's one-query-per-call loop): queries and results live in pinned host memory
        // the kernels address directly, which replaces five blocking copies by two host memcpys
        void *pin;
        RQC(g_staging.get_pinned(qb + 2 * ob + (size_t)nq * 4, &pin));
        void *dev = nullptr;
        HIPC(hipHostGetDevicePointer(&dev, pin, 0));
        char *h = static_cast<char *>(pin), *d = static_cast<char *>(dev);
        memcpy(h, queries, (size_t)nq * len * 4);
        rq_status s = query_device(topk_call(idx, filter, len, probe, topk, heuristic_rank,
                                             {(const float *)d, (float *)(d + qb), (uint32_t *)(d + qb + ob), (uint32_t *)(d + qb + 2 * ob)}), nq, nullptr);
        if (s != RQ_OK && s != RQ_ERR_EMPTY) return s;
        memcpy(out_dist, h + qb, (size_t)nq * topk * 4);
        memcpy(out_id, h + qb + ob, (size_t)nq * topk * 4);
        memcpy(out_n, h + qb + 2 * ob, (size_t)nq * 4);
        return s;
    }
    void *dq, *dd, *di, *dn;
    RQC(g_staging.get(0, (uint64_t)nq * len * 4, &dq));
    RQC(g_staging.get(1, (uint64_t)nq * topk * 4, &dd));
    RQC(g_staging.get(2, (uint64_t)nq * topk * 4, &di));
    RQC(g_staging.get(3, (uint64_t)nq * 4, &dn));
    HIPC(hipMemcpy(dq, queries, (uint64_t)nq * len * 4, hipMemcpyHostToDevice));
    rq_status s = query_device(topk_call(idx, filter, len, probe, topk, heuristic_rank, {(const float *)dq, (float *)dd, (uint32_t *)di, (uint32_t *)dn}), nq, nullptr);
    if (s != RQ_OK && s != RQ_ERR_EMPTY) return s;
    HIPC(hipMemcpy(out_dist, dd, (uint64_t)nq * topk * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_id, di, (uint64_t)nq * topk * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_n, dn, nq * 4, hipMemcpyDeviceToHost));
    return s;
}

rq_status rq_query_batch(const rq_index *idx, const float *queries, uint32_t nq, uint32_t len, uint32_t probe,
                         uint32_t topk, int heuristic_rank, float *out_dist, uint32_t *out_id, uint32_t *out_n) {
    return query_batch_host(idx, nullptr, queries, nq, len, probe, topk, heuristic_rank, out_dist, out_id, out_n);
}
rq_status rq_query_batch_filtered(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                  uint32_t probe, uint32_t topk, int heuristic_rank, float *out_dist, uint32_t *out_id,
                                  uint32_t *out_n) {
    return query_batch_host(idx, filter, queries, nq, len, probe, topk, heuristic_rank, out_dist, out_id, out_n);
}

// ---- adaptive probing: each query's probe list cut by centroid distance (kernels_coarse.h: probe_cut_kernel) ----
static rq_status probe_rule_check(const rq_probe_rule_t *rule, const uint32_t *d_caps, uint32_t *d_out_nprobe, ProbeRule *out) {
    if (!rule) return fail(RQ_ERR_INVALID, "null rule");
    if (rule->struct_size != sizeof(rq_probe_rule_t)) return fail(RQ_ERR_INVALID, "rq_probe_rule_t: struct_size is not this library's sizeof(rq_probe_rule_t)");
    if (rule->min_probe == 0) return fail(RQ_ERR_INVALID, "rq_probe_rule_t: min_probe must be >= 1");
    if (!(rule->ratio >= 0.0f)) return fail(RQ_ERR_INVALID, "rq_probe_rule_t: ratio must be >= 0 or +inf");
    if (rule->reserved != 0) return fail(RQ_ERR_INVALID, "rq_probe_rule_t: reserved must be 0");
    out->ratio = rule->ratio, out->min_probe = rule->min_probe, out->caps = d_caps, out->out_nprobe = d_out_nprobe;
    return RQ_OK;
}

rq_status rq_query_batch_device_adaptive(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                         uint32_t probe, uint32_t topk, int heuristic_rank, const rq_probe_rule_t *rule,
                                         float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n, uint32_t *d_out_nprobe) {
    QueryCall call = topk_call(idx, filter, len, probe, topk, heuristic_rank, {d_queries, d_out_dist, d_out_id, d_out_n});
    RQC(probe_rule_check(rule, rule ? rule->max_probe : nullptr, d_out_nprobe, &call.rule));
    return query_device(call, nq, nullptr);
}

rq_status rq_probe_counts_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len, uint32_t probe,
                                 const rq_probe_rule_t *rule, uint32_t *d_out_nprobe) {
    QueryCall call = topk_call(idx, nullptr, len, probe, 1, 0, {d_queries});
    call.filter = nullptr;  // (no row is read: pending removals change nothing here)
    RQC(probe_rule_check(rule, rule ? rule->max_probe : nullptr, d_out_nprobe, &call.rule));
    return probe_counts_device(call, nq);
}

// (host pointers: queries, caps and the four outputs staged through one device block of this thread)
static thread_local HostStaging g_staging_adaptive;
rq_status rq_query_batch_adaptive(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                  uint32_t probe, uint32_t topk, int heuristic_rank, const rq_probe_rule_t *rule, float *out_dist,
                                  uint32_t *out_id, uint32_t *out_n, uint32_t *out_nprobe) {
    RQC(ensure_device());
    if (!idx || !queries || !out_dist || !out_id || !out_n) return fail(RQ_ERR_INVALID, "null argument");
    ProbeRule pr;
    RQC(probe_rule_check(rule, nullptr, nullptr, &pr));
    if (filter && filter->idx != idx) return fail(RQ_ERR_INVALID, "the filter was made for another index");
    if (nq == 0) return RQ_OK;
    if (topk == 0) return fail(RQ_ERR_UNSUPPORTED, "topk must be in [1, 2048]");
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t qb = pad((size_t)nq * len * 4), ob = pad((size_t)nq * topk * 4), nb = pad((size_t)nq * 4);
    void *blk;
    RQC(g_staging_adaptive.get(0, qb + 2 * ob + 3 * nb, &blk));
    char *d = static_cast<char *>(blk);
    float *dq = (float *)d, *dd = (float *)(d + qb);
    uint32_t *di = (uint32_t *)(d + qb + ob), *dn = (uint32_t *)(d + qb + 2 * ob), *dnp = (uint32_t *)(d + qb + 2 * ob + nb),
             *dcap = (uint32_t *)(d + qb + 2 * ob + 2 * nb);
    HIPC(hipMemcpy(dq, queries, (size_t)nq * len * 4, hipMemcpyHostToDevice));
    if (rule->max_probe) HIPC(hipMemcpy(dcap, rule->max_probe, (size_t)nq * 4, hipMemcpyHostToDevice));
    QueryCall call = topk_call(idx, filter, len, probe, topk, heuristic_rank, {dq, dd, di, dn});
    call.rule = pr, call.rule.caps = rule->max_probe ? dcap : nullptr, call.rule.out_nprobe = dnp;
    const rq_status s = query_device(call, nq, nullptr);
    if (s != RQ_OK && s != RQ_ERR_EMPTY) return s;
    HIPC(hipMemcpy(out_dist, dd, (size_t)nq * topk * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_id, di, (size_t)nq * topk * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_n, dn, (size_t)nq * 4, hipMemcpyDeviceToHost));
    if (out_nprobe) HIPC(hipMemcpy(out_nprobe, dnp, (size_t)nq * 4, hipMemcpyDeviceToHost));
    return s;
}

// ---- range search: every neighbour inside a per-query radius, as a result object sized by the library (host_range.h) ----
rq_status rq_range_search_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                 uint32_t probe, const float *d_radius, rq_range_result **out) {
    return range_device(const_cast<rq_index *>(idx), live_or(idx, filter), d_queries, nq, len, probe, d_radius, out);
}
rq_status rq_range_search(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                          uint32_t probe, const float *radius, rq_range_result **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    RQC(ensure_device());
    if (!idx || (nq && (!queries || !radius))) return fail(RQ_ERR_INVALID, "null argument");
    void *dq = nullptr, *dr = nullptr;
    if (nq) {
        RQC(g_staging.get(0, (uint64_t)nq * len * 4, &dq));
        RQC(g_staging.get(3, (uint64_t)nq * 4, &dr));
        HIPC(hipMemcpy(dq, queries, (uint64_t)nq * len * 4, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(dr, radius, (uint64_t)nq * 4, hipMemcpyHostToDevice));
    }
    return range_device(const_cast<rq_index *>(idx), live_or(idx, filter), (const float *)dq, nq, len, probe, (const float *)dr, out);
}
rq_status rq_range_result_info(const rq_range_result *r, uint32_t *out_nq, uint64_t *out_total) {
    if (!r || !out_nq || !out_total) return fail(RQ_ERR_INVALID, "null argument");
    *out_nq = r->nq, *out_total = r->total;
    return RQ_OK;
}
rq_status rq_range_result_device_ptrs(const rq_range_result *r, const uint64_t **d_lims, const float **d_dist, const uint32_t **d_id) {
    if (!r || !d_lims || !d_dist || !d_id) return fail(RQ_ERR_INVALID, "null argument");
    *d_lims = reinterpret_cast<const uint64_t *>(r->lims.p), *d_dist = r->dist.p, *d_id = r->id.p;
    return RQ_OK;
}
rq_status rq_range_result_copy(const rq_range_result *r, uint64_t *lims, float *dist, uint32_t *id) {
    if (!r || !lims || (r->total && (!dist || !id))) return fail(RQ_ERR_INVALID, "null argument");
    HIPC(hipMemcpy(lims, r->lims.p, ((size_t)r->nq + 1) * 8, hipMemcpyDeviceToHost));
    if (r->total) {
        HIPC(hipMemcpy(dist, r->dist.p, (size_t)r->total * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(id, r->id.p, (size_t)r->total * 4, hipMemcpyDeviceToHost));
    }
    return RQ_OK;
}
void rq_range_result_free(rq_range_result *r) { delete r; }

// ---- filters: the allow-list in the index's terms (position bitmap + admitted rows per list), made once ----
rq_status rq_filter_create(const rq_index *idx, const uint32_t *allow_bits, uint64_t nbits, int bits_on_device, rq_filter **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    RQC(id_bits_check(allow_bits, nbits));
    RQC(ensure_device());
    std::unique_ptr<rq_filter> f(new rq_filter());
    hipStream_t st = nullptr;
    HIPC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamDestroy(s); }
    } sg{st};
    // (on an index with pending removals, rq_remove_lazy: admitted = allowed AND live)
    RQC(position_bits(idx, allow_bits, nbits, bits_on_device, false, 0u, st, f->pos_bits, f->h_sub_off));
    RQC(filter_finish(idx, f.get()));
    *out = f.release();
    return RQ_OK;
}
rq_status rq_filter_rows(const rq_filter *f, uint64_t *out_admitted) {
    if (!f || !out_admitted) return fail(RQ_ERR_INVALID, "null argument");
    *out_admitted = f->rows;
    return RQ_OK;
}
void rq_filter_free(rq_filter *f) { delete f; }

// ---- exact search (host_exact.h): brute-force top-k over the stored rows ----
rq_status rq_exact_search_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len, uint32_t topk,
                                 const rq_exact_params_t *params, float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n) {
    return exact_search_device(idx, live_or(idx, filter), d_queries, nq, len, topk, params, d_out_dist, d_out_id, d_out_n);
}
rq_status rq_exact_search(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len, uint32_t topk,
                          const rq_exact_params_t *params, float *out_dist, uint32_t *out_id, uint32_t *out_n) {
    return exact_search_host(idx, live_or(idx, filter), queries, nq, len, topk, params, out_dist, out_id, out_n);
}
// ---- exact range search (host_exact_range.h): every stored row within a per-query radius, as an rq_range_result ----
rq_status rq_exact_range_search_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                       const float *d_radius, const rq_exact_params_t *params, rq_range_result **out) {
    return exact_range_device(idx, live_or(idx, filter), d_queries, nq, len, d_radius, params, out);
}
rq_status rq_exact_range_search(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                const float *radius, const rq_exact_params_t *params, rq_range_result **out) {
    return exact_range_host(idx, live_or(idx, filter), queries, nq, len, radius, params, out);
}
rq_status rq_last_exact_stats(rq_exact_stats_t *out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    return copy_out_sized(out, g_exact_stats);
}

// ---- in-place mutation (host_mutate.h): the index afterwards equals a fresh build of its live rows, bit for bit ----
static rq_status mutate_done(const rq_index *idx, rq_status s, std::chrono::steady_clock::time_point t0) {
    if (s != RQ_OK) (void)hipGetLastError();  // (a failed hipMalloc's sticky error must not fail the next call)
    if (idx) g_mutate_stats.rows_after = idx->n;
    g_mutate_stats.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return s;
}
rq_status rq_add(rq_index *idx, const float *rows, uint64_t m, uint32_t d, const uint32_t *ids, int rows_on_device,
                 uint32_t *out_first_id) {
    const auto t0 = std::chrono::steady_clock::now();
    return mutate_done(idx, index_add(idx, rows, m, d, ids, rows_on_device, out_first_id), t0);
}
rq_status rq_remove(rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, uint64_t *out_removed) {
    const auto t0 = std::chrono::steady_clock::now();
    return mutate_done(idx, index_remove(idx, id_bits, nbits, bits_on_device, out_removed), t0);
}
// merge / extract (host_mutate.h): the same invariant with no pass 1 -- rows, codes and factors move as they stand
rq_status rq_merge_from(rq_index *dst, rq_index *src, uint32_t id_mode, uint32_t id_shift, uint32_t *out_shift) {
    const auto t0 = std::chrono::steady_clock::now();
    return mutate_done(dst, index_merge_from(dst, src, id_mode, id_shift, out_shift), t0);
}
rq_status rq_extract(rq_index *src, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, rq_index **out) {
    const auto t0 = std::chrono::steady_clock::now();
    const rq_status s = index_extract(src, id_bits, nbits, bits_on_device, out);
    return mutate_done(out ? *out : nullptr, s, t0);  // (rows_after: the new index's)
}
// lazy removal (host_mutate.h): mark rows dead in the index's live filter, drop them in one relayout later
rq_status rq_remove_lazy(rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, uint64_t *out_marked) {
    const rq_status s = index_remove_lazy(idx, id_bits, nbits, bits_on_device, out_marked);
    if (s != RQ_OK) (void)hipGetLastError();  // (a failed hipMalloc's sticky error must not fail the next call)
    return s;
}
rq_status rq_compact(rq_index *idx, uint64_t *out_removed) {
    const auto t0 = std::chrono::steady_clock::now();
    return mutate_done(idx, index_compact(idx, out_removed), t0);
}
rq_status rq_pending_removals(const rq_index *idx, uint64_t *out_dead) {
    if (!idx || !out_dead) return fail(RQ_ERR_INVALID, "null argument");
    *out_dead = idx->pending();
    return RQ_OK;
}
rq_status rq_last_mutate_stats(rq_mutate_stats_t *out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    return copy_out_sized(out, g_mutate_stats);
}

// ---- rows by id (host_directory.h): they read the index and write nothing of it ----
static rq_status by_id_done(rq_status s) {
    if (s != RQ_OK) (void)hipGetLastError();  // (a failed hipMalloc's sticky error must not fail the next call)
    return s;
}
rq_status rq_locate(const rq_index *idx, const uint32_t *ids, uint64_t m, uint32_t *out_pos) { return by_id_done(locate_host(idx, ids, m, out_pos)); }
rq_status rq_locate_device(const rq_index *idx, const uint32_t *d_ids, uint64_t m, uint32_t *d_out_pos) { return by_id_done(locate_device(idx, d_ids, m, d_out_pos)); }
rq_status rq_fetch_rows(const rq_index *idx, const uint32_t *ids, uint64_t m, float *out_rows, uint32_t *out_found) {
    return by_id_done(fetch_host(idx, ids, m, false, out_rows, out_found));
}
rq_status rq_fetch_rows_device(const rq_index *idx, const uint32_t *d_ids, uint64_t m, float *d_out_rows, uint32_t *d_out_found) {
    return by_id_done(fetch_device(idx, d_ids, m, false, d_out_rows, d_out_found));
}
rq_status rq_fetch_stored(const rq_index *idx, const uint32_t *ids, uint64_t m, void *out_rows, uint32_t *out_found) {
    return by_id_done(fetch_host(idx, ids, m, true, out_rows, out_found));
}
rq_status rq_fetch_stored_device(const rq_index *idx, const uint32_t *d_ids, uint64_t m, void *d_out_rows, uint32_t *d_out_found) {
    return by_id_done(fetch_device(idx, d_ids, m, true, d_out_rows, d_out_found));
}
rq_status rq_pair_distances(const rq_index *idx, const float *queries, uint32_t nq, uint32_t length, const uint32_t *ids, uint32_t c,
                            float *out_dist) {
    return by_id_done(pair_distances_host(idx, queries, nq, length, ids, c, out_dist));
}
rq_status rq_pair_distances_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t length, const uint32_t *d_ids,
                                   uint32_t c, float *d_out_dist) {
    return by_id_done(pair_distances_device(idx, d_queries, nq, length, d_ids, c, d_out_dist));
}
rq_status rq_neighbours_of(const rq_index *idx, const uint32_t *ids, uint32_t m, uint32_t probe, uint32_t topk, int heuristic_rank,
                           const rq_filter *filter, float *out_dist, uint32_t *out_ids, uint32_t *out_found) {
    return by_id_done(neighbours_host(idx, ids, m, false, probe, topk, heuristic_rank, filter, nullptr, out_dist, out_ids, out_found));
}
rq_status rq_neighbours_of_device(const rq_index *idx, const uint32_t *d_ids, uint32_t m, uint32_t probe, uint32_t topk,
                                  int heuristic_rank, const rq_filter *filter, float *d_out_dist, uint32_t *d_out_ids,
                                  uint32_t *d_out_found) {
    return by_id_done(neighbours_device(idx, d_ids, m, false, probe, topk, heuristic_rank, filter, nullptr, d_out_dist, d_out_ids, d_out_found));
}
rq_status rq_neighbours_of_exact(const rq_index *idx, const uint32_t *ids, uint32_t m, uint32_t topk, const rq_filter *filter,
                                 const rq_exact_params_t *params, float *out_dist, uint32_t *out_ids, uint32_t *out_found) {
    return by_id_done(neighbours_host(idx, ids, m, true, 1, topk, 0, filter, params, out_dist, out_ids, out_found));
}
rq_status rq_neighbours_of_exact_device(const rq_index *idx, const uint32_t *d_ids, uint32_t m, uint32_t topk, const rq_filter *filter,
                                        const rq_exact_params_t *params, float *d_out_dist, uint32_t *d_out_ids,
                                        uint32_t *d_out_found) {
    return by_id_done(neighbours_device(idx, d_ids, m, true, 1, topk, 0, filter, params, d_out_dist, d_out_ids, d_out_found));
}
rq_status rq_last_by_id_stats(rq_by_id_stats_t *out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    return copy_out_sized(out, g_by_id_stats);
}

// ---- attribute columns and predicate filters (host_attr.h) ----
rq_status rq_attr_create(rq_index *idx, const char *name, uint32_t type, rq_attr_value_t fill) { return by_id_done(attr_create(idx, name, type, fill)); }
rq_status rq_attr_drop(rq_index *idx, const char *name) { return attr_drop(idx, name); }
rq_status rq_attr_count(const rq_index *idx, uint32_t *out) {
    if (!idx || !out) return fail(RQ_ERR_INVALID, "null argument");
    *out = (uint32_t)idx->attrs.size();
    return RQ_OK;
}
rq_status rq_attr_info(const rq_index *idx, uint32_t i, rq_attr_info_t *out) { return attr_info(idx, i, out); }
rq_status rq_attr_index(const rq_index *idx, const char *name, uint32_t *out) {
    AttrColumn *c = nullptr;
    RQC(attr_named(idx, name, !out, &c));
    *out = (uint32_t)attr_find(idx, name);
    return RQ_OK;
}
rq_status rq_attr_set(rq_index *idx, const char *name, const uint32_t *ids, const void *values, uint64_t m, uint64_t *out_absent) {
    return by_id_done(attr_set_host(idx, name, ids, values, m, out_absent));
}
rq_status rq_attr_set_device(rq_index *idx, const char *name, const uint32_t *d_ids, const void *d_values, uint64_t m, uint64_t *out_absent) {
    return by_id_done(attr_set_device(idx, name, d_ids, d_values, m, out_absent));
}
rq_status rq_attr_get(const rq_index *idx, const char *name, const uint32_t *ids, uint64_t m, void *out_values, uint32_t *out_found) {
    return by_id_done(attr_get_host(idx, name, ids, m, out_values, out_found));
}
rq_status rq_attr_get_device(const rq_index *idx, const char *name, const uint32_t *d_ids, uint64_t m, void *d_out_values, uint32_t *d_out_found) {
    return by_id_done(attr_get_device(idx, name, d_ids, m, d_out_values, d_out_found));
}
rq_status rq_attr_get_array(const rq_index *idx, const char *name, void *dst, uint64_t dst_bytes) { return attr_get_array(idx, name, dst, dst_bytes); }
rq_status rq_filter_create_where(const rq_index *idx, const rq_where_term_t *terms, uint32_t nterms, const uint8_t *program, uint32_t ntokens,
                                 rq_filter **out) {
    return by_id_done(filter_create_where(idx, terms, nterms, program, ntokens, out));
}
rq_status rq_last_where_stats(rq_where_stats_t *out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    return copy_out_sized(out, g_where_stats);
}
rq_status rq_filter_combine(const rq_index *idx, const rq_filter *a, const rq_filter *b, uint32_t op, rq_filter **out) {
    return by_id_done(filter_combine(idx, a, b, op, out));
}
rq_status rq_filter_id_bits(const rq_filter *f, uint32_t *bits, uint64_t nbits, int bits_on_device) {
    return by_id_done(filter_id_bits(f, bits, nbits, bits_on_device));
}
rq_status rq_filter_ids_device(const rq_filter *f, uint32_t *d_out_ids, uint64_t cap, uint64_t *out_count) {
    return by_id_done(filter_ids_device(f, d_out_ids, cap, out_count));
}

// ---- grouped search (host_group.h): at most group_size rows per value of a column, the topk nearest values ----
static GroupIn group_in_query(const rq_filter *filter, const float *q, uint32_t len, uint32_t probe, int heuristic_rank) {
    GroupIn in;
    in.src = GROUP_SRC_QUERY, in.filter = filter, in.q = q, in.len = len, in.probe = probe, in.heuristic = heuristic_rank;
    return in;
}
static GroupIn group_in_exact(const rq_filter *filter, const float *q, uint32_t len, const rq_exact_params_t *exact) {
    GroupIn in;
    in.src = GROUP_SRC_EXACT, in.filter = filter, in.q = q, in.len = len, in.exact = exact;
    return in;
}
static GroupIn group_in_results(const float *dist, const uint32_t *id, const uint32_t *cnt) {
    GroupIn in;
    in.src = GROUP_SRC_RESULTS, in.dist = dist, in.id = id, in.cnt = cnt;
    return in;
}
rq_status rq_query_batch_grouped(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len, uint32_t probe,
                                 int heuristic_rank, const char *column, const rq_group_params_t *params, float *out_dist, uint32_t *out_id,
                                 uint64_t *out_key, uint32_t *out_group_n, uint32_t *out_n, uint32_t *out_fetched) {
    return by_id_done(group_host(idx, group_in_query(filter, queries, len, probe, heuristic_rank), nq, column, params,
                                 GroupOut{out_dist, out_id, out_key, out_group_n, out_n, out_fetched}));
}
rq_status rq_query_batch_grouped_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                        uint32_t probe, int heuristic_rank, const char *column, const rq_group_params_t *params,
                                        float *d_out_dist, uint32_t *d_out_id, uint64_t *d_out_key, uint32_t *d_out_group_n, uint32_t *d_out_n,
                                        uint32_t *d_out_fetched) {
    return by_id_done(group_device(idx, group_in_query(filter, d_queries, len, probe, heuristic_rank), nq, column, params,
                                   GroupOut{d_out_dist, d_out_id, d_out_key, d_out_group_n, d_out_n, d_out_fetched}));
}
rq_status rq_exact_search_grouped(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                  const rq_exact_params_t *exact, const char *column, const rq_group_params_t *params, float *out_dist,
                                  uint32_t *out_id, uint64_t *out_key, uint32_t *out_group_n, uint32_t *out_n, uint32_t *out_fetched) {
    return by_id_done(group_host(idx, group_in_exact(filter, queries, len, exact), nq, column, params,
                                 GroupOut{out_dist, out_id, out_key, out_group_n, out_n, out_fetched}));
}
rq_status rq_exact_search_grouped_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                         const rq_exact_params_t *exact, const char *column, const rq_group_params_t *params,
                                         float *d_out_dist, uint32_t *d_out_id, uint64_t *d_out_key, uint32_t *d_out_group_n,
                                         uint32_t *d_out_n, uint32_t *d_out_fetched) {
    return by_id_done(group_device(idx, group_in_exact(filter, d_queries, len, exact), nq, column, params,
                                   GroupOut{d_out_dist, d_out_id, d_out_key, d_out_group_n, d_out_n, d_out_fetched}));
}
rq_status rq_group_results(const rq_index *idx, const float *dist, const uint32_t *id, const uint32_t *cnt, uint32_t nq, const char *column,
                           const rq_group_params_t *params, float *out_dist, uint32_t *out_id, uint64_t *out_key, uint32_t *out_group_n,
                           uint32_t *out_n) {
    return by_id_done(group_host(idx, group_in_results(dist, id, cnt), nq, column, params, GroupOut{out_dist, out_id, out_key, out_group_n, out_n, nullptr}));
}
rq_status rq_group_results_device(const rq_index *idx, const float *d_dist, const uint32_t *d_id, const uint32_t *d_cnt, uint32_t nq,
                                  const char *column, const rq_group_params_t *params, float *d_out_dist, uint32_t *d_out_id,
                                  uint64_t *d_out_key, uint32_t *d_out_group_n, uint32_t *d_out_n) {
    return by_id_done(group_device(idx, group_in_results(d_dist, d_id, d_cnt), nq, column, params,
                                   GroupOut{d_out_dist, d_out_id, d_out_key, d_out_group_n, d_out_n, nullptr}));
}
rq_status rq_last_group_stats(rq_group_stats_t *out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    return copy_out_sized(out, g_group_stats);
}

// ---- diverse search (host_diverse.h): the topk rows maximal marginal relevance takes out of `fetch` candidates ----
rq_status rq_query_batch_diverse(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len, uint32_t probe,
                                 int heuristic_rank, const rq_diverse_params_t *params, float *out_dist, uint32_t *out_id, float *out_div,
                                 uint32_t *out_n, uint32_t *out_fetched) {
    return by_id_done(diverse_host(idx, group_in_query(filter, queries, len, probe, heuristic_rank), nq, params,
                                   DiverseOut{out_dist, out_id, out_div, out_n, out_fetched}));
}
rq_status rq_query_batch_diverse_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                        uint32_t probe, int heuristic_rank, const rq_diverse_params_t *params, float *d_out_dist,
                                        uint32_t *d_out_id, float *d_out_div, uint32_t *d_out_n, uint32_t *d_out_fetched) {
    return by_id_done(diverse_device(idx, group_in_query(filter, d_queries, len, probe, heuristic_rank), nq, params,
                                     DiverseOut{d_out_dist, d_out_id, d_out_div, d_out_n, d_out_fetched}));
}
rq_status rq_exact_search_diverse(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                  const rq_exact_params_t *exact, const rq_diverse_params_t *params, float *out_dist, uint32_t *out_id,
                                  float *out_div, uint32_t *out_n, uint32_t *out_fetched) {
    return by_id_done(diverse_host(idx, group_in_exact(filter, queries, len, exact), nq, params, DiverseOut{out_dist, out_id, out_div, out_n, out_fetched}));
}
rq_status rq_exact_search_diverse_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                         const rq_exact_params_t *exact, const rq_diverse_params_t *params, float *d_out_dist,
                                         uint32_t *d_out_id, float *d_out_div, uint32_t *d_out_n, uint32_t *d_out_fetched) {
    return by_id_done(diverse_device(idx, group_in_exact(filter, d_queries, len, exact), nq, params,
                                     DiverseOut{d_out_dist, d_out_id, d_out_div, d_out_n, d_out_fetched}));
}
rq_status rq_diversify_results(const rq_index *idx, const float *dist, const uint32_t *id, const uint32_t *cnt, uint32_t nq,
                               const rq_diverse_params_t *params, float *out_dist, uint32_t *out_id, float *out_div, uint32_t *out_n) {
    return by_id_done(diverse_host(idx, group_in_results(dist, id, cnt), nq, params, DiverseOut{out_dist, out_id, out_div, out_n, nullptr}));
}
rq_status rq_diversify_results_device(const rq_index *idx, const float *d_dist, const uint32_t *d_id, const uint32_t *d_cnt, uint32_t nq,
                                      const rq_diverse_params_t *params, float *d_out_dist, uint32_t *d_out_id, float *d_out_div,
                                      uint32_t *d_out_n) {
    return by_id_done(diverse_device(idx, group_in_results(d_dist, d_id, d_cnt), nq, params, DiverseOut{d_out_dist, d_out_id, d_out_div, d_out_n, nullptr}));
}
rq_status rq_last_diverse_stats(rq_diverse_stats_t *out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    return copy_out_sized(out, g_diverse_stats);
}

rq_status rq_query(const rq_index *idx, const float *query, uint32_t len, uint32_t probe, uint32_t topk,
                   int heuristic_rank, float *out_dist, uint32_t *out_id, uint32_t *out_n) {
    return rq_query_batch(idx, query, 1, len, probe, topk, heuristic_rank, out_dist, out_id, out_n);
}

#include "host_shard.h"

rq_status rq_metrics(rq_metrics_t *out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    out->rough = g_rough.load(), out->precise = g_precise.load(), out->query = g_query.load(), out->miss = g_miss.load();
    return RQ_OK;
}
rq_status rq_metrics_reset(void) {
    g_rough = 0, g_precise = 0, g_query = 0, g_miss = 0;
    return RQ_OK;
}

rq_status rq_set_option(const char *name, int value) {
    if (!name) return fail(RQ_ERR_INVALID, "null option name");
    const OptionRow *o = nullptr;
    for (const OptionRow &r : g_options)
        if (!strcmp(r.name, name)) o = &r;
    if (!o) return fail(RQ_ERR_INVALID, std::string("unknown option ") + name);
    // the rules that are not a plain range (host_options.h names them on their rows)
#ifndef RQ_DEV_ABLATIONS
    if (o->var == &g_seg_opt && value == 3)
        return fail(RQ_ERR_INVALID, "survivor_segments = 3 (allocation-failure injection) exists in the developer build only (make dev)");
#endif
    const bool odd = (o->var == &g_stage_growth && value == 1) || (o->var == &g_scan_dbg && (value & ~RQ_OPT_DEBUG_BITS));
    if (value < o->lo || value > o->hi || odd) return fail(RQ_ERR_INVALID, o->refused);
    if (o->var) *o->var = value;
    else if (!strcmp(name, "base_device_mb")) g_base_device_mb = value;
    else g_max_scan_blocks = value == 0 ? RQ_MAX_BLOCKS_256 : std::min<uint32_t>((uint32_t)value, RQ_MAX_BLOCKS_256);  // "max_scan_blocks"
    return RQ_OK;
}

rq_status rq_set_profiling(int level) {
    if (level < 0 || level > 2) return fail(RQ_ERR_INVALID, "profiling level must be 0, 1 or 2");
    g_profiling = level;
    return RQ_OK;
}
rq_status rq_last_profile(rq_profile_t *out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    return copy_out_sized(out, g_profile);
}

// ---- per-stage entry points --------------------------------------------------------------------
rq_status rq_rotate(const float *x, uint64_t n, uint32_t dim, const float *orthogonal, int use_mfma, float *out) {
    RQC(ensure_device());
    if (!x || !orthogonal || !out) return fail(RQ_ERR_INVALID, "null argument");
    if (dim == 0 || dim % 64) return fail(RQ_ERR_DIM_MISMATCH, "dim must be a multiple of 64");
    DevBuf<float> dx, dp, dout;
    RQC(dx.upload(x, n * dim));
    RQC(dp.upload(orthogonal, (size_t)dim * dim));
    RQC(dout.alloc(n * dim));
    launch_rotate(dx.p, dp.p, dout.p, n, dim, use_mfma != 0, nullptr);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(out, dout.p, n * dim * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

rq_status rq_rotate_device(const rq_index *idx, const float *d_x, uint64_t n, float *d_out, float *out_ms) {
    RQC(ensure_device());
    if (!idx || !d_x || !d_out) return fail(RQ_ERR_INVALID, "null argument");
    hipEvent_t e0, e1;
    HIPC(hipEventCreate(&e0));
    HIPC(hipEventCreate(&e1));
    HIPC(hipEventRecord(e0, nullptr));
    launch_rotate(d_x, idx->P.p, d_out, n, idx->dim, true, nullptr);
    HIPC(hipEventRecord(e1, nullptr));
    HIPC(hipEventSynchronize(e1));
    HIPC(hipGetLastError());
    float ms = 0;
    HIPC(hipEventElapsedTime(&ms, e0, e1));
    if (out_ms) *out_ms = ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return RQ_OK;
}

rq_status rq_quantize_pack(const float *x_rot, uint64_t n, uint32_t dim, const float *centroids_rot, uint32_t k,
                           uint32_t *out_label, float *out_dist, uint64_t *out_codes, rq_factor_t *out_factors) {
    RQC(ensure_device());
    RQC(ensure_kernel_attributes());
    if (!x_rot || !centroids_rot || !out_label || !out_dist || !out_codes || !out_factors)
        return fail(RQ_ERR_INVALID, "null argument");
    if (dim == 0 || dim % 64 || k == 0) return fail(RQ_ERR_DIM_MISMATCH, "dim must be a multiple of 64, k > 0");
    rq_index tmp;
    tmp.dim = dim, tmp.k = k, tmp.W = dim / 64;
    DevBuf<float> dx, dd;
    DevBuf<uint32_t> dl;
    DevBuf<uint64_t> dc;
    DevBuf<float4> df;
    RQC(dx.upload(x_rot, n * dim));
    RQC(tmp.centroids.upload(centroids_rot, (size_t)k * dim));
    RQC(tmp.cent_t.alloc((size_t)k * dim));
    RQC(dd.alloc(n));
    RQC(dl.alloc(n));
    RQC(dc.alloc(n * tmp.W));
    RQC(df.alloc(n));
    transpose_kernel<<<dim3(ceil_div(dim, 32), ceil_div(k, 32)), dim3(32, 8)>>>(tmp.centroids.p, tmp.cent_t.p, k, dim);
    AssignAux ax;  // the build's assignment path: matrix-core pre-filter + exact refinement (option assign_impl)
    HIPC(hipDeviceSynchronize());
    if (bf16_tile_has(tmp.W) && g_assign_impl.load() != 1) RQC(assign_aux_init(&tmp, ax, std::min<uint64_t>(std::max<uint64_t>(n, 1), 1ull << 20)));
    for (uint64_t i0 = 0; i0 < n; i0 += (1ull << 20)) {  // chunked: launches stay far below 2^32 threads
        const uint64_t m = std::min<uint64_t>(1ull << 20, n - i0);
        RQC(launch_assign_prefiltered(dx.p + i0 * dim, &tmp, ax, m, dl.p + i0, dd.p + i0));
        quantize_kernel<<<ceil_div(m, 32), 256>>>(dx.p + i0 * dim, tmp.centroids.p, dl.p + i0, m, dim,
                                                  dc.p + i0 * tmp.W, df.p + i0);
    }
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    if (n) {
        HIPC(hipMemcpy(out_label, dl.p, n * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out_dist, dd.p, n * 4, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out_codes, dc.p, n * tmp.W * 8, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(out_factors, df.p, n * 16, hipMemcpyDeviceToHost));
    }
    return RQ_OK;
}

rq_status rq_coarse_rank(const rq_index *idx, const float *queries, uint32_t nq, uint32_t len, uint32_t probe,
                         float *out_y, uint32_t *out_cluster, float *out_dist) {
    RQC(ensure_device());
    if (!idx || !queries || !out_cluster || !out_dist) return fail(RQ_ERR_INVALID, "null argument");
    RQC(raw_len_check(idx, "query", len));
    if (probe == 0) return fail(RQ_ERR_INVALID, "probe == 0");
    const uint32_t dim = idx->dim, k = idx->k, nprobe = std::min(probe, k);
    if (nprobe > RQ_MAX_PROBE) return fail(RQ_ERR_UNSUPPORTED, "probe > 16384");
    DevBuf<float> dq, qpad, y, dist, pd;
    DevBuf<uint32_t> pc;
    RQC(dq.upload(queries, (uint64_t)nq * len));
    RQC(y.alloc((uint64_t)nq * dim));
    RQC(dist.alloc((uint64_t)nq * k));
    RQC(pd.alloc((uint64_t)nq * nprobe));
    RQC(pc.alloc((uint64_t)nq * nprobe));
    const float *qrows;
    RQC(transform_queries(idx, dq.p, nq, len, /*want_padded=*/true, qpad, nullptr, &qrows));
    launch_rotate(qrows, idx->P.p, y.p, nq, dim, nq >= 32, nullptr);
    coarse_dist_kernel<4><<<dim3(ceil_div(nq, 4), ceil_div(k, 256)), 256, 4 * dim * sizeof(float)>>>(
        idx->cent_t.p, y.p, dist.p, k, dim, nq, k);
    launch_select(dist.p, k, nprobe, pc.p, pd.p, 0, nprobe, nq, nullptr);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    if (out_y) HIPC(hipMemcpy(out_y, y.p, (uint64_t)nq * dim * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_cluster, pc.p, (uint64_t)nq * nprobe * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_dist, pd.p, (uint64_t)nq * nprobe * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

rq_status rq_query_prep(const rq_index *idx, const float *y, uint32_t nq, const uint32_t *cluster, float *out_lower,
                        float *out_delta, uint32_t *out_sum, uint64_t *out_planes) {
    RQC(ensure_device());
    if (!idx || !y || !cluster || !out_lower || !out_delta || !out_sum || !out_planes)
        return fail(RQ_ERR_INVALID, "null argument");
    const uint32_t dim = idx->dim, W = idx->W;
    for (uint32_t i = 0; i < nq; ++i)
        if (cluster[i] >= idx->k) return fail(RQ_ERR_INVALID, "cluster id out of range");
    DevBuf<float> dy, ycd;
    DevBuf<uint32_t> dc, dsum;
    DevBuf<PairScalars> scal;
    DevBuf<uint64_t> planes;
    RQC(dy.upload(y, (uint64_t)nq * dim));
    RQC(ycd.alloc(nq));
    RQC(dc.upload(cluster, nq));
    RQC(dsum.alloc(nq));
    RQC(scal.alloc(nq));
    RQC(planes.alloc((uint64_t)nq * 4 * W));
    HIPC(hipMemset(ycd.p, 0, nq * 4));
    prep_kernel<<<ceil_div(nq, 4), 256>>>(dy.p, idx->centroids.p, idx->offsets.p, dc.p, ycd.p, nq, 1, dim, scal.p,
                                          planes.p, nullptr, nullptr, dsum.p, idx->k, 0u);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    std::vector<PairScalars> hs(nq);
    HIPC(hipMemcpy(hs.data(), scal.p, nq * sizeof(PairScalars), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < nq; ++i) out_lower[i] = hs[i].lower, out_delta[i] = hs[i].delta;
    HIPC(hipMemcpy(out_sum, dsum.p, nq * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(out_planes, planes.p, (uint64_t)nq * 4 * W * 8, hipMemcpyDeviceToHost));
    return RQ_OK;
}

rq_status rq_scan(const rq_index *idx, uint32_t cluster, float y_c_distance_square, const uint64_t *planes,
                  float lower_bound, float scalar_sum, float delta, float *out_rough) {
    RQC(ensure_device());
    if (!idx || !planes || !out_rough) return fail(RQ_ERR_INVALID, "null argument");
    if (cluster >= idx->k) return fail(RQ_ERR_INVALID, "cluster id out of range");
    uint32_t off[2];
    HIPC(hipMemcpy(off, idx->offsets.p + cluster, 8, hipMemcpyDeviceToHost));
    const uint32_t len = off[1] - off[0];
    if (len == 0) return RQ_OK;
    DevBuf<uint64_t> dpl;
    DevBuf<float> dout;
    RQC(dpl.upload(planes, 4 * idx->W));
    RQC(dout.alloc(len));
    scan_dense_kernel<<<ceil_div(len, 256), 256>>>(reinterpret_cast<const uint32_t *>(idx->codes.p), idx->factors.p,
                                                   off[0], len, idx->W, reinterpret_cast<const uint32_t *>(dpl.p),
                                                   lower_bound, delta, scalar_sum, y_c_distance_square, dout.p);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(out_rough, dout.p, len * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

rq_status rq_rerank(const rq_index *idx, const float *query_padded, const uint32_t *pos, uint32_t m,
                    float *out_accurate) {
    RQC(ensure_device());
    if (!idx || !query_padded || !pos || !out_accurate) return fail(RQ_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < m; ++i)
        if (pos[i] >= idx->n) return fail(RQ_ERR_INVALID, "position out of range");
    if (m == 0) return RQ_OK;
    DevBuf<float> dq, dout;
    DevBuf<uint32_t> dp;
    RQC(dq.upload(query_padded, idx->dim));
    RQC(dout.alloc(m));
    RQC(dp.upload(pos, m));
    accurate_flat_kernel<<<ceil_div(m, 32), 256>>>(dp.p, m, idx->view(), dq.p, idx->dim, dout.p);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(out_accurate, dout.p, m * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}

}  // extern "C"
