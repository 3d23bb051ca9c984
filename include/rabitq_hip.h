/*
 * rabitq_hip.h -- C ABI of librabitq_hip.so, the MI355X (gfx950) engine for the RaBitQ build/query
 * hot path of kemingy/rabitq.  Plain pointers and sizes only; no C++/torch types.
 *
 * The reference has no FFI seam of its own; the seam is cut at the public
 * methods of `RaBitQ` (src/lib.rs:12), which is exactly what a Rust `extern "C"` block would bind
 * (INTEGRATION.md shows that binding).  Every entry point cites the reference interface it
 * replaces as file:line relative to the reference repository root.
 *
 * Conventions
 *   - All functions return rq_status (0 = RQ_OK).  The reference panics (`expect`/`assert!`,
 *     release profile panic = "abort", Cargo.toml:43) where these return an error; a Rust wrapper
 *     keeps that behaviour by `expect()`-ing the status.  rq_last_error() gives the message.
 *   - "host" pointers are ordinary CPU memory; "_device" variants take HIP device pointers
 *     (hipMalloc) and enqueue on an internal stream, returning after the results are complete.
 *   - Query entry points are safe to call concurrently on one index (read-only index, per-call
 *     workspace + stream), as `RaBitQ::query(&self)` is (src/rabitq.rs:268); build/load/dump/free
 *     are single-caller.
 *   - Matrices are row-major.  `dim` is the dimension padded to a multiple of 64
 *     (src/rabitq.rs:168-179).  Ids and positions are u32 (src/rabitq.rs:64-65).
 */
#ifndef RABITQ_HIP_H
#define RABITQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t rq_status;
enum {
    RQ_OK = 0,
    RQ_ERR_INVALID = -1,      /* bad argument (null pointer, probe == 0, topk == 0 ...)            */
    RQ_ERR_DIM_MISMATCH = -2, /* src/rabitq.rs:165 / :275 assert failures                          */
    RQ_ERR_IO = -3,           /* src/rabitq.rs:73-155 `expect("open ... error")`                    */
    RQ_ERR_HIP = -4,          /* a HIP runtime call failed                                         */
    RQ_ERR_NO_DEVICE = -5,    /* no gfx950 device visible: there is NO CPU fallback                */
    RQ_ERR_UNSUPPORTED = -6,  /* size outside the engine's limits (documented per function)        */
    RQ_ERR_EMPTY = -7,        /* heuristic ranker produced no candidate (src/rerank.rs:173 panics) */
    RQ_ERR_OOM = -8
};

/* Opaque index handle: the device-resident state of `RaBitQ` (src/rabitq.rs:57-68). */
typedef struct rq_index rq_index;

/* `Factor`, src/rabitq.rs:21-32 (repr(C), 16 bytes, same field order). */
typedef struct {
    float factor_ip, factor_ppc, error_bound, center_distance_square;
} rq_factor_t;

/* `Metrics`, src/metrics.rs:7-18: process-global counters. */
typedef struct {
    uint64_t rough, precise, query, miss;
} rq_metrics_t;

/* Out-structs (rq_info_t, rq_build_stats_t, rq_profile_t) are versioned by size: the caller sets `struct_size` to
 * sizeof(the struct it was compiled against) before the call and the library writes at most that many bytes, so a
 * host built against an older header is never written past its struct when fields are appended (fields are only ever
 * appended).  struct_size == 0 (an unset field) is refused with RQ_ERR_INVALID. */
typedef struct {
    uint32_t struct_size;  /* in: sizeof(rq_info_t) of the caller */
    uint32_t dim;          /* padded dimension */
    uint32_t k;            /* number of clusters */
    uint32_t max_list_len; /* longest IVF list */
    uint64_t n;            /* number of vectors */
    uint64_t n_hbm;        /* raw vectors resident in HBM; the other n - n_hbm (list tails) are in pinned host memory */
    uint32_t split_rows;   /* 1: the raw vectors are stored as split rows (option "split_rows"); appended in 0.5.0 */
    uint32_t metric;       /* RQ_METRIC_L2, RQ_METRIC_COSINE or RQ_METRIC_IP (was reserved0, always 0, before 0.8.0) */
} rq_info_t;

/* ---- library ------------------------------------------------------------------------------- */
/* ABI revision of this header: bumped whenever a struct layout or the meaning of an entry point changes (3: sized
 * out-structs, rq_get_device_ptr refuses RQ_ARR_BASE on tiered indexes; options "scan_dense" and the round-2 "coarse_impl" = 3 removed.
 * 4: rq_set_option("scan_debug") refuses the timing-ablation bits -- they exist in the developer build only --, the matrix-core
 * scan's step counters in rq_profile_t are always filled, new option "scan_gate", "coarse_impl" = 3 is back with a new meaning,
 * rq_profile_t.reserved became coarse_fallback_rows, .reserved2 matrix_additive_launches; later in revision 4, additions only: "coarse_impl" = 4,
 * "coarse_tiled_from", "rerank_shadow" = 2 -- the new default; 0.5.0: option "split_rows", rq_info_t.split_rows appended, RQ_ARR_BASE
 * refused for split rows as for tiers; 0.6.0: filtered queries -- rq_filter_* and rq_query_batch*_filtered, additions only;
 * 0.7.0: in-place mutation -- rq_add / rq_remove / rq_last_mutate_stats, additions only; a filter made before a mutation of its
 * index is refused; later in 0.7, additions only: range search -- rq_range_search* and rq_range_result_*;
 * 0.8.0: cosine metric -- rq_*_metric, rq_normalize*, rq_info_t.reserved0 became metric, additions only;
 * later in 0.8, additions only: rq_query_batch_device_begin_filtered, option "small_batch_filtered" -- filtered batches of <= 64
 * queries on the small-batch path;
 * 0.9.0: inner-product metric, additions only -- RQ_METRIC_IP, rq_*_ip, rq_ip_*, rq_augment*, rq_row_sqnorm_max*;
 * 0.10.0: half-precision rows, additions only -- RQ_ROWS_*, rq_*_rows, rq_row_type, rq_widen*, RQ_ARR_BASE_ROWS;
 * 0.11.0: byte rows, two more values of row_type and no new symbol -- RQ_ROWS_U8, RQ_ROWS_I8;
 * later in 0.11, additions only: exact search -- rq_exact_search*, rq_last_exact_stats; exact range search --
 * rq_exact_range_search*; rq_exact_stats_t.reserved0 became scan_subtiles;
 * later in 0.11, additions only: adaptive probing -- rq_probe_rule_t, rq_query_batch_adaptive, rq_query_batch_device_adaptive,
 * rq_probe_counts_device;
 * later in 0.11, additions only: centroid training -- rq_train_params_t, rq_train_stats_t, rq_train_centroids,
 * rq_train_centroids_device;
 * 0.12.0: merge and extract, additions only -- RQ_MERGE_IDS_*, rq_merge_from, rq_extract; rq_last_mutate_stats reports them too;
 * 0.13.0: lazy removal, additions only -- rq_remove_lazy, rq_compact, rq_pending_removals; an index with pending removals
 * refuses the entries that have no filtered form, and a filter made before a marking rq_remove_lazy is refused;
 * 0.14.0: rows by id, additions only -- rq_locate*, rq_fetch_rows*, rq_fetch_stored*, rq_pair_distances*, rq_neighbours_of*,
 * rq_neighbours_of_exact*, rq_by_id_stats_t, rq_last_by_id_stats; they read the index and change nothing of it;
 * 0.15.0: attribute columns, additions only -- RQ_ATTR_*, rq_attr_value_t, rq_attr_info_t, rq_attr_create / _drop / _count / _info /
 * _index / _set* / _get* / _get_array, RQ_WHERE_*, rq_where_term_t, rq_filter_create_where, rq_where_stats_t, rq_last_where_stats,
 * RQ_FILTER_*, rq_filter_combine, rq_filter_id_bits, rq_filter_ids_device; an index without columns behaves, allocates and dumps
 * exactly as before; rq_last_mutate_stats.gather_bytes counts the column bytes a relayout moves);
 * 0.16.0: grouped search, additions only -- rq_group_params_t, rq_group_stats_t, rq_query_batch_grouped*, rq_exact_search_grouped*,
 * rq_group_results*, rq_last_group_stats; no existing call, refusal or output changes;
 * 0.17.0: diverse search, additions only -- rq_diverse_params_t, rq_diverse_stats_t, rq_query_batch_diverse*, rq_exact_search_diverse*,
 * rq_diversify_results*, rq_last_diverse_stats; no existing call, refusal or output changes.
 * A host checks rq_abi_version() == RQ_ABI_VERSION once after loading the library. */
#define RQ_ABI_VERSION 4
uint32_t rq_abi_version(void);
const char *rq_version(void);
const char *rq_last_error(void);              /* thread-local message of the last failure        */
rq_status rq_init(int device);                /* select the HIP device for this process          */

/* ---- metric ---------------------------------------------------------------------------------- */
/* The metric is a property of the index.  RQ_METRIC_L2 (what every entry point without a metric argument means) is the
 * reference's squared L2 distance.  RQ_METRIC_COSINE normalises on the GPU every raw row that enters the index (build,
 * streamed build, rq_add) and every raw query row (every query entry point that takes queries: plain, filtered, range,
 * _begin / _end, probed, seeded, rq_coarse_topk_device, rq_coarse_rank, the sharded step), and is otherwise the L2 engine:
 * a cosine index made from (base, centroids, P) equals, bit for bit, the L2 index made from (N(base) row by row, centroids,
 * P) -- every array (RQ_ARR_BASE returns the normalised rows), rq_info, the five files of rq_dump_dir -- and a query q
 * returns exactly what that L2 index returns for N(q): ids, order, distance bits, out_n, status and counters.  Distances
 * are therefore |N(x) - N(q)|^2 = 2 - 2 cos(x, q), unscaled; radii (rq_range_search*) and initial thresholds
 * (rq_query_batch_device_seeded) are in that unit.  Centroids are used as given (train them on normalised rows:
 * rq_normalize_device).  The reference has no counterpart (its README lists cosine similarity as missing).
 * N(x), on the row zero-padded to dim = ceil64(d): s = vector_dot_product(x, x) in the order of src/simd.rs:257-314 (eight
 * lanes, one fused multiply-add per lane and 8-element chunk in sequence, then the 8-lane fold); nrm = sqrtf(s), correctly
 * rounded; if nrm is a normal number (f32::is_normal, the test of src/rabitq.rs:210-215) N(x)_i = x_i / nrm, an IEEE f32
 * division; otherwise N(x) = x bit for bit (a zero row, a subnormal or overflowed norm, a row holding inf or NaN).
 * rq_rerank and rq_query_prep take already-prepared inputs (a padded query, rotated queries) and do not normalise:
 * pass N(q) / its rotation.  An unknown metric is refused with RQ_ERR_INVALID. */
enum { RQ_METRIC_L2 = 0, RQ_METRIC_COSINE = 1, RQ_METRIC_IP = 2 };
/* N(x) of n rows of d floats; out is n x ceil64(d) (d <= 4096).  rq_normalize: host pointers; rq_normalize_device: device
 * pointers, returns with `out` complete. */
rq_status rq_normalize(const float *x, uint64_t n, uint32_t d, float *out);
rq_status rq_normalize_device(const float *d_x, uint64_t n, uint32_t d, float *d_out);

/* ---- inner-product metric (maximum inner product search) -------------------------------------- */
/* RQ_METRIC_IP answers "which rows have the largest dot product with q" with the L2 engine, by the standard reduction: with S
 * a bound on the squared row norms, every row gets one more coordinate sqrt(S - |x|^2) and every query a zero, so that
 * |A(x) - Q(q)|^2 = S + |q|^2 - 2<x, q> and ascending L2 order is descending inner-product order.  An IP index has three
 * parameters: d, the raw row length (1 <= d <= 4095); dim = ceil64(d + 1); S, an f32, finite and >= 0.
 * Row map A(x; S), on the row zero-padded to dim: s = vector_dot_product(x, x) in the order of src/simd.rs:257-314 (the chain
 * of N(x) above); the row is valid iff s is finite and s <= S (f32 compare); A(x)_i = x_i bit for bit for i < d; A(x)_d =
 * sqrtf(S - s), one f32 subtraction and a correctly rounded root; every other coordinate is 0.
 * Query map Q(q): q zero-padded to dim (slot d is 0); no arithmetic.
 * An IP index of (base, centroids, P, S) equals, bit for bit, the L2 index of (A(base), centroids zero-extended to dim, P):
 * every array (RQ_ARR_BASE returns the augmented rows), rq_info (metric = RQ_METRIC_IP), the dump.  A query of exactly d
 * floats (otherwise RQ_ERR_DIM_MISMATCH) returns exactly what that L2 index returns for Q(q): ids, order, distance bits,
 * out_n, status, counters -- on every query entry (plain, filtered, range, _begin / _end, probed, seeded, coarse, sharded).
 * Distances are D = |A(x) - Q(q)|^2, unscaled; radii and seeded thresholds are in that unit.  The two conversions, in f32 with
 * s_q = vector_dot_product(Q(q), Q(q)) in the same order:  ip = 0.5f * ((S + s_q) - D);  radius = (S + s_q) - 2.0f * min_ip.
 * The index dimension grows by the extra coordinate: for d a multiple of 64 that is one more 64-wide word (128 -> 192).
 * The *_metric entries take no d / S and keep refusing metric id 2.
 *
 * The builds are the L2 signatures plus centroid_cols and sq_bound.  centroids are k x centroid_cols, d <= centroid_cols <=
 * dim, missing columns are zero (a caller who trains on augmented rows, rq_augment_device, passes d + 1 or dim).  sq_bound:
 * NaN = automatic, S = the largest s of the input, bit for bit (the streamed builder has no automatic mode and refuses NaN:
 * take rq_row_sqnorm_max_device over the chunks).  A negative or infinite bound, or an invalid row, is RQ_ERR_INVALID,
 * rq_last_error names the first offending row, and no index is made; a builder whose chunk was refused can only be freed. */
rq_status rq_build_ip(const float *base, uint64_t n, uint32_t d, const float *centroids, uint32_t k, const float *orthogonal,
                      uint64_t seed, uint32_t centroid_cols, float sq_bound, rq_index **out);
rq_status rq_build_device_ip(const float *d_base, uint64_t n, uint32_t d, const float *d_centroids, uint32_t k,
                             const float *orthogonal_host, uint64_t seed, uint32_t centroid_cols, float sq_bound, rq_index **out);
/* (the centroid file's records have centroid_cols = their length) */
rq_status rq_build_from_path_ip(const char *base_fvecs, const char *centroid_fvecs, const float *orthogonal, uint64_t seed,
                                float sq_bound, rq_index **out);
/* d of an IP index and its S; RQ_ERR_INVALID on an index of another metric */
rq_status rq_ip_params(const rq_index *idx, uint32_t *d, float *sq_bound);
/* A(x; sq_bound) of n rows of d floats into out, n x ceil64(d + 1); the refusals of the builds (sq_bound = NaN: automatic). */
rq_status rq_augment(const float *x, uint64_t n, uint32_t d, float sq_bound, float *out);
rq_status rq_augment_device(const float *d_x, uint64_t n, uint32_t d, float sq_bound, float *d_out);
/* The largest s of n rows of d floats (0 for n = 0) into *out_max (host memory in both forms); a row whose s is inf or NaN:
 * RQ_ERR_INVALID. */
rq_status rq_row_sqnorm_max(const float *x, uint64_t n, uint32_t d, float *out_max);
rq_status rq_row_sqnorm_max_device(const float *d_x, uint64_t n, uint32_t d, float *out_max);
/* ip of returned distances: dist and out_ip are nq x topk, n (nullable) the nq result counts: slots at or past n[q] get -inf.
 * radius of a smallest wanted inner product per query: min_ip and out_radius are nq floats.  queries: nq x len, len = d.
 * Plain form: host pointers; _device: device pointers, returns with the output complete. */
rq_status rq_ip_from_dist(const rq_index *idx, const float *queries, uint32_t nq, uint32_t len, const float *dist, uint32_t topk,
                          const uint32_t *n, float *out_ip);
rq_status rq_ip_from_dist_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len, const float *d_dist,
                                 uint32_t topk, const uint32_t *d_n, float *d_out_ip);
rq_status rq_ip_radius(const rq_index *idx, const float *queries, uint32_t nq, uint32_t len, const float *min_ip, float *out_radius);
rq_status rq_ip_radius_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len, const float *d_min_ip,
                              float *d_out_radius);

/* ---- half-precision rows: f16 / bf16 raw vectors stored as given (0.10.0, additions only) ------ */
/* The row type is a property of the index.  RQ_ROWS_F32 (what every entry point without a row_type means) stores 4*dim bytes per
 * raw vector.  RQ_ROWS_F16 (IEEE binary16) and RQ_ROWS_BF16 store the caller's 2-byte elements as given, n x dim of them, the
 * padding slots +0: 2*dim bytes per vector, no f32 copy, no shadow rows, no split rows (the options "rerank_shadow" and
 * "split_rows" do not apply), and the build never holds an n x dim f32 array either (typed chunks are widened into a bounded
 * staging buffer).  Widening W is exact: f16 -> f32 the IEEE conversion (subnormals kept; a NaN stays a NaN, payload unspecified),
 * bf16 -> f32 bits << 16.  A half-row L2 index made from rows h (n x d), centroids (f32, k x d), P and seed equals, bit for bit,
 * the index rq_build_device makes from W(h): codes, factors, offsets, map_ids, centroids; RQ_ARR_BASE returns W(h) in cluster
 * order, zero-padded; rq_info is equal (n_hbm == n, split_rows == 0); every query entry (plain, filtered, range, _begin / _end,
 * probed, seeded, coarse, rq_rerank, shards of rq_shard_index -- they inherit the row type) returns the same ids, order, distance
 * bits, counts, status and counters.  Queries stay f32 (rq_widen* converts a caller's half-precision queries).  The reference
 * has no counterpart.
 * Cosine: the stored row is R_t(N(W(h))), R_t = round to nearest even to the row type (f16: subnormal results kept, overflow to
 * inf; bf16, non-NaN: (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the f32 bits u), and the index equals the L2 index of
 * W(R_t(N(W(h)))): rotation, assignment and quantisation see the rounded rows.  Rows N leaves untouched stay bit for bit.
 * Refused: RQ_METRIC_IP with half rows (the extra coordinate is not representable), rq_add / rq_remove on a half-row index, a
 * half-row index that does not fit the HBM budget (option "base_device_mb" included; there are no tiers for half rows),
 * rq_get_device_ptr(RQ_ARR_BASE) -- all RQ_ERR_UNSUPPORTED; an unknown row_type: RQ_ERR_INVALID.
 * RQ_ARR_BASE_ROWS (rq_get_array, rq_get_device_ptr): the stored n x dim 2-byte rows, n * dim * 2 bytes; RQ_ERR_INVALID on an f32
 * index.  Persistence: rq_dump_dir writes the crate's files with base.fvecs widened (the reference loads it and answers
 * identically) plus a file `rows` holding "f16\n" / "bf16\n"; rq_load_dir with a `rows` file stores half rows (a value of
 * base.fvecs the type cannot hold, or an unknown text: RQ_ERR_IO); the JSON image carries "rows":"f16" / "bf16" likewise.
 *
 * Byte rows (0.11.0): RQ_ROWS_U8 and RQ_ROWS_I8 store the caller's n x d one-byte elements as given, n x dim of them, the padding
 * slots 0x00: dim bytes per vector, no f32 copy, no shadow rows, no split rows, no tiers, and the build never holds an n x dim f32
 * array.  W(u8) = the integer as f32, W(i8) = the two's-complement integer as f32; both are exact, and the narrowing the loaders
 * use is the exact inverse on representable values.  A byte-row L2 index of (b, centroids, P) equals, bit for bit, the f32 L2 index
 * of (W(b), centroids, P): every array, rq_info, and the ids, order, distance bits, counts, status and counters of every query
 * entry listed above.  Queries, centroids and P stay f32.  Every _rows entry, rq_row_type and rq_widen* (`count` one-byte elements,
 * any alignment) take the two values; RQ_ARR_BASE returns W(b), RQ_ARR_BASE_ROWS the stored n * dim bytes.
 * Refused, each leaving nothing allocated and the index untouched: RQ_METRIC_COSINE (a normalised row is not a value of the type)
 * and RQ_METRIC_IP with byte rows, rq_add / rq_remove, an index over the HBM budget, rq_get_device_ptr(RQ_ARR_BASE) -- all
 * RQ_ERR_UNSUPPORTED.  Values 3, 6 and above remain RQ_ERR_INVALID.  Persistence: base.fvecs holds W(b), the `rows` file "u8\n" /
 * "i8\n", the JSON member "rows":"u8" / "i8"; a load whose base.fvecs holds a value the named type cannot represent (0.5, 256,
 * -1 or -0 under u8, a NaN), or an unknown text, is RQ_ERR_IO. */
enum { RQ_ROWS_F32 = 0, RQ_ROWS_F16 = 1, RQ_ROWS_BF16 = 2, RQ_ROWS_U8 = 4, RQ_ROWS_I8 = 5 };
struct rq_builder;
/* rq_build_metric / rq_build_device_metric with typed rows: base is n x d elements of row_type (host / device memory; 2-byte
 * aligned is enough), centroids stay f32. */
rq_status rq_build_rows(const void *base, uint64_t n, uint32_t d, const float *centroids, uint32_t k, const float *orthogonal,
                        uint64_t seed, uint32_t metric, uint32_t row_type, rq_index **out);
rq_status rq_build_device_rows(const void *d_base, uint64_t n, uint32_t d, const float *d_centroids, uint32_t k,
                               const float *orthogonal_host, uint64_t seed, uint32_t metric, uint32_t row_type, rq_index **out);
/* The streamed build with typed chunks: a builder made with row_type != RQ_ROWS_F32 takes its chunks (m x d elements of its
 * type, device memory) through the two _rows calls and refuses the plain chunk calls (RQ_ERR_INVALID); a plain builder, this
 * entry with RQ_ROWS_F32 included, the other way round.  order / finish / free / stats are the plain builder's. */
rq_status rq_builder_create_rows(uint64_t n, uint32_t d, const float *d_centroids, uint32_t k, const float *orthogonal_host,
                                 uint64_t seed, uint64_t max_device_base_bytes, uint32_t metric, uint32_t row_type,
                                 struct rq_builder **out);
rq_status rq_builder_assign_chunk_rows(struct rq_builder *b, const void *d_rows, uint64_t i0, uint64_t m);
rq_status rq_builder_place_chunk_rows(struct rq_builder *b, const void *d_rows, uint64_t i0, uint64_t m);
/* rq_from_arrays_metric with base n x dim elements of row_type (cluster order), taken as they are. */
rq_status rq_from_arrays_rows(uint32_t dim, uint64_t n, uint32_t k, const void *base, const float *orthogonal,
                              const float *centroids, const uint32_t *offsets, const uint32_t *map_ids, const uint64_t *codes,
                              const rq_factor_t *factors, uint32_t metric, uint32_t row_type, rq_index **out);
rq_status rq_row_type(const rq_index *idx, uint32_t *out);
/* out[i] = W(x[i]) for `count` elements of row_type (any count; x 2-byte aligned, byte elements: any alignment).  rq_widen: host pointers; rq_widen_device:
 * device pointers, returns with `out` complete. */
rq_status rq_widen(const void *x, uint32_t row_type, uint64_t count, float *out);
rq_status rq_widen_device(const void *d_x, uint32_t row_type, uint64_t count, float *d_out);

/* ---- build: RaBitQ::from_path, src/rabitq.rs:159-265 ---------------------------------------- */
/* `orthogonal` is the dim x dim rotation P (row-major, P[r][c]); the reference draws it from an
 * unseeded RNG (src/utils.rs:16-20), so for reproducibility it is an input.  NULL = generate a
 * Gaussian-QR orthogonal matrix from `seed` (same construction, seeded). */
rq_status rq_build(const float *base, uint64_t n, uint32_t d, const float *centroids, uint32_t k,
                   const float *orthogonal, uint64_t seed, rq_index **out);
/* Same with base/centroids already in device memory (n x d and k x d, row-major f32).  `base` is
 * only read; the index keeps its own cluster-ordered copy (src/rabitq.rs:245-247). */
rq_status rq_build_device(const float *d_base, uint64_t n, uint32_t d, const float *d_centroids,
                          uint32_t k, const float *orthogonal_host, uint64_t seed, rq_index **out);
/* From .fvecs files exactly as RaBitQ::from_path(base_path, centroid_path). */
rq_status rq_build_from_path(const char *base_fvecs, const char *centroid_fvecs,
                             const float *orthogonal, uint64_t seed, rq_index **out);
/* The three builds with a metric (RQ_METRIC_L2: exactly the calls above). */
rq_status rq_build_metric(const float *base, uint64_t n, uint32_t d, const float *centroids, uint32_t k,
                          const float *orthogonal, uint64_t seed, uint32_t metric, rq_index **out);
rq_status rq_build_device_metric(const float *d_base, uint64_t n, uint32_t d, const float *d_centroids,
                                 uint32_t k, const float *orthogonal_host, uint64_t seed, uint32_t metric, rq_index **out);
rq_status rq_build_from_path_metric(const char *base_fvecs, const char *centroid_fvecs,
                                    const float *orthogonal, uint64_t seed, uint32_t metric, rq_index **out);

/* ---- streamed two-pass build: from_path for inputs that need not be resident (e.g. 100M x 768 = 307 GB) ---- */
/* The same result as rq_build_device, with the n x d input fed chunk by chunk, twice:
 *   rq_builder_create -> rq_builder_assign_chunk (every row once: rotate src/rabitq.rs:188, nearest list :203, sign-pack +
 *   factors :205-229) -> rq_builder_order (cluster ordering :232-243) -> rq_builder_place_chunk (every row once more:
 *   raw vectors to their cluster-order positions :244-247) -> rq_builder_finish.
 * Chunks are m x d row-major f32 in DEVICE memory covering rows [i0, i0 + m); any order, any sizes, but every row exactly
 * once per pass: a chunk that overlaps rows already fed to the same pass is refused (RQ_ERR_INVALID), and
 * rq_builder_order / rq_builder_finish refuse to run while rows are missing.  Each call returns
 * when the chunk buffer may be reused.  max_device_base_bytes: HBM budget of the raw vectors (0 = automatic: what is
 * free minus a reserve; UINT64_MAX = all in HBM).  Beyond it the split is per list: the head of every list (the vectors
 * nearest its centroid, which the re-ranker asks for most) stays in HBM, the tail goes to pinned host memory and is
 * gathered over the host link by the rerank (results identical).  rq_builder_finish consumes the builder (also on
 * error); rq_builder_free abandons one. */
typedef struct rq_builder rq_builder;
typedef struct {
    uint32_t struct_size;                      /* in: sizeof(rq_build_stats_t) of the caller */
    float ms_rotate, ms_assign, ms_quantize;   /* device time of the three pass-1 kernels, HIP events, summed over chunks */
    uint64_t rows_assigned;                    /* rotation flops so far = 2 * rows_assigned * dim^2 */
    uint64_t rows_in_hbm, rows_in_host_memory; /* base tiers (known after rq_builder_order) */
    uint64_t rows_exact_redo;                  /* rows whose nearest list the exact-order kernel decided alone: the bf16 pre-filter
                                                  left none or more than 16 candidates (appended in revision 3) */
} rq_build_stats_t;
rq_status rq_builder_create(uint64_t n, uint32_t d, const float *d_centroids, uint32_t k, const float *orthogonal_host,
                            uint64_t seed, uint64_t max_device_base_bytes, rq_builder **out);
/* rq_builder_create with a metric: on a cosine builder both passes normalise their chunks (the same kernel, the same bits). */
rq_status rq_builder_create_metric(uint64_t n, uint32_t d, const float *d_centroids, uint32_t k, const float *orthogonal_host,
                                   uint64_t seed, uint64_t max_device_base_bytes, uint32_t metric, rq_builder **out);
/* The streamed build of an inner-product index: both passes augment their chunks with sq_bound (the same kernel, the same
 * bits); a chunk holding an invalid row is refused with RQ_ERR_INVALID, after which the builder can only be freed. */
rq_status rq_builder_create_ip(uint64_t n, uint32_t d, const float *d_centroids, uint32_t k, const float *orthogonal_host,
                               uint64_t seed, uint64_t max_device_base_bytes, uint32_t centroid_cols, float sq_bound,
                               rq_builder **out);
rq_status rq_builder_assign_chunk(rq_builder *b, const float *d_rows, uint64_t i0, uint64_t m);
rq_status rq_builder_order(rq_builder *b);
rq_status rq_builder_place_chunk(rq_builder *b, const float *d_rows, uint64_t i0, uint64_t m);
rq_status rq_builder_finish(rq_builder *b, rq_index **out);
void rq_builder_free(rq_builder *b);
rq_status rq_builder_stats(const rq_builder *b, rq_build_stats_t *out);

/* ---- centroid training (scripts/cluster.py:63-108 does this offline with faiss k-means) -------- */
/* Lloyd k-means on a sample of min(n, points_per_centroid * k) vectors (points_per_centroid = 256
 * in the reference script); d_base is n x d in device memory, d_centroids_out receives k x d.
 * No parity target (faiss is not available; results depend on the seed): judged by recall. */
rq_status rq_kmeans_device(const float *d_base, uint64_t n, uint32_t d, uint32_t k, uint32_t iters,
                           uint32_t points_per_centroid, uint64_t seed, float *d_centroids_out);

/* ---- centroid training with a contract: deterministic k-means for every build ------------------ */
/* Trains the k centroids a build of (rows, metric, row_type) takes, reproducibly to the bit: two runs of one seed, the host and
 * the device entry, and both values of option "assign_impl" return the same bits, and tests/train_model.py computes them on the
 * CPU.  With cols = d (RQ_METRIC_IP: d + 1) and dim = ceil64(cols):
 *  1. sample: ns = min(n, max(points_per_centroid, 1) * k) rows; every row in order when ns == n, else row r of the sample is row
 *     lo + mix64(seed * 0x100000001B3 + r) mod (hi - lo) with lo = floor(r n / ns), hi = floor((r + 1) n / ns) (u64; mix64 is
 *     splitmix64's finaliser as rq_kmeans_device uses it): distinct, ascending, one per stratum;
 *  2. the sampled rows are widened (W) and transformed as the build transforms them (N(x) for cosine, A(x; S) for the inner
 *     product, zero padding to dim);
 *  3. centroid j starts as transformed sample row floor(j ns / k);
 *  4. iteration t = 0 .. iters - 1: label and distance of every sample row (the build's nearest-list rule: exact-order f32
 *     distance, first minimum); if t > 0 and no label changed, stop with iters_run = t; centroid = f32 sum of its members in
 *     ascending sample position, strictly left to right, divided by (float)count; objective[t] = the members' distances summed in
 *     f64, per cluster in ascending sample position, then over the clusters ascending; then every empty cluster e, ascending, takes
 *     half of the largest cluster (lowest index on ties; fewer than 2 members: e keeps its centroid): with eps = 2^-10,
 *     cent[e][c] = cent[donor][c] * (c even ? 1 + eps : 1 - eps), cent[donor][c] *= (c even ? 1 - eps : 1 + eps),
 *     count[e] = count[donor] / 2, count[donor] -= count[e], splits += 1;
 *  5. out: k x cols f32 (an inner-product build takes them with centroid_cols = d + 1).
 * Refused: n < k, k == 0, d == 0 or NULL arguments, a sample row with a non-finite element or (inner product) one A refuses, an
 * sq_bound that is neither NaN nor finite and >= 0 (RQ_ERR_INVALID); a row type the metric does not go with, dim > 4096,
 * n >= 2^32, ns * dim > 2^31 (RQ_ERR_UNSUPPORTED).  Nothing is written to the outputs then. */
typedef struct {
    uint32_t struct_size;         /* in: sizeof(rq_train_params_t) */
    uint32_t iters;               /* iteration cap */
    uint32_t points_per_centroid; /* sample size per centroid (0 counts as 1) */
    uint64_t seed;
    uint32_t metric;              /* RQ_METRIC_* */
    uint32_t row_type;            /* RQ_ROWS_*: the element type of the rows */
    float sq_bound;               /* RQ_METRIC_IP: S; NaN = the largest squared row norm over all n rows (rq_row_sqnorm_max*) */
} rq_train_params_t;
typedef struct {
    uint32_t struct_size; /* in: sizeof(rq_train_stats_t) of the caller */
    uint32_t iters_run;   /* iterations whose centroid update ran (== iters when the cap ended the training) */
    uint32_t sample_rows; /* ns */
    uint32_t splits;
} rq_train_stats_t;
/* d_rows: n x d elements of params->row_type, device; d_centroids_out: k x cols f32, device; objective_out: host, params->iters
 * doubles of which the first iters_run are written (may be NULL); stats_out: host (may be NULL). */
rq_status rq_train_centroids_device(const void *d_rows, uint64_t n, uint32_t d, uint32_t k, const rq_train_params_t *params,
                                    float *d_centroids_out, double *objective_out, rq_train_stats_t *stats_out);
/* The same with rows and centroids_out in host memory: the sample is drawn on the host and only its ns rows are uploaded (an
 * inner-product run with sq_bound NaN first asks rq_row_sqnorm_max, which stages all n rows once). */
rq_status rq_train_centroids(const void *rows, uint64_t n, uint32_t d, uint32_t k, const rq_train_params_t *params,
                             float *centroids_out, double *objective_out, rq_train_stats_t *stats_out);

/* ---- persistence: load_from_dir / dump_to_dir, src/rabitq.rs:84-156 -------------------------- */
/* Byte-compatible with the crate's five-file directory (vecs framing: src/utils.rs:280-364).  A cosine index writes a sixth
 * file, `metric`, holding the text "cosine\n" (an L2 dump stays exactly the five files); rq_load_dir sets the metric when the
 * file is present (unknown content: RQ_ERR_IO).  An inner-product index writes "ip <d> <S as 8 hex digits>\n". */
rq_status rq_load_dir(const char *dir, rq_index **out);
rq_status rq_dump_dir(const rq_index *idx, const char *dir);
/* load_from_json / dump_to_json, src/rabitq.rs:72-81: the serde_json image of the `RaBitQ` struct (faer `Mat`s as
 * {"nrows","ncols","data": row-major}; base dim x n, centroids dim x k).  A debugging format in the reference too: the
 * text is ~10x the binary directory, so use rq_load_dir / rq_dump_dir for anything large.  A cosine index adds the member
 * "metric":"cosine" (serde ignores unknown members: the reference still loads the file); rq_load_json reads it when present.  An
 * inner-product index adds "metric":"ip","ip_d":<d>,"ip_sq_bound_bits":<the bits of S as an integer>. */
rq_status rq_load_json(const char *path, rq_index **out);
rq_status rq_dump_json(const rq_index *idx, const char *path);
void rq_free(rq_index *idx);

/* Construct an index from the reference's in-memory arrays (what load_from_dir ends up with):
 * base n x dim (cluster order, un-rotated), orthogonal dim x dim, centroids k x dim (rotated;
 * row j = centroid j), offsets k+1, map_ids n, codes n x dim/64 u64, factors n x 4 f32. */
rq_status rq_from_arrays(uint32_t dim, uint64_t n, uint32_t k, const float *base,
                         const float *orthogonal, const float *centroids, const uint32_t *offsets,
                         const uint32_t *map_ids, const uint64_t *codes, const rq_factor_t *factors,
                         rq_index **out);
/* The same with a metric.  The arrays are taken as they are (as rq_from_arrays trusts codes and factors: `base` of a cosine
 * index holds normalised rows already); the metric only marks the index, so that its queries and added rows are normalised. */
rq_status rq_from_arrays_metric(uint32_t dim, uint64_t n, uint32_t k, const float *base,
                                const float *orthogonal, const float *centroids, const uint32_t *offsets,
                                const uint32_t *map_ids, const uint64_t *codes, const rq_factor_t *factors,
                                uint32_t metric, rq_index **out);
/* The same for an inner-product index of row length d and bound sq_bound (dim = ceil64(d + 1), else RQ_ERR_DIM_MISMATCH);
 * `base` holds augmented rows already. */
rq_status rq_from_arrays_ip(uint32_t dim, uint64_t n, uint32_t k, const float *base,
                            const float *orthogonal, const float *centroids, const uint32_t *offsets,
                            const uint32_t *map_ids, const uint64_t *codes, const rq_factor_t *factors,
                            uint32_t d, float sq_bound, rq_index **out);

rq_status rq_info(const rq_index *idx, rq_info_t *out);
/* Copy one array of the index back to host memory (sizes as in rq_from_arrays). */
enum { RQ_ARR_BASE = 0, RQ_ARR_ORTHOGONAL, RQ_ARR_CENTROIDS, RQ_ARR_OFFSETS, RQ_ARR_MAP_IDS,
       RQ_ARR_CODES, RQ_ARR_FACTORS,
       RQ_ARR_BASE_ROWS /* = 7: the stored rows of a half-precision (n * dim * 2 bytes) or byte-row (n * dim bytes) index (an f32 index: RQ_ERR_INVALID) */ };
rq_status rq_get_array(const rq_index *idx, int which, void *dst, uint64_t dst_bytes);
/* Device pointer of one array (valid until rq_free); for zero-copy hand-over to a caller that
 * already lives on the GPU.  RQ_ARR_BASE: every row at its position -- only when n_hbm == n; on a tiered index (list
 * tails in pinned host memory) or one that stores its raw vectors as split rows (option "split_rows") there is no single f32
 * device array and the call returns RQ_ERR_UNSUPPORTED (use rq_get_array for a host copy of the whole array). */
rq_status rq_get_device_ptr(const rq_index *idx, int which, const void **out_ptr, uint64_t *out_bytes);

/* ---- query: RaBitQ::query, src/rabitq.rs:268-333 --------------------------------------------- */
/* One query of `len` floats (dim must equal ceil(len/64)*64, :275).  out_dist/out_id need room for
 * topk entries; *out_n receives the number written (<= topk).  Heap ranker results come in the
 * reference's heap-internal order (src/rerank.rs:108-113); heuristic results sorted ascending. */
rq_status rq_query(const rq_index *idx, const float *query, uint32_t len, uint32_t probe,
                   uint32_t topk, int heuristic_rank, float *out_dist, uint32_t *out_id,
                   uint32_t *out_n);
/* B independent queries (row-major B x len); the form the GPU wants.  Results of query b are at
 * out_dist/out_id[b*topk ...], count in out_n[b].  Each query's result is identical to rq_query's. */
rq_status rq_query_batch(const rq_index *idx, const float *queries, uint32_t nq, uint32_t len,
                         uint32_t probe, uint32_t topk, int heuristic_rank, float *out_dist,
                         uint32_t *out_id, uint32_t *out_n);
/* Same with queries and outputs in device memory.  Every entry point that takes device pointers runs on
 * HIP streams of its own (non-blocking with respect to the caller's streams) and returns with its outputs
 * complete: inputs produced on another stream must be complete before the call (synchronise that stream). */
rq_status rq_query_batch_device(const rq_index *idx, const float *d_queries, uint32_t nq,
                                uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank,
                                float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n);
/* The same call in two halves, for callers that keep several batches in flight (a serving loop):
 * _begin enqueues the whole batch on a workspace / HIP stream of its own and returns a ticket; _end
 * waits for it, performs the (rare) survivor-buffer re-runs and the counter updates, reports the
 * call's status and frees the ticket.  Queries and outputs must stay valid and untouched in between.
 * Batches begun back to back overlap on the device: one batch's HBM-bound stages (exact rerank) run
 * beside another's compute-bound scan.  Every begun ticket must be ended exactly once.
 * Exceptions to "returns at once": (i) a batch that needs several passes (more queries than one pass holds) runs all but its last
 * pass inside _begin; (ii) on a shard-like index -- fewer than half of its lists have members, i.e. a shard carved by
 * rq_shard_index -- a pass of >= 65 536 (query, list) pairs sizes its launches by the number of pairs whose list lives here, which
 * it reads back once: _begin then returns after rotate, coarse ranking and that split have run (tens of microseconds of device
 * work), so two such batches overlap from the query quantisation on. */
typedef struct rq_ticket rq_ticket;
rq_status rq_query_batch_device_begin(const rq_index *idx, const float *d_queries, uint32_t nq,
                                      uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank,
                                      float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n,
                                      rq_ticket **out_ticket);
rq_status rq_query_batch_device_end(rq_ticket *ticket);
/* (the filtered _begin, rq_query_batch_device_begin_filtered, is declared with the filters below; _end is the same call) */

/* ---- filtered queries: answer from a subset of the index (an allow-list of vector ids) ------------------------ */
/* A filter is a set of admitted ids: the original row ids that map_ids holds (global ids on a shard carved by rq_shard_index).
 * A filtered query returns exactly what the unfiltered query returns on the SUB-INDEX: the same dim, rotation, centroids and
 * k, every list keeping only its admitted rows in their stored order (lists may become empty) -- what rq_from_arrays builds from
 * the arrays with the other rows removed.  "Exactly" covers the ids (heap-internal order for the heap ranker, ascending for the
 * heuristic one), the distance bits, out_n, the status (RQ_ERR_EMPTY where the heuristic ranker of the sub-index finds nothing)
 * and the counters: rough counts the admitted rows of the probed lists only, precise is the sub-index's, query goes up by nq.
 * The reference has no counterpart (its README lists insert / update / delete as missing).  A filter answers "which rows may be
 * returned" per query; rq_remove below takes rows out of the lists for good.  A filter describes the layout it was made on: after
 * rq_add / rq_remove on its index the filtered queries refuse it (RQ_ERR_INVALID) -- make it again.
 *
 * allow_bits: bit (id & 31) of word id >> 5 set = id admitted; ids >= nbits are not admitted (nbits <= 2^32; allow_bits may be
 * NULL when nbits == 0: nothing is admitted).  Host or device memory (bits_on_device).  The filter is made once -- one pass over
 * map_ids into a position bitmap (n / 8 bytes) and per-list admitted counts --, belongs to `idx` (used with another index:
 * RQ_ERR_INVALID), is read-only once made, may be used by concurrent queries, and must be freed before its index. */
typedef struct rq_filter rq_filter;
rq_status rq_filter_create(const rq_index *idx, const uint32_t *allow_bits, uint64_t nbits, int bits_on_device,
                           rq_filter **out);
rq_status rq_filter_rows(const rq_filter *f, uint64_t *out_admitted); /* rows of the index the filter admits */
void rq_filter_free(rq_filter *f);
/* rq_query_batch / rq_query_batch_device with a filter (filter == NULL: the unfiltered call).  Batches of <= 64 queries take the
 * small-batch path (options "small_batch", "small_batch_filtered") like unfiltered ones, with its filtered kernels; a filter too
 * sparse for a query's block to fill the ranker within its reach keeps the staged launches (the rule is under
 * "small_batch_filtered" below).  A filter keeps its own learnt survivor capacities: after calls that overflowed, its capacity can
 * exceed what the small-batch path holds (4 x 4096 records per query), and later batches of that filter then take the staged
 * launches -- with the same results. */
rq_status rq_query_batch_filtered(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq,
                                  uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank, float *out_dist,
                                  uint32_t *out_id, uint32_t *out_n);
rq_status rq_query_batch_device_filtered(const rq_index *idx, const rq_filter *filter, const float *d_queries,
                                         uint32_t nq, uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank,
                                         float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n);
/* rq_query_batch_device_begin with a filter (filter == NULL: rq_query_batch_device_begin itself); the ticket is ended by
 * rq_query_batch_device_end.  The filter is validated as by rq_query_batch_device_filtered (another index's filter, or one made
 * before a mutation: RQ_ERR_INVALID, no ticket) and travels in the ticket: _end's re-runs and capacity updates use it, so the
 * filter must outlive the ticket (free it after _end).  Returning at once: a filtered batch on the small-batch path does; a
 * filtered batch on the staged launches returns from _begin only after its pair split -- the pairs whose list admits nothing are
 * settled and the others counted, one read-back, exactly exception (ii) of rq_query_batch_device_begin. */
rq_status rq_query_batch_device_begin_filtered(const rq_index *idx, const rq_filter *filter, const float *d_queries,
                                               uint32_t nq, uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank,
                                               float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n,
                                               rq_ticket **out_ticket);

/* ---- range search: every neighbour within a per-query radius ----------------------------------------------------- */
/* For query b with radius r_b (f32, squared L2 like every distance of this header), its probe lists as the plain query ranks
 * them, and every stored row u of those lists, the answer is the SET
 *     { (accurate(b,u), id(u)) : rough(b,u) < r_b  and  accurate(b,u) < r_b }
 * with the plain query's own estimate (src/rabitq.rs:336-367) and exact distance (src/simd.rs:14-73), bit for bit: the
 * reference's ranker (src/rerank.rs:83-92) with its threshold held at r_b and no bound on the number kept.  Both comparisons are
 * strict f32 "<": a NaN radius admits nothing, r_b <= 0 returns nothing, f32::MAX returns every probed row whose two distances
 * are finite and below it.  A row whose ESTIMATE is not below r_b is left out even if its exact distance is: that is the
 * reference's gate and the documented approximation of this call (as of rq_query_batch_device_seeded).  Each query's results
 * are ascending by (distance, id).  Counters: rough += rows of the probed lists (with a filter: the admitted ones), precise +=
 * candidates with rough < r_b (admitted ones), query += nq.  An empty answer is RQ_OK with all counts 0.
 * filter: NULL = none; else the same set intersected with the admitted rows (a filter of another index or made before a
 * mutation: RQ_ERR_INVALID).  Validation otherwise as rq_query_batch_device without topk.  Any index the plain query accepts
 * is accepted (tiered, split rows, shards of rq_shard_index: ids are the original ones, a caller unites the shards' answers).
 * The library sizes the result itself -- hit counts, prefix sum, one allocation of exactly `total` entries per array; no
 * result length is bounded by anything but memory (RQ_ERR_OOM when it does not fit; the index is untouched).  On any error
 * *out is NULL.  Safe to call concurrently with other queries on the index.  rq_last_profile() is filled as by the other
 * query calls, re-runs included: retries = queries whose candidates exceeded the pass's uniform buffers and were run again on
 * their own; scan_candidates, scan_launches and the ms_* fields then hold the re-runs' scans as well (the rough counter does not:
 * it counts a probed row once); ms_sort also holds everything behind the hit counts (offsets, emission, sort, split).
 * A range call leaves no trace in how later top-k calls on the index run (their learnt buffer sizes and scan gate).
 * rq_range_search_device: queries (nq x len) and radii (nq) in device memory; rq_range_search: both in host memory.
 * The result owns three DEVICE arrays, valid until it is freed: lims, nq + 1 u64 (lims[0] = 0, lims[nq] = total), and dist /
 * id, `total` entries each; query b's results are entries [lims[b], lims[b + 1]).  rq_range_result_copy copies them to host
 * arrays of those sizes (dist / id may be NULL when total == 0).  Free the result before its index;
 * rq_range_result_free(NULL) is a no-op. */
typedef struct rq_range_result rq_range_result;
rq_status rq_range_search_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq,
                                 uint32_t len, uint32_t probe, const float *d_radius, rq_range_result **out);
rq_status rq_range_search(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                          uint32_t probe, const float *radius, rq_range_result **out);
rq_status rq_range_result_info(const rq_range_result *r, uint32_t *out_nq, uint64_t *out_total);
rq_status rq_range_result_device_ptrs(const rq_range_result *r, const uint64_t **d_lims, const float **d_dist,
                                      const uint32_t **d_id);
rq_status rq_range_result_copy(const rq_range_result *r, uint64_t *lims, float *dist, uint32_t *id);
void rq_range_result_free(rq_range_result *r);

/* ---- exact search: brute-force top-k over the stored rows (later in 0.11, additions only) --------------------------- */
/* The true nearest neighbours, on the GPU: what the approximate entries above are measured against.  Queries are raw, exactly as
 * rq_query_batch_device takes them (the same `len` rules; a cosine index normalises them, an inner-product index pads the zero
 * coordinate); let q' be the padded, transformed query the rerank sees.  For a stored row r let e(r) be the value rq_rerank returns
 * for the row's position against q' (the src/simd.rs:14-73 order).  The result of query b is, of the stored rows the filter admits
 * (filter == NULL: all rows) whose e(r) is below f32::MAX -- the query's own rule: a row at inf / NaN is never returned --, the topk
 * smallest by (Ord32(e), id), ascending, as (distance, id); out_n[b] = how many there are (<= topk); slots past out_n[b] are left
 * untouched, as the top-k query leaves them.  Distances are in the index's space, like the query's: |x - q|^2, 2 - 2 cos for cosine,
 * S + |q|^2 - 2<x, q> for inner product (rq_ip_from_dist converts).  The result does not depend on `params`, on options, on the
 * batch size or on how the work was split.
 * Accepted: L2 / cosine / inner-product indexes whose raw vectors are all in HBM as plain f32, f16 / bf16 or u8 / i8 rows; shards of
 * rq_shard_index (ids are their map_ids); mutated indexes.  filter: as validated by the filtered query (another index's, or one made
 * before a mutation: RQ_ERR_INVALID).  topk in [1, 2048] and dim <= 4096, else RQ_ERR_UNSUPPORTED; a null pointer: RQ_ERR_INVALID;
 * a tiered index (list tails in host memory) or a split-row index: RQ_ERR_UNSUPPORTED with nothing allocated.  nq == 0 is RQ_OK.  An
 * index or filter with no admitted row returns out_n = 0 everywhere with the status of the filtered query (RQ_OK).
 * A row whose squared norm is not a finite f32 (overflow included) is never judged by the approximation below: it always gets its
 * exact distance, so it is returned exactly when its e is below f32::MAX and among the topk smallest, like any other row.
 * Method: (1) a bound T_b >= the topk-th smallest e: the topk-th smallest exact distance over a sample of the admitted
 * rows (every stride-th position, about sqrt(rows x topk) of them; f32::MAX where the sample holds fewer than topk admitted rows);
 * (2) one pass over the rows that approximates every (query, row) distance with bf16 matrix-core products and keeps the pairs within
 * a proven margin of T_b; (3) the exact distance of those pairs and the selection.  The bound changes the work, never the answer.
 * The call touches no counter of rq_metrics.  Dimensions above 2432 run without (1) and (2): every admitted pair gets its exact
 * distance.
 * rq_exact_search_device: queries (nq x len) and outputs (nq x topk, nq x topk, nq) in device memory; rq_exact_search: host memory.
 * params (nullable; sized struct, zero = automatic; TEST HOOKS, results never depend on them): seed_probe = sample rows of the bound
 * per topk (the sample has seed_probe x topk rows); cand_per_query = initial candidate slots per query (a pass whose candidates overflow them is run again with the count it
 * learnt); flags bit 0 = no seed (every bound is f32::MAX), bit 1 = no pre-filter (the exact distance of every admitted pair).
 * rq_last_exact_stats: the calling thread's last exact search -- device time (ms, summed over launches) of the bound (ms_seed: the
 * sample's exact distances and selection), the scan, the exact distances and the selection; seed_probe = rows of the sample (0: no
 * bound was made); seed_unfilled = queries whose bound is f32::MAX; candidates = pairs the scan kept; exact = exact distances
 * computed, the sample's included; reruns = scan launches repeated because a query's candidates did not fit its slots (the capacity
 * learnt is remembered with the index or filter: a later call starts from it); row_bytes_read = bytes of raw rows the scan launches
 * covered (algorithmic: n x row bytes per launch; a batch of up to 4096 queries is ONE launch, re-runs count again); scan_launches =
 * those launches; scan_subtiles = 32-row sub-tiles per block of those launches' scan (4, 2 or 1 by dimension; 0: the scan ran without
 * the pre-filter -- flags bit 1, or a dimension above 2432).  A launch that overflowed stops behind the scan: nothing is computed
 * or written from its candidates. */
typedef struct {
    uint32_t struct_size; /* in: sizeof(rq_exact_params_t) */
    uint32_t seed_probe;
    uint32_t cand_per_query;
    uint32_t flags;
} rq_exact_params_t;
typedef struct {
    uint32_t struct_size; /* in: sizeof(rq_exact_stats_t) of the caller */
    uint32_t seed_probe;
    float ms_seed, ms_scan, ms_exact, ms_select;
    uint32_t seed_unfilled;
    uint32_t reruns;
    uint64_t candidates;
    uint64_t exact;
    uint64_t row_bytes_read;
    uint32_t scan_launches;
    uint32_t scan_subtiles; /* 4, 2 or 1; 0 = the scan ran without the pre-filter (was reserved0, always 0) */
} rq_exact_stats_t;
rq_status rq_exact_search_device(const rq_index *idx, const rq_filter *filter /* nullable */, const float *d_queries, uint32_t nq,
                                 uint32_t len, uint32_t topk, const rq_exact_params_t *params /* nullable */, float *d_out_dist,
                                 uint32_t *d_out_id, uint32_t *d_out_n);
rq_status rq_exact_search(const rq_index *idx, const rq_filter *filter /* nullable */, const float *queries, uint32_t nq, uint32_t len,
                          uint32_t topk, const rq_exact_params_t *params /* nullable */, float *out_dist, uint32_t *out_id,
                          uint32_t *out_n);
rq_status rq_last_exact_stats(rq_exact_stats_t *out);

/* ---- exact range search: every stored row within a per-query radius (later in 0.11, additions only) ----------------- */
/* What rq_range_search* is measured against, as rq_exact_search* is for the top-k entries.  Queries are raw, exactly as
 * rq_exact_search_device takes them (the same `len` rules; cosine normalised, inner product padded); q' and e(r) as defined there.
 * The answer of query b is the SET
 *     { (e(r), id(r)) : r admitted by the filter (NULL: every stored row),  e(r) < radius_b,  e(r) < f32::MAX }
 * with both comparisons strict f32 "<", the comparison rq_range_search uses: a NaN radius or a radius <= 0 admits nothing, +inf and
 * f32::MAX admit every admitted row whose e is below f32::MAX.  Each query's entries ascend by (distance, id).  The result does not
 * depend on `params`, on options, on the batch size or on how the work was split.
 * The result is an ordinary rq_range_result (lims nq + 1 u64, dist / id of exactly `total` entries), served by
 * rq_range_result_info / _device_ptrs / _copy / _free; on any error *out is NULL and nothing stays allocated.  nq == 0 behaves as
 * rq_range_search does.  An index or filter with no admitted row gives all counts 0 with RQ_OK.
 * Accepted and refused as rq_exact_search*: L2 / cosine / inner-product indexes, f32, f16 / bf16, u8 / i8 rows, shards of
 * rq_shard_index (ids are their map_ids), mutated indexes; tiered and split-row indexes: RQ_ERR_UNSUPPORTED before anything is
 * allocated; a foreign or stale filter: RQ_ERR_INVALID; dim <= 4096.  No counter of rq_metrics is touched, and no trace is left in
 * how later top-k, range or exact top-k calls run (the capacity this call learns is a hint of its own).
 * Method: the exact search's scan with T_b = radius_b -- no sample, no seed pass -- appending the kept (query, row)
 * pairs to one arena per launch; one pass over the arena for the exact distances, keys and per-query hit counts; prefix sum, one
 * allocation of exactly the hits, scatter into per-query segments; the range search's segment sort and key split.  A launch whose
 * pairs overflow its arena is run again with the count it learnt (nothing downstream runs on an overflowed launch); a group whose
 * arena would exceed the slot budget is split, down to one query; a single query that still does not fit is RQ_ERR_OOM.
 * params (nullable; the struct and the refusal of unknown flag bits of rq_exact_search; TEST HOOKS): flags bit 1 = no pre-filter
 * (every admitted pair gets its exact distance; also what dimensions above 2432 run); flags bit 0 and seed_probe are accepted and
 * have no effect (there is no sample); cand_per_query = initial arena records of a launch per query of that launch; zero = automatic.
 * rq_last_exact_stats is filled by these calls too: seed_probe = 0, ms_seed = 0, seed_unfilled = 0; ms_scan; ms_exact; ms_select =
 * everything behind the exact distances (counts, offsets, scatter, sort, split); candidates = pairs the scan kept; exact =
 * candidates; reruns, scan_launches and row_bytes_read as above. */
rq_status rq_exact_range_search_device(const rq_index *idx, const rq_filter *filter /* nullable */, const float *d_queries,
                                       uint32_t nq, uint32_t len, const float *d_radius,
                                       const rq_exact_params_t *params /* nullable */, rq_range_result **out);
rq_status rq_exact_range_search(const rq_index *idx, const rq_filter *filter /* nullable */, const float *queries, uint32_t nq,
                                uint32_t len, const float *radius, const rq_exact_params_t *params /* nullable */,
                                rq_range_result **out);

/* ---- adaptive probing: each query's probe list cut by centroid distance (later in 0.11, additions only) ----------------- */
/* Every query of a plain call visits `probe` lists; these entries let each query stop where its centroids stop being near.
 * Let d_0 <= d_1 <= ... <= d_{m-1}, m = min(probe, k), be the query's coarse distances in visiting order (the f32 values the
 * coarse ranking produces, what rq_coarse_rank returns).  The rule:
 *     t = ratio * d_0            one f32 multiplication, round to nearest; ratio = +inf: t = +inf
 *     p = length of the longest prefix whose entries all satisfy d_j <= t   (a NaN compares false)
 *     n = min(cap, max(min_probe, p)), clamped to [1, m];  cap = max_probe[query] clamped to [1, m], or m without the array
 * The query visits its first n lists and no others: its ids, distance bits, count, status and its contribution to the rough /
 * precise counters of rq_metrics are bit for bit those of the same entry called with probe = n, for both rankers.  ratio = +inf
 * (or min_probe >= m) cuts nothing; max_probe with ratio = +inf is a per-query nprobe for callers with a rule of their own.
 * Refused with RQ_ERR_INVALID: a NULL rule, struct_size != sizeof(rq_probe_rule_t), ratio NaN or negative, min_probe == 0,
 * reserved != 0, and whatever the plain entry refuses (NULL outputs among them; out_nprobe alone may be NULL).
 * Accepted wherever the plain (or filtered) entry is: every metric and row type, tiered, split-row and mutated indexes, any nq
 * (a call of more than 65 536 queries applies the rule in every pass).  A call with a rule runs the staged launches at any batch
 * size (never the few-launch path of batches <= 64 queries) and is planned like a call over caller-supplied probe lists
 * (DESIGN 4.15).  Not offered with a rule yet: tickets (_begin / _end), the sharded step, range search. */
typedef struct {
    uint32_t struct_size;       /* in: sizeof(rq_probe_rule_t) */
    uint32_t min_probe;         /* >= 1 */
    float    ratio;             /* >= 0 or +inf */
    uint32_t reserved;          /* 0 */
    const uint32_t *max_probe;  /* nullable; nq entries; device memory for the _device entries, host memory otherwise */
} rq_probe_rule_t;
rq_status rq_query_batch_device_adaptive(const rq_index *idx, const rq_filter *filter /* nullable */, const float *d_queries,
                                         uint32_t nq, uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank,
                                         const rq_probe_rule_t *rule, float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n,
                                         uint32_t *d_out_nprobe /* nullable; nq: the lists each query visited */);
rq_status rq_query_batch_adaptive(const rq_index *idx, const rq_filter *filter /* nullable */, const float *queries,
                                  uint32_t nq, uint32_t len, uint32_t probe, uint32_t topk, int heuristic_rank,
                                  const rq_probe_rule_t *rule, float *out_dist, uint32_t *out_id, uint32_t *out_n,
                                  uint32_t *out_nprobe /* nullable; nq: the lists each query visited */);
/* Only the query transform, the rotation, the coarse ranking and the cut: d_out_nprobe[b] = n of query b under the rule.  The cheap
 * way to look at a rule's distribution before paying for the scans; no counter of rq_metrics moves. */
rq_status rq_probe_counts_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len, uint32_t probe,
                                 const rq_probe_rule_t *rule, uint32_t *d_out_nprobe);

/* ---- in-place mutation: add and remove rows ------------------------------------------------------------------------ */
/* After any sequence of rq_add / rq_remove the index equals, bit for bit, the index rq_build produces from its live rows S in
 * ascending id order (same centroids and rotation) with every map_ids entry j replaced by the j-th smallest id of S: every array
 * rq_get_array returns, rq_info's n / max_list_len, rq_dump_dir's files and the results and counters of every query.  Each call is
 * one relayout into fresh arrays (the old and the new arrays coexist for its duration: RQ_ERR_OOM when they do not fit), moved into
 * the index only when everything has succeeded: on any error the index is unchanged.  The first mutation of an index (and the
 * first after a load) also derives a 4-byte key per stored row, kept with the index from then on.
 * Refused with RQ_ERR_UNSUPPORTED, index untouched: tiered indexes, split-row indexes, shards made by rq_shard_index.  Refused with
 * RQ_ERR_INVALID: an index with a rq_query_batch_device_begin ticket whose _end has not run.  No query may run on the index while
 * it is mutated (the caller serialises, as Rust's &mut self does).  Workspaces and tile tables of the old layout are released.
 *
 * On a cosine index rq_add normalises the new rows, and the invariant reads: the index equals rq_build_metric(live ORIGINAL
 * rows, RQ_METRIC_COSINE).  On an inner-product index rq_add takes rows of the index's d floats and augments them with the
 * index's S; a row with s > S or a non-finite s is RQ_ERR_INVALID with the index untouched; the invariant reads: the index
 * equals rq_build_ip(live ORIGINAL rows, the same S).
 * rq_add: insert m rows (m x d f32, row-major; host or device memory per rows_on_device).  d must pad to the index's dim
 * (ceil64(d) == dim), else RQ_ERR_DIM_MISMATCH.  ids: NULL = the next ids, first = 1 + the largest id the index holds (0 if
 * empty), returned in *out_first_id (RQ_ERR_UNSUPPORTED if the last would pass 2^32 - 1); else m explicit u32 ids in the same
 * memory as the rows, each absent from the index and unique in the batch (else RQ_ERR_INVALID; *out_first_id = the smallest).
 * Removing and then adding an id with a new vector is an update (two relayouts).  m == 0 changes nothing.
 * rq_remove: remove the ids set in the bitmap (the rq_filter_create format: bit (id & 31) of word id >> 5, nbits <= 2^32, host or
 * device memory per bits_on_device); ids that are not in the index are ignored; *out_removed = rows removed (0: nothing changed).
 * Precondition of rq_add: every list of the index is in the build's order -- strictly ascending by (distance of the row to the
 * list's centroid, as the build computes it; then id).  Indexes made by rq_build* and rq_add, and their dumps, are; an index given
 * to rq_from_arrays / rq_load_dir may not be (for example one whose map_ids were remapped to other ids).  The order is checked on
 * the first mutation of an index (with its keys); where it does not hold, rq_add returns RQ_ERR_UNSUPPORTED with the index
 * untouched, and rq_remove still works (it keeps the order the lists have).  Indexes of dim > 4096 are refused (RQ_ERR_UNSUPPORTED).
 * rq_last_mutate_stats: the calling thread's last rq_add / rq_remove, by phase (wall ms; every phase ends in a device
 * synchronisation): keys = deriving the key cache and checking the order (0 when cached), assign = pass 1 + per-list sort of the
 * new rows, alloc = the new layout's arrays, merge, gather, derive = finish_index and the shadow / pass budget decided again after
 * the old layout is freed, free = releasing the old layout; total = the whole call; gather_bytes = what the gather reads + writes. */
typedef struct {
    uint32_t struct_size; /* set to sizeof(rq_mutate_stats_t) before the call */
    uint32_t reserved0;
    float ms_keys, ms_assign, ms_alloc, ms_merge, ms_gather, ms_derive, ms_free, ms_total;
    uint64_t rows_before, rows_after;
    uint64_t gather_bytes;
} rq_mutate_stats_t;
rq_status rq_add(rq_index *idx, const float *rows, uint64_t m, uint32_t d, const uint32_t *ids, int rows_on_device,
                 uint32_t *out_first_id);
rq_status rq_remove(rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, uint64_t *out_removed);
rq_status rq_last_mutate_stats(rq_mutate_stats_t *out);

/* ---- lazy removal: mark rows dead without a relayout, compact later ------------------------------------------------------- */
/* Let D be the ids marked dead since the last relayout (the pending removals).  An index with pending removals answers every query
 * entry that has a filtered form as the same index after rq_remove(D) would, bit for bit: ids in order, distance bits, counts,
 * status and the rough / precise / query counters of rq_metrics.  The dead rows stay stored; the index owns a filter of its live
 * rows and every such entry runs under it (or under the caller's filter, which excludes the dead rows already).  rq_compact
 * turns the index into rq_remove(D)'s: arrays, rq_info, dump files.  An index without pending removals behaves as before.
 * rq_remove_lazy: mark the ids set in the bitmap (rq_remove's format and limits).  Ids the index does not hold and ids already
 *   dead are ignored; *out_marked (nullable) = rows newly dead (0: nothing changed).  One pass over the ids on the device, n / 8
 *   bytes written: no relayout, no second copy of the arrays; the generation is not bumped, tile tables, workspaces and learnt
 *   hints stay.  A call that marks anything bumps the index's removal epoch: filters made before it are refused with
 *   RQ_ERR_INVALID (make them again); a call that marks nothing leaves them valid.  Accepted on every index that accepts a
 *   filter: every metric and row type, tiered and split-row indexes, mutated and merged ones, lists out of the build's order.
 *   Refused, index unchanged: RQ_ERR_UNSUPPORTED a shard made by rq_shard_index; RQ_ERR_INVALID a null handle (checked before the
 *   device is looked for), nbits > 2^32, a null bitmap with nbits > 0, a rq_query_batch_device_begin ticket that has not ended.
 *   No query may run during the call.
 * rq_compact: rq_remove of the pending removals in one relayout; *out_removed (nullable) = rows dropped.  With none pending it
 *   succeeds and changes nothing, the generation included.  It has rq_remove's refusals: a half-precision, byte-row, tiered or
 *   split-row index answers RQ_ERR_UNSUPPORTED and keeps its pending removals (until it is rebuilt).  rq_last_mutate_stats reports
 *   it as a remove.
 * rq_pending_removals: *out_dead = stored rows that are dead.  rq_info.n stays the stored row count.
 * With removals pending:
 *   rq_query*, rq_query_batch* (plain, _device, _begin / _end, _adaptive), rq_range_search*, rq_exact_search*,
 *     rq_exact_range_search* with filter == NULL run under the live filter: the filtered pass, that filter's own hints, the
 *     small-batch rule of filtered batches with the live filter's density;
 *   rq_filter_create admits allowed AND live rows (rq_filter_rows counts those);
 *   rq_probe_counts_device, rq_coarse_rank, rq_rotate*, rq_query_prep are unchanged (they read no row);
 *   rq_remove drops the pending and the requested rows in one relayout (*out_removed counts the rows that were live);
 *   rq_add and rq_merge_from with such a dst compact first (one more relayout; rq_last_mutate_stats adds the phases up; on an
 *     error the index is as it was or compacted, a pending removal is never lost); rq_merge_from with such a src is
 *     RQ_ERR_UNSUPPORTED (src is never written: compact it or extract its live rows first);
 *   rq_extract keeps requested AND live rows;
 *   rq_dump_dir, rq_dump_json, rq_shard_index, rq_query_batch_device_probed, _seeded and rq_query_batch_sharded_device answer
 *     RQ_ERR_UNSUPPORTED ("pending removals: rq_compact first"): they have no filtered form, and a dump would bring the dead rows back;
 *   rq_get_array, rq_get_device_ptr, rq_scan, rq_rerank, rq_quantize_pack see the stored rows, dead ones included. */
rq_status rq_remove_lazy(rq_index *idx, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, uint64_t *out_marked);
rq_status rq_compact(rq_index *idx, uint64_t *out_removed);
rq_status rq_pending_removals(const rq_index *idx, uint64_t *out_dead);

/* ---- rows by id: locate, fetch, exact distances to known ids, the neighbours of a stored row ------------------------------- */
/* Every entry here takes u32 ids, the ids the queries return and the mutations name, and reads the index: no array, hint, option
 * or counter of the index changes, so they are allowed on every index -- every metric and row type, tiered and split-row indexes,
 * shards of rq_shard_index (their ids are global: an id of another shard is absent), with removals pending (a dead row's id is
 * absent) and while rq_query_batch_device_begin tickets are open.  An id the index does not hold is ABSENT; absence is an answer,
 * not an error.  Ids may repeat in a request.  No relayout (rq_add, rq_remove, rq_compact, rq_merge_from) may run during a call.
 * Behind them sits the index's id directory, id -> position: made on the first by-id call after the index was made or last
 * relaid out (one pass over the ids), kept until the next relayout, never touched by a query.  It is a u32 array over the ids
 * below top = 1 + the largest stored id where top <= 4 n + 65536 (4 * top bytes), else a hash table of the power of two >= 2 n
 * 64-bit slots (16 to 32 bytes per row); rq_last_by_id_stats says which.  An index that is never asked by id pays nothing.
 * Each entry has a host-pointer form and a _device form (every pointer in device memory, 16-byte aligned row outputs; it returns
 * with its outputs complete).  m == 0 succeeds and touches nothing.  Refused with RQ_ERR_INVALID before a device is looked for:
 * a null index, a null ids or output pointer with m > 0 (nq > 0, c > 0).
 * rq_locate: out_pos[i] = the cluster-order position of ids[i] (what rq_rerank takes and rq_get_array's rows are ordered by), or
 *   RQ_POS_ABSENT.  A position is valid until the next relayout.
 * rq_fetch_rows: out_rows (m x dim f32) row i = the row RQ_ARR_BASE holds at that position, bit for bit -- W(stored) of a
 *   half-precision or byte row, the joined planes of a split row, either tier of a tiered index, the normalised row of a cosine
 *   index, the augmented row of an inner-product index; out_found[i] = 1.  An absent id: a row of zeros, out_found[i] = 0.
 *   out_found is nullable.
 * rq_fetch_stored: the same rows as RQ_ARR_BASE_ROWS holds them, dim x elem_bytes bytes per row (an absent id: zero bytes); an
 *   index of f32 rows answers RQ_ERR_INVALID, as rq_get_array(RQ_ARR_BASE_ROWS) does.
 * rq_pair_distances: query i (nq x length, raw: it goes through the index's query transform and padding as in every query entry)
 *   against its own c ids, ids[i * c .. i * c + c) -> out_dist[i * c + j], bit for bit what rq_rerank returns for that id's
 *   position and the prepared query; an absent id gives +inf.  (An inner-product index: the L2 distance to the augmented row, as
 *   every entry returns it; rq_ip_from_dist converts.)
 * rq_neighbours_of: the neighbours of stored rows.  Let L = the inner-product index's d, else dim, and q_i = the first L floats
 *   of rq_fetch_rows(ids[i]).  Row i of the outputs (m x topk) is row i of rq_query_batch[_filtered](q, probe, topk + 1,
 *   heuristic_rank, filter) with one entry removed: the first whose id equals ids[i], or, if there is none (the row is outside the
 *   probed lists or the filter, or the ranker dropped it), the last one.  The remaining entries keep the plain call's order; a row
 *   with fewer than topk of them is padded with NaN / 0xFFFFFFFF, and so is the whole row of an absent id (out_found[i] = 0).
 *   filter == NULL with removals pending: the live filter, as in the plain entry.  Status and refusals are the plain entry's at
 *   topk + 1 (so topk <= 2047; RQ_ERR_EMPTY after a heuristic call that left a row empty, outputs written), rq_metrics counts the
 *   plain call.  On the device: lookup, gather into the query buffer, the plain entry's driver, one kernel that drops the entry.
 * rq_neighbours_of_exact: the same over rq_exact_search(q, topk + 1, filter, params) -- ascending by (distance, id), so the row
 *   itself comes first unless a bitwise-equal row has a smaller id; refused where the exact search is (tiered and split-row
 *   indexes: RQ_ERR_UNSUPPORTED).  params as in rq_exact_search (nullable).
 * rq_last_by_id_stats: the calling thread's last by-id call. */
#define RQ_POS_ABSENT 0xFFFFFFFFu
enum { RQ_DIRECTORY_NONE = 0, RQ_DIRECTORY_DENSE = 1, RQ_DIRECTORY_HASH = 2 };
typedef struct {
    uint32_t struct_size;      /* set to sizeof(rq_by_id_stats_t) before the call */
    uint32_t form;             /* RQ_DIRECTORY_* of the directory the call used */
    uint64_t directory_bytes;  /* device memory it takes */
    float ms_build;            /* wall ms its build took (whichever call made it), the scan for the largest id included */
    uint32_t longest_chain;    /* hash form: slots the longest insertion looked at while building (1 = every id in its home slot) */
    uint64_t found, absent;    /* ids of the call that have / do not have a live row */
    uint64_t gather_bytes;     /* the row gather of the call: every found row read once + every destination row written once, + the positions */
    float ms_gather;           /* device ms of that gather (0: the call gathers no rows) */
    float ms_lookup;           /* device ms of the id lookup */
    uint32_t built;            /* 1: this call made the directory */
    uint32_t reserved0;
} rq_by_id_stats_t;
rq_status rq_locate(const rq_index *idx, const uint32_t *ids, uint64_t m, uint32_t *out_pos);
rq_status rq_locate_device(const rq_index *idx, const uint32_t *d_ids, uint64_t m, uint32_t *d_out_pos);
rq_status rq_fetch_rows(const rq_index *idx, const uint32_t *ids, uint64_t m, float *out_rows, uint32_t *out_found);
rq_status rq_fetch_rows_device(const rq_index *idx, const uint32_t *d_ids, uint64_t m, float *d_out_rows, uint32_t *d_out_found);
rq_status rq_fetch_stored(const rq_index *idx, const uint32_t *ids, uint64_t m, void *out_rows, uint32_t *out_found);
rq_status rq_fetch_stored_device(const rq_index *idx, const uint32_t *d_ids, uint64_t m, void *d_out_rows, uint32_t *d_out_found);
rq_status rq_pair_distances(const rq_index *idx, const float *queries, uint32_t nq, uint32_t length, const uint32_t *ids, uint32_t c,
                            float *out_dist);
rq_status rq_pair_distances_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t length, const uint32_t *d_ids,
                                   uint32_t c, float *d_out_dist);
rq_status rq_neighbours_of(const rq_index *idx, const uint32_t *ids, uint32_t m, uint32_t probe, uint32_t topk, int heuristic_rank,
                           const rq_filter *filter, float *out_dist, uint32_t *out_ids, uint32_t *out_found);
rq_status rq_neighbours_of_device(const rq_index *idx, const uint32_t *d_ids, uint32_t m, uint32_t probe, uint32_t topk,
                                  int heuristic_rank, const rq_filter *filter, float *d_out_dist, uint32_t *d_out_ids,
                                  uint32_t *d_out_found);
rq_status rq_neighbours_of_exact(const rq_index *idx, const uint32_t *ids, uint32_t m, uint32_t topk, const rq_filter *filter,
                                 const rq_exact_params_t *params, float *out_dist, uint32_t *out_ids, uint32_t *out_found);
rq_status rq_neighbours_of_exact_device(const rq_index *idx, const uint32_t *d_ids, uint32_t m, uint32_t topk, const rq_filter *filter,
                                        const rq_exact_params_t *params, float *d_out_dist, uint32_t *d_out_ids,
                                        uint32_t *d_out_found);
rq_status rq_last_by_id_stats(rq_by_id_stats_t *out);

/* ---- attribute columns: per-row values, and predicates over them as filters (0.15.0, additions only) ------------------------- */
/* An index may carry up to RQ_ATTR_MAX_COLUMNS named columns of per-row values.  A name is 1-31 bytes of [A-Za-z0-9_], unique per
 * index.  Types: RQ_ATTR_U32, _I32, _F32 (4 bytes), RQ_ATTR_U64, _I64 (8 bytes); rq_attr_value_t is the 8-byte union of the five (a
 * 4-byte value lies in its low 4 bytes; the library ignores the others).  A column is one device array of n x elem bytes in
 * POSITION order: element p belongs to the row at cluster-order position p, beside map_ids[p].  Every column has a fill value;
 * a row holds it until it is set.  The reference has no counterpart.  An index without columns behaves, allocates and dumps
 * exactly as before.
 * rq_attr_create: a new column, every row holding `fill`.  rq_attr_drop: the column goes, the indexes (rq_attr_info order) of the
 *   later columns move down by one.  rq_attr_count / rq_attr_info (a sized struct; bytes = n x elem) / rq_attr_index (name -> index).
 * rq_attr_set[_device]: values[i] (m elements of the column's type) becomes the value of the row with id ids[i]: ids -> positions
 *   through the id directory, as rq_locate, then a scatter.  An id the index does not hold, or a dead one (rq_remove_lazy), is
 *   absent: counted in *out_absent (nullable), not an error.  When an id repeats in the request the LAST occurrence wins, and not
 *   by store order: a first pass gives every asked position to the highest request index that names it (an integer atomic max on a
 *   per-position owner word), a second pass stores only the values whose request index owns their position.  m < 2^32 - 1.
 *   The call changes values, not positions: no generation is bumped, and existing filters stay valid -- a filter is the set its
 *   predicate selected when it was made.
 * rq_attr_get[_device]: out_values[i] = the value of ids[i], out_found[i] (nullable) = 1; an absent id gives the fill value and 0.
 * rq_attr_get_array: the whole column in position order (dst_bytes = n x elem): the counterpart of rq_get_array(RQ_ARR_MAP_IDS).
 * Host forms take host pointers; _device forms take device pointers and return with their outputs complete.  m == 0 succeeds.
 * Columns do not depend on how the raw vectors are stored: these entries are accepted on every metric and row type, tiered and
 * split-row indexes, shards of rq_shard_index, indexes with pending removals and with open tickets.  No query may run during
 * rq_attr_set, rq_attr_create or rq_attr_drop.
 * Refused with RQ_ERR_INVALID before a device is looked for: a null index, name, or (m > 0) ids / values / out_values; a malformed
 * name; an unknown type.  RQ_ERR_INVALID: a name the index already has (create) or does not have; RQ_ERR_UNSUPPORTED: a 17th column.
 *
 * Columns follow their rows.  Every relayout (rq_add, rq_remove, rq_compact, rq_merge_from; rq_extract and so a copy) moves each
 * column with one gather driven by the relayout's own destination-to-source map: a row keeps its value.  The rows of an rq_add
 * hold the fill value.  rq_merge_from: rows of src bring src's value where src has a column of the same name and type, else they
 * hold dst's fill; the same name with another type is refused with RQ_ERR_INVALID, both indexes untouched; columns that only src
 * has are NOT taken (create them on dst first).  rq_extract gives the new index every column of src; rq_shard_index gives a shard
 * every column (each owned list's slice).  rq_last_mutate_stats.gather_bytes counts each column element read once and written once.
 * Persistence: an index with columns writes into rq_dump_dir one more text file `attrs`, one line "<name> <type id> <fill as 16
 * hex digits>\n" per column in rq_attr_info order, and per column one raw little-endian file `attr.<name>` of n x elem bytes in
 * position order; rq_load_dir restores the columns when `attrs` is there (a missing or wrongly sized data file, or a malformed
 * line: RQ_ERR_IO).  An index without columns writes exactly the files it wrote before.  rq_dump_json of an index with columns is
 * RQ_ERR_UNSUPPORTED (JSON is the debugging format). */
#define RQ_ATTR_MAX_COLUMNS 16u
enum { RQ_ATTR_U32 = 0, RQ_ATTR_I32 = 1, RQ_ATTR_F32 = 2, RQ_ATTR_U64 = 3, RQ_ATTR_I64 = 4 };
typedef union {
    uint32_t u32;
    int32_t i32;
    float f32;
    uint64_t u64;
    int64_t i64;
} rq_attr_value_t;
typedef struct {
    uint32_t struct_size; /* set to sizeof(rq_attr_info_t) before the call */
    uint32_t type;        /* RQ_ATTR_* */
    char name[32];        /* zero-terminated */
    rq_attr_value_t fill;
    uint64_t bytes;       /* n x elem: the size of the column (and of rq_attr_get_array's dst) */
} rq_attr_info_t;
rq_status rq_attr_create(rq_index *idx, const char *name, uint32_t type, rq_attr_value_t fill);
rq_status rq_attr_drop(rq_index *idx, const char *name);
rq_status rq_attr_count(const rq_index *idx, uint32_t *out);
rq_status rq_attr_info(const rq_index *idx, uint32_t i, rq_attr_info_t *out);
rq_status rq_attr_index(const rq_index *idx, const char *name, uint32_t *out);
rq_status rq_attr_set(rq_index *idx, const char *name, const uint32_t *ids, const void *values, uint64_t m, uint64_t *out_absent);
rq_status rq_attr_set_device(rq_index *idx, const char *name, const uint32_t *d_ids, const void *d_values, uint64_t m, uint64_t *out_absent);
rq_status rq_attr_get(const rq_index *idx, const char *name, const uint32_t *ids, uint64_t m, void *out_values, uint32_t *out_found);
rq_status rq_attr_get_device(const rq_index *idx, const char *name, const uint32_t *d_ids, uint64_t m, void *d_out_values, uint32_t *d_out_found);
rq_status rq_attr_get_array(const rq_index *idx, const char *name, void *dst, uint64_t dst_bytes);

/* Predicates to filters.  rq_filter_create_where evaluates a boolean expression over the columns for every stored row, on the
 * device, and returns an ordinary rq_filter of the rows it holds for (AND the live rows, where removals are pending): everything
 * that takes a filter takes it, it carries the index's current generation and removal epoch, and it is freed by rq_filter_free.
 * A term compares one column (its index in rq_attr_info order: rq_attr_index) with constants: RQ_WHERE_EQ, _NE, _LT, _LE, _GT, _GE
 * against a; RQ_WHERE_BETWEEN: a <= v <= b; RQ_WHERE_IN: v == s for one of the set_count <= RQ_WHERE_MAX_SET values at `set` (host
 * memory, elements of the column's type; the library sorts and uploads them; an empty set holds for no row); RQ_WHERE_ANY_BITS:
 * (v & a) != 0; RQ_WHERE_ALL_BITS: (v & a) == a -- the two bit ops on integer columns only.  Comparisons are the column type's own:
 * unsigned for U32 / U64, signed for I32 / I64, IEEE for F32 (a NaN value or constant fails everything but NE; -0 == +0).
 * `program` is a postfix string of ntokens one-byte tokens: a value below RQ_WHERE_MAX_TERMS pushes that term's truth value,
 * RQ_WHERE_AND / _OR pop two and push one, RQ_WHERE_NOT negates the top.  At most 32 terms, 64 tokens, stack depth 32; the program
 * must end at depth 1.  program == NULL: the AND of all terms.  nterms == 0 (with program == NULL): every row holds.
 * Refused with RQ_ERR_INVALID (before a device is looked for where no field of the index is needed): null arguments, nterms or
 * ntokens past the limits, an unknown op or token, a program that underflows, overflows depth 32 or does not end at depth 1, an IN
 * term with a null set and set_count > 0 or with more than RQ_WHERE_MAX_SET values; then an unknown column, an op the column's
 * type does not have, a predicate that reads more than RQ_WHERE_MAX_COLUMNS distinct columns.
 * On the device: one kernel streams the referenced columns (n x elem bytes each, coalesced) and writes the position bitmap, 64
 * positions per wave ballot; then the steps of rq_filter_create.  No id bitmap, no upload, no read through map_ids.
 * rq_last_where_stats: the calling thread's last rq_filter_create_where. */
enum { RQ_WHERE_EQ = 0, RQ_WHERE_NE, RQ_WHERE_LT, RQ_WHERE_LE, RQ_WHERE_GT, RQ_WHERE_GE, RQ_WHERE_BETWEEN, RQ_WHERE_IN,
       RQ_WHERE_ANY_BITS, RQ_WHERE_ALL_BITS };
#define RQ_WHERE_MAX_TERMS   32u
#define RQ_WHERE_MAX_TOKENS  64u
#define RQ_WHERE_MAX_COLUMNS 8u
#define RQ_WHERE_MAX_SET     4096u
#define RQ_WHERE_AND 0x80u
#define RQ_WHERE_OR  0x81u
#define RQ_WHERE_NOT 0x82u
typedef struct {
    uint32_t column;       /* index of the column in rq_attr_info order */
    uint32_t op;           /* RQ_WHERE_EQ .. RQ_WHERE_ALL_BITS */
    rq_attr_value_t a, b;  /* the constants (b: RQ_WHERE_BETWEEN only) */
    const void *set;       /* RQ_WHERE_IN: set_count elements of the column's type, host memory */
    uint32_t set_count;
    uint32_t reserved0;    /* 0 */
} rq_where_term_t;
typedef struct {
    uint32_t struct_size;  /* set to sizeof(rq_where_stats_t) before the call */
    uint32_t columns;      /* distinct columns the predicate read */
    uint64_t rows;         /* stored rows evaluated */
    uint64_t admitted;     /* rows of the filter */
    uint64_t bytes_read;   /* column bytes the kernel streamed: rows x the elem sizes of the columns read */
    float ms_eval;         /* device ms of the predicate kernel (HIP events) */
    float ms_finish;       /* wall ms of everything behind it: live AND, per-list counts, the filter's derived state */
} rq_where_stats_t;
rq_status rq_filter_create_where(const rq_index *idx, const rq_where_term_t *terms, uint32_t nterms, const uint8_t *program,
                                 uint32_t ntokens, rq_filter **out);
rq_status rq_last_where_stats(rq_where_stats_t *out);
/* rq_filter_combine: *out = a new filter of idx admitting a AND b, a OR b, a AND NOT b, or NOT a (b ignored, may be NULL) -- one
 * word-wise pass over the two position bitmaps, ANDed with the live rows and cut at n (NOT never admits a dead row or a position
 * past the last), then the steps of rq_filter_create.  This is how a predicate and an id allow-list meet.  A filter of another
 * index, or a stale one (made before a relayout or a marking rq_remove_lazy), is RQ_ERR_INVALID, exactly as the queries refuse it.
 * rq_filter_id_bits: the id bitmap of the admitted rows in the format rq_remove, rq_remove_lazy, rq_extract and rq_filter_create
 * take -- (nbits + 31) / 32 words, zeroed first, ids at or past nbits left out; host or device memory (bits_on_device).  "Delete
 * where" and "extract where" are rq_filter_create_where, this call and rq_remove / rq_extract.
 * rq_filter_ids_device: the admitted ids in position order into d_out_ids (device memory, room for `cap` ids): the first
 * min(cap, admitted) of them are written; *out_count (host) = the number admitted.  The two read the filter's own bitmap and the
 * ids of its index: a stale filter is RQ_ERR_INVALID here too. */
enum { RQ_FILTER_AND = 0, RQ_FILTER_OR = 1, RQ_FILTER_ANDNOT = 2, RQ_FILTER_NOT = 3 };
rq_status rq_filter_combine(const rq_index *idx, const rq_filter *a, const rq_filter *b, uint32_t op, rq_filter **out);
rq_status rq_filter_id_bits(const rq_filter *f, uint32_t *bits, uint64_t nbits, int bits_on_device);
rq_status rq_filter_ids_device(const rq_filter *f, uint32_t *d_out_ids, uint64_t cap, uint64_t *out_count);

/* ---- grouped search: at most group_size rows per value of a column, the topk nearest values (0.16.0, additions only) ------------ */
/* "The topk nearest documents, at most group_size passages each" (group_by / collapse / dedup by field), on the device: the
 * result rows of an existing call at topk = fetch are grouped by a column without travelling to the host.
 * SOURCE.  For query b, the result row of the plain call at topk = fetch: cnt_b <= fetch pairs (dist, id).  rq_query_batch_grouped
 *   runs rq_query_batch[_filtered](probe, fetch, heuristic_rank), rq_exact_search_grouped runs rq_exact_search(fetch, exact params),
 *   both under `filter` (nullable; with removals pending and no filter: the live filter, as in the plain entries);
 *   rq_group_results takes the rows from the caller (dist / id of stride fetch, cnt[b] valid entries, a larger cnt is cut at fetch):
 *   the results of tickets, the adaptive call, rq_neighbours_of or the sharded step.  The order of the pairs inside a row is
 *   arbitrary (the heap ranker returns its heap-internal order) and nothing depends on it.
 * KEYS.  The group key of a candidate is the u64 image of its row's value in the named column: 4-byte types zero-extended (as
 *   rq_attr_info's fill is), 8-byte types as stored.  Two rows are in one group iff the images are equal.  Integer columns only
 *   (RQ_ATTR_U32 / _I32 / _U64 / _I64); an RQ_ATTR_F32 column is RQ_ERR_INVALID (-0 / +0 and NaNs have no agreed equality here).
 * ABSENT IDS.  A candidate whose id has no live row (rq_locate would answer RQ_POS_ABSENT) is skipped and counted in
 *   rq_group_stats_t.absent.  Only rq_group_results can meet one.
 * SELECTION.  Sort the candidates ascending by the 64-bit key ord32_biased(dist) << 32 | id, the library's (distance, id) order.
 *   ord(key) = the number of distinct keys whose first occurrence in that order precedes this key's first occurrence; rank(c) = the
 *   number of earlier candidates with the same key as c.  c is kept iff ord(key_c) < topk and rank(c) < group_size.  This equals the
 *   sequential walk "open a group while fewer than topk are open; take a row while its group holds fewer than group_size", and
 *   does not depend on any processing order.
 * OUTPUT, group-major: out_id / out_dist[b, ord * group_size + rank] (nq x topk x group_size), out_key[b, ord] (u64 images) and
 *   out_group_n[b, ord] (rows kept of the group; nq x topk), out_n[b] = the number of groups.  Every slot without a row is written
 *   on every call: id 0xFFFFFFFF, dist NaN (0x7FC00000, as rq_neighbours_of pads), key 0, group_n 0.  The same inputs give the same
 *   bits on every run.
 * COMPLETENESS.  The two query entries also write out_fetched[b] = cnt_b (nullable).  out_fetched[b] < fetch: the source had
 *   nothing more to give -- behind the exact source the grouped answer is then the true one over all admitted rows.  Behind the
 *   exact source with group_size == 1, out_n[b] == topk proves it too.  Otherwise the answer is "grouped top-fetch": raise fetch.
 * LIMITS.  1 <= topk, 1 <= group_size, topk * group_size <= fetch <= 2048, else RQ_ERR_UNSUPPORTED.  Refused with RQ_ERR_INVALID
 *   before a device is looked for: a null index, column name, params or output (out_fetched excepted), a null input with nq > 0,
 *   params->struct_size != sizeof(rq_group_params_t), a set bit in flags, a malformed or unknown column name, an f32 column; the
 *   limits likewise.  Then the source call's own refusals at topk = fetch (a stale or foreign filter; the exact form on tiered and
 *   split-row indexes: RQ_ERR_UNSUPPORTED).  RQ_ERR_EMPTY from the source passes through with the outputs written, as in
 *   rq_neighbours_of.  nq == 0 is RQ_OK.  Accepted wherever the source call and the by-id entries both are: every metric and row
 *   type, shards of rq_shard_index, pending removals, after any relayout (the columns and a fresh directory follow).  rq_metrics
 *   counts the source call.  _device forms: every pointer but column and params in device memory; they return with their outputs
 *   complete.  No relayout and no rq_attr_set may run during a call.
 * rq_last_group_stats: the calling thread's last grouped call. */
typedef struct {
    uint32_t struct_size; /* sizeof(rq_group_params_t) */
    uint32_t topk;        /* groups per query */
    uint32_t group_size;  /* rows per group */
    uint32_t fetch;       /* candidates per query the source is asked for */
    uint32_t flags;       /* 0 */
} rq_group_params_t;
typedef struct {
    uint32_t struct_size;     /* set to sizeof(rq_group_stats_t) before the call */
    uint32_t fetch;
    float ms_source;          /* wall ms of the source call (0: rq_group_results) */
    float ms_group;           /* device ms of the selection kernel (HIP events) */
    uint64_t candidates;      /* sum of cnt_b */
    uint64_t absent;          /* candidates without a live row */
    uint64_t kept;            /* rows written */
    uint64_t groups;          /* sum of out_n */
    uint32_t directory_built; /* 1: this call made the id directory */
    uint32_t reserved0;
} rq_group_stats_t;
rq_status rq_query_batch_grouped(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len, uint32_t probe,
                                 int heuristic_rank, const char *column, const rq_group_params_t *params, float *out_dist, uint32_t *out_id,
                                 uint64_t *out_key, uint32_t *out_group_n, uint32_t *out_n, uint32_t *out_fetched);
rq_status rq_query_batch_grouped_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                        uint32_t probe, int heuristic_rank, const char *column, const rq_group_params_t *params,
                                        float *d_out_dist, uint32_t *d_out_id, uint64_t *d_out_key, uint32_t *d_out_group_n, uint32_t *d_out_n,
                                        uint32_t *d_out_fetched);
rq_status rq_exact_search_grouped(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                  const rq_exact_params_t *exact, const char *column, const rq_group_params_t *params, float *out_dist,
                                  uint32_t *out_id, uint64_t *out_key, uint32_t *out_group_n, uint32_t *out_n, uint32_t *out_fetched);
rq_status rq_exact_search_grouped_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                         const rq_exact_params_t *exact, const char *column, const rq_group_params_t *params,
                                         float *d_out_dist, uint32_t *d_out_id, uint64_t *d_out_key, uint32_t *d_out_group_n,
                                         uint32_t *d_out_n, uint32_t *d_out_fetched);
rq_status rq_group_results(const rq_index *idx, const float *dist, const uint32_t *id, const uint32_t *cnt, uint32_t nq, const char *column,
                           const rq_group_params_t *params, float *out_dist, uint32_t *out_id, uint64_t *out_key, uint32_t *out_group_n,
                           uint32_t *out_n);
rq_status rq_group_results_device(const rq_index *idx, const float *d_dist, const uint32_t *d_id, const uint32_t *d_cnt, uint32_t nq,
                                  const char *column, const rq_group_params_t *params, float *d_out_dist, uint32_t *d_out_id,
                                  uint64_t *d_out_key, uint32_t *d_out_group_n, uint32_t *d_out_n);
rq_status rq_last_group_stats(rq_group_stats_t *out);

/* ---- diverse search: the topk rows maximal marginal relevance takes out of `fetch` candidates (0.17.0, additions only) ---------- */
/* "The topk nearest rows, but not topk copies of the same passage" (MMR), on the device: the result rows of an existing call at
 * topk = fetch are re-selected greedily, trading a row's distance to the query against its distance to the rows already taken,
 * without the rows travelling to the host.
 * SOURCE.  As in grouped search: rq_query_batch_diverse runs rq_query_batch[_filtered](probe, fetch, heuristic_rank),
 *   rq_exact_search_diverse runs rq_exact_search(fetch, exact params), both under `filter` (nullable; with removals pending and no
 *   filter: the live filter); rq_diversify_results takes the rows from the caller (dist / id of stride fetch, cnt[b] valid entries,
 *   a larger cnt is cut at fetch).  The order of the pairs inside a row is arbitrary and nothing depends on it.
 * CANDIDATES.  Sort a row's cnt_b pairs ascending by the 64-bit key ord32_biased(dist) << 32 | id, the library's (distance, id)
 *   order.  A pair whose id has no live row (rq_locate would answer RQ_POS_ABSENT) is skipped and counted in
 *   rq_diverse_stats_t.absent; of the others, a pair whose distance is not finite is skipped and counted in .skipped.  The rest are
 *   the candidates c_0 .. c_{m-1} in that order, place(c_j) = j.  Equal ids in a caller's row are separate candidates.
 * PAIR DISTANCE.  D(c, s) = the engine's exact squared L2 between the STORED row of c and the row of s as rq_fetch_rows returns it
 *   (f32, widened, dim long): bit for bit rq_rerank(prepared query = that row, position of c).  On a cosine index that is
 *   2 - 2 cos of the two rows, on an inner-product index the distance in the augmented space -- not the metric's own score.
 * SELECTION, greedy and sequential.  lambda = params->lambda, mu = 1.0f - lambda (f32, computed once).  Step 0 takes c_0; div(c) =
 *   +inf for every candidate.  After taking s, every candidate not yet taken has div(c) = fminf(div(c), D(c, s)).  Step t >= 1:
 *   score(c) = (lambda * rel(c)) - (mu * div(c)) with rel the source's distance -- two f32 multiplications and one f32 subtraction,
 *   each rounded to nearest, never contracted; a NaN score is replaced by 0x7FC00000; the candidate not yet taken with the smallest
 *   ord32_biased(score) << 32 | place is taken.  min(topk, m) steps.  lambda == 1 gives the source's first topk candidates in
 *   (distance, id) order; topk == 1 gives c_0.
 * OUTPUT, in selection order (nq x topk): out_id, out_dist (rel: the source's bits), out_div (div at the moment of selection; +inf
 *   in slot 0); out_n[b] = rows taken.  Every slot without a row is written on every call: id 0xFFFFFFFF, dist and div NaN
 *   (0x7FC00000).  The two query entries also write out_fetched[b] = cnt_b (nullable).  The same inputs give the same bits on every
 *   run.
 * LIMITS.  Refused with RQ_ERR_INVALID before a device is looked for: a null index, params or output (out_fetched excepted), a
 *   null input with nq > 0, params->struct_size != sizeof(rq_diverse_params_t), a set bit in flags, lambda NaN or outside [0, 1].
 *   RQ_ERR_UNSUPPORTED likewise: topk == 0, topk > fetch, fetch > 2048 (RQ_MAX_TOPK).  Then the source call's own refusals at
 *   topk = fetch (a stale or foreign filter; the exact form on tiered and split-row indexes), and dim > 4096: the kernel holds the
 *   taken row in LDS beside the state of 2048 candidates (16 KB + 38 KB of the 64 KB a block gets), RQ_ERR_UNSUPPORTED.
 *   RQ_ERR_EMPTY from the source passes through with the outputs written.  nq == 0 is RQ_OK.  Accepted wherever the source call and
 *   the by-id entries both are: every metric and row type, shards, pending removals, after any relayout, the hash directory, and
 *   tiered and split-row indexes for the approximate source and rq_diversify_results.  rq_metrics counts the source call.  _device
 *   forms: every pointer but params in device memory; they return with their outputs complete.  No relayout may run during a call.
 * rq_last_diverse_stats: the calling thread's last diverse call. */
typedef struct {
    uint32_t struct_size; /* sizeof(rq_diverse_params_t) */
    uint32_t topk;        /* rows per query */
    uint32_t fetch;       /* candidates per query the source is asked for */
    float lambda;         /* 1: relevance alone ... 0: diversity alone */
    uint32_t flags;       /* 0 */
} rq_diverse_params_t;
typedef struct {
    uint32_t struct_size;     /* set to sizeof(rq_diverse_stats_t) before the call */
    uint32_t fetch;
    float ms_source;          /* wall ms of the source call (0: rq_diversify_results) */
    float ms_select;          /* device ms of the selection kernel (HIP events) */
    uint64_t candidates;      /* sum of cnt_b */
    uint64_t absent;          /* pairs without a live row */
    uint64_t skipped;         /* pairs with a live row whose distance is not finite */
    uint64_t taken;           /* sum of out_n */
    uint64_t pair_distances;  /* evaluations of D */
    uint32_t directory_built; /* 1: this call made the id directory */
    uint32_t reserved0;
} rq_diverse_stats_t;
rq_status rq_query_batch_diverse(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len, uint32_t probe,
                                 int heuristic_rank, const rq_diverse_params_t *params, float *out_dist, uint32_t *out_id, float *out_div,
                                 uint32_t *out_n, uint32_t *out_fetched);
rq_status rq_query_batch_diverse_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                        uint32_t probe, int heuristic_rank, const rq_diverse_params_t *params, float *d_out_dist,
                                        uint32_t *d_out_id, float *d_out_div, uint32_t *d_out_n, uint32_t *d_out_fetched);
rq_status rq_exact_search_diverse(const rq_index *idx, const rq_filter *filter, const float *queries, uint32_t nq, uint32_t len,
                                  const rq_exact_params_t *exact, const rq_diverse_params_t *params, float *out_dist, uint32_t *out_id,
                                  float *out_div, uint32_t *out_n, uint32_t *out_fetched);
rq_status rq_exact_search_diverse_device(const rq_index *idx, const rq_filter *filter, const float *d_queries, uint32_t nq, uint32_t len,
                                         const rq_exact_params_t *exact, const rq_diverse_params_t *params, float *d_out_dist,
                                         uint32_t *d_out_id, float *d_out_div, uint32_t *d_out_n, uint32_t *d_out_fetched);
rq_status rq_diversify_results(const rq_index *idx, const float *dist, const uint32_t *id, const uint32_t *cnt, uint32_t nq,
                               const rq_diverse_params_t *params, float *out_dist, uint32_t *out_id, float *out_div, uint32_t *out_n);
rq_status rq_diversify_results_device(const rq_index *idx, const float *d_dist, const uint32_t *d_id, const uint32_t *d_cnt, uint32_t nq,
                                      const rq_diverse_params_t *params, float *d_out_dist, uint32_t *d_out_id, float *d_out_div,
                                      uint32_t *d_out_n);
rq_status rq_last_diverse_stats(rq_diverse_stats_t *out);

/* ---- merge two indexes, extract a sub-index ------------------------------------------------------------------------------ */
/* Both work on stored rows as they stand: nothing is rotated, assigned, quantised -- or, on a cosine or inner-product index,
 * transformed -- again.  A row's list, order key, codes and factors depend only on the row, the rotation and the centroids, so
 * two indexes over the same rotation and centroids merge by a per-list two-way merge of their order keys and one gather.
 *
 * rq_merge_from: dst receives the live rows of src.  With S = the live rows of dst joined with those of src under their new ids,
 * dst afterwards equals canonical(S) of the section above, bit for bit: every array, rq_info, rq_dump_dir's files, and the ids,
 * distance bits, counts, status and counters of every query.  For a cosine or inner-product index that is rq_build_metric /
 * rq_build_ip of the ORIGINAL rows (the same S for inner product) -- which no sequence of rq_add can produce, since rq_add
 * would transform the stored rows a second time.
 *   id_mode: RQ_MERGE_IDS_KEEP = src's ids as they are; RQ_MERGE_IDS_SHIFT = src id + id_shift; RQ_MERGE_IDS_APPEND = src id +
 *   (1 + the largest id dst holds; 0 if dst is empty), id_shift ignored.  *out_shift (nullable) = the shift applied (0 for KEEP).
 *   src is not changed (its key cache may be derived); it stays a valid index and the caller still frees it.  dst's generation
 *   is bumped (filters made before are refused), its tile tables and workspaces are released, its learnt hints stay; its key
 *   cache is valid afterwards, so a following rq_add / rq_remove derives nothing.  An empty src succeeds and leaves dst as it
 *   was, generation included (as an empty rq_add); an empty dst is allowed.
 *   Memory: the merged arrays are built beside the old ones and moved into dst only after everything has succeeded, so the peak
 *   is dst + src + the merged arrays; RQ_ERR_OOM leaves both indexes as they were.
 * rq_extract: *out = a new index over src's rotation, centroids, metric (with its S and d) and dim, holding exactly the live rows
 * of src whose id bit is set (the rq_filter_create / rq_remove bitmap format; ids at or past nbits are not taken, bits of ids src
 * does not hold are ignored), ids kept: what rq_remove of the complement would leave in src, which is canonical of those rows.
 * src is unchanged.  No bit set (or nbits == 0) gives a valid empty index.  id_bits == NULL with nbits == RQ_EXTRACT_ALL_IDS takes
 * every row: a copy of src, for which no bitmap is made.  Every list keeps the order it has, so -- like
 * rq_remove -- extraction does not need the order precondition.  The caller frees *out with rq_free.
 * Refused with both indexes untouched and nothing left allocated (rq_last_error says which check failed):
 *   RQ_ERR_INVALID: a null handle (checked before the device is looked for: these two entries answer RQ_ERR_INVALID to it on a
 *   machine without a GPU too, where rq_add / rq_remove, which look for the device first, answer RQ_ERR_NO_DEVICE); dst == src; an unknown id_mode; dim, k or metric differ, or the inner-product S (compared as
 *   bits) or d; the rotation or the rotated centroids differ in any bit (compared on the device as bit patterns; the message names
 *   the array and the first differing element); a rq_query_batch_device_begin ticket of either index has not ended; under KEEP (and
 *   SHIFT) ids of src that dst already holds -- the message gives their count.
 *   RQ_ERR_UNSUPPORTED: either index is one rq_add refuses (tiered, split rows, half-precision or byte rows, a shard, dim > 4096);
 *   a list of either index is out of the build's order (rq_merge_from only; see the precondition of rq_add); the shifted ids
 *   would pass 2^32 - 1 or the row count what u32 ids allow (a largest new id of exactly 2^32 - 1 is accepted).
 * rq_last_mutate_stats reports the calling thread's last rq_merge_from / rq_extract as well: ms_assign is 0 (there is no pass 1),
 * ms_keys covers both indexes' key caches, gather_bytes counts what the gather of these entries moves, rows_after is dst's (the
 * new index's) row count. */
#define RQ_MERGE_IDS_KEEP   0u  /* src ids as they are; none may be in dst */
#define RQ_MERGE_IDS_SHIFT  1u  /* src id + id_shift; none may be in dst */
#define RQ_MERGE_IDS_APPEND 2u  /* src id + (1 + largest id dst holds; 0 if dst is empty); id_shift ignored */
rq_status rq_merge_from(rq_index *dst, rq_index *src, uint32_t id_mode, uint32_t id_shift, uint32_t *out_shift);
#define RQ_EXTRACT_ALL_IDS  0xFFFFFFFFFFFFFFFFull  /* nbits of rq_extract with id_bits == NULL: every row of src */
rq_status rq_extract(rq_index *src, const uint32_t *id_bits, uint64_t nbits, int bits_on_device, rq_index **out);

/* ---- sharded deployments (one index shard per GPU / process) ----------------------------------- */
/* The coarse ranking of src/rabitq.rs:283-297 restricted to lists [list_lo, list_hi): the `probe`
 * nearest of them per query, ascending, as (global list id, distance); rows are `probe` wide, padded
 * with (0xFFFFFFFF, +inf) when the range holds fewer lists.  A shard ranks only the lists it owns;
 * the per-shard rows are all-gathered and merged by the caller (rabitq_amd/sharding.py). */
rq_status rq_coarse_topk_device(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len,
                                uint32_t list_lo, uint32_t list_hi, uint32_t probe, uint32_t *d_out_cluster,
                                float *d_out_dist);
/* Shard merge: per query the m_out smallest of the world x width u64 keys in d_in[world][nq][width] (rows in
 * any order), ascending, into d_out[nq][m_out] (padded with ~0).  Keys: (f32 distance bits << 32 | list id) for
 * probe lists, (Ord32 image << 32 | global id) for per-shard top-k.  Launched asynchronously on the legacy
 * default stream (ordered with the caller's default-stream work, e.g. the all-gather that produced d_in). */
rq_status rq_merge_smallest_u64_device(const uint64_t *d_in, uint32_t world, uint32_t nq, uint32_t width,
                                       uint32_t m_out, uint64_t *d_out);
/* rq_query_batch_device with the probe lists supplied by the caller (nq x probe, visiting order,
 * 0xFFFFFFFF = no list; probe <= k) instead of ranked internally. */
rq_status rq_query_batch_device_probed(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len,
                                       const uint32_t *d_probe_cluster, const float *d_probe_dist, uint32_t probe,
                                       uint32_t topk, int heuristic_rank, float *d_out_dist, uint32_t *d_out_id,
                                       uint32_t *d_out_n);

/* The same with a per-query INITIAL threshold (device, nq floats; f32::MAX = none): a candidate is re-ranked only if
 * rough < threshold and kept only if accurate < threshold, from the first candidate on -- the multi-GPU step seeds every
 * shard with the k-th best distance the owner of the query's nearest list found there (one all-reduce(min)), so that
 * a shard which does not hold a query's neighbourhood stops re-ranking its far candidates (per-shard
 * thresholds).  The whole candidate stream runs as one stage.  A query may return fewer than topk results: everything
 * left out is at or above its initial threshold.  No reference counterpart (single process). */
rq_status rq_query_batch_device_seeded(const rq_index *idx, const float *d_queries, uint32_t nq, uint32_t len,
                                       const uint32_t *d_probe_cluster, const float *d_probe_dist, uint32_t probe,
                                       uint32_t topk, int heuristic_rank, const float *d_thr_init, float *d_out_dist,
                                       uint32_t *d_out_id, uint32_t *d_out_n);

/* List partitioner: whole IVF lists to `world` shards, greedy by list length (longest first,
 * each to the least-loaded shard; deterministic).  out_owner[c] = shard of list c (k entries, host);
 * out_load (world entries, host, may be NULL) = vectors per shard.  The reference has no counterpart (single process). */
rq_status rq_partition_lists(const rq_index *idx, uint32_t world, uint32_t *out_owner, uint64_t *out_load);
/* Carve shard `rank` out of an index: a new index with the same dim / k / rotation / (replicated) centroids that
 * holds only the lists with owner[c] == rank (the others are empty); map_ids keep the ORIGINAL ids, so per-shard
 * results are global.  The source index is unchanged; free both with rq_free. */
rq_status rq_shard_index(const rq_index *idx, const uint32_t *owner, uint32_t rank, rq_index **out);
/* The whole multi-GPU step behind the C ABI, for hosts without torch.  Every rank holds all (replicated) rotated centroids
 * and a subset of the lists.  `nccl_comm` is an ncclComm_t of `world` ranks created by the caller with ncclCommInitRank
 * (may be NULL when world == 1).  The step, all on one HIP stream of the engine:
 *   handshake  one ncclAllReduce(max) of three int32 (a hash of the call's parameters and an error flag);
 *   coarse     rank r ranks lists [r k / world, (r+1) k / world) only, one ncclAllGather of the nq x probe
 *              (distance, list) keys + merge: the same global probe list on every rank;
 *   answer     the shard's own lists of that probe list, with thresholds shared between the shards (option
 *              "shared_thresholds": the nearest list first, one ncclAllReduce(min) of the k-th best distances found
 *              there, the rest seeded with it; see rq_query_batch_device_seeded) or on the shard's own thresholds;
 *   merge      ONE ncclAllGather of the per-shard top-k as u64 keys (+ a status word per rank), k-way merge.
 * Every rank receives the same global top-k, ascending by (distance, id); ids are shard-local map_ids + id_offset (u32).
 * COLLECTIVE CONTRACT: all ranks of the communicator call this entry with the same nq, len, probe, topk, world,
 * heuristic_rank and the same "shared_thresholds" option, in the same order.  The handshake detects a violation (and a
 * rank that failed validation or allocation) and makes every rank return an error before any data collective; after
 * it a rank that fails locally keeps taking part in every collective and reports through its status word, so no peer is
 * left blocked and all ranks return an error for that step.  Limits: world * topk <= 8192, nq * topk < 2^32.
 * RCCL is resolved at first use from the host process (or RABITQ_RCCL_LIB), so the library itself does not link against it.
 * rq_last_profile() afterwards holds the sum over the step's engine passes. */
rq_status rq_query_batch_sharded_device(const rq_index *shard, void *nccl_comm, uint32_t world, uint32_t id_offset,
                                        const float *d_queries, uint32_t nq, uint32_t len, uint32_t probe, uint32_t topk,
                                        int heuristic_rank, float *d_out_dist, uint32_t *d_out_id, uint32_t *d_out_n);
/* The collectives rq_query_batch_sharded_device calls, for hosts with another transport than RCCL (or a test harness):
 * same signatures and semantics as ncclAllGather / ncclAllReduce / ncclCommUserRank (device buffers, enqueued on
 * `hip_stream` or completed before returning; dtype / op are the ncclDataType_t / ncclRedOp_t values: int32 = 2,
 * uint64 = 5, float32 = 7; max = 2, min = 3; return 0 on success).  `comm` is passed through untouched.  NULL = back to
 * RCCL (the default).  Process-wide; set it before the first sharded call. */
typedef struct {
    uint32_t struct_size; /* in: sizeof(rq_collectives_t) */
    uint32_t reserved;
    int (*all_gather)(const void *send, void *recv, size_t send_count, int dtype, void *comm, void *hip_stream);
    int (*all_reduce)(const void *send, void *recv, size_t count, int dtype, int op, void *comm, void *hip_stream);
    int (*comm_user_rank)(void *comm, int *rank);
} rq_collectives_t;
rq_status rq_set_collectives(const rq_collectives_t *collectives);

/* ---- metrics: METRICS, src/metrics.rs:65 ------------------------------------------------------ */
rq_status rq_metrics(rq_metrics_t *out);
rq_status rq_metrics_reset(void);

/* ---- per-stage entry points (each hot kernel testable in isolation; all host pointers) -------- */
/* Rotation X' = X P in the reference's `project` order (src/utils.rs:237-258, src/simd.rs:257-314):
 * x is n x dim, out is n x dim.  use_mfma = 1 runs the MFMA kernel (bit-identical by construction),
 * 0 the VALU kernel. */
rq_status rq_rotate(const float *x, uint64_t n, uint32_t dim, const float *orthogonal, int use_mfma,
                    float *out);
/* Same rotation on device-resident rows with the index's own P (the build's rotate step,
 * src/rabitq.rs:188): d_x and d_out are n x dim device arrays.  If out_ms is non-NULL it receives
 * the MFMA kernel's duration measured with HIP events on the launch stream (bench.py's rotation
 * roofline). */
rq_status rq_rotate_device(const rq_index *idx, const float *d_x, uint64_t n, float *d_out, float *out_ms);
/* Nearest rotated centroid + residual sign-pack + factors for already-rotated vectors
 * (src/utils.rs:261-277, :53-67; src/rabitq.rs:203-229): out_label n, out_dist n,
 * out_codes n x dim/64, out_factors n. */
rq_status rq_quantize_pack(const float *x_rot, uint64_t n, uint32_t dim, const float *centroids_rot,
                           uint32_t k, uint32_t *out_label, float *out_dist, uint64_t *out_codes,
                           rq_factor_t *out_factors);
/* Rotate + coarse-rank a query batch (src/rabitq.rs:282-297): out_y nq x dim (may be NULL),
 * out_cluster / out_dist nq x min(probe,k). */
rq_status rq_coarse_rank(const rq_index *idx, const float *queries, uint32_t nq, uint32_t len,
                         uint32_t probe, float *out_y, uint32_t *out_cluster, float *out_dist);
/* Per-(query,cluster) query quantisation (src/rabitq.rs:304-317; src/simd.rs:117-247, :83-107):
 * y is nq x dim rotated queries, cluster[i] is the cluster paired with y row i.
 * out_planes nq x 4*dim/64 u64. */
rq_status rq_query_prep(const rq_index *idx, const float *y, uint32_t nq, const uint32_t *cluster,
                        float *out_lower, float *out_delta, uint32_t *out_sum, uint64_t *out_planes);
/* calculate_rough_distance (src/rabitq.rs:336-367) for the whole list of `cluster` with the
 * given query-side scalars and bit planes; out_rough needs list-length floats. */
rq_status rq_scan(const rq_index *idx, uint32_t cluster, float y_c_distance_square,
                  const uint64_t *planes, float lower_bound, float scalar_sum, float delta,
                  float *out_rough);
/* Exact f32 L2 rerank distance (src/simd.rs:14-73 order) of the padded, un-rotated query against
 * base rows at cluster-order positions pos[0..m) (src/rerank.rs:85-90). */
rq_status rq_rerank(const rq_index *idx, const float *query_padded, const uint32_t *pos, uint32_t m,
                    float *out_accurate);

/* ---- instrumentation ------------------------------------------------------------------------- */
/* Per-kernel device time of the LAST rq_query_batch* call on this thread, measured with HIP events
 * on the stream the kernels ran on.  Names: "rotate", "coarse", "select", "prep", "scan",
 * "rerank", "sort", "replay", "total".  Also the algorithmic bytes the scan launches covered
 * (sum over probed lists of len * (dim/8 + 16)) and the number of scan launches. */
typedef struct {
    uint32_t struct_size;      /* in: sizeof(rq_profile_t) of the caller */
    uint32_t coarse_fallback_rows; /* queries whose pre-filtered coarse ranking (option "coarse_impl") fell back to all-lists exact order */
    float ms_rotate, ms_coarse, ms_select, ms_prep, ms_group, ms_scan, ms_rerank, ms_sort, ms_replay,
        ms_total;
    uint64_t scan_bytes;       /* algorithmic bytes over all scan launches of the call */
    uint64_t scan_candidates;  /* (query, candidate) pairs scanned                      */
    uint64_t rerank_candidates;/* accurate distances computed (superset of `precise`)   */
    uint32_t scan_launches;    /* scan kernel launches (a stage whose grid is issued in chunks counts each of them) */
    uint32_t retries;          /* queries re-run because a survivor buffer overflowed   */
    /* the matrix-core launches alone (a subset of the scan figures above) */
    float ms_scan_matrix;      /* device time of the scan_mfma_kernel launches           */
    uint32_t matrix_launches;
    uint64_t matrix_pairs;     /* (query, candidate) pairs they scored                   */
    /* 32x32 (query x candidate) sub-tile steps of the matrix-core scan, and how many of them were flagged by its gate and took
     * the exact f32 path (always filled since ABI revision 4) */
    uint64_t matrix_subtile_steps, matrix_exact_steps;
    /* of rerank_candidates: survivors the shadow rows (8-bit or fp16, option "rerank_shadow") proved to be at or above their stage's threshold, whose
     * 4*dim-byte row was therefore never fetched (option "rerank_shadow"; large batches) */
    uint64_t rerank_shadow_rejects;
    /* small-batch path (<= 64 queries: rotate + coarse in one launch, then one block per query doing probe selection, query
     * quantisation and the early stages in LDS): device time of that second launch, and how many passes took the path */
    float ms_early;
    uint32_t small_batch_passes;
    /* survivor records + run directories (+ the shared arena) of the call's largest pass, bytes; passes in which a stage
     * appended its survivors to the shared arena and scattered them into per-query segments sized by their exact counts,
     * instead of one capacity for every query */
    uint64_t survivor_workspace_bytes;
    uint32_t segmented_passes;
    uint32_t matrix_additive_launches; /* of matrix_launches: those that ran the additive gate (no threshold MFMA; option "scan_gate") */
} rq_profile_t;
/* level: 0 = off; 1 = every kernel group bracketed (each event costs a few microseconds of stream
 * time); 2 = only the scan launches and the whole pass (ms_scan, ms_total; the other fields stay 0). */
rq_status rq_set_profiling(int level);
/* Engine options.  "scan_impl": 0 = auto (default: fp6 matrix-core scan when many queries share each
 * list, v_dot8 VALU scan otherwise), 1 = VALU only, 2 = matrix cores wherever available.  All
 * settings return identical results; the option exists for tests and measurements.
 * "base_device_mb": HBM budget (MiB) of the raw vectors of indexes built / loaded from now on (-1 = automatic, the
 * default); vectors beyond it live in pinned host memory.  Results never depend on it.
 * "pass_overlap": a call that needs several passes (more than 65 536 queries) keeps two of them in flight, each on a workspace
 * and stream of its own (1, default), or runs them one after the other (0).  Results are identical.
 * "split_rows": indexes built / loaded from now on whose raw vectors leave no room for shadow rows -- tiered ones (both tiers),
 * and untiered ones where the shadow of "rerank_shadow" would not fit -- keep each raw vector as two 16-bit planes inside its own
 * 4*dim bytes (1, default: the upper halves of the f32 words rounded to nearest, then the lower halves; every word is restored
 * exactly), or as plain f32 (0); 2 = split rows always (test hook).  The re-ranker of large batches reads the first plane alone
 * and fetches the second one only for survivors the first cannot prove out of the top-k.  Such an index has no f32 device array
 * of its raw vectors (rq_get_device_ptr(RQ_ARR_BASE) -> RQ_ERR_UNSUPPORTED; rq_get_array restores them).  Results are
 * bit-identical for every value.
 * "rerank_shadow": shadow rows of indexes built / loaded from now on whose raw vectors are all in HBM (when that still leaves
 * the query workspaces their room): 2 (default) = 8-bit rows (dim bytes per vector; one affine map per list, error bound
 * measured while the codes are written), 1 = fp16 rows (2*dim bytes per vector), 0 = none.  The re-ranker of large batches
 * reads the shadow row first and fetches the f32 row only when the shadow cannot prove that the exact distance is at or
 * above the stage's threshold (then the reference rejects it whatever its value).  Results are bit-identical for every value.
 * "max_scan_blocks": test hook, blocks per scan launch (0 = hardware bound).
 * "coarse_impl": coarse ranking (identical probe lists and distance bits for every value): 0 = automatic (default: batches of
 * >= 2048 queries rank through the bf16 matrix-core pre-filter + exact-order refinement of the candidates within a proven margin
 * of the nprobe-th approximate distance, where it applies -- dim/64 in {1, 2, 3, 4, 6, 8, 12}, <= 65536 lists, nprobe <= 64; the
 * nprobe-th approximate distance is bounded from the minima of 32-list tiles from 4096 lists up (dim <= 512) and always
 * beyond 8192 lists, with the row in one wave's registers otherwise --, else the exact-order distance kernels over all lists),
 * 1 = exact-order kernel with the query rows through LDS, 2 = exact-order kernel with the query rows in scalar registers,
 * 3 = the pre-filter wherever it applies, row in registers up to 8192 lists (tests), 4 = the pre-filter with the tile-minima
 * selection wherever a row has at least nprobe tiles (tests).  rq_profile_t.coarse_fallback_rows counts queries whose
 * candidate set exceeded the refinement's 256 slots (near-equidistant centroids) or whose margin was not finite: they are
 * ranked in exact order over all lists (per row).
 * "pair_split": test hook, 1 (default) = passes over an index most of whose lists are empty (a shard: the probe lists name the lists
 * of every shard) settle the (query, list) pairs with nothing to scan by one thread each and run the query quantisation and the final
 * stage's record fill over a compacted list of the others, 0 = every pair takes the full path.  Identical results.
 * "coarse_tiled_from": developer knob, list count from which the automatic choice selects through tile minima (default 4096).
 * "shared_thresholds": rq_query_batch_sharded_device: 1 (default) = with more than one shard the step runs the nearest
 * list first, all-reduces (min) the k-th best distances and seeds the rest of the probe list with them (see
 * rq_query_batch_device_seeded); 0 = every shard prunes with its own thresholds only; 2 = also with one shard (tests).
 * "survivor_segments": 1 (default) = once an index has shown that its batches overflow the default survivor capacity, large
 * batches (>= 256 queries) size the survivor buffers of the stages that can exceed it PER QUERY (the scan appends to one shared
 * arena while counting per query; exact counts + prefix sum + a scatter pass) instead of giving every query the worst one's
 * capacity; 0 = never, 2 = every large batch (tests).  A pass whose arena cannot be had -- no memory, or it keeps overflowing --
 * is repeated on the uniform buffers; the failure injection that exercises this (value 3: as 2 with every arena stage failing
 * through a real, oversized allocation) exists in the developer build only (`make dev`, -DRQ_DEV_ABLATIONS) and is refused
 * here.  Identical results.
 * "small_batch": 0 (default) = batches of <= 64 queries (the reference's one-query-per-call loop included) run as a handful
 * of fat launches (kernels_small.h) whenever the shape allows (nprobe <= 64, <= 8192 lists, topk <= 256, dim in {64, 128,
 * 256, 512, 768, 1024}), 1 = never (test hook).  Identical results.
 * "small_batch_filtered": filtered batches on the small-batch path: 1 (default) = automatic -- taken when 16 x topk admitted
 * candidates, which fill the ranker, lie within the 65 536 stored stream positions a query's block scans at most, i.e.
 * 16 x topk x (stored rows of the lists that admit anything) / (admitted rows) <= 65 536; the block's stage boundaries are stretched
 * by the same ratio --, 0 = never (filtered batches take the staged launches), 2 = whenever the shape allows (tests).
 * Identical results.
 * "dense_dir": test hook, 1 (default) = the VALU stages of large batches write their survivor runs into a directory
 * indexed by stream position (nothing to sort), 0 = runs are appended and the directory is sorted.
 * "prep_placement": 1 (default) = a pass whose only matrix-core stage is the final one groups that stage before the query
 * quantisation, which then writes the fp6 operand rows straight into the stage's tile images (large stages placed by rank; not
 * filtered, shard-like, arena, seeded or re-run passes), 0 = the pair-major operand and the copying fill everywhere.  Read once
 * per pass.  Identical results.
 * "group_rank": test hook, placement of a cluster-major stage's (query, list) pairs: 0 = one atomic per pair,
 * 1 = automatic (default: per-block LDS histograms for big stages), 2 = histograms whenever they fit.
 * "assign_impl": nearest-list assignment of builds from now on: 0 (default) = bf16 matrix-core pre-filter + exact-order
 * refinement wherever the shape is supported, 1 = exact-order kernels only (test hook); bit-identical labels and distances.
 * "scan_tile_table": test hook, grids of the list-major scan stages: 0 = lists x tiles-of-the-longest-list everywhere,
 * 1 (default) = one block per existing (list, tile) when most of the plain grid would be empty blocks, 2 = always.
 * "small_batch_span": developer knob, stream positions a query's block of the small-batch path scans itself at most
 * (default 2560; results are identical for every value).
 * "scan_gate": gate of the matrix-core scan (results never depend on it): 0 (default) = the additive bound S* >= B_q + G_c
 * where it exists (dim 64 / 128, stages on the uniform survivor buffers: no threshold MFMA) until an index shows that it sends
 * more than 3 % of the sub-tile steps down the exact path, 1 = the bf16 rank-5 threshold MFMA always, 2 = the additive bound
 * wherever it exists (test hook).
 * Developer knobs (results are identical for every value): "stage_growth" (geometric growth of the early stages, 0 = default),
 * "large_batch_from" (queries from which a batch takes the large-batch form of the stages -- full-chip rerank / ordering / replay
 * launches, thin early stages, dense run directories, survivor arena; default 256), "cluster_major_div" (a VALU stage goes
 * list-major once its (query, list) pairs reach k / this; default 32), "stage_settle_pct" (where a large batch's early stages end,
 * in percent of the average list length; default 100), "scan_debug": measurement hooks under which every result is UNCHANGED -- 128 (kept for older hosts: the sub-tile /
 * exact-path step counters of rq_profile_t are always on since ABI revision 4), 512 no shadow rows in the rerank,
 * 2048 long run directories skip the cell bitmap (they are ordered by the slot buckets, or the bitonic sort: a test hook),
 * 4096 the phases of the small-batch kernel, 16384 the stage list of every pass (stderr; with one `[rabitq_hip] plan:` line of
 * key=value tokens per pass, per stage and per coarse ranking, which tests/test_option_paths_gpu.py reads; a large batch's stages whose survivors go through
 * the 8-bit shadow rows add a line `stage <i>: rerank=ring` or `rerank=regs`), 32768 the 8-bit rerank pre-filter reads its shadow rows
 * into registers (accurate_filtered8_kernel) where it would send them through the LDS ring (dimensions 64, 128, 192, 256 with at most
 * 1024 probed lists: accurate_ring8_kernel) -- the switch for A/B runs, bench.py --option scan_debug=32768 --, 65536 the pre-filtered coarse ranking of
 * a big batch over 4096 .. 8192 lists (dim <= 256) writes the nq x k matrix of approximate distances and selects from it
 * (coarse_approx_kernel + select_refine_tiled_kernel, trace `coarse=prefilter_tiled`) where it would emit candidates straight from the
 * matrix-core pass (coarse_candidates_kernel + refine_candidates_kernel, `coarse=prefilter_fused`).  Any other bit is refused with
 * RQ_ERR_INVALID by this library: the TIMING ABLATIONS of the matrix-core scan (1, 2, 4, 64, 1024, 8192: results are WRONG) and
 * its in-kernel cycle counters (256) are compiled only into the developer build (make -C rabitq_amd/csrc dev ->
 * librabitq_hip_dev.so, -DRQ_DEV_ABLATIONS; scripts/exp/ select it through RABITQ_HIP_SO), so the shipped kernels carry none
 * of those branches.
 *
 * Threading: options are process-global and result-neutral (every value of every option leaves ids, distances and counters
 * unchanged: tests/test_gpu_parity.py::test_every_option_value_keeps_golden_results on a small golden, and
 * tests/test_option_paths_gpu.py::test_option_value_runs_its_path_and_keeps_results on indexes and batches where the value's
 * code path is shown to run).  A pass reads the ones its plan depends on ONCE, before anything is enqueued (plan_pass: the batch
 * form of "large_batch_from", the stage boundaries, engines, record layouts); whatever executes the pass asks the plan.  Changing
 * an option while queries are in flight on other threads therefore only changes which kernels later passes use
 * (test_options_flipped_under_concurrent_queries).
 * Removed in ABI revision 3: "scan_dense", "coarse_impl" = 3 (both answer RQ_ERR_INVALID). */
rq_status rq_set_option(const char *name, int value);
rq_status rq_last_profile(rq_profile_t *out);

#ifdef __cplusplus
}
#endif
#endif
