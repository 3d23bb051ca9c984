// host_options.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  The process-global options: every atomic rq_set_option stores to, and the one table it looks
// a name up in.  An option is added HERE and nowhere else: its row declares the atomic (with the default), and gives the name, the
// accepted range and the text of the refusal.  (tests/test_option_cases.py reads the names and defaults from the rows.)
#pragma once

// HIP silently wraps a launch whose gridDim.x * blockDim.x reaches 2^32: every launcher keeps
// blocks * threads below this bound (rows are chunked, big kernels are grid-stride).
#define RQ_MAX_BLOCKS_256 ((1u << 23) - 1)  // blocks of 256 threads: < 2^31 threads per launch

#define RQ_OPT_ANY 0x7FFFFFFF  // "highest accepted value" of an option that is bounded from below only
#ifdef RQ_DEV_ABLATIONS
#define RQ_OPT_SEG_HI 3
#define RQ_OPT_SEG_TEXT "survivor_segments must be 0, 1, 2 or 3"
#define RQ_OPT_DEBUG_BITS 0x7FFFFFFF
#else
#define RQ_OPT_SEG_HI 2
#define RQ_OPT_SEG_TEXT "survivor_segments must be 0, 1 or 2"
#define RQ_OPT_DEBUG_BITS (128 | 512 | 2048 | 4096 | 16384 | 32768 | 65536)
#endif

// X(name, atomic<int>, default, lowest accepted, highest accepted, text of the refusal)
#define RQ_OPTIONS(X)                                                                                                                              \
    /* scan implementation: 0 = auto (matrix cores when many queries share each list, VALU otherwise), 1 = VALU (v_dot8_u32_u4) only,             \
       2 = matrix cores wherever the kernel exists (test hook) */                                                                                  \
    X("scan_impl", g_scan_impl, 0, 0, 2, "scan_impl must be 0 (auto), 1 (valu) or 2 (mfma)")                                                       \
    /* gate of the matrix-core scan (results never depend on it): 0 = auto (additive bound where it exists -- dim 64 / 128, uniform survivor       \
       buffers -- unless the index has shown that it flags too much), 1 = the bf16 rank-5 threshold MFMA always, 2 = additive wherever it          \
       exists (test hook) */                                                                                                                       \
    X("scan_gate", g_scan_gate, 0, 0, 2, "scan_gate must be 0, 1 or 2")                                                                            \
    /* developer knob (results identical for every value): a VALU stage goes list-major once its (query, list) pairs reach k / this */             \
    X("cluster_major_div", g_cluster_major_div, 32, 1, 4096, "cluster_major_div must be in [1, 4096]")                                             \
    /* developer knob (results identical for every value): queries from which a batch runs the large-batch form of the stages (full-chip           \
       rerank / ordering / replay launches, thin early stages, dense run directories, survivor arena); below: one fused launch per stage */        \
    X("large_batch_from", g_large_from, 256, 2, (1 << 20), "large_batch_from must be in [2, 2^20]")                                                \
    /* developer knob (results identical for every value): where a large batch's early (VALU) stages end and the final (matrix-core) stage         \
       begins, in percent of the average list length */                                                                                            \
    X("stage_settle_pct", g_stage_settle_pct, 100, 1, 400, "stage_settle_pct must be in [1, 400]")                                                 \
    /* geometric growth of the early stages: 0 (= the default schedule: 16 below 32 768 queries, 8 from there on), or in [2, 64] -- 1 is           \
       refused (rq_set_option) */                                                                                                                  \
    X("stage_growth", g_stage_growth, 0, 0, 64, "stage_growth must be 0 or in [2, 64]")                                                            \
    /* a call of several passes keeps two of them in flight (1, default) or runs them one after the other (0); results identical */                \
    X("pass_overlap", g_pass_overlap, 1, 0, 1, "pass_overlap must be 0 or 1")                                                                      \
    /* tiered indexes built / loaded from now on with no room for shadow rows keep their raw vectors as two 16-bit planes (1, default) or          \
       as plain f32 (0: the round-4 layout); 2: always split */                                                                                    \
    X("split_rows", g_split_rows, 1, 0, 2, "split_rows must be 0, 1 or 2")                                                                         \
    /* full-list stages launch one block per existing (list, tile): 0 never (plain list x tile grids everywhere: test / measurement hook),         \
       1 auto, 2 always */                                                                                                                         \
    X("scan_tile_table", g_scan_tile_table, 1, 0, 2, "scan_tile_table must be 0 (never), 1 (auto) or 2 (always)")                                  \
    /* sharded passes: 1 (default) = pairs of empty lists settled by a thread each, quantisation over the listed others; 0 = lane group per        \
       pair (test hook) */                                                                                                                         \
    X("pair_split", g_pair_split, 1, 0, 1, "pair_split must be 0 or 1")                                                                            \
    /* developer knob: list count from which the pre-filtered coarse ranking selects through tile minima */                                        \
    X("coarse_tiled_from", g_coarse_tiled_from, 4096, 0, RQ_OPT_ANY, "coarse_tiled_from must be >= 0")                                             \
    /* coarse ranking (test hook): 0 auto, 1 LDS-broadcast kernels, 2 scalar-register kernel, 3 bf16-MFMA pre-filter + exact refinement            \
       wherever it applies (row in registers up to 8192 lists), 4 the same with the tile-minima selection wherever it applies */                   \
    X("coarse_impl", g_coarse_impl, 0, 0, 4, "coarse_impl must be 0, 1, 2, 3 or 4")                                                                \
    /* per-query survivor segments in the final stage: 0 never, 1 once the index has shown that the default capacity overflows (default),          \
       2 every large batch (tests); developer build: 3 = 2 with every arena stage failing (the fall-back; the ordinary build refuses it            \
       with a text of its own: rq_set_option) */                                                                                                   \
    X("survivor_segments", g_seg_opt, 1, 0, RQ_OPT_SEG_HI, RQ_OPT_SEG_TEXT)                                                                        \
    /* nearest-list assignment of builds started from now on: 0 = matrix-core pre-filter + exact refinement where the kernel exists                \
       (default), 1 = exact-order VALU kernels only */                                                                                             \
    X("assign_impl", g_assign_impl, 0, 0, 1, "assign_impl must be 0 or 1")                                                                         \
    /* developer knob (results identical for every value): stream positions a query's block scans itself at most (small-batch path) */             \
    X("small_batch_span", g_sb_span, 2560, 1, RQ_OPT_ANY, "small_batch_span must be >= 1")                                                         \
    /* small-batch path (kernels_small.h): 0 = batches of <= 64 queries take the few-launch path whenever it applies (default), 1 = never          \
       (test hook) */                                                                                                                              \
    X("small_batch", g_small_batch, 0, 0, 1, "small_batch must be 0 or 1")                                                                         \
    /* filtered passes on the small-batch path (results identical for every value): 0 = never (staged launches), 1 = automatic (plan_pass),        \
       2 = whenever the shape allows (tests) */                                                                                                    \
    X("small_batch_filtered", g_sb_filtered, 1, 0, 2, "small_batch_filtered must be 0, 1 or 2")                                                    \
    /* dense run directories for the VALU stages of large batches where they fit (1); 0 = descriptors always appended and sorted (test hook) */    \
    X("dense_dir", g_dense_dir, 1, 0, 1, "dense_dir must be 0 or 1")                                                                               \
    /* rq_query_batch_sharded_device: thresholds shared between the shards (0 never: every shard on its own, 1 world > 1, 2 always) */             \
    X("shared_thresholds", g_shared_thr, 1, 0, 2, "shared_thresholds must be 0, 1 or 2")                                                           \
    /* group_rank_kernel for cluster-major stages (test hook): 0 never (atomics per pair), 1 big stages (auto), 2 always */                        \
    X("group_rank", g_group_rank, 1, 0, 2, "group_rank must be 0, 1 or 2")                                                                         \
    /* 1 (default) = the final matrix-core stage is planned before the query quantisation, which writes its operand rows in place (where it        \
       applies); 0 = pair-major operand + stage_fill_kernel everywhere: the older kernels (results identical) */                                   \
    X("prep_placement", g_prep_placement, 1, 0, 1, "prep_placement must be 0 or 1")                                                                \
    /* shadow rows for the rerank pre-filter, for indexes built / loaded from now on: 0 never, 1 fp16 when they fit, 2 8-bit (one affine           \
       map per list) when they fit */                                                                                                              \
    X("rerank_shadow", g_rerank_shadow, 2, 0, 2, "rerank_shadow must be 0 (never), 1 (fp16 rows when they fit) or 2 (8-bit rows when they fit)")   \
    /* A bit mask (every bit outside RQ_OPT_DEBUG_BITS is refused: rq_set_option).  Measurement hooks that leave every result unchanged:           \
       128 (kept for older hosts: the step counters are always on now), 512 (rerank without the fp16 shadow rows), 2048 (long run                  \
       directories are ordered without the cell bitmap), 4096 (phase stamps of the small-batch block), 16384 (stage list on stderr),               \
       32768 (the 8-bit rerank pre-filter reads its shadow rows into registers: the kernel from before the LDS ring), 65536 (the                   \
       pre-filtered coarse ranking of 4096 .. 8192 lists writes the nq x k matrix of approximate distances and selects from it: the two            \
       kernels from before coarse_candidates_kernel).  The timing ablations (1, 2, 4, 64, 1024, 8192: results are WRONG) and the                   \
       in-kernel cycle counters (256) exist in the developer build only (make dev -> librabitq_hip_dev.so, -DRQ_DEV_ABLATIONS). */                 \
    X("scan_debug", g_scan_dbg, 0, 0, RQ_OPT_ANY, "scan_debug: this bit exists in the developer build only (librabitq_hip_dev.so)")

// The two options whose storage is not an int (OptionRow::var is null: rq_set_option stores them itself).
// "base_device_mb": HBM budget of the raw vectors for indexes built / loaded from now on: -1 = automatic (default), else MiB; the rest
// goes to pinned host memory.  64-bit: the budget in bytes is this value << 20.
static std::atomic<int64_t> g_base_device_mb{-1};
// "max_scan_blocks" (test hook: forces chunked stages): blocks per scan launch.  0 = the hardware bound, which is what is stored then;
// larger values are clamped to it.
static std::atomic<uint32_t> g_max_scan_blocks{RQ_MAX_BLOCKS_256};

#define RQ_OPTION_ATOMIC(NAME, VAR, DEF, LO, HI, TEXT) static std::atomic<int> VAR{DEF};
RQ_OPTIONS(RQ_OPTION_ATOMIC)
#undef RQ_OPTION_ATOMIC

struct OptionRow {
    const char *name;
    std::atomic<int> *var;
    int def, lo, hi;      // def: the value that sets the option back to what the process started with
    const char *refused;  // rq_last_error() after a value outside [lo, hi]
};
#define RQ_OPTION_ROW(NAME, VAR, DEF, LO, HI, TEXT) {NAME, &VAR, DEF, LO, HI, TEXT},
static const OptionRow g_options[] = {
    RQ_OPTIONS(RQ_OPTION_ROW)
    {"base_device_mb", nullptr, -1, -1, RQ_OPT_ANY, "base_device_mb must be >= -1"},
    {"max_scan_blocks", nullptr, 0, 0, RQ_OPT_ANY, "max_scan_blocks must be >= 0"},
};
#undef RQ_OPTION_ROW

static bool rq_large_batch(uint32_t nq) { return nq >= (uint32_t)g_large_from.load(); }
