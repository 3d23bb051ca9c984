// host_state.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  Errors, device buffers, metrics / profiling, the per-call workspace, struct rq_index and rq_filter,
// the workspace pool and the small kernels that belong to those structures.  (The options: host_options.h; the kernel launch
// helpers: host_launch.h, those of the metrics: host_metric.h.)
#pragma once
// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static rq_status fail(rq_status s, const std::string &msg) {
    g_err = msg;
    return s;
}
#define HIPC(expr)                                                                                   \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return fail(_e == hipErrorOutOfMemory ? RQ_ERR_OOM : RQ_ERR_HIP,                         \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                          \
    } while (0)
#define RQC(expr)                        \
    do {                                 \
        rq_status _s = (expr);           \
        if (_s != RQ_OK) return _s;      \
    } while (0)

static rq_status ensure_device() {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(RQ_ERR_NO_DEVICE, "no HIP device visible (librabitq_hip has no CPU fallback)");
    return RQ_OK;
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        count = 0;
    }
    rq_status alloc(size_t n) {
        release();
        count = n;
        if (n == 0) n = 1;
        hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            count = 0;
            return fail(RQ_ERR_OOM, "hipMalloc of " + std::to_string(n * sizeof(T)) + " bytes failed: " +
                                        hipGetErrorString(e));
        }
        return RQ_OK;
    }
    rq_status ensure(size_t n) { return n <= count && p ? RQ_OK : alloc(n); }
    rq_status upload(const T *host, size_t n) {  // a fresh allocation of n elements holding the host array (nothing is copied for n == 0)
        if (rq_status s = alloc(n)) return s;
        hipError_t e = n ? hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
        return e == hipSuccess ? RQ_OK : fail(RQ_ERR_HIP, std::string("hipMemcpy to the device: ") + hipGetErrorString(e));
    }
    void take(DevBuf &o) {  // this buffer becomes o's allocation (o is left empty)
        release();
        p = o.p, count = o.count;
        o.p = nullptr, o.count = 0;
    }
};

// Sized out-structs (include/rabitq_hip.h): write at most the bytes the caller's struct has.
template <typename T>
static rq_status copy_out_sized(T *out, T full) {
    const uint32_t sz = out->struct_size;
    if (sz < 8) return fail(RQ_ERR_INVALID, "struct_size is not set (set it to sizeof(the struct) before the call)");
    const uint32_t w = std::min<uint32_t>(sz, (uint32_t)sizeof(T));
    full.struct_size = w;
    memcpy(out, &full, w);
    return RQ_OK;
}
static inline uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
static inline uint32_t pow2_ceil(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ------------------------------------------------------------------------------------------------
// metrics (src/metrics.rs:65: process-global relaxed atomics)
// ------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_rough{0}, g_precise{0}, g_query{0}, g_miss{0};

// ------------------------------------------------------------------------------------------------
// profiling
// ------------------------------------------------------------------------------------------------
enum { PF_ROTATE = 0, PF_COARSE, PF_SELECT, PF_PREP, PF_GROUP, PF_SCAN, PF_SCAN_MATRIX, PF_RERANK, PF_SORT, PF_REPLAY, PF_EARLY, PF_TOTAL, PF_N };
static std::atomic<int> g_profiling{0};
static thread_local rq_profile_t g_profile;

struct Prof {
    bool on = false;
    bool light = false;  // level 2: only the scan launches and the whole pass are bracketed
    hipStream_t stream = nullptr;
    struct Span {
        hipEvent_t a, b;
        int cat;
    };
    std::vector<Span> spans;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    bool open = false;          // the last begin() was recorded (not filtered out)
    hipEvent_t last_b = nullptr;  // end event of the previous span, reusable as the next begin while nothing ran since
    bool failed = false;  // an event could not be created: this pass reports no timings (never a wrong one)
    hipEvent_t get() {
        if (used == pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess || !e) {
                failed = true;
                on = false;
                return nullptr;
            }
            pool.push_back(e);
        }
        return pool[used++];
    }
    // An event record costs ~5 us of stream time: adjacent spans share their boundary event.
    void begin(int cat) {
        open = on && !(light && cat != PF_SCAN && cat != PF_SCAN_MATRIX && cat != PF_TOTAL);
        if (!open) {
            last_b = nullptr;
            return;
        }
        Span s{last_b, get(), cat};
        if (s.b && !s.a) {
            s.a = get();
            if (s.a) (void)hipEventRecord(s.a, stream);
        }
        last_b = nullptr;
        if (!s.a || !s.b) {  // event creation failed: profiling is off for the rest of the pass
            open = false;
            spans.clear();
            return;
        }
        spans.push_back(s);
    }
    void end() {
        if (!open) return;
        (void)hipEventRecord(spans.back().b, stream);
        last_b = spans.back().b;
        open = false;
    }
    void reset(int level, hipStream_t st) {
        on = level != 0;
        light = level == 2;
        stream = st;
        spans.clear();
        used = 0;
        open = false;
        last_b = nullptr;
        failed = false;
    }
    void collect(float *ms /*PF_N*/) {
        if (failed) return;
        for (auto &s : spans) {
            float t = 0;
            (void)hipEventElapsedTime(&t, s.a, s.b);
            ms[s.cat] += t;
        }
    }
    ~Prof() {
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

// ------------------------------------------------------------------------------------------------
// query workspace
// ------------------------------------------------------------------------------------------------
struct StreamRange {
    uint32_t s_lo, s_hi;
};
#define RQ_MAX_STAGES 40  // stages of one pass (host_plan.h): the geometric schedule ends within 32 doublings of a 32-bit stream position
// context of a pass that has been enqueued but not yet finished: run_pass assigns it once, finish_pass reads it
struct PendingPass {
    uint64_t seg_slots = 0;  // slots of the final stage's segments (0: uniform geometry)
    uint32_t cap = 0;        // uniform capacity of the pass
    uint32_t nq = 0;
    StreamRange matrix_ranges[RQ_MAX_STAGES];  // stream ranges scanned on the matrix cores (profiling only)
    uint32_t n_matrix_ranges = 0;
    const struct rq_filter *filter = nullptr;  // the pass's filter (its stream lengths are in stream_len; its hints)
    bool additive = false;        // the pass ran a matrix-core stage with the additive gate (finish_pass reads its flag rate)
    uint32_t matrix_stages = 0;   // matrix-core stages of the pass
    bool prefiltered = false;     // the pass ranked its lists through the matrix-core pre-filter (totals[12] = rows that fell back)
    bool range = false;           // a range pass (it orders no run directories: the long-directory hint keeps its value)
    bool large = false;           // the pass ran the large-batch form of the stages (PassPlan::large)
};
struct Workspace {
    hipStream_t stream = nullptr;
    bool busy = false;
    PendingPass pend;
    DevBuf<float> qpad, y, dist, probe_dist, thr, recent;
    DevBuf<float> qnorm;  // cosine indexes, small-batch path: N(q), which sb_front_kernel reads in place of the caller's rows
    DevBuf<float> retry_q, retry_pd, retry_pc;  // overflow re-runs: the affected queries (and their probe lists)
    DevBuf<uint32_t> retry_rows;
    DevBuf<uint32_t> q_hist, q_start, q_order;  // rerank order of a large batch (queries grouped by nearest list)
    DevBuf<uint32_t> live_list;                 // sharded passes: the (query, list) pairs whose list has members here, + their count
    DevBuf<uint32_t> probe_n;                   // adaptive probing: per query, the lists its cut row keeps (probe_cut_kernel)
    DevBuf<uint32_t> coarse_redo;               // pre-filtered coarse ranking over more than 8192 lists: rows left to the block-per-query selection
    DevBuf<uint32_t> pair_rank, rank_base;      // group_rank_kernel: places of a big stage's pairs inside their groups
    // final stage placed ahead of the quantisation (option prep_placement): its tile images, the pairs' stream positions, and its own
    // grouping (ws.recs / pair_rank / rank_base / grp_cnt / grp_start serve the early stages in between)
    DevBuf<uint32_t> img_final, pair_begin, fin_rank, fin_rank_base, fin_grp_cnt, fin_grp_start;
    DevBuf<uint32_t> probe_cluster, recs, grp_cnt, grp_start, heap_len, heap_id, precise, need,
        nsurv, nshadow, win_count, arr_len, row_map, big_list;
    DevBuf<int32_t> heap_key;
    DevBuf<PairScalars> scal;
    DevBuf<uint64_t> planes;
    DevBuf<uint32_t> qnib;
    DevBuf<uint32_t> qf6;
    DevBuf<unsigned long long> rough_cnt, totals, surv_cnt, stat;
    DevBuf<unsigned long long> stream_len;  // filtered passes: per query, the stream's length (rough_cnt holds the admitted rows)
    DevBuf<float4> grp_vref;  // additive gate: per list, centre and half-range of v' over the stage's pairs (group_vrange_kernel)
    DevBuf<SurvRec> surv, arr;
    DevBuf<RunRec> runs, runs_tmp;
    bool use_runs_tmp = false;
    bool arena_failed = false;  // the last pass gave up inside an arena stage (no room for the arena): the caller repeats it on the uniform buffers
    // multi-GPU step (rq_query_batch_sharded_device): this shard's results, the all-gathered keys, the merged keys
    DevBuf<float> sh_dist;
    DevBuf<uint32_t> sh_id, sh_n;
    DevBuf<unsigned long long> sh_packed, sh_gathered, sh_merged;
    DevBuf<uint32_t> range_hits;               // range passes (host_range.h): per query, the candidates inside its radius
    DevBuf<uint32_t> range_lists;              //   the segmented sort's three segment lists (by length class) ...
    DevBuf<unsigned long long> range_counters; //   ... and their lengths + the longest segment
    DevBuf<uint32_t> ovf, q_cap;               // per query: overflow flag; segment capacity of the final stage (segmented passes)
    DevBuf<unsigned long long> q_base;         // per query: first slot of its segment
    DevBuf<SurvRec> arena_recs;                // arena stages: survivors of all queries, unordered (256 shards)
    DevBuf<RunRec> arena_runs;                 //   their run descriptors as uint4 {pos, slot | cnt << 16, query, offset}
    DevBuf<uint2> arena_places;                //   per descriptor: the run's place in its query's segment {first record, directory slot}
    DevBuf<unsigned long long> arena_cur;      //   RQ_ARENA_SHARDS shard cursors (records | runs << 32), overflow flag, total, cursor of the common area
    DevBuf<unsigned int> arena_fail;           //   per shard: first run index it turned away
    DevBuf<ScanExtra> scan_extra;              //   what the scan reads on its survivor path in arena mode
    DevBuf<uint32_t> sh_flag;                 // handshake / status words of the step
    DevBuf<uint32_t> sh_pc, sh_id_b, sh_n_b;  // shared-threshold step: probe lists (whole | nearest | rest), second call's results
    DevBuf<float> sh_pd, sh_thr, sh_dist_b;
    // by-id calls (host_directory.h): positions of the asked ids, the gathered query rows of rq_neighbours_of and its plain call's results
    DevBuf<uint32_t> id_pos, id_res_id, id_res_n;
    DevBuf<float> id_rows, id_rows_raw, id_res_dist;
    DevBuf<unsigned long long> id_found;
    unsigned long long *h_totals = nullptr;  // pinned, 16
    Prof prof;
    ~Workspace() {
        if (h_totals) (void)hipHostFree(h_totals);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The metric of an index (what it decides is in host_metric.h).  RQ_METRIC_COSINE: raw rows were normalised on their way in, raw
// queries are on theirs.  RQ_METRIC_IP: rows of d floats were augmented (A(x; S), slot d = sqrtf(S - |x|^2)) on their way in, dim =
// ceil64(d + 1); queries have exactly d floats and are zero-padded to dim by the ordinary pad path.  d and S are zero otherwise.
struct MetricSpec {
    uint32_t id = RQ_METRIC_L2;
    uint32_t d = 0;
    float S = 0.0f;
};

// The id directory of an index (host_directory.h, kernels_directory.h): id -> position, read-only, made on the first
// by-id call of a generation.  One of its two buffers is set.
struct IdDirectory {
    uint64_t generation = 0;  // idx->generation it was made for
    uint64_t top = 0;         // 1 + the largest stored id (0: an empty index)
    uint32_t bits = 0;        // hash form: log2 of the table's capacity
    DevBuf<uint32_t> dense;   // dense form: top entries
    DevBuf<unsigned long long> slots;  // hash form: 2^bits slots
    bool hashed = false;
    uint64_t bytes = 0;       // of the buffer
    float ms_build = 0.0f;    // wall time of the build, the scan for `top` included
    uint32_t longest_chain = 0;  // hash form: slots the worst insertion looked at
};

// One attribute column of an index (host_attr.h, kernels_attr.h): n elements of 4 or 8 bytes in position order.
struct AttrColumn {
    std::string name;
    uint32_t type = 0;   // RQ_ATTR_*
    uint64_t fill = 0;   // the u64 image of the fill value (a 4-byte type: the high word is zero)
    DevBuf<uint8_t> data;
};

struct rq_index {
    uint32_t dim = 0, k = 0, W = 0, max_list_len = 0;
    uint32_t min_list_len = 0;  // 0 if some list is empty (then no slot bound can be derived from stream positions)
    uint64_t n = 0;
    MetricSpec metric;
    // raw vectors (cluster order, un-rotated).  Untiered (n_dev == n, the usual case): row p at base + p*dim.  Tiered
    // (they do not fit the HBM budget): per list the first h_c members in HBM, the tail in pinned host memory mapped
    // into the device address space (BaseView / ListTier); n_dev = sum of h_c.
    uint64_t n_dev = 0;
    float *base_host = nullptr;      // hipHostMalloc'ed (mapped); host address
    float *base_host_dev = nullptr;  // the same memory as the kernels address it
    DevBuf<ListTier> list_tier;      // k entries, tiered indexes only
    std::vector<ListTier> h_list_tier;
    bool split_rows = false;         // the raw vectors are split rows (common.h; set with the tiers, tiered indexes only)
    // the row type (rows.h): a half-precision index keeps the caller's 2-byte elements in `base` (n x dim of them, 2*dim bytes per row, padding
    // +0), a byte-row index (RQ_ROWS_U8 / RQ_ROWS_I8) the caller's one-byte elements (dim bytes per row, padding 0x00): always
    // untiered, never split, no shadow rows, never mutated
    RowSpec rows;
    size_t row_bytes() const { return rows.row_bytes(dim); }
    BaseView view() const { return BaseView{base.p, base_host_dev, list_tier.p, k, split_rows ? 1u : 0u, rows.id}; }
    ~rq_index();  // (defined below struct rq_filter: it frees the live filter)
    DevBuf<float> base, P, centroids, cent_t;
    DevBuf<_Float16> base_h;  // fp16 shadow of `base` (rerank pre-filter, derived; untiered indexes with HBM to spare; option rerank_shadow = 1)
    DevBuf<uint8_t> base_q8;  // 8-bit shadow of `base`, one affine map per list (the default pre-filter: half the fp16 shadow's bytes per survivor)
    DevBuf<float4> list_q8;   //   per list: {lo, s, max |x_i - x^_i| over the list's rows, -}
    DevBuf<uint32_t> offsets, map_ids;
    DevBuf<uint64_t> codes;
    DevBuf<float4> factors;
    DevBuf<float4> list_uref;  // per list: mean of u' = (1, cds, ., eb) / factor_ip over its regular vectors (additive gate of the matrix-core scan; derived)
    DevBuf<uint16_t> cent_bf;  // k x dim bf16 image of the rotated centroids and their squared norms (coarse pre-filter; derived)
    DevBuf<float> cent_sqnorm;
    float cent_norm_max = INFINITY;  // largest centroid norm (inf: no pre-filter)
    uint32_t nonempty_lists = 0;  // lists with at least one vector (a shard of a multi-GPU index owns only some of the k lists)
    std::atomic<int> additive_loose{0};  // the additive gate flagged too many sub-tile steps on this index: later passes use the bf16 threshold
    std::mutex ws_mu;
    std::vector<std::unique_ptr<Workspace>> ws_pool;
    FactorStats fstats{0, 0, 0, 0};
    std::atomic<uint32_t> cap_hint{0};  // survivor-buffer capacity learnt from earlier batches
    std::atomic<uint64_t> arena_hint{0};  // slots the largest arena stage of earlier batches needed (+ headroom)
    std::atomic<uint32_t> big_dirs_hint{0};  // most long run directories (> 512 runs) a stage of a recent pass produced
    std::atomic<uint32_t> exact_cap_hint{0};  // candidate slots per query the exact search learnt on this index (host_exact.h)
    std::atomic<uint32_t> range_cap_hint{0};  // survivor-buffer capacity learnt from range passes most of whose queries overflowed (host_range.h)
    std::atomic<uint32_t> exact_range_cap_hint{0};  // arena records per query the exact range search learnt on this index (host_exact_range.h)
    uint64_t pass_budget = 24ull << 30;  // bytes of survivor / run buffers one query pass may use (set by finish_index)
    // tile tables of the cluster-major scans: per tile size, one {list, first, list begin, list length} entry per
    // existing (list, tile); built on first use from the host copy of the offsets
    std::vector<uint32_t> h_offsets;
    std::mutex tt_mu;
    std::map<uint32_t, std::unique_ptr<DevBuf<uint4>>> tile_tables;
    // in-place mutation (host_mutate.h)
    DevBuf<uint32_t> row_key;     // per position: ord32_biased(distance to its list's centroid), the high word of the build's order key (derived, not dumped)
    bool row_key_valid = false;   // computed on the first mutation (again after a load); moved along by every relayout
    bool row_order_ok = true;     // every list strictly ascending by row_key << 32 | id (checked with the keys; rq_add needs it)
    bool is_shard = false;        // made by rq_shard_index: added ids would collide with other ranks' ids, so it is never mutated
    uint64_t generation = 0;      // bumped by every relayout; a filter made for an older generation is refused
    std::atomic<int> open_tickets{0};  // rq_query_batch_device_begin tickets whose _end has not run
    // lazy removal (rq_remove_lazy): the filter of the live rows, owned; null while no removal is pending.  Every query
    // entry that has a filtered form runs under it when the caller brings no filter of their own (live_or).  Updated in place by
    // rq_remove_lazy (its hints stay), dropped by every relayout (commit_layout).
    struct rq_filter *live = nullptr;
    // rows by id (host_directory.h): null until the first by-id call of this generation; dropped by every relayout (commit_layout).
    // No query path reads it.
    std::mutex dir_mu;
    std::unique_ptr<IdDirectory> dir;
    uint64_t removal_epoch = 0;   // bumped by every rq_remove_lazy that marks a row; a filter made under an older epoch is refused
    // attribute columns (host_attr.h), in rq_attr_info order; empty on an index that was given none.  Moved along by every relayout.
    std::vector<std::unique_ptr<AttrColumn>> attrs;
    inline uint64_t pending() const;  // stored rows that are dead
};

// A query-time allow-list (rq_filter_create), in the index's own terms: one bit per cluster-order position and the admitted rows
// of every list.  Made once, read-only afterwards (concurrent queries share it).
struct rq_filter {
    const rq_index *idx = nullptr;  // the index it was made for (another index is refused)
    uint64_t generation = 0;        // idx->generation when it was made (a relayout since then: refused)
    DevBuf<uint32_t> pos_bits;      // bit pos of word pos >> 5 = the row at position pos is admitted
    DevBuf<uint32_t> sub_off;       // k + 1: list offsets of the sub-index (admitted rows of list c = sub_off[c + 1] - sub_off[c])
    DevBuf<ScanExtra> extra;        // what the filtered scans read through ScanArgs::x outside arena stages: only `allow` is set
    uint64_t rows = 0;              // admitted rows of the whole index
    uint64_t live_rows = 0;         // stored rows of the lists that admit anything (rows / live_rows: the filter's density inside the lists a pass scans)
    // what its passes learnt about their survivor buffers (as rq_index::cap_hint / arena_hint / big_dirs_hint): a filter whose rows
    // are far from the queries lets many more candidates through than the unfiltered query, and must not resize the index's
    // unfiltered passes -- nor they its
    std::atomic<uint32_t> cap_hint{0};
    std::atomic<uint64_t> arena_hint{0};
    std::atomic<uint32_t> big_dirs_hint{0};
    std::atomic<uint32_t> exact_cap_hint{0};  // as rq_index::exact_cap_hint, for the exact searches under this filter
    std::atomic<uint32_t> exact_range_cap_hint{0};  // as rq_index::exact_range_cap_hint, for the exact range searches under this filter
    uint64_t removal_epoch = 0;     // idx->removal_epoch when it was made (a marking rq_remove_lazy since then: refused)
    std::vector<uint32_t> h_sub_off;  // host copy of sub_off (k + 1)
};
inline rq_index::~rq_index() {
    if (base_host) (void)hipHostFree(base_host);
    delete live;
}
inline uint64_t rq_index::pending() const { return live ? n - live->rows : 0; }
// The filter a query entry runs under: the caller's, else the index's live filter (null while no removal is pending).  A caller's
// filter made on an index with pending removals already excludes the dead rows (rq_filter_create).
static const rq_filter *live_or(const rq_index *idx, const rq_filter *filter) { return filter ? filter : (idx ? idx->live : nullptr); }
static const char *const kPendingRefusal = "pending removals: rq_compact first (this entry has no filtered form, and a dump would bring the dead rows back)";
// The learnt survivor-buffer hints a pass reads and updates: the index's own, or the filter's on a filtered pass.
struct PassHints {
    std::atomic<uint32_t> &cap;
    std::atomic<uint64_t> &arena;
    std::atomic<uint32_t> &big_dirs;
};
static PassHints hints_of(const rq_index *idx, const rq_filter *f) {
    if (f) {
        rq_filter *m = const_cast<rq_filter *>(f);
        return PassHints{m->cap_hint, m->arena_hint, m->big_dirs_hint};
    }
    rq_index *m = const_cast<rq_index *>(idx);
    return PassHints{m->cap_hint, m->arena_hint, m->big_dirs_hint};
}

static Workspace *ws_acquire(rq_index *idx) {
    std::lock_guard<std::mutex> g(idx->ws_mu);
    for (auto &w : idx->ws_pool)
        if (!w->busy) {
            w->busy = true;
            return w.get();
        }
    idx->ws_pool.emplace_back(new Workspace());
    idx->ws_pool.back()->busy = true;
    return idx->ws_pool.back().get();
}
static void ws_release(rq_index *idx, Workspace *w) {
    std::lock_guard<std::mutex> g(idx->ws_mu);
    w->busy = false;
}
// A workspace's stream and pinned block, made on its first use.
static rq_status ws_ensure_stream(Workspace &ws) {
    if (!ws.stream) HIPC(hipStreamCreateWithFlags(&ws.stream, hipStreamNonBlocking));
    if (!ws.h_totals) HIPC(hipHostMalloc((void **)&ws.h_totals, 16 * sizeof(unsigned long long)));
    return RQ_OK;
}
// A workspace held for a scope: goes back to the index's pool at its end (w == nullptr: nothing held).
struct WsLease {
    rq_index *idx;
    Workspace *w;
    WsLease(rq_index *i, Workspace *ws) : idx(i), w(ws) {}
    WsLease(const WsLease &) = delete;
    WsLease &operator=(const WsLease &) = delete;
    ~WsLease() { if (w) ws_release(idx, w); }
};

// ------------------------------------------------------------------------------------------------
// small init kernels
// ------------------------------------------------------------------------------------------------
__global__ void fill_f32_kernel(float *p, float v, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void gather_rows_kernel(const float *__restrict__ in, const uint32_t *__restrict__ rows,
                                   uint32_t nrows, uint32_t len, float *__restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nrows * len) return;
    uint32_t r = (uint32_t)(i / len), c = (uint32_t)(i - (uint64_t)r * len);
    out[i] = in[(uint64_t)rows[r] * len + c];
}

// ------------------------------------------------------------------------------------------------
// multi-GPU helpers: carving a shard out of an index, (distance, id) <-> u64 merge keys
// ------------------------------------------------------------------------------------------------
// one wave per destination position p of the shard: its list c is found by bisection over the shard's offsets,
// its source position is old_offsets[c] + (p - new_offsets[c])
__global__ __launch_bounds__(256) void shard_gather_kernel(const uint32_t *__restrict__ new_off, const uint32_t *__restrict__ old_off,
                                                           uint32_t k, uint64_t n_local, uint32_t dim,
                                                           const BaseView base_in, const uint64_t *__restrict__ codes_in,
                                                           const float4 *__restrict__ factors_in, const uint32_t *__restrict__ ids_in,
                                                           const BaseView base_out, uint64_t *__restrict__ codes_out,
                                                           float4 *__restrict__ factors_out, uint32_t *__restrict__ ids_out) {
    const uint32_t lane = threadIdx.x & 63, W = dim >> 6;
    for (uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < n_local; p += (uint64_t)gridDim.x * 4) {
        uint32_t lo = 0, hi = k;  // largest c with new_off[c] <= p (empty lists share their start with the next one)
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (new_off[mid] <= p) lo = mid;
            else hi = mid;
        }
        const uint64_t src = (uint64_t)old_off[lo] + (p - new_off[lo]);
        const RowRef srow = base_in.row(src, dim), drow = base_out.row(p, dim);
        if (RowSpec{base_in.fmt}.bytes() || RowSpec{base_out.fmt}.bytes()) {  // (a shard inherits the row type: bytes are copied as they are)
            const uint8_t *s = reinterpret_cast<const uint8_t *>(srow.p);
            uint8_t *d = reinterpret_cast<uint8_t *>(const_cast<float *>(drow.p));
            for (uint32_t e = lane; e < dim; e += 64) d[e] = s[e];
        } else {  // (fmt & 3: no byte type here -- said so that the loop is compiled without the byte forms of get / put, as it was)
            const RowRef s{srow.p, srow.split, srow.fmt & 3u}, d{drow.p, drow.split, drow.fmt & 3u};
            for (uint32_t e = lane; e < dim; e += 64) rq_row_put(d, dim, e, rq_row_get(s, dim, e));
        }
        for (uint32_t w = lane; w < W; w += 64) codes_out[p * W + w] = codes_in[src * W + w];
        if (lane == 0) {
            factors_out[p] = factors_in[src];
            ids_out[p] = ids_in[src];
        }
    }
}
// per-shard top-k -> merge keys (Ord32 image << 32 | global id); entries past the valid count sort last
__global__ void pack_topk_keys_kernel(const float *__restrict__ dist, const uint32_t *__restrict__ id, const uint32_t *__restrict__ cnt,
                                      uint32_t nq, uint32_t topk, uint32_t id_offset, unsigned long long *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nq * topk) return;
    const uint32_t b = (uint32_t)(i / topk), e = (uint32_t)(i - (uint64_t)b * topk);
    keys[i] = e < cnt[b] ? (((unsigned long long)ord32_biased(dist[i]) << 32) | (uint32_t)(id[i] + id_offset)) : ~0ull;
}
// shared-threshold multi-GPU step: the merged probe lists split into the nearest list and the rest
__global__ void split_probe_kernel(const uint32_t *__restrict__ pc, const float *__restrict__ pd, uint32_t nq, uint32_t npb,
                                   uint32_t *__restrict__ pc_a, float *__restrict__ pd_a, uint32_t *__restrict__ pc_b,
                                   float *__restrict__ pd_b) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nq * npb) return;
    const uint32_t b = (uint32_t)(i / npb), c = (uint32_t)(i - (uint64_t)b * npb);
    if (c == 0) pc_a[b] = pc[i], pd_a[b] = pd[i];
    else pc_b[(uint64_t)b * (npb - 1) + c - 1] = pc[i], pd_b[(uint64_t)b * (npb - 1) + c - 1] = pd[i];
}
// a query's seed threshold: the k-th best distance its nearest list gave, if the list gave k; f32::MAX otherwise
__global__ void kth_threshold_kernel(const float *__restrict__ dist, const uint32_t *__restrict__ cnt, uint32_t nq, uint32_t topk,
                                     float *__restrict__ thr) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nq) return;
    float m = 3.402823466e+38f;
    if (cnt[b] == topk) {
        m = dist[(uint64_t)b * topk];
        for (uint32_t e = 1; e < topk; ++e) m = dist[(uint64_t)b * topk + e] > m ? dist[(uint64_t)b * topk + e] : m;
    }
    thr[b] = m;
}
// per-shard top-k -> merge keys, written at columns [col0, col0 + topk) of rows of `width` keys
__global__ void pack_topk_keys_at_kernel(const float *__restrict__ dist, const uint32_t *__restrict__ id, const uint32_t *__restrict__ cnt,
                                         uint32_t nq, uint32_t topk, uint32_t id_offset, uint32_t width, uint32_t col0,
                                         unsigned long long *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nq * topk) return;
    const uint32_t b = (uint32_t)(i / topk), e = (uint32_t)(i - (uint64_t)b * topk);
    keys[(uint64_t)b * width + col0 + e] =
        e < cnt[b] ? (((unsigned long long)ord32_biased(dist[i]) << 32) | (uint32_t)(id[i] + id_offset)) : ~0ull;
}
__global__ void unpack_topk_keys_kernel(const unsigned long long *__restrict__ keys, uint32_t nq, uint32_t topk,
                                        float *__restrict__ dist, uint32_t *__restrict__ id, uint32_t *__restrict__ cnt) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nq) return;
    uint32_t c = 0;
    for (uint32_t e = 0; e < topk; ++e) {
        const unsigned long long key = keys[(uint64_t)b * topk + e];
        if (key == ~0ull) break;  // ascending: the padding comes last
        dist[(uint64_t)b * topk + e] = ord32_unbias((uint32_t)(key >> 32));
        id[(uint64_t)b * topk + e] = (uint32_t)key;
        ++c;
    }
    cnt[b] = c;
}
