// host_metric.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  Everything that depends on an index's metric, each decision once: what a MetricSpec
// (host_state.h, next to struct rq_index) allows, the row transform (raw rows -> what the index stores), the query transform (raw
// queries -> what gets rotated) and the metric's stored tag.  A new metric, or a change to how one treats its input, belongs here.
#pragma once

// ---- the spec: lengths, validity, refusals ----
static uint32_t ceil64(uint32_t v) { return (v + 63) / 64 * 64; }
static MetricSpec metric_ip(uint32_t d, float S) { return MetricSpec{RQ_METRIC_IP, d, S}; }
// the index dim of raw rows of `raw` floats (rabitq.rs:168-179; an inner-product index keeps one more coordinate, slot d)
static uint32_t metric_dim(const MetricSpec &m, uint32_t raw) { return ceil64(raw + (m.id == RQ_METRIC_IP ? 1u : 0u)); }

// The ids the *_metric entries take: they carry no d / S, so RQ_METRIC_IP has the _ip entries.
static rq_status metric_entry_check(uint32_t id) {
    if (id == RQ_METRIC_L2 || id == RQ_METRIC_COSINE) return RQ_OK;
    return fail(RQ_ERR_INVALID, "unknown metric " + std::to_string(id) +
                                    (id == RQ_METRIC_IP ? ": the inner-product metric takes a row length and a norm bound, use the _ip entries" : ""));
}

// An inner-product index: d in [1, 4095], so that dim = ceil64(d + 1) <= 4096 -- and is the caller's dim (0: it has none yet); S finite
// and >= 0.  The loaders answer RQ_ERR_IO where either fails, rq_from_arrays_ip RQ_ERR_DIM_MISMATCH to the first.
static bool ip_d_ok(uint32_t d, uint32_t dim = 0) { return d >= 1 && d <= 4095 && (dim == 0 || ceil64(d + 1) == dim); }
static bool ip_bound_ok(float S) { return S >= 0.0f && S <= 3.402823466e+38f; }
// ... as the entries that take a raw row length refuse it, before anything is staged or allocated for it
static rq_status ip_d_check(uint32_t d) {
    return ip_d_ok(d) ? RQ_OK : fail(d ? RQ_ERR_UNSUPPORTED : RQ_ERR_INVALID, "d must be in [1, 4095] for the inner-product metric");
}

// The values a centroid record of a build may hold for rows of d floats: d; an inner-product build d .. ceil64(d + 1) (a caller who
// trains on augmented rows passes the slot, or whole padded rows; missing columns are zero).
static bool metric_centroid_cols_ok(const MetricSpec &m, uint32_t d, uint32_t cols) {
    return m.id == RQ_METRIC_IP ? cols >= d && cols <= metric_dim(m, d) : cols == d;
}

// The length a raw query or a raw added row of this index must have (rabitq.rs:275), and the one refusal of another (what: "query" / "row").
static rq_status raw_len_check(const rq_index *idx, const char *what, uint32_t len) {
    const MetricSpec &m = idx->metric;
    if (m.id == RQ_METRIC_IP ? len == m.d : (len != 0 && idx->dim == ceil64(len))) return RQ_OK;
    const std::string head = std::string(what) + " length " + std::to_string(len);
    if (m.id == RQ_METRIC_IP) return fail(RQ_ERR_DIM_MISMATCH, head + " is not the inner-product index's row length " + std::to_string(m.d));
    return fail(RQ_ERR_DIM_MISMATCH, head + " does not pad to index dim " + std::to_string(idx->dim));
}

// the spec folded into the sharded step's handshake hash (ranks must agree on it)
static uint32_t metric_hash(const MetricSpec &m, uint32_t h) {
    for (uint32_t v : {m.id, m.d, __builtin_bit_cast(uint32_t, m.S)}) h = (h ^ v) * 0x01000193u;
    return h;
}

// ---- launchers of the row kernels (normalize_rows_kernel, augment_rows_kernel, row_sqnorm_kernel: one chain, RQ_SQCHAIN_* in kernels_build.h) ----
// The launch shape the three share: RW rows per wave (dim <= 4096), their LDS image, a grid-stride grid, and whether both ends allow 16-byte accesses.
struct SqnormLaunch {
    uint32_t vec, rw, grid;
    size_t lds;
    SqnormLaunch(const float *in, const float *out, uint64_t n, uint32_t d, uint32_t dim) {
        vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
        rw = dim <= 512 ? 8 : dim <= 1024 ? 4 : dim <= 2048 ? 2 : 1;
        lds = ((size_t)rw * (dim + 8) + rw) * sizeof(float);
        grid = (uint32_t)std::min<uint64_t>(ceil_div(n, rw), 256u * 10u * 8u);  // grid-stride: ten waves per CU, eight rounds
    }
    template <typename F>
    void with_rw(F &&f) const {  // f(integral_constant<RW>): the instantiation of this shape
        switch (rw) {
            case 8: f(std::integral_constant<int, 8>{}); break;
            case 4: f(std::integral_constant<int, 4>{}); break;
            case 2: f(std::integral_constant<int, 2>{}); break;
            default: f(std::integral_constant<int, 1>{}); break;
        }
    }
};
// Cosine metric: pad + normalise n rows of length d (normalize_rows_kernel).  place == nullptr: into the dense n x dim `out`;
// else row r goes to position place[i0 + r] of `view` (the build's pass 2).  dim <= 4096.
static void launch_normalize(const float *in, uint64_t n, uint32_t d, uint32_t dim, float *out, hipStream_t st,
                             const uint32_t *place = nullptr, uint64_t i0 = 0, const BaseView view = BaseView{}) {
    if (n == 0) return;
    const SqnormLaunch L(in, out, n, d, dim);
    L.with_rw([&](auto rw) {
        constexpr int RW = decltype(rw)::value;
        if (place) normalize_rows_kernel<RW, true><<<L.grid, 64, L.lds, st>>>(in, n, d, dim, L.vec, nullptr, place, i0, view);
        else normalize_rows_kernel<RW, false><<<L.grid, 64, L.lds, st>>>(in, n, d, dim, L.vec, out, nullptr, 0, view);
    });
}
// s of n rows (row_sqnorm_kernel); stat: three device words preset to {0, 0xFFFFFFFF, 0}; rows are numbered from i0 in stat[1]
static void launch_row_sqnorm(const float *in, uint64_t n, uint32_t d, uint32_t dim, float sq_bound, uint64_t i0, float *out_s,
                              uint32_t *stat, hipStream_t st) {
    if (n == 0) return;
    const SqnormLaunch L(in, nullptr, n, d, dim);
    L.with_rw([&](auto rw) { row_sqnorm_kernel<decltype(rw)::value><<<L.grid, 64, L.lds, st>>>(in, n, d, dim, L.vec, sq_bound, i0, out_s, stat); });
}
static const uint32_t RQ_SQNORM_STAT_INIT[3] = {0u, 0xFFFFFFFFu, 0u};

// ---- the row transform: raw rows -> what the index stores (cosine N(x), inner product A(x; S), otherwise the padded row) ----
#define RQ_NO_BAD_ROW 0xFFFFFFFFu
// The refusal of row `bad` (RQ_NO_BAD_ROW: none) whose squared norm is not finite or, where a bound applied, exceeds it.
// where: what follows the row number (":" / " of the batch:"); bound: what the bound is called (nullptr: none applied).
static rq_status bad_row_refusal(uint32_t bad, const char *where, const char *bound) {
    if (bad == RQ_NO_BAD_ROW) return RQ_OK;
    return fail(RQ_ERR_INVALID, "row " + std::to_string(bad) + where + " its squared norm is not finite" + (bound ? std::string(" or exceeds ") + bound : ""));
}
// ... of the first row the inner-product transform just refused (the device word it recorded it in; synchronises)
static rq_status bad_row_check(const uint32_t *d_bad_row, const char *where, const char *bound) {
    uint32_t bad = RQ_NO_BAD_ROW;
    HIPC(hipMemcpy(&bad, d_bad_row, 4, hipMemcpyDeviceToHost));
    return bad_row_refusal(bad, where, bound);
}

// whether the row transform of this metric can refuse a row (the caller then owns a bad_row word and asks bad_row_check)
static bool metric_refuses_rows(const MetricSpec &m) { return m.id == RQ_METRIC_IP; }
// n raw rows of d floats (device), numbered from i0 -> the rows of an index of this spec, on the null stream: densely into `out`
// (n x dim), or (place != nullptr) row r to position place[i0 + r] of `view`.  Dense: *rows is where they are -- `out`, or `in`
// itself when an L2 row needs no padding (nothing is launched then).  Inner product (augment_rows_kernel): s_pre (nullable) holds s
// of row r at s_pre[i0 + r]; bad_row (a metric that refuses rows) is the device word the first refused row lands in.
static rq_status transform_rows(const MetricSpec &m, uint32_t dim, const float *in, uint64_t n, uint32_t d, uint64_t i0, float *out,
                                const uint32_t *place, const BaseView view, const float *s_pre, uint32_t *bad_row, const float **rows = nullptr) {
    if (rows) *rows = out;
    if (m.id == RQ_METRIC_COSINE) {  // pad + normalise in one launch: everything behind it sees N(x)
        launch_normalize(in, n, d, dim, out, nullptr, place, i0, view);
    } else if (m.id == RQ_METRIC_IP) {  // pad + augment in one launch: everything behind it sees A(x)
        HIPC(hipMemset(bad_row, 0xFF, 4));
        const SqnormLaunch L(in, out, n, d, dim);
        if (n) L.with_rw([&](auto rw) {
            constexpr int RW = decltype(rw)::value;
            if (place) augment_rows_kernel<RW, true><<<L.grid, 64, L.lds>>>(in, n, d, dim, L.vec, m.S, s_pre, nullptr, place, i0, view, bad_row);
            else augment_rows_kernel<RW, false><<<L.grid, 64, L.lds>>>(in, n, d, dim, L.vec, m.S, s_pre, out, nullptr, i0, view, bad_row);
        });
    } else if (place) {
        if (n) place_rows_kernel<<<(uint32_t)std::min<uint64_t>(ceil_div(n, 4), 1u << 20), 256>>>(in, i0, n, d, dim, place, view);
    } else if (d != dim) {
        if (n) pad_rows_kernel<<<ceil_div(n * dim, 256), 256>>>(in, out, n, d, dim);
    } else if (rows) {
        *rows = in;
    }
    return RQ_OK;
}

// ---- the query transform: raw queries -> the rows that get rotated ----
// nq raw queries of len floats (device) -> *out, rows of *out_len floats (nullable: who asked for padded rows knows it is dim).
// Cosine: N(q), padded to dim, in `scratch` (one launch, also when nothing is padded: rotation and rerank see N(q)).  Otherwise the
// queries zero-padded to dim in `scratch` when want_padded and len != dim; else the input itself (the small-batch front kernel pads
// while it loads).  `scratch` is grown as needed.
static rq_status transform_queries(const rq_index *idx, const float *d_q, uint32_t nq, uint32_t len, bool want_padded, DevBuf<float> &scratch,
                                   hipStream_t st, const float **out, uint32_t *out_len = nullptr) {
    const uint32_t dim = idx->dim;
    const bool cosine = idx->metric.id == RQ_METRIC_COSINE;
    const bool untouched = !cosine && !(want_padded && len != dim);
    if (out_len) *out_len = untouched ? len : dim;
    *out = d_q;
    if (untouched) return RQ_OK;
    RQC(scratch.ensure((uint64_t)nq * dim));
    if (cosine) launch_normalize(d_q, nq, len, dim, scratch.p, st);
    else pad_rows_kernel<<<ceil_div((uint64_t)nq * dim, 256), 256, 0, st>>>(d_q, scratch.p, nq, len, dim);
    *out = scratch.p;
    return RQ_OK;
}

// ---- the stored tag: the `metric` file of a dumped directory, the metric members of a JSON dump ----
// "cosine\n", "ip <d> <S as 8 lower-case hex digits>\n"; empty for L2 (an L2 dump stays the crate's five files)
static std::string metric_file_text(const MetricSpec &m) {
    if (m.id == RQ_METRIC_COSINE) return "cosine\n";
    if (m.id != RQ_METRIC_IP) return "";
    char text[32];
    snprintf(text, sizeof text, "ip %u %08x\n", m.d, __builtin_bit_cast(uint32_t, m.S));
    return text;
}
// false: not a text metric_file_text writes, nor "l2\n"
static bool metric_from_file_text(const std::string &text, MetricSpec *m) {
    *m = MetricSpec{};
    if (text == "l2\n") return true;
    unsigned d = 0, bits = 0;
    if (text == "cosine\n") m->id = RQ_METRIC_COSINE;
    else if (sscanf(text.c_str(), "ip %u %8x", &d, &bits) == 2) *m = metric_ip(d, __builtin_bit_cast(float, (uint32_t)bits));
    else return false;
    return text == metric_file_text(*m);  // exactly as written: no other spelling of the same numbers
}
// ",\"metric\":...": nothing for L2; unknown members to the reference's serde derive, which ignores them
static std::string metric_json_members(const MetricSpec &m) {
    if (m.id == RQ_METRIC_COSINE) return ",\"metric\":\"cosine\"";
    if (m.id != RQ_METRIC_IP) return "";
    return ",\"metric\":\"ip\",\"ip_d\":" + std::to_string(m.d) + ",\"ip_sq_bound_bits\":" + std::to_string(__builtin_bit_cast(uint32_t, m.S));
}
// name: the "metric" member's value as it stands in the text (empty: absent); ip_d, ip_bits: those members, 2^32 where absent (read only for "ip")
static bool metric_from_json(const std::string &name, unsigned long long ip_d, unsigned long long ip_bits, MetricSpec *m) {
    *m = MetricSpec{};
    if (name.empty() || name == "\"l2\"") return true;
    if (name == "\"cosine\"") m->id = RQ_METRIC_COSINE;
    else if (name == "\"ip\"" && !(ip_d >> 32) && !(ip_bits >> 32)) *m = metric_ip((uint32_t)ip_d, __builtin_bit_cast(float, (uint32_t)ip_bits));
    else return false;
    return true;
}
