// host_attr.h -- part of the host side of librabitq_hip.so (one translation unit: rabitq_hip.hip includes the host_*.h files in order;
// they are not stand-alone headers).  Attribute columns (kernels_attr.h): the columns of an index and their entries
// (rq_attr_*), how they follow a relayout, a shard and a dump (columns_follow, columns_shard, attr_dump_dir / attr_load_dir), the
// predicate filter (rq_filter_create_where) and the small entries on a filter's bitmap (rq_filter_combine, _id_bits, _ids_device).
// Merging: a row of src brings src's value where src has a column of the same name and type, else it holds dst's fill; columns that
// only src has are not taken.
#pragma once

static thread_local rq_where_stats_t g_where_stats;  // the calling thread's last rq_filter_create_where (rq_last_where_stats)

// ---- columns ---------------------------------------------------------------------------------------------------------------------------
static uint32_t attr_elem(uint32_t type) { return type >= RQ_ATTR_U64 ? 8u : 4u; }
static uint64_t attr_image(uint32_t type, rq_attr_value_t v) { return attr_elem(type) == 8 ? v.u64 : (uint64_t)v.u32; }
static uint32_t attr_grid(uint64_t count) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(count, 256), 2048)); }
static bool attr_name_ok(const char *name) {
    size_t len = 0;
    for (; name[len]; ++len) {
        const char c = name[len];
        if (len >= 31 || !((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_')) return false;
    }
    return len >= 1;
}
static int attr_find(const rq_index *idx, const std::string &name) {
    for (size_t i = 0; i < idx->attrs.size(); ++i)
        if (idx->attrs[i]->name == name) return (int)i;
    return -1;
}
// what every entry that names a column starts with: nulls and the name's form before anything of the index is read
static rq_status attr_named(const rq_index *idx, const char *name, bool args_null, AttrColumn **out) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    if (!name || args_null) return fail(RQ_ERR_INVALID, "null argument");
    if (!attr_name_ok(name)) return fail(RQ_ERR_INVALID, "a column name is 1-31 bytes of [A-Za-z0-9_]");
    const int i = attr_find(idx, name);
    if (i < 0) return fail(RQ_ERR_INVALID, std::string("the index has no column named ") + name);
    *out = idx->attrs[(size_t)i].get();
    return RQ_OK;
}
// a new column of n elements in device memory, not yet part of an index
static rq_status attr_new_column(const std::string &name, uint32_t type, uint64_t fill, uint64_t n, std::unique_ptr<AttrColumn> &out) {
    out.reset(new AttrColumn());
    out->name = name, out->type = type, out->fill = fill;
    return out->data.alloc(n * attr_elem(type));
}

static rq_status attr_create(rq_index *idx, const char *name, uint32_t type, rq_attr_value_t fill) {
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    if (!name) return fail(RQ_ERR_INVALID, "null argument");
    if (!attr_name_ok(name)) return fail(RQ_ERR_INVALID, "a column name is 1-31 bytes of [A-Za-z0-9_]");
    if (type > RQ_ATTR_I64) return fail(RQ_ERR_INVALID, "unknown column type " + std::to_string(type) + " (RQ_ATTR_U32 .. RQ_ATTR_I64)");
    RQC(ensure_device());
    if (attr_find(idx, name) >= 0) return fail(RQ_ERR_INVALID, std::string("the index already has a column named ") + name);
    if (idx->attrs.size() >= RQ_ATTR_MAX_COLUMNS) return fail(RQ_ERR_UNSUPPORTED, "an index holds at most 16 columns");
    std::unique_ptr<AttrColumn> c;
    RQC(attr_new_column(name, type, attr_image(type, fill), idx->n, c));
    if (idx->n) {
        if (attr_elem(type) == 8) attr_fill_kernel<uint64_t><<<attr_grid(idx->n), 256>>>(reinterpret_cast<uint64_t *>(c->data.p), idx->n, c->fill);
        else attr_fill_kernel<uint32_t><<<attr_grid(idx->n), 256>>>(reinterpret_cast<uint32_t *>(c->data.p), idx->n, (uint32_t)c->fill);
    }
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    idx->attrs.push_back(std::move(c));
    return RQ_OK;
}
static rq_status attr_drop(rq_index *idx, const char *name) {
    AttrColumn *c = nullptr;
    RQC(attr_named(idx, name, false, &c));
    idx->attrs.erase(idx->attrs.begin() + attr_find(idx, name));
    return RQ_OK;
}
static rq_status attr_info(const rq_index *idx, uint32_t i, rq_attr_info_t *out) {
    if (!idx || !out) return fail(RQ_ERR_INVALID, "null argument");
    if (i >= idx->attrs.size()) return fail(RQ_ERR_INVALID, "column index " + std::to_string(i) + " of " + std::to_string(idx->attrs.size()));
    const AttrColumn &c = *idx->attrs[i];
    rq_attr_info_t full{};
    full.type = c.type, full.fill.u64 = c.fill, full.bytes = idx->n * attr_elem(c.type);
    memcpy(full.name, c.name.c_str(), c.name.size());
    return copy_out_sized(out, full);
}

// ids (device, m) -> the column's values: set (three passes, kernels_attr.h) and get
static rq_status attr_set_device(rq_index *idx, const char *name, const uint32_t *d_ids, const void *d_values, uint64_t m, uint64_t *out_absent) {
    AttrColumn *c = nullptr;
    RQC(attr_named(idx, name, m && (!d_ids || !d_values), &c));
    if (out_absent) *out_absent = 0;
    if (m >= 0xFFFFFFFFull) return fail(RQ_ERR_UNSUPPORTED, "m must be below 2^32 - 1 (a request index is a u32)");
    RQC(ensure_device());
    if (m == 0) return RQ_OK;
    if (idx->n == 0) {  // every id is absent
        if (out_absent) *out_absent = m;
        return RQ_OK;
    }
    ByIdCall call;
    RQC(call.begin(idx));
    RQC(call.ws->id_pos.ensure(m));
    DevBuf<uint32_t> owner;  // per position; only the asked positions are written and read
    RQC(owner.alloc(idx->n));
    RQC(call.lookup(d_ids, m, call.ws->id_pos.p));
    const uint32_t *pos = call.ws->id_pos.p;
    const uint32_t grid = attr_grid(m);
    attr_owner_reset_kernel<<<grid, 256, 0, call.st>>>(pos, m, owner.p);
    attr_owner_claim_kernel<<<grid, 256, 0, call.st>>>(pos, m, owner.p);
    if (attr_elem(c->type) == 8)
        attr_scatter_kernel<uint64_t><<<grid, 256, 0, call.st>>>(pos, static_cast<const uint64_t *>(d_values), m, owner.p, reinterpret_cast<uint64_t *>(c->data.p));
    else
        attr_scatter_kernel<uint32_t><<<grid, 256, 0, call.st>>>(pos, static_cast<const uint32_t *>(d_values), m, owner.p, reinterpret_cast<uint32_t *>(c->data.p));
    RQC(call.finish());
    if (out_absent) *out_absent = g_by_id_stats.absent;
    return RQ_OK;
}
static rq_status attr_set_host(rq_index *idx, const char *name, const uint32_t *ids, const void *values, uint64_t m, uint64_t *out_absent) {
    AttrColumn *c = nullptr;
    RQC(attr_named(idx, name, m && (!ids || !values), &c));
    RQC(ensure_device());
    DevBuf<uint32_t> d_ids;
    DevBuf<uint8_t> d_values;
    RQC(d_ids.upload(ids, m));
    RQC(d_values.upload(static_cast<const uint8_t *>(values), m * attr_elem(c->type)));
    return attr_set_device(idx, name, d_ids.p, d_values.p, m, out_absent);
}
static rq_status attr_get_device(const rq_index *idx, const char *name, const uint32_t *d_ids, uint64_t m, void *d_out_values, uint32_t *d_out_found) {
    AttrColumn *c = nullptr;
    RQC(attr_named(idx, name, m && (!d_ids || !d_out_values), &c));
    RQC(ensure_device());
    if (m == 0) return RQ_OK;
    ByIdCall call;
    RQC(call.begin(idx));
    RQC(call.ws->id_pos.ensure(m));
    if (idx->n == 0) HIPC(hipMemsetAsync(call.ws->id_pos.p, 0xFF, m * 4, call.st));  // every id is absent
    else RQC(call.lookup(d_ids, m, call.ws->id_pos.p));
    if (attr_elem(c->type) == 8)
        attr_fetch_kernel<uint64_t><<<attr_grid(m), 256, 0, call.st>>>(call.ws->id_pos.p, m, reinterpret_cast<const uint64_t *>(c->data.p), c->fill,
                                                                       static_cast<uint64_t *>(d_out_values), d_out_found);
    else
        attr_fetch_kernel<uint32_t><<<attr_grid(m), 256, 0, call.st>>>(call.ws->id_pos.p, m, reinterpret_cast<const uint32_t *>(c->data.p), (uint32_t)c->fill,
                                                                       static_cast<uint32_t *>(d_out_values), d_out_found);
    RQC(call.finish());
    if (idx->n == 0) g_by_id_stats.absent = m;
    return RQ_OK;
}
static rq_status attr_get_host(const rq_index *idx, const char *name, const uint32_t *ids, uint64_t m, void *out_values, uint32_t *out_found) {
    AttrColumn *c = nullptr;
    RQC(attr_named(idx, name, m && (!ids || !out_values), &c));
    RQC(ensure_device());
    const size_t elem = attr_elem(c->type);
    DevBuf<uint32_t> d_ids, d_found;
    DevBuf<uint8_t> d_values;
    RQC(d_ids.upload(ids, m));
    RQC(d_found.alloc(m));
    RQC(d_values.alloc(m * elem));
    RQC(attr_get_device(idx, name, d_ids.p, m, d_values.p, d_found.p));
    if (m) HIPC(hipMemcpy(out_values, d_values.p, m * elem, hipMemcpyDeviceToHost));
    if (m && out_found) HIPC(hipMemcpy(out_found, d_found.p, m * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}
static rq_status attr_get_array(const rq_index *idx, const char *name, void *dst, uint64_t dst_bytes) {
    AttrColumn *c = nullptr;
    RQC(attr_named(idx, name, false, &c));
    const uint64_t bytes = idx->n * attr_elem(c->type);
    if (!dst || dst_bytes < bytes) return fail(RQ_ERR_INVALID, "destination too small");
    if (bytes) HIPC(hipMemcpy(dst, c->data.p, bytes, hipMemcpyDeviceToHost));
    return RQ_OK;
}

// ---- columns follow their rows -----------------------------------------------------------------------------------------------------------
static rq_status attr_merge_check(const rq_index *dst, const rq_index *src) {
    for (const auto &c : dst->attrs) {
        const int j = attr_find(src, c->name);
        if (j >= 0 && src->attrs[(size_t)j]->type != c->type)
            return fail(RQ_ERR_INVALID, "the two indexes differ in the type of column " + c->name);
    }
    return RQ_OK;
}
// (declared in host_relayout.h) enqueued behind the layout's own gather; the caller synchronises
static rq_status columns_follow(const rq_index *a, const rq_index *b, const uint32_t *src_of_dst, uint64_t n, rq_index *nx, uint64_t *bytes) {
    const uint32_t n_a = (uint32_t)a->n, n_b = b ? (uint32_t)b->n : 0u;
    for (const auto &ca : a->attrs) {
        std::unique_ptr<AttrColumn> c;
        RQC(attr_new_column(ca->name, ca->type, ca->fill, n, c));
        const int j = b ? attr_find(b, ca->name) : -1;
        const void *col_b = j >= 0 && b->attrs[(size_t)j]->type == ca->type ? b->attrs[(size_t)j]->data.p : nullptr;
        const uint32_t grid = attr_grid(ceil_div(n, 4));
        if (n && attr_elem(ca->type) == 8)
            column_gather_kernel<uint64_t><<<grid, 256>>>(src_of_dst, n, n_a, n_b, reinterpret_cast<const uint64_t *>(ca->data.p),
                                                          static_cast<const uint64_t *>(col_b), ca->fill, reinterpret_cast<uint64_t *>(c->data.p));
        else if (n)
            column_gather_kernel<uint32_t><<<grid, 256>>>(src_of_dst, n, n_a, n_b, reinterpret_cast<const uint32_t *>(ca->data.p),
                                                          static_cast<const uint32_t *>(col_b), (uint32_t)ca->fill, reinterpret_cast<uint32_t *>(c->data.p));
        *bytes += 2 * n * attr_elem(ca->type);
        nx->attrs.push_back(std::move(c));
    }
    return RQ_OK;
}
// rq_shard_index: the slice of every owned list, list by list (adjacent owned lists are one copy): off / noff are the source's and
// the shard's list offsets
static rq_status columns_shard(const rq_index *idx, rq_index *sh, const std::vector<uint32_t> &off, const std::vector<uint32_t> &noff,
                               const uint32_t *owner, uint32_t rank) {
    for (const auto &ca : idx->attrs) {
        std::unique_ptr<AttrColumn> c;
        RQC(attr_new_column(ca->name, ca->type, ca->fill, sh->n, c));
        const size_t elem = attr_elem(ca->type);
        for (uint32_t l = 0; l < idx->k;) {
            if (owner[l] != rank) {
                ++l;
                continue;
            }
            uint32_t e = l + 1;
            while (e < idx->k && owner[e] == rank) ++e;
            const size_t rows = off[e] - off[l];
            if (rows) HIPC(hipMemcpyAsync(c->data.p + noff[l] * elem, ca->data.p + off[l] * elem, rows * elem, hipMemcpyDeviceToDevice, nullptr));
            l = e;
        }
        sh->attrs.push_back(std::move(c));
    }
    return RQ_OK;
}

// ---- persistence -------------------------------------------------------------------------------------------------------------------------
static rq_status attr_dump_dir(const rq_index *idx, const std::string &d) {
    if (idx->attrs.empty()) {
        remove((d + "/attrs").c_str());  // (a directory that held a dump with columns before)
        return RQ_OK;
    }
    std::string text;
    for (const auto &c : idx->attrs) {
        char line[96];
        snprintf(line, sizeof line, "%s %u %016llx\n", c->name.c_str(), c->type, (unsigned long long)c->fill);
        text += line;
        const uint64_t bytes = idx->n * attr_elem(c->type);
        std::vector<uint8_t> host(bytes);
        if (bytes) HIPC(hipMemcpy(host.data(), c->data.p, bytes, hipMemcpyDeviceToHost));
        const std::string path = d + "/attr." + c->name;
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) return fail(RQ_ERR_IO, "cannot create " + path);
        const bool ok = !bytes || fwrite(host.data(), 1, bytes, f) == bytes;
        if (fclose(f) != 0 || !ok) return fail(RQ_ERR_IO, "write error on " + path);
    }
    FILE *f = fopen((d + "/attrs").c_str(), "wb");
    if (!f) return fail(RQ_ERR_IO, "cannot create " + d + "/attrs");
    const bool ok = fputs(text.c_str(), f) >= 0;
    if (fclose(f) != 0 || !ok) return fail(RQ_ERR_IO, "write error on " + d + "/attrs");
    return RQ_OK;
}
// the columns of a dump into a freshly loaded index (no `attrs` file: none)
static rq_status attr_load_dir(const std::string &d, rq_index *idx) {
    FILE *af = fopen((d + "/attrs").c_str(), "rb");
    if (!af) return RQ_OK;
    std::string text;
    char buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, af)) > 0;) text.append(buf, got);
    fclose(af);
    const auto bad = [&](const std::string &why) { return fail(RQ_ERR_IO, "attrs: " + why + " in " + d + "/attrs"); };
    if (text.empty() || text.back() != '\n') return bad("no final newline");
    size_t at = 0;
    while (at < text.size()) {
        const size_t end = text.find('\n', at);
        const std::string line = text.substr(at, end - at);
        at = end + 1;
        const size_t s1 = line.find(' '), s2 = s1 == std::string::npos ? s1 : line.find(' ', s1 + 1);
        if (s2 == std::string::npos) return bad("a malformed line");
        const std::string name = line.substr(0, s1), type_s = line.substr(s1 + 1, s2 - s1 - 1), fill_s = line.substr(s2 + 1);
        if (!attr_name_ok(name.c_str()) || type_s.size() != 1 || type_s[0] < '0' || type_s[0] > '4' || fill_s.size() != 16) return bad("a malformed line");
        uint64_t fill = 0;
        for (char ch : fill_s) {
            const int v = ch >= '0' && ch <= '9' ? ch - '0' : (ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1);
            if (v < 0) return bad("a malformed fill value");
            fill = (fill << 4) | (uint64_t)v;
        }
        const uint32_t type = (uint32_t)(type_s[0] - '0');
        if (attr_elem(type) == 4 && (fill >> 32)) return bad("a fill value wider than its type");
        if (attr_find(idx, name) >= 0) return bad("a column named twice");
        if (idx->attrs.size() >= RQ_ATTR_MAX_COLUMNS) return bad("more than 16 columns");
        const uint64_t bytes = idx->n * attr_elem(type);
        const std::string path = d + "/attr." + name;
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) return fail(RQ_ERR_IO, "cannot open " + path);
        std::vector<uint8_t> host(bytes + 1);
        const size_t got = fread(host.data(), 1, bytes + 1, f);
        fclose(f);
        if (got != bytes) return fail(RQ_ERR_IO, path + " does not hold n x elem = " + std::to_string(bytes) + " bytes");
        std::unique_ptr<AttrColumn> c;
        RQC(attr_new_column(name, type, fill, idx->n, c));
        if (bytes) HIPC(hipMemcpy(c->data.p, host.data(), bytes, hipMemcpyHostToDevice));
        idx->attrs.push_back(std::move(c));
    }
    return RQ_OK;
}

// ---- predicates to filters ---------------------------------------------------------------------------------------------------------------
// The checks that need nothing of the index, and the program as tokens (program == nullptr: the AND of all terms, two deep).
static rq_status where_program(const rq_where_term_t *terms, uint32_t nterms, const uint8_t *program, uint32_t ntokens, std::vector<uint8_t> &tokens) {
    if (nterms && !terms) return fail(RQ_ERR_INVALID, "null argument");
    if (nterms > RQ_WHERE_MAX_TERMS) return fail(RQ_ERR_INVALID, "a predicate has at most 32 terms");
    for (uint32_t i = 0; i < nterms; ++i) {
        const rq_where_term_t &t = terms[i];
        if (t.op > RQ_WHERE_ALL_BITS) return fail(RQ_ERR_INVALID, "term " + std::to_string(i) + ": unknown op " + std::to_string(t.op));
        if (t.op == RQ_WHERE_IN && t.set_count > RQ_WHERE_MAX_SET) return fail(RQ_ERR_INVALID, "term " + std::to_string(i) + ": a set holds at most 4096 values");
        if (t.op == RQ_WHERE_IN && t.set_count && !t.set) return fail(RQ_ERR_INVALID, "term " + std::to_string(i) + ": null set with set_count > 0");
    }
    tokens.clear();
    if (!program) {
        for (uint32_t i = 0; i < nterms; ++i) {
            tokens.push_back((uint8_t)i);
            if (i) tokens.push_back((uint8_t)RQ_WHERE_AND);
        }
        return RQ_OK;
    }
    if (ntokens > RQ_WHERE_MAX_TOKENS) return fail(RQ_ERR_INVALID, "a program has at most 64 tokens");
    uint32_t depth = 0;
    for (uint32_t i = 0; i < ntokens; ++i) {
        const uint32_t tok = program[i];
        if (tok < RQ_WHERE_MAX_TERMS) {
            if (tok >= nterms) return fail(RQ_ERR_INVALID, "token " + std::to_string(i) + " pushes term " + std::to_string(tok) + " of " + std::to_string(nterms));
            if (++depth > 32) return fail(RQ_ERR_INVALID, "the program's stack passes depth 32 at token " + std::to_string(i));
        } else if (tok == RQ_WHERE_AND || tok == RQ_WHERE_OR) {
            if (depth < 2) return fail(RQ_ERR_INVALID, "the program underflows at token " + std::to_string(i));
            --depth;
        } else if (tok == RQ_WHERE_NOT) {
            if (depth < 1) return fail(RQ_ERR_INVALID, "the program underflows at token " + std::to_string(i));
        } else
            return fail(RQ_ERR_INVALID, "token " + std::to_string(i) + ": unknown token " + std::to_string(tok));
    }
    if (depth != 1) return fail(RQ_ERR_INVALID, "the program ends at depth " + std::to_string(depth) + ", not 1");
    tokens.assign(program, program + ntokens);
    return RQ_OK;
}
// the set of an IN term as the kernel searches it: ascending in the type's own order, no value twice; F32: no NaN, -0 as +0
template <typename T>
static void where_sorted_set(const void *set, uint32_t count, std::vector<uint8_t> &out, uint32_t *out_count) {
    std::vector<T> v(count);
    if (count) memcpy(v.data(), set, (size_t)count * sizeof(T));
    if constexpr (std::is_same<T, float>::value) {
        v.erase(std::remove_if(v.begin(), v.end(), [](float x) { return x != x; }), v.end());
        for (float &x : v) x = x + 0.0f;
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    out.resize(v.size() * sizeof(T));
    if (!v.empty()) memcpy(out.data(), v.data(), out.size());
    *out_count = (uint32_t)v.size();
}

// The kernel's instantiation: the slot count rounded up to 1, 2, 4 or 8 (the spare slots are copies of slot 0, whose loads hit the
// lines slot 0 brought in), WIDE where a column of 8-byte elements is read.  R = 4 runs of 64 positions per wave in flight.
template <int NS>
static void launch_where_ns(const WhereArgs &wa, bool wide, uint64_t n, uint64_t nruns, uint32_t *pos_bits, hipStream_t st) {
    constexpr int R = 4;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(nruns, 4 * R), 2048));
    if (wide) where_kernel<NS, true, R><<<grid, 256, 0, st>>>(wa, n, nruns, pos_bits);
    else where_kernel<NS, false, R><<<grid, 256, 0, st>>>(wa, n, nruns, pos_bits);
}
static void launch_where(WhereArgs &wa, uint64_t n, uint64_t nruns, uint32_t *pos_bits, hipStream_t st) {
    bool wide = false;
    for (uint32_t s = 0; s < wa.nslots; ++s) wide = wide || wa.slots[s].wide;
    for (uint32_t s = wa.nslots; s < RQ_WHERE_MAX_COLUMNS; ++s) wa.slots[s] = wa.slots[0];
    if (wa.nslots <= 1) launch_where_ns<1>(wa, wide, n, nruns, pos_bits, st);
    else if (wa.nslots <= 2) launch_where_ns<2>(wa, wide, n, nruns, pos_bits, st);
    else if (wa.nslots <= 4) launch_where_ns<4>(wa, wide, n, nruns, pos_bits, st);
    else launch_where_ns<8>(wa, wide, n, nruns, pos_bits, st);
}

static rq_status filter_create_where(const rq_index *idx, const rq_where_term_t *terms, uint32_t nterms, const uint8_t *program, uint32_t ntokens,
                                     rq_filter **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    std::vector<uint8_t> tokens;
    RQC(where_program(terms, nterms, program, ntokens, tokens));
    // what the index decides: the columns, their types, the slots
    WhereArgs wa{};
    int slot_of[RQ_ATTR_MAX_COLUMNS];
    for (int &s : slot_of) s = -1;
    bool used[RQ_WHERE_MAX_TERMS] = {};
    for (uint8_t tok : tokens)
        if (tok < RQ_WHERE_MAX_TERMS) used[tok] = true;
    uint64_t elem_bytes = 0;
    for (uint32_t i = 0; i < nterms; ++i) {
        const rq_where_term_t &t = terms[i];
        if (t.column >= idx->attrs.size()) return fail(RQ_ERR_INVALID, "term " + std::to_string(i) + ": the index has no column " + std::to_string(t.column));
        const AttrColumn &c = *idx->attrs[t.column];
        if ((t.op == RQ_WHERE_ANY_BITS || t.op == RQ_WHERE_ALL_BITS) && c.type == RQ_ATTR_F32)
            return fail(RQ_ERR_INVALID, "term " + std::to_string(i) + ": the bit ops are for integer columns (column " + c.name + " is f32)");
        if (!used[i]) continue;
        if (slot_of[t.column] < 0) {
            if (wa.nslots >= RQ_WHERE_MAX_COLUMNS) return fail(RQ_ERR_INVALID, "a predicate reads at most 8 distinct columns");
            slot_of[t.column] = (int)wa.nslots;
            wa.slots[wa.nslots].col = c.data.p, wa.slots[wa.nslots].type = c.type, wa.slots[wa.nslots].wide = attr_elem(c.type) == 8 ? 1u : 0u;
            elem_bytes += attr_elem(c.type);
            ++wa.nslots;
        }
        WhereTerm &k = wa.terms[i];
        k.a = attr_image(c.type, t.a), k.b = attr_image(c.type, t.b);
        k.slot = (uint8_t)slot_of[t.column], k.op = (uint8_t)t.op;
    }
    wa.ntokens = (uint32_t)tokens.size();
    if (!tokens.empty()) memcpy(wa.tokens, tokens.data(), tokens.size());
    RQC(ensure_device());
    g_where_stats = rq_where_stats_t{};
    g_where_stats.struct_size = sizeof(rq_where_stats_t);
    std::vector<std::unique_ptr<DevBuf<uint8_t>>> sets;  // the uploaded IN sets, alive until the kernel has run
    for (uint32_t i = 0; i < nterms; ++i) {
        if (!used[i] || terms[i].op != RQ_WHERE_IN) continue;
        std::vector<uint8_t> sorted;
        uint32_t count = 0;
        switch (idx->attrs[terms[i].column]->type) {
        case RQ_ATTR_U32: where_sorted_set<uint32_t>(terms[i].set, terms[i].set_count, sorted, &count); break;
        case RQ_ATTR_I32: where_sorted_set<int32_t>(terms[i].set, terms[i].set_count, sorted, &count); break;
        case RQ_ATTR_F32: where_sorted_set<float>(terms[i].set, terms[i].set_count, sorted, &count); break;
        case RQ_ATTR_U64: where_sorted_set<uint64_t>(terms[i].set, terms[i].set_count, sorted, &count); break;
        default: where_sorted_set<int64_t>(terms[i].set, terms[i].set_count, sorted, &count); break;
        }
        sets.emplace_back(new DevBuf<uint8_t>());
        RQC(sets.back()->upload(sorted.data(), sorted.size()));
        WhereTerm &k = wa.terms[i];
        k.set = sets.back()->p, k.set_count = count, k.top = count ? 1u : 0u;
        while (k.top && k.top * 2 <= count) k.top *= 2;
    }
    std::unique_ptr<rq_filter> f(new rq_filter());
    hipStream_t st = nullptr;
    HIPC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~StreamGuard() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            (void)hipStreamDestroy(s);
        }
    } sg{st};
    HIPC(hipEventCreate(&sg.e0));
    HIPC(hipEventCreate(&sg.e1));
    const uint64_t n = idx->n, nwords = pos_bitmap_words(n), nruns = nwords / 2;
    RQC(f->pos_bits.alloc(nwords));
    HIPC(hipEventRecord(sg.e0, st));
    if (n && wa.nslots) {
        launch_where(wa, n, nruns, f->pos_bits.p, st);
    } else if (n) {  // no term is read: every row holds -- NOT of the empty set, cut at n
        HIPC(hipMemsetAsync(f->pos_bits.p, 0, nwords * 4, st));
        filter_combine_kernel<<<bitmap_grid(nwords), 256, 0, st>>>(f->pos_bits.p, nullptr, RQ_FILTER_NOT, nullptr, n, nwords, f->pos_bits.p);
    } else
        HIPC(hipMemsetAsync(f->pos_bits.p, 0, nwords * 4, st));
    HIPC(hipEventRecord(sg.e1, st));
    HIPC(hipStreamSynchronize(st));
    HIPC(hipGetLastError());
    PhaseClock clk;
    if (idx->live)  // dead rows are never admitted
        bitmap_and_live_kernel<<<bitmap_grid(nwords), 256, 0, st>>>(f->pos_bits.p, 0u, idx->live->pos_bits.p, nwords);
    RQC(list_prefix_sums(idx, f->pos_bits.p, st, f->h_sub_off));
    RQC(filter_finish(idx, f.get()));
    g_where_stats.ms_finish = clk.lap();
    (void)hipEventElapsedTime(&g_where_stats.ms_eval, sg.e0, sg.e1);
    g_where_stats.columns = wa.nslots, g_where_stats.rows = n, g_where_stats.admitted = f->rows, g_where_stats.bytes_read = n * elem_bytes;
    *out = f.release();
    return RQ_OK;
}

// ---- entries on a filter's bitmap ----------------------------------------------------------------------------------------------------
// a filter the queries of idx would accept (validate_call's three checks, in its words)
static rq_status filter_current(const rq_index *idx, const rq_filter *f) {
    if (f->idx != idx) return fail(RQ_ERR_INVALID, "the filter was made for another index");
    if (f->generation != idx->generation)
        return fail(RQ_ERR_INVALID, "the filter was made before the index was last mutated (rq_add / rq_remove): make it again");
    if (f->removal_epoch != idx->removal_epoch)
        return fail(RQ_ERR_INVALID, "the filter was made before rows of the index were last marked dead (rq_remove_lazy): make it again");
    return RQ_OK;
}
static rq_status filter_combine(const rq_index *idx, const rq_filter *a, const rq_filter *b, uint32_t op, rq_filter **out) {
    if (!out) return fail(RQ_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!idx) return fail(RQ_ERR_INVALID, "null index");
    if (op > RQ_FILTER_NOT) return fail(RQ_ERR_INVALID, "unknown op " + std::to_string(op) + " (RQ_FILTER_AND, _OR, _ANDNOT or _NOT)");
    if (!a || (op != RQ_FILTER_NOT && !b)) return fail(RQ_ERR_INVALID, "null filter");
    RQC(filter_current(idx, a));
    if (op != RQ_FILTER_NOT) RQC(filter_current(idx, b));
    RQC(ensure_device());
    std::unique_ptr<rq_filter> f(new rq_filter());
    const uint64_t nwords = pos_bitmap_words(idx->n);
    RQC(f->pos_bits.alloc(nwords));
    filter_combine_kernel<<<bitmap_grid(nwords), 256>>>(a->pos_bits.p, op != RQ_FILTER_NOT ? b->pos_bits.p : nullptr, op,
                                                        idx->live ? idx->live->pos_bits.p : nullptr, idx->n, nwords, f->pos_bits.p);
    RQC(list_prefix_sums(idx, f->pos_bits.p, nullptr, f->h_sub_off));
    RQC(filter_finish(idx, f.get()));
    *out = f.release();
    return RQ_OK;
}
static rq_status filter_id_bits(const rq_filter *f, uint32_t *bits, uint64_t nbits, int bits_on_device) {
    if (!f) return fail(RQ_ERR_INVALID, "null filter");
    RQC(id_bits_check(bits, nbits));
    RQC(filter_current(f->idx, f));
    RQC(ensure_device());
    const rq_index *idx = f->idx;
    const uint64_t words = (nbits + 31) / 32;
    if (words == 0) return RQ_OK;
    DevBuf<uint32_t> staged;
    uint32_t *d_bits = bits;
    if (!bits_on_device) {
        RQC(staged.alloc(words));
        d_bits = staged.p;
    }
    HIPC(hipMemset(d_bits, 0, words * 4));
    if (idx->n) filter_id_bits_kernel<<<attr_grid(idx->n), 256>>>(f->pos_bits.p, idx->map_ids.p, idx->n, nbits, d_bits);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    if (!bits_on_device) HIPC(hipMemcpy(bits, d_bits, words * 4, hipMemcpyDeviceToHost));
    return RQ_OK;
}
static rq_status filter_ids_device(const rq_filter *f, uint32_t *d_out_ids, uint64_t cap, uint64_t *out_count) {
    if (!f || !out_count) return fail(RQ_ERR_INVALID, "null argument");
    *out_count = 0;
    if (cap && !d_out_ids) return fail(RQ_ERR_INVALID, "null output with cap > 0");
    RQC(filter_current(f->idx, f));
    RQC(ensure_device());
    const rq_index *idx = f->idx;
    const uint64_t n = idx->n, nwords = pos_bitmap_words(n);
    const uint32_t nblocks = ceil_div(nwords, 256);
    DevBuf<uint32_t> counts;
    RQC(counts.alloc(nblocks));
    filter_block_counts_kernel<<<nblocks, 256>>>(f->pos_bits.p, nwords, n, counts.p);
    std::vector<uint32_t> h_counts(nblocks);
    HIPC(hipMemcpy(h_counts.data(), counts.p, (size_t)nblocks * 4, hipMemcpyDeviceToHost));
    HIPC(hipGetLastError());
    std::vector<unsigned long long> h_off(nblocks);
    uint64_t total = 0;
    for (uint32_t b = 0; b < nblocks; ++b) h_off[b] = total, total += h_counts[b];
    *out_count = total;
    if (total == 0 || cap == 0) return RQ_OK;
    DevBuf<unsigned long long> off;
    RQC(off.upload(h_off.data(), nblocks));
    filter_emit_ids_kernel<<<nblocks, 256>>>(f->pos_bits.p, nwords, n, idx->map_ids.p, off.p, cap, d_out_ids);
    HIPC(hipDeviceSynchronize());
    HIPC(hipGetLastError());
    return RQ_OK;
}
