// keyed_plan.h -- the work plan of a keyed exact search (host_keyed.h): plain C++ over host arrays, no HIP call, no
// device wait -- the keys are routing metadata and live on the host.  (Stand-alone on purpose: a CPU program can include it.)
//
// A SEGMENT is the postings of one value: positions [starts[s], starts[s + 1]).  Every query is looked up by binary search, the
// queries are sorted by (segment, query index), each segment's queries are cut into TILES of at most 32 (a tile is one operand of
// the matrix pass: 32 plan slots, the slots behind a short tile are padding), each segment's rows into CHUNKS, and one work item is
// emitted per (tile, chunk).  A query whose key the postings do not hold is in no tile: it is answered with nothing.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

#define RQ_KEYED_PAD 0xFFFFFFFFu     // a plan slot without a query
#define RQ_KEYED_MATRIX 0x80000000u  // KeyedItem::stride bit 31: the item's rows go through the matrix pass

struct KeyedItem {      // 16 bytes: one block's work
    uint32_t tile;      // the 32 plan slots [32 tile, 32 tile + 32)
    uint32_t first;     // index of the chunk's first posting
    uint32_t rows;      // postings of the item: first + v * stride, v < rows
    uint32_t stride;    // bits 0 .. 30: the step between them (1: every row; the bound's sample: every stride-th); bit 31: RQ_KEYED_MATRIX
};

// stride and sample size of a segment of `rows` postings (the exact search's rule, host_exact.h)
typedef uint32_t (*keyed_stride_fn)(uint64_t rows, uint32_t topk, uint32_t asked, uint32_t *sample_rows);

struct KeyedPlan {
    std::vector<uint32_t> order;     // 32 x tiles: plan slot -> query of the call, or RQ_KEYED_PAD
    std::vector<KeyedItem> scan;     // every row of every asked segment
    std::vector<KeyedItem> seed;     // the bound's sample (segments of at least small_rows postings only)
    uint32_t tiles = 0, keys_distinct = 0, queries_absent = 0;
    uint32_t largest_segment = 0;    // postings of the largest asked segment (a query keeps at most that many rows)
    uint32_t largest_sample = 0;     // likewise of the largest sample
    uint64_t rows_scan = 0;          // sum over the scan items of their rows
    uint64_t rows_matrix = 0;        // of them, the rows of the items that take the matrix pass: what the scan gathers
    bool any_matrix = false;
};

// the column types' own comparison on u64 images (a 4-byte value: zero-extended): wide = 8-byte elements
static inline bool keyed_less(uint64_t a, uint64_t b, bool is_signed, bool wide) {
    if (!is_signed) return a < b;
    return wide ? (int64_t)a < (int64_t)b : (int32_t)(uint32_t)a < (int32_t)(uint32_t)b;
}
// the segment of `key` in the sorted values, or nv
static inline uint32_t keyed_find(const uint64_t *values, uint32_t nv, uint64_t key, bool is_signed, bool wide) {
    uint32_t lo = 0, hi = nv;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keyed_less(values[mid], key, is_signed, wide)) lo = mid + 1;
        else hi = mid;
    }
    return lo < nv && values[lo] == key ? lo : nv;
}

// m keys as the caller holds them (8-byte rq_attr_value_t images; a 4-byte type reads the low 4 bytes) -> their segments, or
// RQ_KEYED_PAD for a key the values do not hold (multi-vector search by postings, host form: DESIGN §4.26)
static inline void keyed_segments(const uint64_t *values, uint32_t nv, bool is_signed, bool wide, const uint64_t *keys, uint64_t m, uint32_t *out) {
    for (uint64_t i = 0; i < m; ++i) {
        const uint32_t s = keyed_find(values, nv, wide ? keys[i] : keys[i] & 0xFFFFFFFFull, is_signed, wide);
        out[i] = s < nv ? s : RQ_KEYED_PAD;
    }
}

// values[nv] ascending in the column's order, starts[nv + 1]; keys[nq]: the u64 images of the queries' keys.  matrix: the call runs
// the matrix pass at all; seeded: it makes bounds.  Segments below small_rows postings take neither.
static inline void keyed_plan(const uint64_t *values, const uint64_t *starts, uint32_t nv, bool is_signed, bool wide, const uint64_t *keys,
                              uint32_t nq, uint32_t topk, uint32_t seed_probe, bool matrix, bool seeded, uint32_t chunk_rows, uint32_t small_rows,
                              keyed_stride_fn stride_of, KeyedPlan *out) {
    KeyedPlan &p = *out;
    p = KeyedPlan{};
    std::vector<uint64_t> by_seg;  // segment << 32 | query
    by_seg.reserve(nq);
    for (uint32_t b = 0; b < nq; ++b) {
        const uint32_t s = keyed_find(values, nv, keys[b], is_signed, wide);
        if (s == nv || starts[s + 1] == starts[s]) ++p.queries_absent;
        else by_seg.push_back(((uint64_t)s << 32) | b);
    }
    std::sort(by_seg.begin(), by_seg.end());
    if (chunk_rows < 32) chunk_rows = 32;
    for (size_t i = 0; i < by_seg.size();) {
        const uint32_t s = (uint32_t)(by_seg[i] >> 32);
        size_t e = i;
        while (e < by_seg.size() && (uint32_t)(by_seg[e] >> 32) == s) ++e;
        ++p.keys_distinct;
        const uint32_t first = (uint32_t)starts[s], rows = (uint32_t)(starts[s + 1] - starts[s]);
        const bool big = rows >= small_rows;
        const uint32_t flag = matrix && big ? RQ_KEYED_MATRIX : 0u;
        p.any_matrix = p.any_matrix || flag != 0;
        p.largest_segment = std::max(p.largest_segment, rows);
        uint32_t sample = 0, stride = 1;
        if (seeded && big) {
            stride = stride_of(rows, topk, seed_probe, &sample);
            p.largest_sample = std::max(p.largest_sample, sample);
        }
        for (size_t t0 = i; t0 < e; t0 += 32) {
            const uint32_t tile = p.tiles++;
            for (size_t j = 0; j < 32; ++j) p.order.push_back(t0 + j < e ? (uint32_t)by_seg[t0 + j] : RQ_KEYED_PAD);
            for (uint32_t r0 = 0; r0 < rows; r0 += chunk_rows) {
                const uint32_t m = std::min(chunk_rows, rows - r0);
                p.scan.push_back(KeyedItem{tile, first + r0, m, 1u | flag});
                p.rows_scan += m;
                if (flag) p.rows_matrix += m;
            }
            for (uint32_t r0 = 0; r0 < sample; r0 += chunk_rows)
                p.seed.push_back(KeyedItem{tile, first + r0 * stride, std::min(chunk_rows, sample - r0), stride});
        }
        i = e;
    }
}
