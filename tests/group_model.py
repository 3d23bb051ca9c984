"""A numpy model of grouped search (include/rabitq_hip.h, "grouped search").  Input: the source call's arrays -- dist /
ids (B x fetch) and cnt (B), the pairs of a row in ANY order -- and a map {id: u64 image of its row's value in the column}; an id
the map does not hold is absent (no live row) and is skipped.  Output: what rq_group_results writes, every array whole.

The selection in its two forms, which must agree (tests/test_group_model.py):
  select_by_rank -- sort by the key ord32_biased(dist) << 32 | id; ord(key) = distinct keys whose first occurrence precedes this
                    key's first occurrence, rank(c) = earlier candidates with c's key; keep iff ord < topk and rank < group_size.
                    Every candidate is judged on its own: independent of any processing order.
  select_by_walk -- the sequential walk over the same order: open a group while fewer than topk are open, take a row while its
                    group holds fewer than group_size.
"""
import numpy as np

PAD_ID = 0xFFFFFFFF
PAD_DIST_BITS = 0x7FC00000


def ord32_biased(dist):
    """common.h: the unsigned-sortable image of an f32 (all bit patterns, NaNs included)."""
    bits = np.asarray(dist, dtype=np.float32).view(np.int32).astype(np.int64)
    mask = ((bits >> 31) & 0xFFFFFFFF) >> 1
    return ((bits ^ mask) & 0xFFFFFFFF) ^ 0x80000000


def key_image(values):
    """The u64 image of column values: 4-byte types zero-extended, 8-byte types as stored."""
    v = np.ascontiguousarray(values)
    if v.dtype.itemsize == 4:
        return v.view(np.uint32).astype(np.uint64)
    return v.view(np.uint64)


def sorted_present(dist_row, id_row, cnt, keymap):
    """The candidates of one query that have a live row, ascending by (ord32_biased(dist), id): [(dist bits, id, key)], absent count."""
    n = int(cnt)
    d = np.asarray(dist_row[:n], dtype=np.float32)
    i = np.asarray(id_row[:n], dtype=np.uint32)
    sk = (ord32_biased(d).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
    order = np.argsort(sk, kind="stable")
    out, absent = [], 0
    for j in order:
        if int(i[j]) in keymap:
            out.append((int(d[j:j + 1].view(np.uint32)[0]), int(i[j]), int(keymap[int(i[j])])))
        else:
            absent += 1
    return out, absent


def select_by_rank(cands, topk, group_size):
    """-> [(ord, rank, candidate)] of the kept candidates; every candidate decided from the two counts alone."""
    first = {}
    for pos, (_, _, key) in enumerate(cands):
        first.setdefault(key, pos)
    kept = []
    for pos, c in enumerate(cands):
        o = sum(1 for k, f in first.items() if f < first[c[2]])
        r = sum(1 for e in cands[:pos] if e[2] == c[2])
        if o < topk and r < group_size:
            kept.append((o, r, c))
    return kept


def select_by_walk(cands, topk, group_size):
    """-> the same list from the sequential walk."""
    opened, held, kept = {}, {}, []
    for c in cands:
        key = c[2]
        if key not in opened:
            if len(opened) >= topk:
                continue
            opened[key] = len(opened)
            held[key] = 0
        if held[key] < group_size:
            kept.append((opened[key], held[key], c))
            held[key] += 1
    return kept


def group_rows(dist, ids, cnt, keymap, topk, group_size, select=select_by_walk):
    """-> dict of the output arrays: dist (f32 bits as u32) and ids B x topk x group_size, keys (u64) and group_n B x topk, n B,
    and the totals absent / kept / groups."""
    dist, ids = np.asarray(dist, dtype=np.float32), np.asarray(ids, dtype=np.uint32)
    B, F = dist.shape
    od = np.full((B, topk, group_size), PAD_DIST_BITS, dtype=np.uint32)
    oi = np.full((B, topk, group_size), PAD_ID, dtype=np.uint32)
    ok = np.zeros((B, topk), dtype=np.uint64)
    gn = np.zeros((B, topk), dtype=np.uint32)
    on = np.zeros(B, dtype=np.uint32)
    absent = kept_n = 0
    for b in range(B):
        cands, a = sorted_present(dist[b], ids[b], min(int(cnt[b]), F), keymap)
        absent += a
        for o, r, (dbits, i, key) in select(cands, topk, group_size):
            od[b, o, r], oi[b, o, r], ok[b, o] = dbits, i, key
            gn[b, o] += 1
            kept_n += 1
        on[b] = int(np.count_nonzero(gn[b]))
    return {"dist_bits": od, "ids": oi, "keys": ok, "group_n": gn, "n": on, "absent": absent, "kept": kept_n, "groups": int(on.sum())}


def keymap_of(index_ids, column_values, live=None):
    """{id: key image} of an index: its map_ids and the column in position order (attr_array); live: a boolean per position."""
    img = key_image(column_values)
    return {int(i): int(k) for p, (i, k) in enumerate(zip(index_ids, img)) if live is None or live[p]}
