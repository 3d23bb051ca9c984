"""A numpy model of diverse search (include/rabitq_hip.h, "diverse search").  Input: the source call's arrays -- dist /
ids (B x fetch) and cnt (B), the pairs of a row in ANY order -- a map {id: position} of the ids that have a live row, and the
widened stored rows `base` (f32, position order).  Output: what rq_diversify_results writes, every array whole.

Candidates: the pairs sorted ascending by ord32_biased(dist) << 32 | id; one whose id the map does not hold is absent, one of the
others whose distance is not finite is skipped; place = the index among the rest.  D(c, s) = oracle.l2_squared_distance_rows(row of
s, base, [pos(c)]).  The selection in its two forms, which must agree (tests/test_diverse_model.py):
  select_incremental -- div(c) = fmin(div(c), D(c, s)) after every taken s;
  select_from_matrix -- div(c) recomputed at every step as the minimum of the full m x m matrix of D over the taken set.
Every step takes the smallest ord32_biased(score) << 32 | place with score = (lambda * rel) - (mu * div), each operation rounded to
f32, a NaN score replaced by 0x7FC00000.
"""
import numpy as np

import oracle

PAD_ID = 0xFFFFFFFF
NAN_BITS = 0x7FC00000
INF = np.float32(np.inf)


def ord32_biased(x):
    """common.h: the unsigned-sortable image of an f32 (all bit patterns, NaNs included)."""
    bits = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    mask = ((bits >> 31) & 0xFFFFFFFF) >> 1
    return ((bits ^ mask) & 0xFFFFFFFF) ^ 0x80000000


def candidates(dist_row, id_row, cnt, posmap):
    """-> [(rel as f32, id, position)] in candidate order, absent count, skipped count."""
    n = int(cnt)
    d = np.asarray(dist_row[:n], dtype=np.float32)
    i = np.asarray(id_row[:n], dtype=np.uint32)
    sk = (ord32_biased(d).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
    out, absent, skipped = [], 0, 0
    for j in np.argsort(sk, kind="stable"):
        if int(i[j]) not in posmap:
            absent += 1
        elif not np.isfinite(d[j]):
            skipped += 1
        else:
            out.append((d[j], int(i[j]), int(posmap[int(i[j])])))
    return out, absent, skipped


def pair_row(base, pos_s, positions):
    """D(c, s) for the candidates at `positions` against the row at pos_s."""
    return oracle.l2_squared_distance_rows(base[pos_s], base, positions)


def score_keys(lam, mu, rel, div, places):
    """ord32_biased(score) << 32 | place of the candidates `places` (arrays), score rounded to f32 after every operation"""
    with np.errstate(invalid="ignore", over="ignore"):
        score = (lam * rel).astype(np.float32) - (mu * div).astype(np.float32)
    score = np.where(np.isnan(score), np.array([NAN_BITS], dtype=np.uint32).view(np.float32)[0], score.astype(np.float32)).astype(np.float32)
    return (ord32_biased(score).astype(np.uint64) << np.uint64(32)) | places.astype(np.uint64)


def score_key(lam, mu, rel, div, place):
    return int(score_keys(np.float32(lam), np.float32(mu), np.array([rel], dtype=np.float32), np.array([div], dtype=np.float32),
                          np.array([place]))[0])


def select_incremental(cands, base, topk, lam):
    """-> [(place, div at selection)], the number of D evaluations."""
    lam = np.float32(lam)
    mu = np.float32(np.float32(1.0) - lam)
    m = len(cands)
    if m == 0:
        return [], 0
    rel = np.array([c[0] for c in cands], dtype=np.float32)
    pos = np.array([c[2] for c in cands], dtype=np.uint64)
    div = np.full(m, INF, dtype=np.float32)
    free = np.ones(m, dtype=bool)
    free[0] = False
    taken, pairs = [0], 0
    for _ in range(1, min(topk, m)):
        left = np.flatnonzero(free)
        div[left] = np.fmin(div[left], pair_row(base, int(pos[taken[-1]]), pos[left]))
        pairs += left.size
        j = int(left[np.argmin(score_keys(lam, mu, rel[left], div[left], left))])
        taken.append(j)
        free[j] = False
    return [(j, div[j]) for j in taken], pairs


def select_from_matrix(cands, base, topk, lam):
    """-> the same list, div recomputed from the full matrix D[c, s] over the taken set at every step."""
    lam = np.float32(lam)
    mu = np.float32(np.float32(1.0) - lam)
    m = len(cands)
    if m == 0:
        return [], 0
    rel = np.array([c[0] for c in cands], dtype=np.float32)
    pos = np.array([c[2] for c in cands], dtype=np.uint64)
    D = np.stack([pair_row(base, int(pos[s]), pos) for s in range(m)], axis=1)      # D[c, s]
    taken, out, pairs = [0], [(0, INF)], 0
    for _ in range(1, min(topk, m)):
        left = np.array([j for j in range(m) if j not in taken])
        div = np.fmin.reduce(D[np.ix_(left, taken)], axis=1)
        pairs += left.size
        at = int(np.argmin(score_keys(lam, mu, rel[left], div, left)))
        taken.append(int(left[at]))
        out.append((int(left[at]), div[at]))
    return out, pairs


def diversify_rows(dist, ids, cnt, posmap, base, topk, lam, select=select_incremental):
    """-> dict of the output arrays: dist_bits / ids / div_bits B x topk (u32), n B, and the totals."""
    dist, ids = np.asarray(dist, dtype=np.float32), np.asarray(ids, dtype=np.uint32)
    B, F = dist.shape
    od = np.full((B, topk), NAN_BITS, dtype=np.uint32)
    oi = np.full((B, topk), PAD_ID, dtype=np.uint32)
    ov = np.full((B, topk), NAN_BITS, dtype=np.uint32)
    on = np.zeros(B, dtype=np.uint32)
    tot = {"candidates": 0, "absent": 0, "skipped": 0, "pair_distances": 0}
    for b in range(B):
        n = min(int(cnt[b]), F)
        cands, absent, skipped = candidates(dist[b], ids[b], n, posmap)
        sel, pairs = select(cands, base, topk, lam)
        for s, (j, dv) in enumerate(sel):
            od[b, s] = np.array([cands[j][0]], dtype=np.float32).view(np.uint32)[0]
            oi[b, s] = cands[j][1]
            ov[b, s] = np.array([dv], dtype=np.float32).view(np.uint32)[0]
        on[b] = len(sel)
        tot["candidates"] += n
        tot["absent"] += absent
        tot["skipped"] += skipped
        tot["pair_distances"] += pairs
    return {"dist_bits": od, "ids": oi, "div_bits": ov, "n": on, "taken": int(on.sum()), **tot}


def posmap_of(index_ids, live=None):
    """{id: position} of an index: its map_ids in position order; live: a boolean per position."""
    return {int(i): p for p, i in enumerate(index_ids) if live is None or live[p]}
