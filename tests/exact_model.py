"""The CPU answer of the exact search (include/rabitq_hip.h, "exact search"): for an index's arrays -- `base` in cluster order, n x dim
f32 (half / byte rows widened: tests/half_model.py, tests/byte_model.py), and `map_ids` -- and the transformed, padded query q', the
exact-order distance e of EVERY row (oracle.l2_squared_distance_rows: the src/simd.rs:14-73 chain), the `< f32::MAX` rule, the order
(Ord32(e), id), the cut at topk.  Nothing here asks the engine what the answer is.  Not a conftest: import it."""
import numpy as np

from tests import cosine_model, ip_model

F32_MAX = np.float32(np.finfo(np.float32).max)
NO_ID = np.uint32(0xFFFFFFFF)


def ord32(e):
    """oracle.ord32_from_f32 on an array (src/ord32.rs:12-26): bits ^ ((bits >> 31) as u32 >> 1), as int32.
    (tests/test_exact_model.py holds it against the oracle's own function.)"""
    bits = np.ascontiguousarray(e, dtype=np.float32).view(np.int32)
    mask = ((bits >> 31).view(np.uint32) >> np.uint32(1)).view(np.int32)
    return bits ^ mask


def transformed_queries(oracle, queries, metric, dim):
    """q' of every raw query row: what the rerank of an index of this metric and dim sees."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    if metric == "cosine":
        out = cosine_model.normalize_rows(oracle, q)
    elif metric == "ip":
        out = ip_model.pad_cols(q, dim)
    else:
        out = cosine_model.pad64(q)
    assert out.shape[1] == dim
    return out


def admitted_positions(map_ids, allow_mask=None):
    """Positions of the rows a filter admits; allow_mask is a bool array over IDS (ids at or past its end are not admitted)."""
    map_ids = np.asarray(map_ids, dtype=np.uint32)
    if allow_mask is None:
        return np.arange(map_ids.size, dtype=np.uint64)
    allow_mask = np.asarray(allow_mask, dtype=bool)
    inside = map_ids < allow_mask.size
    ok = np.zeros(map_ids.size, dtype=bool)
    ok[inside] = allow_mask[map_ids[inside]]
    return np.flatnonzero(ok).astype(np.uint64)


def exact_one(oracle, base, map_ids, qprime, topk, positions=None):
    """-> (dist f32[m], ids u32[m]), m <= topk: the answer of one transformed query over the rows at `positions` (None: all)."""
    map_ids = np.asarray(map_ids, dtype=np.uint32)
    pos = np.arange(map_ids.size, dtype=np.uint64) if positions is None else np.asarray(positions, dtype=np.uint64)
    e = oracle.l2_squared_distance_rows(qprime, base, pos)
    with np.errstate(invalid="ignore"):
        keep = e < F32_MAX                      # (a NaN fails the comparison: never returned, like inf)
    e, ids = e[keep], map_ids[pos[keep].astype(np.int64)]
    order = np.lexsort((ids, ord32(e)))[:topk]  # by (Ord32(e), id), ascending
    return e[order], ids[order]


def exact_batch(oracle, base, map_ids, qprimes, topk, allow_mask=None):
    """-> (dist B x topk f32, ids B x topk u32, counts B u32) in the layout of RaBitQ.exact_search: slots past a query's count hold
    NaN / 0xFFFFFFFF."""
    base = np.ascontiguousarray(base, dtype=np.float32)
    pos = admitted_positions(map_ids, allow_mask)
    B = len(qprimes)
    dist = np.full((B, topk), np.nan, dtype=np.float32)
    ids = np.full((B, topk), NO_ID, dtype=np.uint32)
    cnt = np.zeros(B, dtype=np.uint32)
    for b in range(B):
        d, i = exact_one(oracle, base, map_ids, qprimes[b], topk, pos)
        dist[b, :d.size], ids[b, :i.size], cnt[b] = d, i, d.size
    return dist, ids, cnt


def index_answer(oracle, index, queries, topk, metric="l2", allow_mask=None, base=None):
    """The model on a built index's own arrays (index.base is the widened f32 image for half / byte rows too)."""
    base = index.base if base is None else base
    return exact_batch(oracle, base, index.map_ids, transformed_queries(oracle, queries, metric, index.dim), topk, allow_mask)
