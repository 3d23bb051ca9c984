"""The CPU answer of the exact range search (include/rabitq_hip.h, "exact range search"): from exact_model's distances -- the
exact-order distance e of EVERY admitted row, the `< f32::MAX` rule, the order (Ord32(e), id) -- the answer of a radius is the rows with
e < r (strict f32, so a NaN radius or one <= 0 admits nothing), in RangeResult's lims / dist / ids layout.  Nothing here asks the
engine what the answer is.  Not a conftest: import it."""
import numpy as np

from tests import exact_model as em


def range_one(oracle, base, map_ids, qprime, radius, positions=None):
    """-> (dist f32[m], ids u32[m]): the answer of one transformed query at one radius over the rows at `positions` (None: all)."""
    map_ids = np.asarray(map_ids, dtype=np.uint32)
    pos = np.arange(map_ids.size, dtype=np.uint64) if positions is None else np.asarray(positions, dtype=np.uint64)
    e = oracle.l2_squared_distance_rows(qprime, base, pos)
    with np.errstate(invalid="ignore"):
        keep = (e < np.float32(radius)) & (e < em.F32_MAX)      # (a NaN on either side fails the comparison)
    e, ids = e[keep], map_ids[pos[keep].astype(np.int64)]
    order = np.lexsort((ids, em.ord32(e)))                      # by (Ord32(e), id), ascending
    return e[order], ids[order]


def pack(answers):
    """[(dist, ids)] per query -> (lims u64[B + 1], dist f32[total], ids u32[total])."""
    lims = np.zeros(len(answers) + 1, dtype=np.uint64)
    lims[1:] = np.cumsum([d.size for d, _ in answers], dtype=np.uint64)
    dist = np.concatenate([d for d, _ in answers]).astype(np.float32) if answers else np.zeros(0, np.float32)
    ids = np.concatenate([i for _, i in answers]).astype(np.uint32) if answers else np.zeros(0, np.uint32)
    return lims, dist, ids


def range_batch(oracle, base, map_ids, qprimes, radii, allow_mask=None):
    """The model's answer of a batch; radii: a scalar or one per query."""
    base = np.ascontiguousarray(base, dtype=np.float32)
    pos = em.admitted_positions(map_ids, allow_mask)
    r = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(qprimes),))
    return pack([range_one(oracle, base, map_ids, qprimes[b], r[b], pos) for b in range(len(qprimes))])


def cut_full(full, radii, nq=None):
    """The same answer from a whole ranking `full` = exact_model.exact_batch(..., topk = n): every query's prefix with e < r.  (The
    ranking is ascending in Ord32(e), and e >= 0 there, so the rows below a radius are a prefix.)"""
    fd, fi, fc = full
    nq = fd.shape[0] if nq is None else nq
    r = np.broadcast_to(np.asarray(radii, dtype=np.float32), (nq,))
    out = []
    for b in range(nq):
        with np.errstate(invalid="ignore"):
            m = int(np.count_nonzero(fd[b, :fc[b]] < r[b]))
        out.append((fd[b, :m], fi[b, :m]))
    return pack(out)


def index_answer(oracle, index, queries, radii, metric="l2", allow_mask=None, base=None):
    """The model on a built index's own arrays (index.base is the widened f32 image for half / byte rows too)."""
    base = index.base if base is None else base
    return range_batch(oracle, base, index.map_ids, em.transformed_queries(oracle, queries, metric, index.dim), radii, allow_mask)
