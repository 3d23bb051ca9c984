"""The expected answers the GPU test modules and the fuzz drivers share, built on the CPU oracle (oracle/) alone: bit views, the
sub-index a filter stands for, the live rows of a mutated index and their canonical build, the top-k comparison and the range
answer assembled from the oracle's stage functions.  Nothing here asks the engine what the answer is.  Not a conftest: import it.

tests/test_fuzz_models.py checks the assembly itself (range and filter answers) against plain float64."""
import ctypes as C

import numpy as np

ARRAYS = ("base", "orthogonal", "centroids", "offsets", "codes", "factors")
FMAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def sub_arrays(g, allowed, ids=None):
    """The reference arrays of the sub-index: every list keeps its admitted rows (allowed: bool mask over ids; ids beyond it are
    not admitted) in stored order.  g: an engine index or an oracle.OracleIndex; ids: translation of g's map_ids (the oracle's
    build of a mutated index's live rows numbers them 0 .. n-1, ids[j] is the id row j stands for)."""
    offs, mids = g.offsets.astype(np.int64), g.map_ids
    if ids is not None:
        mids = np.asarray(ids, dtype=np.uint32)[mids]
    keep = np.zeros(mids.size, dtype=bool)
    inr = mids < allowed.size
    keep[inr] = allowed[mids[inr]]
    lists = np.repeat(np.arange(g.k), np.diff(offs))
    new_off = np.zeros(g.k + 1, dtype=np.uint32)
    new_off[1:] = np.cumsum(np.bincount(lists[keep], minlength=g.k))
    return g.base[keep], g.orthogonal, g.centroids, new_off, mids[keep], g.codes[keep], g.factors[keep]


class Live:
    """The live rows S of a mutated index, kept on the host: id -> row."""

    def __init__(self, ids, rows):
        self.rows = {int(i): r for i, r in zip(ids, rows)}

    def add(self, ids, rows):
        for i, r in zip(ids, rows):
            assert int(i) not in self.rows
            self.rows[int(i)] = r

    def remove(self, ids):
        for i in ids:
            self.rows.pop(int(i), None)

    def sorted(self):
        ids = np.array(sorted(self.rows), dtype=np.uint32)
        d = len(next(iter(self.rows.values()))) if self.rows else 0
        rows = np.array([self.rows[int(i)] for i in ids], dtype=np.float32).reshape(len(ids), d)
        return ids, rows


def check_oracle(oracle, g, live, centres, P, what="", keep=False):
    """The contract of a mutated index against the CPU oracle's build (oracle.rqo_build) of S in id order, map_ids translated.
    keep: -> (the oracle index, ids) for further comparisons (the caller closes it)."""
    ids, rows = live.sorted()
    o = oracle.OracleIndex.build(rows, centres, P)
    try:
        assert (g.n, g.k) == (o.n, o.k), what
        for name in ARRAYS:
            assert np.array_equal(bits(getattr(g, name)), bits(getattr(o, name))), (what, "oracle", name)
        assert np.array_equal(g.map_ids, ids[o.map_ids]), (what, "oracle", "map_ids")
    except BaseException:
        o.close()
        raise
    if keep:
        return o, ids
    o.close()


def oracle_topk(oracle, oidx, queries, probe, topk, heur, ids=None, seen=None):
    """The oracle's side of compare_with_oracle on its own: -> (rough, precise) summed; seen: a list that takes every query's
    (distances, ids) as it is answered (what was answered stays in it when a later query raises where the reference panics)."""
    tot_r = tot_p = 0
    for q in queries:
        oracle.metrics_reset()
        od, oi = oidx.query(q, probe, topk, heur)
        m = oracle.metrics()
        tot_r += m["rough"]
        tot_p += m["precise"]
        if seen is not None:
            seen.append((od, oi if ids is None else ids[oi]))
    return tot_r, tot_p


def compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, heur, ids=None, filter=None, seen=None):
    """query_batch against the oracle, query by query: counts, ids in order, distance bits, then the counters.
    ids: translation of the oracle's ids (see sub_arrays).  filter: (the engine's filter, its bool mask over ids): the oracle
    answers on its view of sub_arrays(oidx, mask, ids).  seen: as in oracle_topk."""
    ov = None
    if filter is not None:
        filt, allowed = filter
        ov = oracle.OracleIndex.view(oidx.dim, *sub_arrays(oidx, allowed, ids))
        oidx, ids = ov, None
    try:
        rq.metrics_reset()
        if filter is None:
            d, gids, cnt = gidx.query_batch(queries, probe, topk, heur)
        else:
            d, gids, cnt = gidx.query_batch(queries, probe, topk, heur, filter=filt)
        tot_r = tot_p = 0
        for qi, q in enumerate(queries):
            oracle.metrics_reset()
            od, oi = oidx.query(q, probe, topk, heur)
            m = oracle.metrics()
            tot_r += m["rough"]
            tot_p += m["precise"]
            if ids is not None:
                oi = ids[oi]
            if seen is not None:
                seen.append((od, oi))
            n = int(cnt[qi])
            assert n == oi.size, (qi, n, oi.size)
            assert np.array_equal(gids[qi, :n], oi), (qi, gids[qi, :n], oi)
            assert np.array_equal(bits(d[qi, :n]), bits(od)), qi
        m = rq.metrics()
        assert (m["rough"], m["precise"], m["query"]) == (tot_r, tot_p, len(queries))
    finally:
        if ov is not None:
            ov.close()


class Ref:
    """The expected range answer from the oracle's stage functions: rough and accurate of every probed row, the two strict
    comparisons, the order.  `oidx`: an oracle.OracleIndex (built, or a view of arrays); ids: translation of its map_ids."""

    def __init__(self, oracle, oidx, ids=None):
        self.o, self.idx = oracle, oidx
        self.offsets = oidx.offsets.astype(np.int64)
        self.map_ids = oidx.map_ids if ids is None else np.asarray(ids, dtype=np.uint32)[oidx.map_ids]
        self.base = np.ascontiguousarray(oidx.base)
        self.dim = oidx.dim
        self.candidates = np.zeros(0, np.int64)   # per query of the last answer(): rows with rough < r

    def rows(self, q, probe):
        """-> (positions, rough) of every stored row of the query's probe lists, in visiting order."""
        y = self.idx.rotate_query(q)
        cl, cd = self.idx.coarse_rank(y, probe)
        cl = cl.astype(np.int64)
        begin, end = self.offsets[cl], self.offsets[cl + 1]
        total = int((end - begin).sum())
        if total == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.float32)
        # rqo_query_prep + rqo_scan_cluster per list, each list's rough distances written straight to their place in `rough` (the
        # calls of OracleIndex.query_prep / scan_cluster without their per-call arrays, which cost seconds over 100 000 lists)
        L, ptr = self.o.lib(), self.idx._ptr
        f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        rough = np.empty(total, dtype=np.float32)
        planes = np.zeros(self.dim // 64 * 4, dtype=np.uint64)
        yp, pp, ra = y.ctypes.data_as(f32p), planes.ctypes.data_as(u64p), rough.ctypes.data
        lo, delta, s = C.c_float(), C.c_float(), C.c_uint32()
        at = 0
        for c, ycd, ln in zip(cl.tolist(), cd.tolist(), (end - begin).tolist()):
            if ln == 0:
                continue
            L.rqo_query_prep(ptr, yp, c, C.byref(lo), C.byref(delta), C.byref(s), pp)
            L.rqo_scan_cluster(ptr, c, ycd, pp, lo, C.c_float(s.value), delta, C.cast(ra + 4 * at, f32p))
            at += ln
        return np.concatenate([np.arange(b, e) for b, e in zip(begin.tolist(), end.tolist()) if e > b]), rough

    def accurate(self, q, positions):
        """rqo_l2_squared_distance(query, row) of every position (one call: rqo_l2_squared_distance_rows)."""
        qp = np.zeros(self.dim, dtype=np.float32)
        qp[:q.size] = q
        return self.o.l2_squared_distance_rows(qp, self.base, positions)

    def answer(self, queries, probe, radii):
        """-> lims u64[nq + 1], dist, ids, counters {rough, precise}."""
        lims, dist, ids, cands = [0], [], [], []
        tot_rough = tot_precise = 0
        for q, r in zip(queries, radii):
            r = np.float32(r)
            pos, rough = self.rows(q, probe)
            tot_rough += pos.size
            cand = pos[rough < r]          # (False for a NaN radius)
            tot_precise += cand.size
            cands.append(cand.size)
            acc = self.accurate(q, cand)
            hit = acc < r
            d, i = acc[hit], self.map_ids[cand[hit]]
            order = np.lexsort((i, d.view(np.int32)))   # accurate >= +0: Ord32 is the bit pattern
            dist.append(d[order])
            ids.append(i[order])
            lims.append(lims[-1] + int(hit.sum()))
        self.candidates = np.array(cands, dtype=np.int64)
        return (np.array(lims, dtype=np.uint64), np.concatenate(dist).astype(np.float32) if dist else np.zeros(0, np.float32),
                np.concatenate(ids).astype(np.uint32) if ids else np.zeros(0, np.uint32), {"rough": tot_rough, "precise": tot_precise})

    def gated_rows(self, q, probe, r):
        """rows of the probe lists with accurate < r <= rough: what the reference's gate leaves out."""
        r = np.float32(r)
        pos, rough = self.rows(q, probe)
        out = pos[~(rough < r)]
        return int((self.accurate(q, out) < r).sum())


def same_range(got, want, what=""):
    gl, gd, gi = got
    wl, wd, wi = want
    assert gl.dtype == np.uint64 and gd.dtype == np.float32 and gi.dtype == np.uint32
    assert np.array_equal(gl, wl), (what, "lims", np.nonzero(gl != wl)[0][:5], gl[:8], wl[:8])
    assert np.array_equal(gi, wi), (what, "ids", np.nonzero(gi != wi)[0][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, "distance bits", np.nonzero(gd.view(np.uint32) != wd.view(np.uint32))[0][:5])


def run_range(rq, gidx, queries, probe, radii, filter=None):
    """-> (lims, dist, ids), counter deltas, profile"""
    from rabitq_amd import index as ix
    rq.metrics_reset()
    got = gidx.range_search(queries, probe, radii, filter=filter)
    m = rq.metrics()
    return got, m, ix.last_profile()


def tied_entries(lims, dist):
    """entries of a range answer whose distance bits equal their predecessor's inside the same query's segment."""
    if dist.size < 2:
        return 0
    eq = dist.view(np.uint32)[1:] == dist.view(np.uint32)[:-1]
    starts = np.asarray(lims[1:-1], dtype=np.int64)       # an entry that opens a segment has no predecessor in it
    starts = starts[(starts > 0) & (starts < dist.size)]
    eq[starts - 1] = False
    return int(eq.sum())
