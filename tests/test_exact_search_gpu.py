"""Exact search (rq_exact_search*, include/rabitq_hip.h): the brute-force top-k over the stored rows, on the GPU.

Ids, distance bits and counts are compared BIT FOR BIT with the CPU model (tests/exact_model.py: the oracle's exact-order distance of
every row, the `< f32::MAX` rule, the order (Ord32(e), id)).  The model of a fixture is computed once, over all its rows and for the
whole ranking, and every test takes prefixes of it.

Run on the GPU box:  python -m pytest tests/test_exact_search_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import byte_model as bm
from tests import exact_model as em
from tests import half_model as hm
from tests import ip_model as im
from tests import synth
from tests.models import Live, bits

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, UNSUPPORTED = -1, -6
QGROUP = 4096        # queries one scan launch takes (include/rabitq_hip.h: "a batch of up to 4096 queries is ONE launch")
NO_SEED, NO_PREFILTER = 1, 2
# d -> (n, k, queries).  n: many row tiles of the scan and a ragged tail.  The dims here are tile heights RT = 4 (128 rows: up to dim 192)
# and RT = 1 (32 rows: dim 512 .. 2432) only; RT = 2 (64 rows: dim 256 .. 448) and the boundary dims of every height are in
# tests/test_exact_scan_instantiations_gpu.py
SHAPES = {64: (3001, 16, 300), 100: (4003, 64, 40), 128: (6000, 64, 300), 192: (3005, 16, 40), 768: (3003, 16, 40)}


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def stats(rq):
    return rq.last_exact_stats()


_WORLD = {}


@pytest.fixture(scope="module")
def world(rq, oracle):
    """d -> the clustered L2 fixture of that dimension: the index, its data, and `full`: the model's whole ranking (topk = n) of its
    queries.  Built on first use, shared by the tests of the module."""
    def get(d):
        if d not in _WORLD:
            n, k, nq = SHAPES[d]
            x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=100 + d, centre_scale=1.0)
            q, _, _ = synth.mixture(nq, d, k, sigma=0.3, seed=200 + d, centre_scale=1.0)
            q[0] = x[7]                                    # a query equal to a stored row: distance 0
            if nq > 1:
                q[1] = 0.0                                 # the zero query
            P = synth.random_orthogonal((d + 63) // 64 * 64, seed=300 + d)
            gidx = rq.RaBitQ.build(x, centres, P)
            oidx = oracle.OracleIndex.build(x, centres, P)
            full = em.exact_batch(oracle, oidx.base, oidx.map_ids, em.transformed_queries(oracle, q, "l2", gidx.dim), n)
            _WORLD[d] = dict(d=d, n=n, k=k, x=x, centres=centres, P=P, q=q, gidx=gidx, oidx=oidx, full=full)
        return _WORLD[d]
    yield get
    for c in _WORLD.values():
        c["gidx"].close()
        c["oidx"].close()
    _WORLD.clear()


def expect(full, nq, topk):
    """The first nq queries of a whole-ranking model answer cut at topk, in RaBitQ.exact_search's layout."""
    fd, fi, fc = full
    w = min(topk, fd.shape[1])
    dist = np.full((nq, topk), np.nan, dtype=np.float32)
    ids = np.full((nq, topk), em.NO_ID, dtype=np.uint32)
    cnt = np.minimum(fc[:nq], topk).astype(np.uint32)
    live = np.arange(w)[None, :] < cnt[:, None]
    dist[:, :w][live] = fd[:nq, :w][live]
    ids[:, :w][live] = fi[:nq, :w][live]
    return dist, ids, cnt


def assert_same(got, want, what=""):
    (gd, gi, gc), (wd, wi, wc) = got, want
    assert np.array_equal(gc, wc), (what, "counts", gc[:8], wc[:8])
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert bad.size == 0, (what, "ids", int(bad[0]), gi[bad[0]][:12], wi[bad[0]][:12])
    assert np.array_equal(bits(gd), bits(wd)), (what, "distance bits")     # (NaN fill of the unused slots included)


# ---- sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sorted(SHAPES))
def test_sizes_and_topk(rq, world, d):
    """Every dimension (64; 100, padded; 128; 192; 768), batches of 1 / 40 / 300, topk 1 / 10 / 100 / 2048: the host entry equals the
    model; the first query sits on a stored row (distance 0 first), the second is the zero query."""
    c = world(d)
    nqs = sorted({1, 40, len(c["q"])})
    for nq, topk in [(nqs[0], 10), (nqs[1], 1), (nqs[1], 100), (nqs[-1], 10), (nqs[1], 2048)]:
        got = c["gidx"].exact_search(c["q"][:nq], topk)
        assert_same(got, expect(c["full"], nq, topk), (d, nq, topk))
        assert got[0][0, 0] == 0.0 and got[1][0, 0] <= 7                      # the stored row itself (or an equal row of a lower id)
        assert np.all(got[2] == min(topk, c["n"]))
        finite = np.nan_to_num(got[0], nan=np.inf).astype(np.float64)
        assert np.all(np.diff(finite, axis=1) >= 0)                          # ascending
    assert c["gidx"].exact_search(np.zeros((0, d), np.float32), 5)[2].size == 0     # nq == 0 is OK


def test_device_entry_equals_host_entry(rq, world):
    import torch
    c = world(128)
    nq, topk = 300, 10
    qd = torch.from_numpy(c["q"][:nq]).cuda()
    od = torch.full((nq, topk), float("nan"), device="cuda", dtype=torch.float32)
    oi = torch.full((nq, topk), -1, device="cuda", dtype=torch.int32)
    on = torch.zeros((nq,), device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()
    c["gidx"].exact_search_device(qd.data_ptr(), nq, qd.shape[1], topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
    torch.cuda.synchronize()
    got = (od.cpu().numpy(), oi.cpu().numpy().view(np.uint32), on.cpu().numpy().view(np.uint32))
    assert_same(got, expect(c["full"], nq, topk), "device")
    assert_same(got, c["gidx"].exact_search(c["q"][:nq], topk), "device vs host")


def test_one_query_group_plus_one(rq, oracle, world):
    """4097 queries: two scan launches, the second with a single query; the answer is the model's, query by query."""
    c = world(64)
    nq, topk = QGROUP + 1, 5
    q, _, _ = synth.mixture(nq, 64, c["k"], sigma=0.3, seed=991, centre_scale=1.0)
    got = c["gidx"].exact_search(q, topk)
    st = stats(rq)
    assert st["scan_launches"] == 2 + st["reruns"] and st["row_bytes_read"] == st["scan_launches"] * c["n"] * 64 * 4
    want = em.exact_batch(oracle, c["oidx"].base, c["oidx"].map_ids, em.transformed_queries(oracle, q, "l2", 64), topk)
    assert_same(got, want, "4097 queries")


def test_topk_larger_than_n(rq, oracle):
    n, d, k = 500, 64, 4
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=41)
    q, _, _ = synth.mixture(40, d, k, sigma=0.3, seed=42)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=43))
    try:
        want = em.index_answer(oracle, g, q, 2048)
        assert np.all(want[2] == n)
        assert_same(g.exact_search(q, 2048), want, "topk > n")
        assert stats(rq)["seed_unfilled"] == 40                               # no seed can hold 2048 of 500 rows
        assert_same(g.exact_search(q, 600), em.index_answer(oracle, g, q, 600), "topk = 600 > n")
    finally:
        g.close()


# ---- where the pre-filter can go wrong ---------------------------------------------------------------------------------------
def test_rows_far_from_the_origin(rq, oracle):
    """Rows of 1000 + N(0, 1): the norms are a thousand times the distances, the bf16 approximation says nothing, the margin must
    carry the answer."""
    n, d, k = 3001, 128, 16
    rng = np.random.default_rng(51)
    centres = (1000.0 + 0.5 * rng.standard_normal((k, d))).astype(np.float32)
    x = (centres[rng.integers(0, k, n)] + rng.standard_normal((n, d))).astype(np.float32)
    q = (centres[rng.integers(0, k, 40)] + rng.standard_normal((40, d))).astype(np.float32)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=52))
    try:
        for topk in (10, 64):
            assert_same(g.exact_search(q, topk), em.index_answer(oracle, g, q, topk), ("far", topk))
        # nothing can be pruned here: the first call outgrew the default candidate slots, and the index remembers what it learnt
        assert stats(rq)["reruns"] == 0 and stats(rq)["candidates"] > 40 * 1024
        g2 = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=52))
        try:
            g2.exact_search(q, 10)
            assert stats(rq)["reruns"] >= 1
            g2.exact_search(q, 10)
            assert stats(rq)["reruns"] == 0
        finally:
            g2.close()
    finally:
        g.close()


def test_near_ties_at_the_cut(rq, oracle):
    """Hundreds of rows on a thin shell around each query centre: their distances differ in the last bits, the cut at topk falls among
    them, and the bf16 approximation cannot tell them apart."""
    n, d, k = 3001, 64, 8
    rng = np.random.default_rng(61)
    centres = rng.standard_normal((k, d)).astype(np.float32)
    u = rng.standard_normal((n, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    radius = 1.0 + 1e-6 * rng.integers(0, 8, n)                               # eight shells a few ulps apart
    x = (centres[rng.integers(0, k, n)] + u * radius[:, None]).astype(np.float32)
    q = centres[np.arange(16) % k].copy()
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=62))
    try:
        for topk in (16, 64):
            assert_same(g.exact_search(q, topk), em.index_answer(oracle, g, q, topk), ("near ties", topk))
    finally:
        g.close()


def test_exact_ties_duplicates_nan_inf_and_overflowing_rows(rq, oracle):
    """The identity-rotation fixture of test_keys_and_ties with small-integer rows: distances are exact integers, ties are everywhere
    and go by id; exact duplicates of stored rows (the lower id first); a NaN row and an inf row are never returned; a row whose squared
    norm overflows f32 is still returned by the query next to it, with its exact distance (the header's guarantee)."""
    d, k = 128, 16
    rng = np.random.default_rng(5)
    centres = np.zeros((k, d), np.float32)
    for c in range(k):
        centres[c, c % d] = 4.0 if c % 2 == 0 else -4.0
        centres[c, (c // 2) + 32] = 1.0
    x0 = (centres[rng.integers(0, k, 3000)] + rng.integers(-2, 3, (3000, d))).astype(np.float32)
    g = rq.RaBitQ.build(x0, centres, np.eye(d, dtype=np.float32))
    try:
        dup = x0[[5, 17, 17, 2999]]
        bad = np.stack([np.full(d, np.nan, np.float32), np.full(d, np.inf, np.float32)])
        huge = np.full((1, d), 2.0e19, np.float32)                            # |x|^2 = 128 * 4e38: above f32::MAX
        new = np.concatenate([dup, bad, huge]).astype(np.float32)
        got_ids = g.add(new)
        nan_id, inf_id, huge_id = int(got_ids[4]), int(got_ids[5]), int(got_ids[6])
        q = (centres[rng.integers(0, k, 40)] + rng.integers(-2, 3, (40, d))).astype(np.float32)
        q[0], q[1] = x0[17], x0[5]
        q[2] = huge[0] * F32(1.0 + 2.0 ** -10)                                # next to the overflowing row: e = 128 * (2e19 * 2^-10)^2, finite
        q[3] = 0.0
        base, mids = g.base, g.map_ids
        qp = em.transformed_queries(oracle, q, "l2", d)
        with np.errstate(all="ignore"):
            for topk in (1, 10, 100, 2048):
                want = em.exact_batch(oracle, base, mids, qp, topk)
                got = g.exact_search(q, topk)
                assert_same(got, want, ("ties", topk))
        assert got[1][0, :3].tolist() == [17, int(got_ids[1]), int(got_ids[2])] and not got[0][0, :3].any()   # row 17 and its two copies
        assert got[1][1, :2].tolist() == [5, int(got_ids[0])]
        assert got[1][2, 0] == huge_id and got[2][2] == 1 and np.isfinite(got[0][2, 0])    # every other row is at inf from q[2]
        for qi in (0, 1, 3, 4):
            assert nan_id not in got[1][qi] and inf_id not in got[1][qi] and huge_id not in got[1][qi]
        ties = sum(int((np.diff(got[0][qi, :got[2][qi]]) == 0).sum()) for qi in range(4, 40))
        assert ties > 100                                                     # the fixture does what it is for
    finally:
        g.close()


@pytest.mark.parametrize("d,n", [(1024, 1301), (2496, 301)])
def test_wide_dimensions(rq, oracle, d, n):
    """dim 1024: the 32-row tile needs more LDS than a launch gets without the function attribute (set in another unit than the
    host's); dim 2496: no tile fits, the call runs without the pre-filter -- every admitted pair gets its exact distance."""
    k, nq = 4, 8
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=d)
    q, _, _ = synth.mixture(nq, d, k, sigma=0.3, seed=d + 1)
    q[0] = x[3]
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=d + 2))
    try:
        for topk in (10, 64):
            assert_same(g.exact_search(q, topk), em.index_answer(oracle, g, q, topk), (d, topk))
        st = stats(rq)
        if d > 2432:
            assert st["exact"] == nq * n and st["seed_probe"] == 0
        else:
            assert st["exact"] < nq * n and st["seed_probe"] > 0
    finally:
        g.close()


# ---- result-neutral parameters ---------------------------------------------------------------------------------------------
def test_parameters_never_change_the_answer(rq, world):
    c = world(128)
    g, n, nq, topk = c["gidx"], c["n"], 100, 10
    want = expect(c["full"], nq, topk)
    assert_same(g.exact_search(c["q"][:nq], topk), want, "defaults")
    st = stats(rq)
    assert st["candidates"] < st["exact"] < nq * n and st["seed_unfilled"] == 0 and st["seed_probe"] >= 2 * topk   # (exact: the sample's too)
    assert st["row_bytes_read"] == st["scan_launches"] * n * 128 * 4
    for prm in (dict(seed_probe=1), dict(seed_probe=c["k"]), dict(flags=NO_SEED), dict(flags=NO_PREFILTER), dict(cand_per_query=1),
                dict(flags=NO_SEED | NO_PREFILTER, cand_per_query=7)):
        assert_same(g.exact_search(c["q"][:nq], topk, params=prm), want, prm)
        st = stats(rq)
        if prm.get("cand_per_query"):
            assert st["reruns"] >= 1, st
        if prm.get("flags", 0) & NO_PREFILTER:
            assert st["exact"] == nq * n, st
        if "seed_probe" in prm:                                              # the bound's sample: seed_probe rows per topk (+ the stride's rounding)
            assert prm["seed_probe"] * topk <= st["seed_probe"] <= 2 * prm["seed_probe"] * topk, st
    with pytest.raises(rq.RabitqError) as e:
        g.exact_search(c["q"][:4], topk, params=dict(flags=4))
    assert e.value.status == INVALID


# ---- filters -----------------------------------------------------------------------------------------------------------------
def test_filters(rq, oracle, world):
    c = world(128)
    g, o, n, nq = c["gidx"], c["oidx"], c["n"], 40
    qp = em.transformed_queries(oracle, c["q"][:nq], "l2", g.dim)
    rng = np.random.default_rng(71)
    offs, mids = o.offsets.astype(np.int64), o.map_ids
    by_list = np.zeros(n, dtype=bool)
    by_list[mids[offs[3]:offs[5]]] = True                                     # everything in lists 3 and 4
    few = np.zeros(n, dtype=bool)
    few[rng.choice(n, 6, replace=False)] = True
    masks = {"dense": rng.random(n) < 0.5, "sparse": rng.random(n) < 0.005, "by-list": by_list, "few": few, "empty": np.zeros(n, dtype=bool)}
    for name, mask in masks.items():
        with g.make_filter(mask=mask) as f:
            for topk in (10, 64):
                want = em.exact_batch(oracle, o.base, mids, qp, topk, mask)
                assert_same(g.exact_search(c["q"][:nq], topk, filter=f), want, (name, topk))
                st = stats(rq)
                if name == "empty":
                    assert np.all(want[2] == 0)
                if name == "few":                                             # fewer admitted rows than topk: exactly those rows
                    assert np.all(want[2] == 6) and st["seed_unfilled"] == nq
                    assert_same(g.exact_search(c["q"][:nq], topk, filter=f, params=dict(flags=NO_PREFILTER)), want, (name, "all pairs"))
                    assert stats(rq)["exact"] == nq * 6


def test_stale_and_foreign_filters_are_refused(rq):
    n, d, k = 1000, 64, 4
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=81)
    P = synth.random_orthogonal(d, seed=82)
    g, other = rq.RaBitQ.build(x[:900], centres, P), rq.RaBitQ.build(x[:900], centres, P)
    try:
        f = g.make_filter(mask=np.ones(n, dtype=bool))
        assert g.exact_search(x[:3], 5, filter=f)[2].tolist() == [5, 5, 5]
        with pytest.raises(rq.RabitqError) as e:
            other.exact_search(x[:3], 5, filter=f)
        assert e.value.status == INVALID
        g.add(x[900:])
        with pytest.raises(rq.RabitqError) as e:
            g.exact_search(x[:3], 5, filter=f)
        assert e.value.status == INVALID
        f.close()
    finally:
        g.close()
        other.close()


# ---- row types and metrics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["f16", "bf16", "u8", "i8"])
def test_typed_rows_equal_the_f32_index_of_the_widened_rows(rq, oracle, rows):
    n, d, k, nq = 3001, 128, 16, 40
    P = synth.random_orthogonal(d, seed=91)
    if rows in ("u8", "i8"):
        b, centres, marks = bm.byte_data(rows, n, d, k, seed=92)
        wx, q = bm.widen(b, rows), bm.byte_queries(rows, b, marks, nq, d, k, seed=93)
        typed = b
    else:
        x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=92)
        q, _, _ = synth.mixture(nq, d, k, sigma=0.3, seed=93)
        h = hm.narrow(x, rows)
        wx = hm.widen(h, rows)
        typed = h.view(np.float16) if rows == "f16" else h
    g = rq.RaBitQ.build(typed, centres, P, rows=rows)
    twin = rq.RaBitQ.build(wx, centres, P)
    try:
        for topk in (10, 64):
            a, b_ = g.exact_search(q, topk), twin.exact_search(q, topk)
            assert_same(a, b_, (rows, topk, "twin"))
            assert_same(a, em.index_answer(oracle, twin, q, topk), (rows, topk, "model"))
        g.exact_search(q, 10)
        assert stats(rq)["row_bytes_read"] == stats(rq)["scan_launches"] * n * d * (1 if rows in ("u8", "i8") else 2)
    finally:
        g.close()
        twin.close()


@pytest.mark.parametrize("metric,d", [("cosine", 100), ("cosine", 128), ("ip", 100), ("ip", 128)])
def test_cosine_and_ip_against_the_model(rq, oracle, metric, d):
    """The model runs on the index's STORED rows (normalised / augmented) and the transformed queries."""
    n, k, nq = 3001, 16, 40
    x, centres, _ = synth.mixture(n, d, k, sigma=0.4, seed=101 + d)
    q, _, _ = synth.mixture(nq, d, k, sigma=0.4, seed=102 + d)
    x *= np.random.default_rng(9).uniform(0.5, 2.0, (n, 1)).astype(np.float32)      # norms that matter to both metrics
    dim = im.ip_dim(d) if metric == "ip" else (d + 63) // 64 * 64
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(dim, seed=103), metric=metric)
    try:
        assert g.dim == dim
        for topk in (10, 64):
            got = g.exact_search(q, topk)
            assert_same(got, em.index_answer(oracle, g, q, topk, metric=metric), (metric, d, topk))
        if metric == "ip":
            ip = g.inner_product(got[0], q, got[2])
            assert np.all(np.diff(ip.astype(np.float64), axis=1) <= 0)        # the min-side of the reduction: descending products
            best = (q.astype(np.float64) @ x.astype(np.float64).T).max(axis=1)
            np.testing.assert_allclose(ip[:, 0], best, rtol=1e-3, atol=1e-3)
    finally:
        g.close()


# ---- mutated indexes, shards, cross-checks ---------------------------------------------------------------------------------------
def test_mutated_index_equals_its_canonical_rebuild(rq):
    n, d, k = 5000, 128, 16
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=111)
    q, _, _ = synth.mixture(40, d, k, sigma=0.3, seed=112)
    P = synth.random_orthogonal(d, seed=113)
    g = rq.RaBitQ.build(x[:3000], centres, P)
    live = Live(np.arange(3000), x[:3000])
    live.add(g.add(x[3000:]), x[3000:])
    gone = np.random.default_rng(3).choice(n, 700, replace=False)
    g.remove(ids=gone)
    live.remove(gone)
    ids, rows = live.sorted()
    c = rq.RaBitQ.build(rows, centres, P)
    try:
        for topk in (10, 100):
            (ad, ai, an), (bd, bi, bn) = g.exact_search(q, topk), c.exact_search(q, topk)
            assert_same((ad, ai, an), (bd, ids[bi], bn), ("mutated", topk))   # ids translated as tests/test_mutable_gpu.py does
    finally:
        g.close()
        c.close()


def test_shards_are_indexes(rq, oracle, world):
    c = world(128)
    owner = c["gidx"].partition_lists(2)[0]
    for rank in (0, 1):
        s = c["gidx"].shard(owner, rank)
        try:
            want = em.index_answer(oracle, s, c["q"][:40], 10)
            assert_same(s.exact_search(c["q"][:40], 10), want, ("shard", rank))
            assert set(want[1].ravel().tolist()) <= set(s.map_ids.tolist())
        finally:
            s.close()


def test_query_results_appear_in_the_exact_answer(rq):
    """The approximate query at probe = k: every (id, distance) it returns is in the exact answer of topk = n with the same distance
    bits, and its j-th smallest distance is at or above the exact j-th."""
    n, d, k, nq, topk = 2000, 128, 8, 64, 10
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=121)
    q, _, _ = synth.mixture(nq, d, k, sigma=0.3, seed=122)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=123))
    try:
        ed, ei, en = g.exact_search(q, n)
        assert np.all(en == n)
        qd, qi, qn = g.query_batch(q, k, topk)
        for b in range(nq):
            exact = {int(i): F32(v).tobytes() for i, v in zip(ei[b], ed[b])}
            for j in range(int(qn[b])):
                assert exact[int(qi[b, j])] == F32(qd[b, j]).tobytes(), (b, j)
            mine = np.sort(qd[b, :qn[b]])
            assert np.all(mine >= ed[b, :qn[b]])
    finally:
        g.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tiered", "split_rows"])
def test_tiered_and_split_row_indexes_are_refused(rq, kind):
    from rabitq_amd import index as ix
    n, d, k = 12000, 128, 24
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=61, centre_scale=0.6)
    if kind == "tiered":
        ix.set_option("base_device_mb", 1)
    else:
        ix.set_option("split_rows", 2)
    try:
        g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=62))
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)
    try:
        assert (g.n_hbm < n) if kind == "tiered" else g.split_rows
        with pytest.raises(rq.RabitqError) as e:
            g.exact_search(x[:4], 10)
        assert e.value.status == UNSUPPORTED
    finally:
        g.close()


def test_bad_arguments_are_refused(rq, world):
    from rabitq_amd import _lib
    c = world(64)
    g, q = c["gidx"], c["q"][:4]
    for topk in (0, 2049):
        with pytest.raises(rq.RabitqError) as e:
            g.exact_search(q, topk)
        assert e.value.status == UNSUPPORTED
    assert g.exact_search(q[:, :63], 5)[2].tolist() == [5, 5, 5, 5]           # 63 floats pad to 64: fine
    with pytest.raises(rq.RabitqError) as e:
        g.exact_search(np.zeros((2, 65), np.float32), 5)                      # 65 do not
    assert e.value.status == -2
    L = _lib.lib()
    dist, ids, cnt = np.zeros((4, 5), np.float32), np.zeros((4, 5), np.uint32), np.zeros(4, np.uint32)
    addr = lambda a: C.c_void_p(a.ctypes.data)
    assert L.rq_exact_search(g._h, None, addr(q), 4, 64, 5, None, addr(dist), addr(ids), addr(cnt)) == 0
    assert L.rq_exact_search(g._h, None, addr(q), 4, 64, 5, None, addr(dist), None, addr(cnt)) == INVALID      # a null output pointer
    assert L.rq_exact_search(g._h, None, addr(q), 4, 64, 5, None, addr(dist), addr(ids), None) == INVALID
    assert L.rq_exact_search(None, None, addr(q), 4, 64, 5, None, addr(dist), addr(ids), addr(cnt)) == INVALID
    prm = _lib.ExactParamsT()
    prm.struct_size = 0
    assert L.rq_exact_search(g._h, None, addr(q), 4, 64, 5, C.byref(prm), addr(dist), addr(ids), addr(cnt)) == INVALID
    assert L.rq_last_exact_stats(None) == INVALID


# ---- Python helpers and the CLI ---------------------------------------------------------------------------------------------------
def test_recall_and_tune_nprobe(rq, world):
    c = world(100)                                                             # 64 lists
    g, q, topk = c["gidx"], c["q"], 10
    _, eids, ecnt = g.exact_search(q, topk)

    def by_hand(probe):
        _, ids, cnt = g.query_batch(q, probe, topk)
        return float(np.mean([len(set(ids[b, :cnt[b]].tolist()) & set(eids[b, :ecnt[b]].tolist())) / int(ecnt[b]) for b in range(len(q))]))

    curve = {p: by_hand(p) for p in range(1, c["k"] + 1)}
    for p in (1, 3, 64):
        assert g.recall(q, p, topk) == curve[p]
    assert curve[c["k"]] >= curve[1] and curve[c["k"]] > 0.9
    for target in (0.5, 0.9, curve[c["k"]], 1.01):
        passing = [p for p in sorted(curve) if curve[p] >= target]
        want = (passing[0], curve[passing[0]]) if passing else (c["k"], curve[c["k"]])
        assert g.tune_nprobe(q, topk, target) == want, target
    with g.make_filter(mask=np.arange(c["n"]) % 3 == 0) as f:
        r = g.recall(q, 4, topk, filter=f)
        _, fe, fc = g.exact_search(q, topk, filter=f)
        _, fi, fn = g.query_batch(q, 4, topk, filter=f)
        assert r == float(np.mean([len(set(fi[b, :fn[b]].tolist()) & set(fe[b, :fc[b]].tolist())) / int(fc[b]) for b in range(len(q))]))


def test_cli_make_truth(rq, tmp_path):
    from rabitq_amd import cli, vecs
    n, d, k, nq = 2000, 64, 8, 20
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=131)
    q, _, _ = synth.mixture(nq, d, k, sigma=0.3, seed=132)
    paths = {name: str(tmp_path / name) for name in ("b.fvecs", "c.fvecs", "q.fvecs", "t.ivecs", "saved")}
    vecs.write_vecs(paths["b.fvecs"], list(x))
    vecs.write_vecs(paths["c.fvecs"], list(centres))
    vecs.write_vecs(paths["q.fvecs"], list(q))
    argv = ["-b", paths["b.fvecs"], "-c", paths["c.fvecs"], "-q", paths["q.fvecs"], "-t", paths["t.ivecs"], "-s", paths["saved"],
            "-p", "8", "-k", "10", "--make-truth"]
    assert cli.main(argv) == 0
    truth = vecs.read_vecs(paths["t.ivecs"], np.int32)
    g = rq.RaBitQ.load_from_dir(paths["saved"])
    try:
        _, ids, cnt = g.exact_search(q, 100)
    finally:
        g.close()
    assert len(truth) == nq and all(np.array_equal(truth[b].view(np.uint32), ids[b, :cnt[b]]) for b in range(nq))
    vecs.write_ivecs(paths["t.ivecs"], np.zeros((nq, 100), np.int32))         # an existing file is left alone
    before = open(paths["t.ivecs"], "rb").read()
    assert cli.main(argv) == 0
    assert open(paths["t.ivecs"], "rb").read() == before
