"""Exact range search (rq_exact_range_search*, include/rabitq_hip.h): every stored row within a per-query radius, on the GPU.

lims, ids and distance bits are compared BIT FOR BIT with the CPU model (tests/exact_range_model.py: the oracle's exact-order distance
of every row, strict `<` against the radius and f32::MAX, the order (Ord32(e), id)).  The model of a fixture is its whole ranking,
computed once; a test cuts it at its radii.

Run on the GPU box:  python -m pytest tests/test_exact_range_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import byte_model as bm
from tests import exact_model as em
from tests import exact_range_model as erm
from tests import half_model as hm
from tests import synth
from tests.models import Live, bits

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, UNSUPPORTED = -1, -6
QGROUP = 4096        # queries one scan launch takes
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
    queries.  Built on first use, shared by the tests of the module, never changed."""
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


def kth_radii(full, kth, nq=None):
    """Every query's kth-smallest exact distance (the answer then has fewer than kth entries: the comparison is strict)."""
    return full[0][:nq, kth - 1].copy()


def assert_same(got, want, what=""):
    (gl, gd, gi), (wl, wd, wi) = got, want
    assert gl.dtype == np.uint64 and gl[0] == 0 and gd.size == gi.size == int(gl[-1]), what
    assert np.array_equal(gl, wl), (what, "lims", np.diff(gl)[:8], np.diff(wl)[:8])
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, (what, "ids", int(bad[0]), gi[bad[0]:bad[0] + 8], wi[bad[0]:bad[0] + 8])
    assert np.array_equal(bits(gd), bits(wd)), (what, "distance bits")


# ---- sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sorted(SHAPES))
def test_dimensions_and_known_answer_sizes(rq, world, d):
    """Every dimension (64; 100, padded; 128; 192; 768), batches of 1 / 40 / 300, radii at the model's 1st / 10th / 1000th neighbour:
    the host entry equals the model; query 0 sits on a stored row, query 1 is the zero query."""
    c = world(d)
    nqs = sorted({1, 40, len(c["q"])})
    for nq, kth in [(nqs[0], 10), (nqs[1], 1), (nqs[1], 1000), (nqs[-1], 10), (nqs[-1], 1000)]:
        radii = kth_radii(c["full"], kth, nq)
        got = c["gidx"].exact_range_search(c["q"][:nq], radii)
        assert_same(got, erm.cut_full(c["full"], radii, nq), (d, nq, kth))
        counts = np.diff(got[0]).astype(np.int64)
        assert np.all(counts <= kth - 1) and (kth == 1 or counts.max() == kth - 1)      # (fewer only where the kth distance is tied)
        if kth > 1:
            assert got[1][0] == 0.0 and got[2][0] <= 7                        # the stored row itself (or an equal row of a lower id)
        st = stats(rq)
        assert st["seed_probe"] == 0 and st["ms_seed"] == 0 and st["seed_unfilled"] == 0 and st["exact"] == st["candidates"] >= got[0][-1]
    lims, dist, ids = c["gidx"].exact_range_search(np.zeros((0, d), np.float32), np.zeros(0, np.float32))
    assert lims.tolist() == [0] and dist.size == 0 and ids.size == 0          # nq == 0 is OK


@pytest.mark.parametrize("d,n", [(1024, 1301), (2496, 301)])
def test_wide_dimensions(rq, oracle, d, n):
    """dim 1024: one 32-row sub-tile per block in the whole LDS of a CU (the function attribute of the RANGE instantiation); dim 2496:
    no tile fits, the call runs without the pre-filter -- every admitted pair gets its exact distance."""
    k, nq = 4, 8
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=d)
    q, _, _ = synth.mixture(nq, d, k, sigma=0.3, seed=d + 1)
    q[0] = x[3]
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=d + 2))
    try:
        full = em.index_answer(oracle, g, q, n)
        for kth in (10, 64):
            radii = kth_radii(full, kth)
            assert_same(g.exact_range_search(q, radii), erm.cut_full(full, radii), (d, kth))
            st = stats(rq)
            assert (st["candidates"] == nq * n) if d > 2432 else (st["candidates"] < nq * n), st
    finally:
        g.close()


def test_skew_and_arena_overflow(rq, world):
    """One query admits the whole index, the other 299 three rows at most: the arena holds the pairs kept, and a launch that overflows
    it (cand_per_query = 4: 1200 records) is run again with the count it learnt."""
    c = world(128)
    g, n, nq = c["gidx"], c["n"], 300
    radii = kth_radii(c["full"], 3, nq)
    radii[0] = np.inf
    want = erm.cut_full(c["full"], radii, nq)
    assert int(want[0][1]) == n and int(want[0][-1]) <= n + 2 * (nq - 1)
    for prm, forced in ((None, False), (dict(cand_per_query=4), True)):
        assert_same(g.exact_range_search(c["q"][:nq], radii, params=prm), want, ("skew", prm))
        st = stats(rq)
        assert st["scan_launches"] == 1 + st["reruns"] and st["row_bytes_read"] == st["scan_launches"] * n * 128 * 4, st
        assert st["candidates"] >= n
        if forced:
            assert st["reruns"] >= 1, st


def test_one_query_group_plus_one(rq, oracle, world):
    """4097 queries with small radii: two scan launches, the second with a single query; the pieces are united in query order."""
    c = world(64)
    nq, kth = QGROUP + 1, 5
    q, _, _ = synth.mixture(nq, 64, c["k"], sigma=0.3, seed=991, centre_scale=1.0)
    top = em.exact_batch(oracle, c["oidx"].base, c["oidx"].map_ids, em.transformed_queries(oracle, q, "l2", 64), kth)
    radii = kth_radii(top, kth)                                               # (everything below the 5th distance is in the top 5)
    got = c["gidx"].exact_range_search(q, radii)
    st = stats(rq)
    assert st["scan_launches"] == 2 + st["reruns"] and st["row_bytes_read"] == st["scan_launches"] * c["n"] * 64 * 4
    assert_same(got, erm.cut_full(top, radii), "4097 queries")
    assert int(got[0][-1]) > nq                                               # the fixture does what it is for


# ---- radii -----------------------------------------------------------------------------------------------------------------
def test_edge_radii(rq, world):
    c = world(128)
    g, nq = c["gidx"], 40
    q = c["q"][:nq]
    dead = np.array([np.nan, 0.0, -0.0, -1.0, -np.inf], dtype=np.float32)[np.arange(nq) % 5]
    for prm in (None, dict(flags=NO_PREFILTER)):
        lims, dist, ids = g.exact_range_search(q, dead, params=prm)
        assert not lims.any() and lims.size == nq + 1 and dist.size == 0 and ids.size == 0
        assert stats(rq)["candidates"] == 0 and stats(rq)["exact"] == 0       # such a query costs nothing behind the scan
    # a radius exactly at a row's e excludes the row; the next f32 includes it
    at = kth_radii(c["full"], 5, nq)
    up = np.nextafter(at, F32(np.inf))
    got_at, got_up = g.exact_range_search(q, at), g.exact_range_search(q, up)
    assert_same(got_at, erm.cut_full(c["full"], at, nq), "at e")
    assert_same(got_up, erm.cut_full(c["full"], up, nq), "next after e")
    for b in range(nq):
        fifth = c["full"][1][b, 4]
        assert fifth not in got_at[2][int(got_at[0][b]):int(got_at[0][b + 1])]
        assert fifth in got_up[2][int(got_up[0][b]):int(got_up[0][b + 1])]
    # inf and f32::MAX admit every row (all distances are finite here); mixed with dead radii in one batch
    mixed = at.copy()
    mixed[0::4], mixed[1::4], mixed[2::4] = np.inf, np.nan, em.F32_MAX
    got = g.exact_range_search(q, mixed)
    assert_same(got, erm.cut_full(c["full"], mixed, nq), "mixed")
    counts = np.diff(got[0])
    assert np.all(counts[0::4] == c["n"]) and not counts[1::4].any() and np.all(counts[2::4] == c["n"])
    assert_same(g.exact_range_search(q, 2.5), erm.cut_full(c["full"], 2.5, nq), "scalar radius")


def test_duplicates_nan_inf_and_overflowing_rows(rq, oracle):
    """The data recipe of test_exact_ties_duplicates_nan_inf_and_overflowing_rows: integer rows (ties everywhere, by id), exact
    duplicates (the lower id first), a NaN row and an inf row (never returned), a row whose squared norm overflows f32 (returned by
    the query next to it, with its exact distance)."""
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
        got_ids = g.add(np.concatenate([dup, bad, huge]).astype(np.float32))
        nan_id, inf_id, huge_id = int(got_ids[4]), int(got_ids[5]), int(got_ids[6])
        q = (centres[rng.integers(0, k, 40)] + rng.integers(-2, 3, (40, d))).astype(np.float32)
        q[0], q[1] = x0[17], x0[5]
        q[2] = huge[0] * F32(1.0 + 2.0 ** -10)                                # next to the overflowing row: e finite
        q[3] = 0.0
        base, mids = g.base, g.map_ids
        qp = em.transformed_queries(oracle, q, "l2", d)
        with np.errstate(all="ignore"):
            full = em.exact_batch(oracle, base, mids, qp, len(mids))
            for radii in (np.inf, em.F32_MAX, np.where(np.arange(40) < 4, F32(np.inf), F32(600.0)).astype(np.float32), F32(401.0)):
                got = g.exact_range_search(q, radii)
                assert_same(got, erm.range_batch(oracle, base, mids, qp, radii), ("ties", radii))
                assert_same(got, erm.cut_full(full, radii), ("ties, prefix", radii))
        lims, dist, ids = g.exact_range_search(q, np.inf)
        seg = lambda b: slice(int(lims[b]), int(lims[b + 1]))
        assert ids[seg(0)][:3].tolist() == [17, int(got_ids[1]), int(got_ids[2])] and not dist[seg(0)][:3].any()
        assert ids[seg(1)][:2].tolist() == [5, int(got_ids[0])]
        assert ids[seg(2)].tolist() == [huge_id] and np.isfinite(dist[seg(2)][0])        # every other row is at inf from q[2]
        for b in (0, 1, 3, 4):
            assert not np.isin([nan_id, inf_id, huge_id], ids[seg(b)]).any() and lims[b + 1] - lims[b] == 3004
        assert sum(int((np.diff(dist[seg(b)]) == 0).sum()) for b in range(4, 40)) > 100    # ties: the fixture does what it is for
    finally:
        g.close()


# ---- result-neutral parameters ---------------------------------------------------------------------------------------------
def test_parameters_never_change_the_answer(rq, world):
    c = world(128)
    g, n, nq = c["gidx"], c["n"], 100
    radii = kth_radii(c["full"], 10, nq)
    want = erm.cut_full(c["full"], radii, nq)
    for flags in (0, NO_SEED, NO_PREFILTER, NO_SEED | NO_PREFILTER):
        for cand in (0, 1, 64):
            prm = dict(flags=flags, cand_per_query=cand, seed_probe=3 if cand else 0)
            assert_same(g.exact_range_search(c["q"][:nq], radii, params=prm), want, prm)
            st = stats(rq)
            assert st["exact"] == st["candidates"] and st["scan_launches"] == 1 + st["reruns"] and st["seed_probe"] == 0, st
            if flags & NO_PREFILTER:
                assert st["candidates"] == nq * n, st
                assert st["reruns"] >= (1 if cand else 0), st
            else:
                assert want[0][-1] <= st["candidates"] < nq * n, st           # the scan prunes
    with pytest.raises(rq.RabitqError) as e:
        g.exact_range_search(c["q"][:4], radii[:4], params=dict(flags=4))
    assert e.value.status == INVALID


# ---- filters -----------------------------------------------------------------------------------------------------------------
def test_filters(rq, oracle, world):
    c = world(128)
    g, o, n, nq = c["gidx"], c["oidx"], c["n"], 40
    qp = em.transformed_queries(oracle, c["q"][:nq], "l2", g.dim)
    rng = np.random.default_rng(71)
    masks = {"tenth": rng.random(n) < 0.1, "half": rng.random(n) < 0.5, "empty": np.zeros(n, dtype=bool)}
    radii = kth_radii(c["full"], 100, nq)
    for name, mask in masks.items():
        with g.make_filter(mask=mask) as f:
            for r in (radii, np.inf):
                want = erm.range_batch(oracle, o.base, o.map_ids, qp, r, mask)
                assert_same(g.exact_range_search(c["q"][:nq], r, filter=f), want, (name, "radii" if r is radii else "inf"))
            assert_same(g.exact_range_search(c["q"][:nq], radii, filter=f, params=dict(flags=NO_PREFILTER)),
                        erm.range_batch(oracle, o.base, o.map_ids, qp, radii, mask), (name, "all pairs"))
            assert stats(rq)["candidates"] == nq * int(mask.sum())
            if name == "empty":
                assert want[0][-1] == 0


def test_stale_and_foreign_filters_are_refused(rq):
    n, d, k = 1000, 64, 4
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=81)
    P = synth.random_orthogonal(d, seed=82)
    g, other = rq.RaBitQ.build(x[:900], centres, P), rq.RaBitQ.build(x[:900], centres, P)
    try:
        f = g.make_filter(mask=np.ones(n, dtype=bool))
        assert np.diff(g.exact_range_search(x[:3], np.inf, filter=f)[0]).tolist() == [900, 900, 900]
        with pytest.raises(rq.RabitqError) as e:
            other.exact_range_search(x[:3], 1.0, filter=f)
        assert e.value.status == INVALID
        g.add(x[900:])
        with pytest.raises(rq.RabitqError) as e:
            g.exact_range_search(x[:3], 1.0, filter=f)
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
        full = em.index_answer(oracle, twin, q, n)
        for kth in (10, 200):
            radii = kth_radii(full, kth)
            a = g.exact_range_search(q, radii)
            assert stats(rq)["row_bytes_read"] == stats(rq)["scan_launches"] * n * d * (1 if rows in ("u8", "i8") else 2)
            assert_same(a, twin.exact_range_search(q, radii), (rows, kth, "twin"))
            assert_same(a, erm.cut_full(full, radii), (rows, kth, "model"))
    finally:
        g.close()
        twin.close()


@pytest.mark.parametrize("metric,d", [("cosine", 100), ("cosine", 128), ("ip", 100), ("ip", 128)])
def test_cosine_and_ip_against_the_model(rq, oracle, metric, d):
    """The model runs on the index's STORED rows (normalised / augmented) and the transformed queries."""
    from tests import ip_model as im
    n, k, nq = 3001, 16, 40
    x, centres, _ = synth.mixture(n, d, k, sigma=0.4, seed=101 + d)
    q, _, _ = synth.mixture(nq, d, k, sigma=0.4, seed=102 + d)
    x *= np.random.default_rng(9).uniform(0.5, 2.0, (n, 1)).astype(np.float32)      # norms that matter to both metrics
    dim = im.ip_dim(d) if metric == "ip" else (d + 63) // 64 * 64
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(dim, seed=103), metric=metric)
    try:
        full = em.index_answer(oracle, g, q, n, metric=metric)
        for kth in (10, 200):
            radii = kth_radii(full, kth)
            got = g.exact_range_search(q, radii)
            assert_same(got, erm.cut_full(full, radii), (metric, d, kth))
            assert_same(got, erm.index_answer(oracle, g, q, radii, metric=metric), (metric, d, kth, "model"))
        if metric == "ip":
            ip = g.inner_product(full[0][:, :20], q)
            min_ip = ip[:, 15].copy()                                         # "inner product above the 16th best"
            r = g.ip_radius(q, min_ip)
            a, b = g.exact_range_search(q, min_ip=min_ip), g.exact_range_search(q, radius=r)
            assert_same(a, b, "min_ip = radius at ip_radius")
            assert_same(a, erm.cut_full(full, r), "min_ip, model")
            assert int(a[0][-1]) > 0
            with pytest.raises(rq.RabitqError):
                g.exact_range_search(q, radius=r, min_ip=min_ip)
    finally:
        g.close()


# ---- mutated indexes, shards ---------------------------------------------------------------------------------------------------
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
        radii = c.exact_search(q, 100)[0][:, 99].copy()
        for r in (radii, np.inf):
            (al, ad, ai), (bl, bd, bi) = g.exact_range_search(q, r), c.exact_range_search(q, r)
            assert_same((al, ad, ai), (bl, bd, ids[bi].astype(np.uint32)), "mutated")   # ids translated as tests/test_mutable_gpu.py does
        assert int(al[-1]) == 40 * (n - 700)
    finally:
        g.close()
        c.close()


def test_union_of_shards_is_the_whole_index(rq, world):
    c = world(128)
    nq = 40
    radii = kth_radii(c["full"], 200, nq)
    want = erm.cut_full(c["full"], radii, nq)
    owner = c["gidx"].partition_lists(2)[0]
    parts = []
    for rank in (0, 1):
        s = c["gidx"].shard(owner, rank)
        try:
            parts.append(s.exact_range_search(c["q"][:nq], radii))
            assert set(parts[-1][2].tolist()) <= set(s.map_ids.tolist())
        finally:
            s.close()
    united = []
    for b in range(nq):
        d_ = np.concatenate([p[1][int(p[0][b]):int(p[0][b + 1])] for p in parts])
        i_ = np.concatenate([p[2][int(p[0][b]):int(p[0][b + 1])] for p in parts])
        order = np.lexsort((i_, em.ord32(d_)))
        united.append((d_[order], i_[order]))
    assert_same(erm.pack(united), want, "shards")
    assert all(int(p[0][-1]) > 0 for p in parts)


# ---- entries and refusals ------------------------------------------------------------------------------------------------------
def test_device_entry_equals_host_entry(rq, world):
    import torch
    c = world(128)
    nq = 300
    radii = kth_radii(c["full"], 10, nq)
    qd, rd = torch.from_numpy(c["q"][:nq]).cuda(), torch.from_numpy(radii).cuda()
    torch.cuda.synchronize()
    with c["gidx"].exact_range_search_device(qd.data_ptr(), nq, qd.shape[1], rd.data_ptr()) as res:
        assert res.nq == nq and all(res.device_ptrs())
        got = res.to_host()
    assert_same(got, erm.cut_full(c["full"], radii, nq), "device")
    assert_same(got, c["gidx"].exact_range_search(c["q"][:nq], radii), "device vs host")


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
            g.exact_range_search(x[:4], 10.0)
        assert e.value.status == UNSUPPORTED
    finally:
        g.close()


def test_bad_arguments_are_refused(rq, world):
    from rabitq_amd import _lib
    c = world(64)
    g, q = c["gidx"], np.ascontiguousarray(c["q"][:4])
    L = _lib.lib()
    r = np.full(4, 5.0, np.float32)
    addr = lambda a: C.c_void_p(a.ctypes.data)

    def call(idx, qa, ra, prm=None, length=64, fn=L.rq_exact_range_search):
        h = C.c_void_p(0x1234)                                                # (a stale value: every refusal must clear it)
        s = fn(idx, None, qa, 4, length, ra, prm, C.byref(h))
        if s == 0:
            L.rq_range_result_free(h)
        else:
            assert h.value is None, s
        return s

    assert call(g._h, addr(q), addr(r)) == 0
    assert call(None, addr(q), addr(r)) == INVALID
    assert call(g._h, None, addr(r)) == INVALID
    assert call(g._h, addr(q), None) == INVALID
    assert call(g._h, None, addr(r), fn=L.rq_exact_range_search_device) == INVALID
    assert call(g._h, addr(q), None, fn=L.rq_exact_range_search_device) == INVALID
    assert L.rq_exact_range_search(g._h, None, addr(q), 4, 64, addr(r), None, None) == INVALID
    assert L.rq_exact_range_search_device(g._h, None, addr(q), 4, 64, addr(r), None, None) == INVALID
    assert call(g._h, addr(q), addr(r), length=65) == -2                      # 65 floats do not fit dim 64
    prm = _lib.ExactParamsT()
    prm.flags = 4
    assert call(g._h, addr(q), addr(r), C.byref(prm)) == INVALID              # an unknown flag bit
    prm = _lib.ExactParamsT()
    prm.struct_size = 0
    assert call(g._h, addr(q), addr(r), C.byref(prm)) == INVALID
    assert np.diff(g.exact_range_search(q[:, :63], np.inf)[0]).tolist() == [c["n"]] * 4   # 63 floats pad to 64: fine
    # dim > 4096: the entry refuses it through the checks it shares with every query entry (validate_call), but no such index can
    # exist -- every way of making one (here: the build) refuses the dimension first, so that is where the refusal is seen
    x = np.random.default_rng(1).standard_normal((64, 4100)).astype(np.float32)
    with pytest.raises(rq.RabitqError) as e:
        rq.RaBitQ.build(x, x[:2].copy(), np.eye(4160, dtype=np.float32))
    assert e.value.status == UNSUPPORTED


# ---- the approximate range search against the exact one ----------------------------------------------------------------------
def test_range_search_is_a_subset_and_range_recall(rq, world):
    c = world(100)                                                             # 64 lists
    g, q = c["gidx"], c["q"]
    radii = kth_radii(c["full"], 50)
    el, ed, ei = g.exact_range_search(q, radii)
    exact = [{int(i): F32(v).tobytes() for i, v in zip(ei[int(el[b]):int(el[b + 1])], ed[int(el[b]):int(el[b + 1])])} for b in range(len(q))]
    last = -1.0
    for probe in (1, 4, c["k"]):
        al, ad, ai = g.range_search(q, probe, radii)
        found = 0
        for b in range(len(q)):
            for i, v in zip(ai[int(al[b]):int(al[b + 1])], ad[int(al[b]):int(al[b + 1])]):
                assert exact[b].get(int(i)) == F32(v).tobytes(), (probe, b, int(i))     # the same row at the same distance bits
                found += 1
        recall = g.range_recall(q, probe, radii)
        assert recall == found / int(el[-1]) and recall >= last, (probe, recall, last)
        last = recall
    assert last > 0.0
    assert g.range_recall(q, 4, 0.0) == 1.0                                   # E is empty everywhere
    with g.make_filter(mask=np.arange(c["n"]) % 3 == 0) as f:
        fl, _, fi = g.exact_range_search(q, radii, filter=f)
        al, _, ai = g.range_search(q, 4, radii, filter=f)
        hit = sum(len(np.intersect1d(ai[int(al[b]):int(al[b + 1])], fi[int(fl[b]):int(fl[b + 1])])) for b in range(len(q)))
        assert g.range_recall(q, 4, radii, filter=f) == hit / int(fl[-1])


# ---- no side effects --------------------------------------------------------------------------------------------------------
def test_no_trace_in_later_calls(rq):
    """Rows of 1000 + N(0, 1) (nothing can be pruned: a first exact_search on a fresh index outgrows its default slots and re-runs).
    On a twin index an exact range call with a huge answer runs first: the exact search still re-runs exactly as often -- the capacity
    the range call learnt is not the exact search's --, the two answers and the range search's are the same, and rq_metrics does not
    move across the exact range call."""
    n, d, k, nq = 3001, 128, 16, 40
    rng = np.random.default_rng(51)
    centres = (1000.0 + 0.5 * rng.standard_normal((k, d))).astype(np.float32)
    x = (centres[rng.integers(0, k, n)] + rng.standard_normal((n, d))).astype(np.float32)
    q = (centres[rng.integers(0, k, nq)] + rng.standard_normal((nq, d))).astype(np.float32)
    P = synth.random_orthogonal(d, seed=52)
    a, b = rq.RaBitQ.build(x, centres, P), rq.RaBitQ.build(x, centres, P)
    try:
        ea = a.exact_search(q, 10)
        reruns_a = stats(rq)["reruns"]
        assert reruns_a >= 1
        ra = a.range_search(q, 4, 400.0)
        before = rq.metrics()
        lims, _, _ = b.exact_range_search(q, np.inf)
        assert rq.metrics() == before and int(lims[-1]) == nq * n
        lims2, _, _ = b.exact_range_search(q, np.inf)                         # (its own hint: the second call does not overflow)
        assert stats(rq)["reruns"] == 0 and np.array_equal(lims, lims2)
        eb = b.exact_search(q, 10)
        assert stats(rq)["reruns"] == reruns_a
        rb = b.range_search(q, 4, 400.0)
        for u, v in zip(ea + ra, eb + rb):
            assert np.array_equal(bits(u) if u.dtype == np.float32 else u, bits(v) if v.dtype == np.float32 else v)
        assert int(ra[0][-1]) > 0
    finally:
        a.close()
        b.close()
