"""In-place mutation (rq_add / rq_remove): after any sequence of adds and removes the index equals canonical(S), the index a fresh
build of its live rows S produces (rows in ascending id order, the same centroids and rotation) with every map_ids entry j
replaced by the j-th smallest id of S.  Every comparison is bit for bit: the arrays, rq_info, rq_dump_dir's files, and the
ids, distance bits, counts and counters of the query entry points.

Run on the GPU box:  python -m pytest tests/test_mutable_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import synth
from tests.models import ARRAYS, Live, bits, check_oracle, sub_arrays

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def canonical(rq, live, centres, P):
    """canonical(S): the build of S in ascending id order -> (index, ids_sorted); its map_ids entry j stands for ids_sorted[j]."""
    ids, rows = live.sorted()
    return rq.RaBitQ.build(rows, centres, P), ids


def assert_same_arrays(g, c, ids, what=""):
    assert (g.n, g.max_list_len, g.k, g.dim) == (c.n, c.max_list_len, c.k, c.dim), what
    for name in ARRAYS:
        assert np.array_equal(bits(getattr(g, name)), bits(getattr(c, name))), (what, name)
    assert np.array_equal(g.map_ids, ids[c.map_ids]), (what, "map_ids")


def run(rq, idx, queries, probe, topk, heur):
    rq.metrics_reset()
    out = idx.query_batch(queries, probe, topk, heur)
    m = rq.metrics()
    return out, (m["rough"], m["precise"], m["query"])


def assert_same_queries(rq, g, c, ids, queries, probes, topk=10, what=""):
    """query_batch (<= 64 queries: the small-batch path; more: the staged one) with both rankers, rq_query and the device entry."""
    for probe in probes:
        for heur in (False, True):
            for nq in (min(40, len(queries)), len(queries)):
                (a, ma), (b, mb) = run(rq, g, queries[:nq], probe, topk, heur), run(rq, c, queries[:nq], probe, topk, heur)
                assert np.array_equal(a[2], b[2]), (what, probe, heur, nq, "counts")
                for qi in range(nq):
                    n = int(a[2][qi])
                    assert np.array_equal(a[1][qi, :n], ids[b[1][qi, :n]]), (what, probe, heur, nq, qi)
                    assert np.array_equal(bits(a[0][qi, :n]), bits(b[0][qi, :n])), (what, probe, heur, nq, qi)
                assert ma == mb, (what, probe, heur, nq, ma, mb)
    q = queries[0]
    ra, rb = g.query(q, probes[-1], topk), c.query(q, probes[-1], topk)
    assert [(np.float32(d).tobytes(), i) for d, i in ra] == [(np.float32(d).tobytes(), int(ids[i])) for d, i in rb], what
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).cuda()
    nq, L = qd.shape
    res = []
    for idx in (g, c):
        od = torch.empty((nq, topk), device="cuda", dtype=torch.float32)
        oi = torch.empty((nq, topk), device="cuda", dtype=torch.int32)
        on = torch.empty((nq,), device="cuda", dtype=torch.int32)
        idx.query_batch_device(qd.data_ptr(), nq, L, probes[-1], topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        torch.cuda.synchronize()
        res.append((od.cpu().numpy(), oi.cpu().numpy().view(np.uint32), on.cpu().numpy()))
    (da, ia, na), (db, ib, nb) = res
    assert np.array_equal(na, nb), what
    for qi in range(nq):
        n = int(na[qi])
        assert np.array_equal(ia[qi, :n], ids[ib[qi, :n]]) and np.array_equal(bits(da[qi, :n]), bits(db[qi, :n])), (what, qi)


def check(rq, g, live, centres, P, queries, probes, what=""):
    c, ids = canonical(rq, live, centres, P)
    try:
        assert_same_arrays(g, c, ids, what)
        if c.n:
            assert_same_queries(rq, g, c, ids, queries, probes, what=what)
    finally:
        c.close()


@pytest.mark.parametrize("d,k", [(64, 16), (100, 64), (128, 16), (128, 1024), (768, 64)])
def test_add_equals_rebuild(rq, d, k):
    """Build on x[:n0], then add the rest in uneven chunks (0 rows, 1 row, thousands); after every add the index is the rebuild."""
    n = 6000 if d <= 128 and k < 1024 else (20000 if k == 1024 else 3000)
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=d + k, centre_scale=0.6)
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=d + 3)
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=d + 5, centre_scale=0.6)
    n0 = n // 2
    g = rq.RaBitQ.build(x[:n0], centres, P)
    live = Live(np.arange(n0), x[:n0])
    at = n0
    for step, m in enumerate((0, 1, n // 3, n - n0 - 1 - n // 3)):
        got = g.add(x[at:at + m])
        assert got.dtype == np.uint32 and np.array_equal(got, np.arange(at, at + m, dtype=np.uint32))
        live.add(got, x[at:at + m])
        at += m
        if m == 0 and step == 0:
            c, ids = canonical(rq, live, centres, P)
            assert_same_arrays(g, c, ids, "empty add")
            c.close()
            continue
        check(rq, g, live, centres, P, queries, (1, 8, k) if step == 3 else (k,), (d, k, step))
    g.close()


def test_keys_and_ties(rq, oracle):
    """The identity rotation makes distances exact: rows equidistant to two centroids (the lower list wins), duplicates of stored
    rows (the lower id goes first), NaN / inf rows (list 0, key f32::MAX), rows for lists that were empty, and one list grown past
    the 8192 keys the LDS sort holds."""
    d, k = 128, 16
    rng = np.random.default_rng(5)
    centres = np.zeros((k, d), np.float32)
    for c in range(k):
        centres[c, c % d] = 4.0 if c % 2 == 0 else -4.0
        centres[c, (c // 2) + 32] = 1.0
    P = np.eye(d, dtype=np.float32)
    u = rng.integers(0, k // 2, size=3000)          # only the first half of the lists gets rows at build time
    x0 = (centres[u] + 0.5 * rng.standard_normal((3000, d))).astype(np.float32)
    g = rq.RaBitQ.build(x0, centres, P)
    live = Live(np.arange(3000), x0)
    assert (np.diff(g.offsets.astype(np.int64))[k // 2:] == 0).all()
    tie = ((centres[0] + centres[1]) / 2).astype(np.float32)           # equidistant to lists 0 and 1
    tie2 = ((centres[4] + centres[5]) / 2 + 0.25 * np.eye(d, dtype=np.float32)[100]).astype(np.float32)
    dup = x0[[5, 17, 17, 2999]]
    bad = np.stack([np.full(d, np.nan, np.float32), np.full(d, np.inf, np.float32)])
    empty = (centres[[9, 11, 15]] + 0.3 * rng.standard_normal((3, d))).astype(np.float32)
    big = (centres[3] + 0.5 * rng.standard_normal((9000, d))).astype(np.float32)   # list 3 grows past 8192
    new = np.concatenate([tie[None], tie[None], tie2[None], dup, bad, empty, big]).astype(np.float32)
    got = g.add(new)
    live.add(got, new)
    offs = g.offsets.astype(np.int64)
    assert offs[4] - offs[3] > 8192
    assert all(offs[c + 1] > offs[c] for c in (9, 11, 15))
    c, ids = canonical(rq, live, centres, P)
    assert_same_arrays(g, c, ids, "ties")
    c.close()
    check_oracle(oracle, g, live, centres, P, "ties")
    # explicit ids that interleave with the stored ones: the tie-break on id reaches into the middle of the old rows
    rows = np.concatenate([x0[[5, 6]], tie[None]]).astype(np.float32)
    g.remove(ids=[3, 4])
    live.remove([3, 4])
    g.add(rows, ids=np.array([4, 3, 1 << 20]))
    live.add([4, 3, 1 << 20], rows)
    queries = (centres[rng.integers(0, k, 64)] + 0.5 * rng.standard_normal((64, d))).astype(np.float32)
    check(rq, g, live, centres, P, queries, (2, k), "explicit ids")
    # ties across the two sides of the merge, explicit ids on both sides of the stored twin's: the copy of stored row 5 under id 4
    # sits right before its twin, the copy of stored row 7 under a larger id right after it
    g.add(x0[[7]], ids=np.array([(1 << 20) + 1]))
    live.add([(1 << 20) + 1], x0[[7]])
    where = {int(i): p for p, i in enumerate(g.map_ids)}
    assert where[4] + 1 == where[5] and where[3] + 1 == where[6] and where[7] + 1 == where[(1 << 20) + 1]
    check(rq, g, live, centres, P, queries, (k,), "explicit ids, twin above")
    g.close()


def same_as_rebuild(rq, g, live, centres, P, queries, what):
    """offsets, map_ids, codes, factors, base and one query batch of g against the build of its live rows, bit for bit."""
    c, ids = canonical(rq, live, centres, P)
    try:
        assert_same_arrays(g, c, ids, what)
        (a, ma), (b, mb) = run(rq, g, queries, g.k, 10, False), run(rq, c, queries, g.k, 10, False)
        assert np.array_equal(a[2], b[2]), (what, "counts")
        for qi in range(len(queries)):
            n = int(a[2][qi])
            assert np.array_equal(a[1][qi, :n], ids[b[1][qi, :n]]) and np.array_equal(bits(a[0][qi, :n]), bits(b[0][qi, :n])), (what, qi)
        assert ma == mb, (what, ma, mb)
    finally:
        c.close()


@pytest.mark.parametrize("d", [64, 128, 192, 300, 4096])
def test_add_remove_compact_through_every_gather_shape(rq, d):
    """rq_add, rq_remove and rq_remove_lazy + rq_compact through the gather's sub-groups of 16, 32 and 64 lanes (48 of them used at
    dim 192), rows longer than one wave's step (dim 320, from d = 300: padded rows), and the largest dim; no output row count is
    a multiple of 16, the most rows a wave moves per step.  The stored ids are the even numbers, the added ids odd ones given in
    shuffled order, so the two sides interleave in every list."""
    dim, k = (d + 63) // 64 * 64, 8
    n0, m = (301, 101) if dim == 4096 else (1501, 401)
    x, centres, _ = synth.mixture(n0 + m, d, k, sigma=0.8, seed=d + 7, centre_scale=0.6)
    P = synth.random_orthogonal(dim, seed=d + 1) if dim <= 320 else np.eye(dim, dtype=np.float32)[::-1].copy()
    queries, _, _ = synth.mixture(48, d, k, sigma=0.8, seed=d + 9, centre_scale=0.6)
    rng = np.random.default_rng(d)
    b = rq.RaBitQ.build(x[:n0], centres, P)
    stored = (2 * np.arange(n0)).astype(np.uint32)                      # (a monotone renaming: every list keeps the build's order)
    g = rq.RaBitQ.from_arrays(b.base, b.orthogonal, b.centroids, b.offsets, stored[b.map_ids], b.codes, b.factors)
    b.close()
    live = Live(stored, x[:n0])
    new_ids = (2 * rng.choice(n0 + 50, m, replace=False) + 1).astype(np.uint32)    # odd ids in no order, a few past every stored id
    assert np.array_equal(g.add(x[n0:], ids=new_ids), new_ids)
    live.add(new_ids, x[n0:])
    same_as_rebuild(rq, g, live, centres, P, queries, (d, "add"))
    gone = np.array(sorted(live.rows), dtype=np.uint32)[::3]                       # a scattered third, of both sides
    assert g.remove(ids=gone) == gone.size
    live.remove(gone)
    same_as_rebuild(rq, g, live, centres, P, queries, (d, "remove"))
    dead = np.array(sorted(live.rows), dtype=np.uint32)[[0, 7, 100, 101, -1]]
    assert g.remove(ids=dead, lazy=True) == dead.size and g.compact() == dead.size
    live.remove(dead)
    same_as_rebuild(rq, g, live, centres, P, queries, (d, "compact"))
    assert g.n == n0 + m - gone.size - dead.size
    assert all(rows % 16 for rows in (n0 + m, n0 + m - gone.size, g.n))
    g.close()


@pytest.mark.parametrize("d,k", [(128, 64), (64, 1024)])
def test_remove_equals_sub_index(rq, d, k):
    """Remove a random 30 %, then one whole list, then everything: the arrays are rq_from_arrays of the kept rows in stored order,
    the queries those of the filtered query with the complement allow-list on the original index (and canonical(S))."""
    n = 6000 if k < 1024 else 15000
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=11, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=13)
    queries, _, _ = synth.mixture(200, d, k, sigma=0.8, seed=17, centre_scale=0.6)
    orig = rq.RaBitQ.build(x, centres, P)
    g = rq.RaBitQ.build(x, centres, P)
    rng = np.random.default_rng(3)
    alive = np.ones(n, dtype=bool)
    offs, mids = orig.offsets.astype(np.int64), orig.map_ids
    biggest = int(np.argmax(np.diff(offs)))
    steps = [("random", np.nonzero(rng.random(n) < 0.3)[0]), ("list", mids[offs[biggest]:offs[biggest + 1]]),
             ("all", np.arange(n))]
    for name, ids in steps:
        before = int(alive.sum())
        removed = g.remove(ids=ids)
        assert removed == before - int((alive & ~np.isin(np.arange(n), ids)).sum()), name
        alive[ids] = False
        sub = rq.RaBitQ.from_arrays(*sub_arrays(orig, alive))
        assert_same_arrays(g, sub, np.arange(n, dtype=np.uint32), name)
        if alive.any():
            with orig.make_filter(mask=alive) as f:
                for probe, heur in ((4, False), (k, False), (k, True)):
                    rq.metrics_reset()
                    a = g.query_batch(queries, probe, 10, heur)
                    ma = rq.metrics()
                    rq.metrics_reset()
                    b = orig.query_batch(queries, probe, 10, heur, filter=f)
                    mb = rq.metrics()
                    for u, v in zip(a, b):
                        assert np.array_equal(bits(u), bits(v)), (name, probe, heur)
                    assert ma == mb, (name, ma, mb)
            live = Live(np.nonzero(alive)[0], x[alive])
            check(rq, g, live, centres, P, queries[:64], (k,), name)
        sub.close()
    assert g.n == 0 and g.remove(ids=[0, 1]) == 0
    g.close()
    orig.close()


def test_random_sequence(rq, oracle):
    """Eight seeded operations -- default-id adds, explicit-id adds (ids a remove freed among them), removes and updates --
    each followed by the comparison with canonical(S)."""
    d, k = 96, 32
    rng = np.random.default_rng(2024)
    pool, centres, _ = synth.mixture(20000, d, k, sigma=0.7, seed=21, centre_scale=0.6)
    P = synth.random_orthogonal(128, seed=22)
    queries, _, _ = synth.mixture(100, d, k, sigma=0.7, seed=23, centre_scale=0.6)
    g = rq.RaBitQ.build(pool[:4000], centres, P)
    live = Live(np.arange(4000), pool[:4000])
    nxt = 4000
    freed = []
    ops = ["add", "remove", "add_ids", "update", "remove", "add", "update", "add_ids"]
    for step, op in enumerate(ops):
        cur = np.array(sorted(live.rows), dtype=np.int64)
        m = int(rng.integers(1, 1500))
        rows = pool[nxt:nxt + m]
        nxt += m
        if op == "add":
            got = g.add(rows)
            assert got[0] == cur.max() + 1
            live.add(got, rows)
        elif op == "add_ids":
            ids = np.array(freed[:m // 2] + list(int(cur.max()) + 10 + 3 * np.arange(m - min(m // 2, len(freed)))), dtype=np.uint32)
            ids = rng.permutation(ids)[:m]
            rows = rows[:ids.size]
            freed = freed[m // 2:]
            got = g.add(rows, ids=ids)
            assert np.array_equal(got, ids)
            live.add(ids, rows)
        elif op == "remove":
            ids = rng.choice(cur, size=min(cur.size, m), replace=False)
            ids = np.concatenate([ids, [cur.max() + 100]])            # one id the index does not hold: ignored
            assert g.remove(ids=ids) == ids.size - 1
            live.remove(ids)
            freed += [int(i) for i in ids[:-1]]
        else:
            ids = rng.choice(cur, size=min(cur.size, m), replace=False)
            g.update(ids, rows[:ids.size])
            live.remove(ids)
            live.add(ids, rows[:ids.size])
        check(rq, g, live, centres, P, queries, (3, k), (step, op))
        check_oracle(oracle, g, live, centres, P, (step, op))
        st = rq.index.last_mutate_stats()
        assert st["rows_after"] == g.n and st["ms_total"] > 0 and st["gather_bytes"] > 0, st
        assert (st["ms_keys"] > 0) == (step == 0), (step, st)   # the key cache is derived once, on the first mutation
    g.close()


def test_refusals_leave_the_index_unchanged(rq):
    from rabitq_amd import _lib
    L = _lib.lib()
    d, k = 128, 16
    x, centres, _ = synth.mixture(3000, d, k, sigma=0.8, seed=31, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=32)
    queries, _, _ = synth.mixture(50, d, k, sigma=0.8, seed=33, centre_scale=0.6)
    g = rq.RaBitQ.build(x[:2000], centres, P)

    def snap():
        return [bits(getattr(g, a)).copy() for a in ARRAYS + ("map_ids",)] + [bits(np.array([g.n, g.max_list_len]))]

    def unchanged(before, what):
        for u, v in zip(before, snap()):
            assert np.array_equal(u, v), what

    def add_raw(rows, ids=None, dd=None):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
        first = C.c_uint32()
        return L.rq_add(g._h, rows.ctypes.data, rows.shape[0], dd or rows.shape[1], None if idv is None else idv.ctypes.data, 0,
                        C.byref(first))

    before = snap()
    assert add_raw(x[2000:2003], ids=[5000, 5001, 5000]) == -1          # repeated in the batch
    unchanged(before, "dup")
    assert add_raw(x[2000:2003], ids=[5000, 17, 5001]) == -1            # 17 is stored
    unchanged(before, "present")
    assert add_raw(x[2000:2003], dd=64) == -2                           # 64 does not pad to 128
    unchanged(before, "dim")
    with g.make_filter(ids=np.arange(0, 2000, 2)) as stale:
        g.add(x[2000:2001], ids=[0xFFFFFFF0])
        before = snap()
        assert add_raw(x[2001:2101]) == -6                              # the next ids would pass 2^32 - 1
        unchanged(before, "id space")
        st = L.rq_query_batch_filtered(g._h, stale._h, queries.ctypes.data, 5, d, 4, 10, 0,
                                       np.empty((5, 10), np.float32).ctypes.data, np.empty((5, 10), np.uint32).ctypes.data,
                                       np.empty(5, np.uint32).ctypes.data)
        assert st == -1                                                 # made before the add
    with g.make_filter(ids=np.arange(0, 2000, 2)) as fresh:
        live = Live(np.arange(2000), x[:2000])
        live.add([0xFFFFFFF0], x[2000:2001])
        c, ids = canonical(rq, live, centres, P)
        allow = np.zeros(c.n, dtype=bool)
        allow[np.nonzero(ids < 2000)[0][::2]] = True                   # canonical's ids of the even original ids
        with c.make_filter(mask=allow) as cf:
            a, b = g.query_batch(queries, 4, 10, filter=fresh), c.query_batch(queries, 4, 10, filter=cf)
            assert np.array_equal(a[2], b[2])
            for qi in range(len(queries)):
                n = int(a[2][qi])
                assert np.array_equal(a[1][qi, :n], ids[b[1][qi, :n]]) and np.array_equal(bits(a[0][qi, :n]), bits(b[0][qi, :n]))
        c.close()
    # a pending _begin ticket
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(np.tile(queries, (2000 // 50, 1)))).cuda()
    nq = qd.shape[0]
    od = torch.empty((nq, 10), device="cuda", dtype=torch.float32)
    oi = torch.empty((nq, 10), device="cuda", dtype=torch.int32)
    on = torch.empty((nq,), device="cuda", dtype=torch.int32)
    before = snap()
    t = g.query_batch_device_begin(qd.data_ptr(), nq, d, 4, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr())
    assert add_raw(x[2001:2002]) == -1
    words, nb = rq.pack_filter_bits(ids=[1, 2])
    removed = C.c_uint64()
    assert L.rq_remove(g._h, words.ctypes.data, nb, 0, C.byref(removed)) == -1
    g.query_batch_device_end(t)
    unchanged(before, "ticket")
    assert g.remove(ids=[1, 2]) == 2
    # a shard and a tiered index
    owner = np.zeros(k, dtype=np.uint32)
    owner[k // 2:] = 1
    sh = g.shard(owner, 0)
    shb = [bits(sh.map_ids).copy(), bits(sh.codes).copy()]
    first = C.c_uint32()
    row = np.ascontiguousarray(x[2500:2501])
    assert L.rq_add(sh._h, row.ctypes.data, 1, d, None, 0, C.byref(first)) == -6
    assert L.rq_remove(sh._h, words.ctypes.data, nb, 0, C.byref(removed)) == -6
    assert np.array_equal(shb[0], bits(sh.map_ids)) and np.array_equal(shb[1], bits(sh.codes))
    sh.close()
    cd = torch.from_numpy(centres).cuda()
    xd = torch.from_numpy(x[:2000]).cuda()
    b = rq.RaBitQ.builder(2000, d, cd.data_ptr(), k, orthogonal=P, max_device_base_bytes=200 * d * 4)
    b.assign_chunk(xd.data_ptr(), 0, 2000)
    b.order()
    b.place_chunk(xd.data_ptr(), 0, 2000)
    tiered = b.finish()
    assert tiered.n_hbm < tiered.n
    tb = bits(tiered.map_ids).copy()
    assert L.rq_add(tiered._h, row.ctypes.data, 1, d, None, 0, C.byref(first)) == -6
    assert L.rq_remove(tiered._h, words.ctypes.data, nb, 0, C.byref(removed)) == -6
    assert np.array_equal(tb, bits(tiered.map_ids)) and tiered.n == 2000
    tiered.close()
    g.close()


def test_dump_and_reload(rq, tmp_path):
    """dump_to_dir of a mutated index is byte-identical to the dump of canonical(S); loaded again (its key cache is recomputed)
    it keeps equalling canonical(S) through further adds and removes."""
    d, k = 100, 24
    x, centres, _ = synth.mixture(5000, d, k, sigma=0.8, seed=41, centre_scale=0.6)
    P = synth.random_orthogonal(128, seed=42)
    queries, _, _ = synth.mixture(80, d, k, sigma=0.8, seed=43, centre_scale=0.6)
    g = rq.RaBitQ.build(x[:3000], centres, P)
    live = Live(np.arange(3000), x[:3000])
    g.remove(ids=np.arange(0, 3000, 7))
    live.remove(np.arange(0, 3000, 7))
    got = g.add(x[3000:4000])
    live.add(got, x[3000:4000])
    c, ids = canonical(rq, live, centres, P)
    ct = rq.RaBitQ.from_arrays(c.base, c.orthogonal, c.centroids, c.offsets, ids[c.map_ids], c.codes, c.factors)
    g.dump_to_dir(tmp_path / "mut")
    ct.dump_to_dir(tmp_path / "canon")
    names = sorted(os.listdir(tmp_path / "canon"))
    assert names == sorted(os.listdir(tmp_path / "mut"))
    for name in names:
        assert (tmp_path / "mut" / name).read_bytes() == (tmp_path / "canon" / name).read_bytes(), name
    c.close()
    ct.close()
    g.close()
    h = rq.RaBitQ.load_from_dir(tmp_path / "mut")
    got = h.add(x[4000:5000])
    live.add(got, x[4000:5000])
    check(rq, h, live, centres, P, queries, (k,), "reloaded add")
    h.remove(ids=got[::3])
    live.remove(got[::3])
    check(rq, h, live, centres, P, queries, (4,), "reloaded remove")
    h.close()


def test_scale_2m(rq):
    """2M x 128, k = 1024: build 1.9M rows, add 100k, remove 50k; 4096 queries against canonical(S) with the matrix-core scan and
    the 8-bit shadow rows engaged."""
    import torch
    from rabitq_amd import index as ix
    n, d, k = 2_000_000, 128, 1024
    x, cd = synth.device_mixture(n, d, k, 0.9, "cuda", centre_scale=1.0)
    P = synth.random_orthogonal(d, seed=51)
    g = rq.RaBitQ.build_device(x.data_ptr(), 1_900_000, d, cd.data_ptr(), k, orthogonal=P)
    first = g.add_device(x[1_900_000:].data_ptr(), 100_000, d)
    assert first == 1_900_000 and g.n == n
    gone = torch.from_numpy(np.random.default_rng(52).choice(n, 50_000, replace=False)).cuda()
    alive = torch.ones(n, dtype=torch.bool, device="cuda")
    alive[gone] = False
    assert g.remove(ids=gone.cpu().numpy()) == 50_000
    keep = torch.nonzero(alive).flatten()
    xs = x[keep].contiguous()
    c = rq.RaBitQ.build_device(xs.data_ptr(), xs.shape[0], d, cd.data_ptr(), k, orthogonal=P)
    ids = keep.cpu().numpy().astype(np.uint32)
    del xs, x
    torch.cuda.empty_cache()
    assert_same_arrays(g, c, ids, "scale")
    q = synth.device_queries(cd, 4096, 0.9, "cuda", seed=53).cpu().numpy()
    ix.set_profiling(1)
    try:
        for probe in (16, 64):
            (a, ma), (b, mb) = run(rq, g, q, probe, 10, False), run(rq, c, q, probe, 10, False)
            pr = ix.last_profile()
            assert pr["matrix_launches"] > 0 and pr["rerank_shadow_rejects"] > 0, pr
            assert np.array_equal(a[2], b[2]) and ma == mb
            assert np.array_equal(bits(a[0]), bits(b[0]))
            for qi in range(len(q)):
                nn = int(a[2][qi])
                assert np.array_equal(a[1][qi, :nn], ids[b[1][qi, :nn]]), qi
    finally:
        ix.set_profiling(0)
    g.close()
    c.close()


def test_remapped_ids_and_out_of_order_lists(rq):
    """rq_from_arrays of a built index with map_ids remapped to other ids (database keys): with no tied distances every list is
    still in the build's order, so adds work and equal canonical(S) under the new ids.  Two rows of a list swapped make the list
    out of order: rq_add refuses it (RQ_ERR_UNSUPPORTED, index untouched) instead of merging by an order the list does not have;
    rq_remove keeps the lists' order and still equals the sub-index."""
    from rabitq_amd import _lib
    d, k = 128, 16
    x, centres, _ = synth.mixture(3500, d, k, sigma=0.8, seed=61, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=62)
    queries, _, _ = synth.mixture(50, d, k, sigma=0.8, seed=64, centre_scale=0.6)
    b = rq.RaBitQ.build(x[:3000], centres, P)
    perm = np.random.default_rng(63).permutation(1 << 20)[:3000].astype(np.uint32)   # database keys, not build order
    arrs = [b.base, b.orthogonal, b.centroids, b.offsets, perm[b.map_ids], b.codes, b.factors]
    g = rq.RaBitQ.from_arrays(*arrs)
    live = Live(perm, x[:3000])
    new_ids = np.arange(1 << 20, (1 << 20) + 500)
    g.add(x[3000:], ids=new_ids)
    live.add(new_ids, x[3000:])
    check(rq, g, live, centres, P, queries, (4, k), "remapped ids")
    g.close()

    offs = b.offsets.astype(np.int64)
    c = int(np.argmax(np.diff(offs)))
    order = np.arange(3000)
    order[offs[c]], order[offs[c] + 1] = offs[c] + 1, offs[c]                      # swap the first two rows of a list
    arrs = [a[order] if i in (0, 4, 5, 6) else a for i, a in enumerate(arrs)]
    g = rq.RaBitQ.from_arrays(*arrs)
    before = [bits(getattr(g, a)).copy() for a in ARRAYS + ("map_ids",)]
    with pytest.raises(_lib.RabitqError) as e:
        g.add(x[3000:3005], ids=np.array([(1 << 20) + i for i in range(5)]))
    assert e.value.status == -6
    with pytest.raises(_lib.RabitqError) as e:
        g.add(x[3000:3005])
    assert e.value.status == -6
    for u, a in zip(before, ARRAYS + ("map_ids",)):
        assert np.array_equal(u, bits(getattr(g, a))), a
    gone = perm[::4]
    assert g.remove(ids=gone) == gone.size
    keep = ~np.isin(arrs[4], gone)
    lists = np.repeat(np.arange(k), np.diff(offs))
    new_off = np.zeros(k + 1, dtype=np.uint32)
    new_off[1:] = np.cumsum(np.bincount(lists[keep], minlength=k))
    sub = rq.RaBitQ.from_arrays(arrs[0][keep], arrs[1], arrs[2], new_off, arrs[4][keep], arrs[5][keep], arrs[6][keep])
    assert_same_arrays(g, sub, np.arange(1 << 20, dtype=np.uint32), "out-of-order remove")
    sub.close()
    # ... and so do rq_remove_lazy + rq_compact (the keep branch of the merge reads no keys); rq_add is refused as before
    dead = perm[1::8]
    assert g.remove(ids=dead, lazy=True) == dead.size and g.compact() == dead.size
    keep &= ~np.isin(arrs[4], dead)
    new_off[1:] = np.cumsum(np.bincount(lists[keep], minlength=k))
    sub = rq.RaBitQ.from_arrays(arrs[0][keep], arrs[1], arrs[2], new_off, arrs[4][keep], arrs[5][keep], arrs[6][keep])
    assert_same_arrays(g, sub, np.arange(1 << 20, dtype=np.uint32), "out-of-order compact")
    a, c2 = g.query_batch(queries, k, 10), sub.query_batch(queries, k, 10)
    for u, v in zip(a, c2):
        assert np.array_equal(bits(u), bits(v)), "out-of-order compact: queries"
    sub.close()
    with pytest.raises(_lib.RabitqError) as e:
        g.add(x[3000:3005])
    assert e.value.status == -6 and "not in the build's order" in str(e.value)
    g.close()
    b.close()


def test_add_to_an_emptied_index(rq):
    """Remove every row (no row left to gather), then add (side A of the merge has no rows: every row comes from the batch): the
    first default id is 0 again, and the index is canonical(S) of the new rows.  Then empty one list and add a batch that gives that
    list all of its rows and another list none."""
    d, k = 64, 12
    x, centres, _ = synth.mixture(2000, d, k, sigma=0.8, seed=71, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=72)
    queries, _, _ = synth.mixture(50, d, k, sigma=0.8, seed=73, centre_scale=0.6)
    g = rq.RaBitQ.build(x[:1000], centres, P)
    label0 = np.empty(1000, dtype=np.int64)                  # the list of each of the first 1000 rows
    label0[g.map_ids] = np.repeat(np.arange(k), np.diff(g.offsets.astype(np.int64)))
    assert g.remove(ids=np.arange(1000)) == 1000 and g.n == 0
    assert not g.offsets.any() and g.map_ids.size == 0 and g.codes.size == 0 and g.base.size == 0
    got = g.add(x[1000:])
    assert np.array_equal(got, np.arange(1000, dtype=np.uint32))
    live = Live(got, x[1000:])
    check(rq, g, live, centres, P, queries, (3, k), "emptied then added")
    offs = g.offsets.astype(np.int64)
    filled, skipped = 5, 9
    gone = g.map_ids[offs[filled]:offs[filled + 1]].copy()
    assert gone.size and g.remove(ids=gone) == gone.size
    live.remove(gone)
    offs = g.offsets.astype(np.int64)
    assert offs[filled + 1] == offs[filled]
    batch = x[:1000][label0 != skipped]                      # rows for every list but one, the emptied list among them
    in_filled = int((label0 == filled).sum())
    assert in_filled and (label0 == skipped).any()
    got = g.add(batch)
    live.add(got, batch)
    after = g.offsets.astype(np.int64)
    assert after[filled + 1] - after[filled] == in_filled and after[skipped + 1] - after[skipped] == offs[skipped + 1] - offs[skipped] > 0
    check(rq, g, live, centres, P, queries, (3, k), "one list filled by the batch alone, one list without a new row")
    g.close()


def test_mutate_an_index_in_the_reference_dump_format(rq, oracle, tmp_path):
    """An index the CPU oracle wrote in the reference's directory format (rq_load_dir), then added to and removed from."""
    d, k = 128, 16
    x, centres, _ = synth.mixture(4000, d, k, sigma=0.8, seed=81, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=82)
    queries, _, _ = synth.mixture(60, d, k, sigma=0.8, seed=83, centre_scale=0.6)
    o = oracle.OracleIndex.build(x[:2500], centres, P)
    o.dump_to_dir(str(tmp_path / "ref"))
    o.close()
    g = rq.RaBitQ.load_from_dir(tmp_path / "ref")
    live = Live(np.arange(2500), x[:2500])
    got = g.add(x[2500:])
    live.add(got, x[2500:])
    check(rq, g, live, centres, P, queries, (4, k), "reference dump + add")
    check_oracle(oracle, g, live, centres, P, "reference dump + add")
    g.remove(ids=np.arange(0, 4000, 3))
    live.remove(np.arange(0, 4000, 3))
    check(rq, g, live, centres, P, queries, (4,), "reference dump + remove")
    g.close()
