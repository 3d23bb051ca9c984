"""The complete exact grouped search on the GPU: rq_exact_search_grouped_full* bit for bit against tests/group_model.py's
selection applied to the index's own COMPLETE sorted row list (exact_range_search at an infinite radius) with the keys the column
held when the postings were made, and once against plain f64 numpy on integer data whose squared distances are exact in f32.

Run on the GPU box:  python -m pytest tests/test_group_full_gpu.py -m gpu -q
"""
import os

import numpy as np
import pytest

from tests import byte_model as bm
from tests import group_model as gm
from tests import half_model as hm
from tests import synth

pytestmark = pytest.mark.gpu

N, NQ = 5003, 70                       # not a multiple of 32; several scan blocks
INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def build(rq, d, seed, n=N, **kw):
    """n rows of a mixture, the first 200 in twin pairs (equal rows: equal distances to every query), and NQ queries."""
    x, centres, _ = synth.mixture(n, d, 8, sigma=0.6, seed=seed, centre_scale=0.8)
    x[1:200:2] = x[0:200:2]
    q, _, _ = synth.mixture(NQ, d, 8, sigma=0.6, seed=seed + 1, centre_scale=0.8)
    return rq.RaBitQ.build(x, centres, synth.random_orthogonal((d + 63) // 64 * 64, seed=seed + 2), **kw), q


def complete_rows(g, q, filter=None):
    """Every row of every query as (dist, ids, cnt), ascending: the source arrays of the model."""
    lims, dist, ids = g.exact_range_search(q, np.inf, filter=filter)
    cnt = np.diff(lims).astype(np.uint32)
    d = np.zeros((q.shape[0], max(int(cnt.max()), 1)), dtype=np.float32)
    i = np.zeros(d.shape, dtype=np.uint32)
    for b in range(q.shape[0]):
        d[b, :cnt[b]], i[b, :cnt[b]] = dist[lims[b]:lims[b + 1]], ids[lims[b]:lims[b + 1]]
    return d, i, cnt


def same(res, want):
    assert res.complete
    return (np.array_equal(res.dist.view(np.uint32), want["dist_bits"]) and np.array_equal(res.ids, want["ids"])
            and np.array_equal(gm.key_image(res.keys), want["keys"]) and np.array_equal(res.group_counts, want["group_n"])
            and np.array_equal(res.counts, want["n"]))


def snapshot(g, column):
    """{id: key image} of the live rows now: what postings made now hold."""
    return gm.keymap_of(g.map_ids, g.attr_array(column), g.contains(g.map_ids) if g.pending_removals else None)


@pytest.fixture(scope="module")
def world(rq):
    """The 5 003-row index at dim 64: `doc` (about 3 rows per key), `few` (4 keys), `wide` (u64 keys that differ in the high word
    only), `dense` (one key owns the nearest 3 000 rows of query 0), their postings and key maps, and the complete rows of the queries."""
    g, q = build(rq, 64, 700)
    ids, rng = np.arange(N, dtype=np.uint32), np.random.default_rng(5)
    rows = complete_rows(g, q)
    dense = 1000 + np.arange(N, dtype=np.uint32)
    dense[rows[1][0, :3000]] = 7
    cols = {"doc": ("u32", rng.integers(0, N // 3, size=N)), "few": ("i32", rng.integers(-2, 2, size=N)),
            "wide": ("u64", (rng.integers(0, 50, size=N).astype(np.uint64) << np.uint64(32)) | np.uint64(5)), "dense": ("u32", dense)}
    w = dict(g=g, q=q, rows=rows, post={}, keymap={})
    for name, (dtype, vals) in cols.items():
        g.create_attr(name, dtype, fill=0)
        g.set_attr(name, ids, vals)
        w["post"][name], w["keymap"][name] = g.postings(name), snapshot(g, name)
    yield w
    for p in w["post"].values():
        p.close()
    g.close()


def expect(w, column, nq, topk, gs):
    d, i, cnt = w["rows"]
    return gm.group_rows(d[:nq], i[:nq], cnt[:nq], w["keymap"][column], topk, gs)


@pytest.mark.parametrize("nq", [1, 33, 70])
@pytest.mark.parametrize("topk,gs", [(1, 1), (10, 3), (100, 1), (64, 32)])
def test_shapes_bit_for_bit(world, topk, gs, nq):
    """About 3 rows per key, twin rows in different groups; (64, 32) fills the 2048 slots and leaves most groups short."""
    res = world["g"].exact_search_grouped(world["q"][:nq], topk, world["post"]["doc"], group_size=gs)
    assert same(res, expect(world, "doc", nq, topk, gs))
    st = world["g"].last_group_full_stats()
    assert st["hits"] == int(res.fetched.sum()) <= st["records"] and st["plan_queries"] == (nq * topk if gs > 1 else 0)


@pytest.mark.parametrize("column,topk,gs", [("few", 10, 3), ("wide", 10, 2), ("wide", 60, 1), ("doc", 300, 1), ("doc", 2048, 1)])
def test_fewer_groups_than_asked_and_wide_keys(world, column, topk, gs):
    """`few`: 4 groups exist, 10 are asked for: no bound, every row is a hit and the selection runs several chunks.  `wide`: 50 keys
    equal in their low word (topk 60: again fewer than asked).  `doc` at topk 300 and 2048: the selection's 48 KB shape (topk > 256),
    with a bound and -- 1 667 groups exist -- without one."""
    res = world["g"].exact_search_grouped(world["q"][:33], topk, world["post"][column], group_size=gs)
    assert same(res, expect(world, column, 33, topk, gs))
    if topk > len(world["post"][column].values):
        assert np.all(res.fetched == N) and np.all(res.counts == len(world["post"][column].values))


def test_dense_group_is_why_the_complete_form_exists(world):
    """One key owns query 0's nearest 3 000 rows: the fetch-bounded form sees one group at its largest fetch, the complete form five."""
    g, q = world["g"], world["q"][:1]
    old = g.exact_search_grouped(q, 5, "dense", fetch=2048)
    assert old.counts[0] == 1 and not old.complete
    res = g.exact_search_grouped(q, 5, world["post"]["dense"])
    assert res.counts[0] == 5 and res.keys[0, 0] == 7 and same(res, expect(world, "dense", 1, 5, 1))


@pytest.mark.parametrize("params", [dict(flags=1), dict(flags=2), dict(cand_per_query=1)], ids=["no_seed", "no_prefilter", "overflow"])
def test_hooks_and_overflow_keep_the_bits(world, params):
    """cand_per_query = 1: the first launch's arena overflows and is run again with what it counted; the call repeated gives the same bits."""
    g, q = world["g"], world["q"][:33]
    res = g.exact_search_grouped(q, 10, world["post"]["doc"], group_size=3, params=params)
    st = g.last_group_full_stats()
    assert same(res, expect(world, "doc", 33, 10, 3))
    if "cand_per_query" in params:
        assert st["scan_reruns"] >= 1
        again = g.exact_search_grouped(q, 10, world["post"]["doc"], group_size=3, params=params)
        assert np.array_equal(again.dist.view(np.uint32), res.dist.view(np.uint32)) and np.array_equal(again.ids, res.ids)
    assert (st["ms_bound"] == 0) == ("flags" in params)


@pytest.mark.parametrize("kind", ["ids", "where"])
def test_filters(world, kind):
    from rabitq_amd import col
    g, q = world["g"], world["q"][:33]
    f = g.make_filter(ids=np.arange(0, N, 3, dtype=np.uint32)) if kind == "ids" else g.where(col("few") >= 0)
    res = g.exact_search_grouped(q, 10, world["post"]["doc"], group_size=3, filter=f)
    d, i, cnt = complete_rows(g, q, filter=f)
    assert same(res, gm.group_rows(d, i, cnt, world["keymap"]["doc"], 10, 3))
    f.close()


def test_device_form_writes_every_slot_over_junk(world):
    import torch
    g, nq, topk, gs = world["g"], 33, 10, 3
    dev = lambda a: torch.from_numpy(a).cuda()
    junk = lambda shape, dt: torch.full(shape, 0x2B2B2B2B, dtype=torch.int32, device="cuda").view(dt)
    q = dev(np.ascontiguousarray(world["q"][:nq]))
    od, oi = junk((nq, topk * gs), torch.float32), junk((nq, topk * gs), torch.int32)
    ok, gn, on, of = junk((nq, 2 * topk), torch.int64), junk((nq, topk), torch.int32), junk((nq,), torch.int32), junk((nq,), torch.int32)
    g.exact_search_grouped_full_device(q.data_ptr(), nq, q.shape[1], topk, world["post"]["doc"], od.data_ptr(), oi.data_ptr(), ok.data_ptr(),
                                       gn.data_ptr(), on.data_ptr(), of.data_ptr(), group_size=gs)
    want = expect(world, "doc", nq, topk, gs)
    host = lambda t, dt, shape: t.cpu().numpy().view(dt).reshape(shape)
    assert np.array_equal(host(od, np.uint32, want["ids"].shape), want["dist_bits"]) and np.array_equal(host(oi, np.uint32, want["ids"].shape), want["ids"])
    assert np.array_equal(host(ok, np.uint64, (nq, topk)), want["keys"]) and np.array_equal(host(gn, np.uint32, (nq, topk)), want["group_n"])
    assert np.array_equal(host(on, np.uint32, (nq,)), want["n"])


@pytest.mark.parametrize("rows,metric,d", [("f32", "l2", 128), ("f32", "cosine", 64), ("f32", "ip", 63), ("f16", "l2", 64), ("u8", "l2", 64)])
def test_dimension_metrics_and_row_types(rq, rows, metric, d):
    if rows in bm.TYPES:
        b, centres, marks = bm.byte_data(rows, N, d, 8, seed=77)
        x, q = bm.typed(b, rows), bm.byte_queries(rows, b, marks, 33, d, 8, seed=78)
    else:
        x, centres, _ = synth.mixture(N, d, 8, sigma=0.6, seed=77, centre_scale=0.8)
        q, _, _ = synth.mixture(33, d, 8, sigma=0.6, seed=78, centre_scale=0.8)
        x = hm.narrow(x, rows).view(np.float16) if rows == "f16" else x
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal((d + 63) // 64 * 64, seed=79), metric=metric, **({} if rows == "f32" else {"rows": rows}))
    g.create_attr("t", "u32", fill=0)
    g.set_attr("t", np.arange(N, dtype=np.uint32), np.random.default_rng(6).integers(0, N // 3, size=N))
    post = g.postings("t")
    d_, i_, cnt = complete_rows(g, q)
    assert same(g.exact_search_grouped(q, 10, post, group_size=3), gm.group_rows(d_, i_, cnt, snapshot(g, "t"), 10, 3))
    post.close(), g.close()


def test_against_f64_numpy_on_integer_data(rq):
    """Independent of the engine: coordinates are integers in [-8, 8] at dim 64, so every squared distance is an integer below 2^24,
    exact in f32; the reference is the f64 brute force, sorted by (distance, id), and the model's selection."""
    rng = np.random.default_rng(11)
    n, nq, topk, gs = N, 33, 10, 3
    x = rng.integers(-8, 9, size=(n, 64)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, 64)).astype(np.float32)
    vals = rng.integers(0, n // 3, size=n).astype(np.uint32)
    g = rq.RaBitQ.build(x, x[:8].copy(), np.eye(64, dtype=np.float32))
    g.create_attr("t", "u32", fill=0)
    g.set_attr("t", np.arange(n, dtype=np.uint32), vals)
    post = g.postings("t")
    d64 = ((q.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    ids = np.tile(np.arange(n, dtype=np.uint32), (nq, 1))
    want = gm.group_rows(d64.astype(np.float32), ids, np.full(nq, n), dict(enumerate(vals.tolist())), topk, gs)
    res = g.exact_search_grouped(q, topk, post, group_size=gs)
    kept = res.ids != gm.PAD_ID
    assert same(res, want) and np.array_equal(res.dist[kept].astype(np.float64), d64[np.nonzero(kept)[0], res.ids[kept]])
    post.close(), g.close()


def test_lazy_removals_snapshot_keys_and_refusals(rq, world):
    g, q = build(rq, 64, 940, n=3000)
    q, ids = q[:7], np.arange(3000, dtype=np.uint32)
    g.create_attr("doc", "u32", fill=0)
    g.set_attr("doc", ids, np.random.default_rng(7).integers(0, 900, size=3000))
    g.remove(ids=ids[::3], lazy=True)                                         # removals pending before creation: dead rows are in no group
    post, keymap = g.postings("doc"), snapshot(g, "doc")
    d, i, cnt = complete_rows(g, q)
    want = gm.group_rows(d, i, cnt, keymap, 10, 3)
    assert same(g.exact_search_grouped(q, 10, post, group_size=3), want)
    g.set_attr("doc", ids, 1)                                                   # rq_attr_set after creation: the keys stay the snapshot's
    assert same(g.exact_search_grouped(q, 10, post, group_size=3), want)
    refused = [(lambda: g.exact_search_grouped(q, 10, world["post"]["doc"]), INVALID),          # postings of another index
               (lambda: g.exact_search_grouped(q, 10, post, fetch=64), INVALID), (lambda: g.exact_search_grouped(q, 300, post, group_size=7), UNSUPPORTED)]
    g.remove(ids=[1], lazy=True)                                              # a marking lazy removal: stale
    for call, status in refused + [(lambda: g.exact_search_grouped(q, 10, post), INVALID)]:
        with pytest.raises(rq.RabitqError) as e:
            call()
        assert e.value.status == status
    post.close(), g.close()


def test_a_tiered_index_is_refused(rq):
    from rabitq_amd import index as ix
    ix.set_option("base_device_mb", 1)
    try:
        g, q = build(rq, 128, 61)
    finally:
        ix.set_option("base_device_mb", -1)
    g.create_attr("t", "u32", fill=3)
    post = g.postings("t")
    assert g.n_hbm < N
    with pytest.raises(rq.RabitqError) as e:
        g.exact_search_grouped(q[:2], 5, post)
    assert e.value.status == UNSUPPORTED
    post.close(), g.close()
