"""Grouped search on the GPU: every output array of the grouped entries, bit for bit, against the numpy model of
tests/group_model.py applied to the SAME index's plain call at topk = fetch -- so the selection kernel is pinned, whatever the
source returns -- and, behind the exact source, against a brute force over all rows.

Run on the GPU box:  python -m pytest tests/test_group_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import group_model as M
from tests import synth

pytestmark = pytest.mark.gpu

D, K, N = 64, 16, 3000
INVALID, UNSUPPORTED = -1, -6
TWINS = 20                                   # rows 2 j + 1 == rows 2 j for j < TWINS: equal distances under ids of different groups
# column -> (dtype, value of id): id % G for G in {1, 3, 50, n}, negative i32 / i64 keys, u64 keys equal in the low word
COLUMNS = {
    "g1": ("u32", lambda i: i % 1), "g3": ("u32", lambda i: i % 3), "g50": ("u32", lambda i: i % 50), "gn": ("u32", lambda i: i % N),
    "neg32": ("i32", lambda i: i % 7 - 5), "neg64": ("i64", lambda i: (i % 11 - 6) * (1 << 33)),
    "hi64": ("u64", lambda i: ((i % 13) << 32) | 7),
}
NP = {"u32": np.uint32, "i32": np.int32, "u64": np.uint64, "i64": np.int64}
SHAPES = [(1, 1, 1), (10, 1, 10), (10, 1, 64), (10, 3, 63), (10, 3, 64), (10, 3, 65), (5, 4, 256), (7, 5, 257), (100, 2, 2048),
          (2048, 1, 2048), (1, 2048, 2048)]
NQS = (1, 5, 64, 200)                        # the few-launch query path (<= 64 queries) and the staged one


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


_DATA = {}


def make_data(n=N, seed=700, d=D):
    """rows (the first TWINS pairs equal), centres (list K - 1 far from every row: it stays empty), 200 queries (the first TWINS are
    the twin rows themselves: both twins tie for the nearest place)"""
    if (n, seed, d) not in _DATA:
        x, centres, _ = synth.mixture(n, d, K - 1, sigma=0.8, seed=seed, centre_scale=0.6)
        centres = np.vstack([centres, np.full((1, d), 1000.0, dtype=np.float32)])
        q, _, _ = synth.mixture(200, d, K - 1, sigma=0.8, seed=seed + 1, centre_scale=0.6)
        t = min(TWINS, n // 2)
        x[1:2 * t:2] = x[0:2 * t:2]
        q[:t] = x[0:2 * t:2]
        _DATA[(n, seed, d)] = (x, centres, q)
    return _DATA[(n, seed, d)]


def column_values(name, ids):
    dtype, fn = COLUMNS[name]
    return np.array([fn(int(i)) for i in ids], dtype=np.int64).astype(NP[dtype]) if dtype != "u64" else \
        np.array([fn(int(i)) for i in ids], dtype=np.uint64)


def fill_columns(g, ids, names=COLUMNS):
    for name in names:
        g.create_attr(name, COLUMNS[name][0], fill=0)
        assert g.set_attr(name, ids, column_values(name, ids)) == 0


def build(rq, n=N, seed=700, names=COLUMNS, **kw):
    x, centres, _ = make_data(n, seed)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(D, seed=77), **kw)
    assert g.n == n and g.k == K and g.offsets[K] == g.offsets[K - 1], "list K - 1 is empty"
    fill_columns(g, np.arange(n), names)
    return g


@pytest.fixture(scope="module")
def big(rq):
    g = build(rq)
    yield g
    g.close()


_PLAIN, _KEYMAP = {}, {}


def plain(g, tag, q, probe, fetch, heur=False, filter=None):
    """the index's plain call at topk = fetch: computed once per (index state, batch, probe, fetch, ranker)"""
    key = (tag, len(q), probe, fetch, heur)
    if tag is None or key not in _PLAIN:
        src = g.query_batch(q, probe, fetch, heuristic_rank=heur, filter=filter)
        if tag is None:
            return src
        _PLAIN[key] = src
    return _PLAIN[key]


def keymap(g, tag, col, live=None):
    key = (tag, col)
    if tag is None or key not in _KEYMAP:
        km = M.keymap_of(g.map_ids, g.attr_array(col), live)
        if tag is None:
            return km
        _KEYMAP[key] = km
    return _KEYMAP[key]


def same(rq, res, src, km, topk, gs, what, col=None, stats=None, fetch=None):
    """every output array equals the model's, bit for bit; the totals; where the column is f(id), the keys are those of the ids"""
    d, i, c = src
    want = M.group_rows(d, i, c, km, topk, gs)
    B = len(c)
    assert res.dist.shape == res.ids.shape == (B, topk, gs) and res.keys.shape == res.group_counts.shape == (B, topk), what
    assert res.dist.dtype == np.float32 and res.ids.dtype == np.uint32 and res.group_counts.dtype == res.counts.dtype == np.uint32
    assert np.array_equal(res.counts, want["n"]), (what, "counts", res.counts[:8], want["n"][:8])
    assert np.array_equal(res.ids, want["ids"]), (what, "ids", np.argwhere(res.ids != want["ids"])[:4])
    assert np.array_equal(np.ascontiguousarray(res.dist).view(np.uint32), want["dist_bits"]), (what, "dist")
    assert np.array_equal(M.key_image(res.keys), want["keys"]), (what, "keys")
    assert np.array_equal(res.group_counts, want["group_n"]), (what, "group_counts")
    if res.fetched is not None:
        assert np.array_equal(res.fetched, np.minimum(c, fetch if fetch else d.shape[1])), (what, "fetched")
    if stats is not None:
        assert (stats["candidates"], stats["absent"], stats["kept"], stats["groups"]) == \
            (int(np.minimum(c, d.shape[1]).sum()), want["absent"], want["kept"], want["groups"]), (what, stats)
    if col is not None:                                                        # independent of the model's key map
        held = res.ids != M.PAD_ID
        first = res.ids[:, :, 0]
        assert np.array_equal(held[:, :, 0], np.arange(topk)[None, :] < res.counts[:, None]), what
        assert np.array_equal(M.key_image(res.keys)[held[:, :, 0]], M.key_image(column_values(col, first[held[:, :, 0]]))), (what, "keys of ids")
        for r in range(gs):
            at = held[:, :, r]
            assert np.array_equal(M.key_image(column_values(col, res.ids[:, :, r][at])), M.key_image(res.keys)[at]), (what, "group members")
    return want


def check_query(rq, g, tag, q, probe, topk, gs, fetch, col, heur=False, filter=None, live=None, what=""):
    src = plain(g, tag, q, probe, fetch, heur, filter)
    res = g.query_batch_grouped(q, probe, topk, col, group_size=gs, fetch=fetch, heuristic_rank=heur, filter=filter)
    st = rq.last_group_stats()
    assert st["fetch"] == fetch and st["ms_group"] > 0.0
    return same(rq, res, src, keymap(g, tag, col, live), topk, gs, (what, col, len(q), topk, gs, fetch, heur), col=col, stats=st, fetch=fetch), src


# ---- 1. every shape of the kernel, every batch size ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("topk,gs,fetch", SHAPES)
def test_shapes_and_batches(rq, big, topk, gs, fetch):
    _, _, q = make_data()
    for n_i, nq in enumerate(NQS):
        col = ("g50", "g3", "hi64", "neg32")[(n_i + fetch) % 4]
        want, src = check_query(rq, big, "big", q[:nq], K, topk, gs, fetch, col)
        assert (src[2] == min(fetch, N)).all()                                # probe = every list: the source fills its rows
        assert want["kept"] > 0


@pytest.mark.parametrize("col", sorted(COLUMNS))
@pytest.mark.parametrize("heur", [False, True])
def test_key_spreads_and_rankers(rq, big, col, heur):
    _, _, q = make_data()
    for topk, gs, fetch, nq in ((10, 3, 64, 64), (7, 5, 257, 40), (20, 2, 200, 200)):
        want, _ = check_query(rq, big, "big", q[:nq], 5, topk, gs, fetch, col, heur=heur)
        if col == "g1":
            assert (want["n"] <= 1).all()
        if col == "gn":
            assert (want["group_n"] <= 1).all()


def test_ties_between_groups_are_decided_by_id(rq, big):
    """Queries 0 .. TWINS - 1 are rows 2 j == 2 j + 1: both at the same distance, in different groups -- id 2 j opens the first."""
    _, _, q = make_data()
    src = plain(big, "big", q[:TWINS], K, 64)
    res = big.query_batch_grouped(q[:TWINS], K, 2, "g50", group_size=1, fetch=64)
    same(rq, res, src, keymap(big, "big", "g50"), 2, 1, "twins", col="g50")
    j = np.arange(TWINS)
    assert np.array_equal(res.ids[:, 0, 0], 2 * j) and np.array_equal(res.ids[:, 1, 0], 2 * j + 1)
    assert np.array_equal(res.dist[:, 0, 0].view(np.uint32), res.dist[:, 1, 0].view(np.uint32))


def test_short_rows_small_probe_and_small_index(rq, big):
    _, _, q = make_data()
    for topk, gs, fetch in ((10, 3, 64), (100, 2, 2048), (5, 4, 256)):
        want, src = check_query(rq, big, "big", q[:70], 1, topk, gs, fetch, "g50")
        if fetch == 2048:
            assert (src[2] < fetch).all()                                     # one list holds fewer rows than fetch
    g = build(rq, 40, names=("g3", "neg64"))                                  # n < fetch
    try:
        for topk, gs, fetch in ((3, 2, 64), (10, 5, 256), (2048, 1, 2048), (1, 2048, 2048)):
            want, src = check_query(rq, g, None, q[:9], K, topk, gs, fetch, "g3")
            assert (src[2] == 40).all() and (want["n"] == min(3, topk)).all()
            check_query(rq, g, None, q[:9], K, topk, gs, fetch, "neg64")
    finally:
        g.close()


def test_two_identical_calls_give_identical_bits(rq, big):
    _, _, q = make_data()
    for topk, gs, fetch in ((10, 3, 64), (100, 2, 2048)):
        a = big.query_batch_grouped(q, K, topk, "g50", group_size=gs, fetch=fetch)
        b = big.query_batch_grouped(q, K, topk, "g50", group_size=gs, fetch=fetch)
        for name in a.__slots__:
            assert np.array_equal(np.ascontiguousarray(getattr(a, name)).view(np.uint8), np.ascontiguousarray(getattr(b, name)).view(np.uint8)), name


# ---- 2. the selection alone: rq_group_results_device ---------------------------------------------------------------------------------------
def device_group(rq, g, dist, ids, cnt, topk, gs, col):
    """rq_group_results_device over caller-made rows; the outputs are preset to junk: every slot must be written"""
    import torch
    B, F = dist.shape
    td = torch.from_numpy(np.ascontiguousarray(dist)).cuda()
    ti = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32)).cuda()
    tc = torch.from_numpy(np.ascontiguousarray(cnt, dtype=np.uint32).view(np.int32)).cuda()
    od = torch.full((B, topk, gs), 123.0, dtype=torch.float32, device="cuda")
    oi = torch.full((B, topk, gs), 77, dtype=torch.int32, device="cuda")
    ok = torch.full((B, topk), 55, dtype=torch.int64, device="cuda")
    gn = torch.full((B, topk), 9, dtype=torch.int32, device="cuda")
    on = torch.full((B,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.group_results_device(td.data_ptr(), ti.data_ptr(), tc.data_ptr(), B, F, topk, col, od.data_ptr(), oi.data_ptr(), ok.data_ptr(),
                           gn.data_ptr(), on.data_ptr(), group_size=gs)
    st = rq.last_group_stats()
    keys = ok.cpu().numpy().view(np.uint64)
    dt = NP[COLUMNS[col][0]]
    keys = keys.astype(np.uint32).view(dt) if np.dtype(dt).itemsize == 4 else keys.view(dt)
    res = rq.GroupedResult(od.cpu().numpy(), oi.cpu().numpy().view(np.uint32), keys, gn.cpu().numpy().view(np.uint32),
                           on.cpu().numpy().view(np.uint32), None)
    return res, st


def made_rows(rng, map_ids, B, F, absent):
    """B rows of F candidates: distinct stored ids, a few absent ones, distances with many ties, counts from 0 to F"""
    ids = np.stack([rng.choice(map_ids, size=F, replace=False) for _ in range(B)]).astype(np.uint32)
    for b in range(B):
        at = rng.choice(F, size=min(F, len(absent)), replace=False)
        ids[b, at] = absent[:at.size]
    dist = (rng.integers(0, 12, size=(B, F)) / 4).astype(np.float32)
    cnt = rng.integers(0, F + 1, size=B).astype(np.uint32)
    cnt[0], cnt[1 % B] = 0, F
    return dist, ids, cnt


def shuffled(rng, dist, ids, cnt):
    d2, i2 = dist.copy(), ids.copy()
    for b in range(len(cnt)):
        p = rng.permutation(int(cnt[b]))
        d2[b, :cnt[b]], i2[b, :cnt[b]] = dist[b, p], ids[b, p]
    return d2, i2


@pytest.mark.parametrize("topk,gs,F", [(4, 3, 40), (10, 3, 64), (6, 4, 200), (9, 5, 257), (50, 3, 700)])
def test_selection_alone_shuffles_absent_ids_empty_rows(rq, big, topk, gs, F):
    rng = np.random.default_rng(F)
    map_ids = big.map_ids
    absent = np.array([N, N + 12345, 0xFFFFFFFF, 0xFFFFFFFE, 1 << 31], dtype=np.uint32)   # at and past the directory's top
    dist, ids, cnt = made_rows(rng, map_ids, 7, F, absent)
    for col in ("g3", "hi64"):
        res, st = device_group(rq, big, dist, ids, cnt, topk, gs, col)
        want = same(rq, res, (dist, ids, cnt), keymap(big, "big", col), topk, gs, ("made rows", col, F), col=col, stats=st)
        assert want["absent"] > 0 and res.counts[0] == 0 and (res.ids[0] == M.PAD_ID).all() and np.isnan(res.dist[0]).all()
        assert not res.keys[0].any() and not res.group_counts[0].any()
        d2, i2 = shuffled(rng, dist, ids, cnt)                                # any order of a row's pairs: identical output
        res2, _ = device_group(rq, big, d2, i2, cnt, topk, gs, col)
        for name in ("dist", "ids", "keys", "group_counts", "counts"):
            assert np.array_equal(np.ascontiguousarray(getattr(res, name)).view(np.uint8), np.ascontiguousarray(getattr(res2, name)).view(np.uint8)), name
    # the host form takes the same rows
    res3 = big.group_results(dist, ids, cnt, topk, "g3", group_size=gs)
    same(rq, res3, (dist, ids, cnt), keymap(big, "big", "g3"), topk, gs, ("host form", F), col="g3")


# ---- 3. filters, removals, relayouts -------------------------------------------------------------------------------------------------------
def test_filters_pending_removals_and_relayouts(rq):
    from rabitq_amd import col as c_
    x, centres, q = make_data()
    g = build(rq, names=("g50", "neg64"))
    try:
        shapes = ((10, 3, 64), (7, 5, 257))
        rng = np.random.default_rng(5)
        allowed = rng.choice(N, size=900, replace=False)
        with g.make_filter(ids=allowed) as f, g.where(c_("g50") < 20) as w:
            for topk, gs, fetch in shapes:
                want, src = check_query(rq, g, None, q[:80], K, topk, gs, fetch, "g50", filter=f, what="id filter")
                assert np.isin(src[1][src[1] != M.PAD_ID], allowed).all()
                want, _ = check_query(rq, g, None, q[:80], K, topk, gs, fetch, "g50", filter=w, what="where filter")
                assert (want["keys"][want["group_n"] > 0] < 20).all() and (want["n"] > 0).all()
            res = g.exact_search_grouped(q[:30], 10, "neg64", group_size=3, fetch=64, filter=f)
            same(rq, res, g.exact_search(q[:30], 64, filter=f), keymap(g, None, "neg64"), 10, 3, "exact, id filter", col="neg64", fetch=64)
        # pending removals: the source runs under the live filter; a dead id among supplied candidates is absent
        dead = rng.choice(N, size=700, replace=False).astype(np.uint32)
        assert g.remove(ids=dead, lazy=True) == 700
        live = ~np.isin(g.map_ids, dead)
        for topk, gs, fetch in shapes:
            want, src = check_query(rq, g, None, q[:80], K, topk, gs, fetch, "g50", live=live, what="pending")
            assert not np.isin(src[1], dead).any()
        dist, ids, cnt = made_rows(rng, g.map_ids, 5, 100, dead[:30])
        res, st = device_group(rq, g, dist, ids, cnt, 6, 3, "g50")
        want = same(rq, res, (dist, ids, cnt), keymap(g, None, "g50", live), 6, 3, "dead ids", col="g50", stats=st)
        assert want["absent"] > 0 and not np.isin(res.ids, dead).any()
        # compact + add + remove: the keys are those of the moved rows
        assert g.compact() == 700 and g.pending_removals == 0
        new = g.add(x[:300] + np.float32(0.01))
        fill_columns_existing(g, new)
        gone = np.arange(1, N, 9)
        gone = gone[~np.isin(gone, dead)]
        assert g.remove(ids=gone) == gone.size
        for topk, gs, fetch in shapes + ((100, 2, 2048),):
            want, src = check_query(rq, g, None, q[:80], K, topk, gs, fetch, "g50", what="relaid out")
            check_query(rq, g, None, q[:80], K, topk, gs, fetch, "neg64", what="relaid out")
        assert rq.last_group_stats()["directory_built"] == 0                  # ... and the first call after the relayout made a new one
        assert np.isin(new, g.map_ids).all()
    finally:
        g.close()


def fill_columns_existing(g, ids):
    for a in g.attrs():
        assert g.set_attr(a["name"], ids, column_values(a["name"], ids)) == 0


def test_directory_is_made_by_the_first_grouped_call(rq):
    _, _, q = make_data()
    g = build(rq, 500, names=("g3",))
    try:
        g.add(make_data()[0][500:510])                                        # a relayout: no directory of this layout exists
        g.query_batch_grouped(q[:4], K, 2, "g3", fetch=8)
        assert rq.last_group_stats()["directory_built"] == 1
        g.query_batch_grouped(q[:4], K, 2, "g3", fetch=8)
        assert rq.last_group_stats()["directory_built"] == 0
    finally:
        g.close()


def test_sparse_ids_take_the_hash_directory(rq, big):
    _, _, q = make_data()
    sparse = lambda i: (7 * np.asarray(i, dtype=np.uint64) + (1 << 31)).astype(np.uint32)
    g = rq.RaBitQ.from_arrays(big.base, big.orthogonal, big.centroids, big.offsets, sparse(big.map_ids), big.codes, big.factors)
    try:
        for name in ("g50", "hi64"):
            g.create_attr(name, COLUMNS[name][0], fill=0)
            assert g.set_attr(name, sparse(np.arange(N)), column_values(name, np.arange(N))) == 0
        for topk, gs, fetch in ((10, 3, 64), (7, 5, 257), (100, 2, 2048)):
            for col in ("g50", "hi64"):
                src = plain(g, None, q[:70], K, fetch)
                res = g.query_batch_grouped(q[:70], K, topk, col, group_size=gs, fetch=fetch)
                same(rq, res, src, keymap(g, None, col), topk, gs, ("hash", col, fetch), fetch=fetch)
        assert rq.last_by_id_stats()["form"] == "hash"
        rng = np.random.default_rng(9)
        absent = np.array([5, (1 << 31) + 1, 0xFFFFFFFF, sparse(N), 0], dtype=np.uint32)     # between the stored ids, and past them
        for F, topk, gs in ((48, 5, 3), (300, 20, 4)):
            dist, ids, cnt = made_rows(rng, g.map_ids, 6, F, absent)
            res, st = device_group(rq, g, dist, ids, cnt, topk, gs, "g50")
            want = same(rq, res, (dist, ids, cnt), keymap(g, None, "g50"), topk, gs, ("hash, made rows", F), stats=st)
            assert want["absent"] > 0
    finally:
        g.close()


# ---- 4. metrics, row types, a shard --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cosine", "ip", "f16", "u8", "shard"])
def test_metrics_row_types_and_a_shard(rq, kind):
    x, centres, q = make_data()
    P = synth.random_orthogonal(128 if kind == "ip" else D, seed=79)
    if kind in ("cosine", "ip"):
        g = rq.RaBitQ.build(x, centres, P, metric=kind)
    elif kind == "f16":
        g = rq.RaBitQ.build(x.astype(np.float16), centres, P, rows="f16")
    elif kind == "u8":
        g = rq.RaBitQ.build(np.clip(np.rint(x * 40.0 + 128.0), 0, 255).astype(np.uint8), centres * 40.0 + 128.0, P, rows="u8")
        q = q * np.float32(40.0) + np.float32(128.0)
    else:
        g = rq.RaBitQ.build(x, centres, P)
    fill_columns(g, np.arange(N), ("g50", "neg32"))
    held = [g]
    try:
        if kind == "shard":
            owner, _ = g.partition_lists(2)
            g = g.shard(owner, 0)
            held.append(g)
            assert 0 < g.n < N
        for topk, gs, fetch in ((10, 3, 64), (7, 5, 257)):
            for col in ("g50", "neg32"):
                check_query(rq, g, None, q[:70], K, topk, gs, fetch, col, what=kind)
        res = g.exact_search_grouped(q[:20], 10, "g50", group_size=2, fetch=100)
        same(rq, res, g.exact_search(q[:20], 100), keymap(g, None, "g50"), 10, 2, (kind, "exact"), col="g50", fetch=100)
    finally:
        for h in held[::-1]:
            h.close()


# ---- 5. truth ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1, 3])
def test_exact_grouped_is_the_true_grouped_answer(rq, gs):
    """n = 1500 < fetch = 2048: every query fetches every row, so the grouped answer must be the brute force over all rows -- rows
    ascending by (exact distance, id), the first gs per key, the first topk keys.  The distances are those exact_search returns."""
    n, topk, col = 1500, 12, "g50"
    _, _, q = make_data()
    g = build(rq, n, names=(col,))
    try:
        d, i, c = g.exact_search(q[:50], n)
        assert (c == n).all() and np.array_equal(np.sort(i, axis=1), np.tile(np.arange(n, dtype=np.uint32), (50, 1)))
        res = g.exact_search_grouped(q[:50], topk, col, group_size=gs, fetch=2048)
        assert (res.fetched == n).all() and (res.fetched < 2048).all()        # complete for every query: none is left out
        assert (res.counts == topk).all()
        for b in range(50):
            order = np.lexsort((i[b], M.ord32_biased(d[b])))                  # ascending by (distance, id)
            groups = {}
            for j in order:
                key = int(i[b, j]) % 50
                if key not in groups and len(groups) == topk:
                    continue
                rows = groups.setdefault(key, [])
                if len(rows) < gs:
                    rows.append(j)
            for o, (key, rows) in enumerate(groups.items()):
                assert res.keys[b, o] == key and res.group_counts[b, o] == len(rows), (b, o)
                assert np.array_equal(res.ids[b, o, :len(rows)], i[b, rows]), (b, o)
                assert np.array_equal(res.dist[b, o, :len(rows)].view(np.uint32), d[b, rows].view(np.uint32)), (b, o)
                assert (res.ids[b, o, len(rows):] == M.PAD_ID).all()
    finally:
        g.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(rq, big):
    from rabitq_amd import _lib
    from rabitq_amd import index as ix
    _, _, q = make_data()
    x, centres, _ = make_data()

    def refused(status, text, fn):
        with pytest.raises(rq.RabitqError) as e:
            fn()
        assert e.value.status == status and text in str(e.value), (status, text, str(e.value))

    g = build(rq, 300, names=("g3",))
    try:
        g.create_attr("w", "f32", fill=0.5)
        for call in (lambda **kw: g.query_batch_grouped(q[:4], 4, group_by=kw.pop("col", "g3"), **kw),
                     lambda **kw: g.exact_search_grouped(q[:4], group_by=kw.pop("col", "g3"), **kw)):
            refused(INVALID, "f32", lambda: call(topk=2, col="w"))
            refused(INVALID, "no column named", lambda: call(topk=2, col="nope"))
            refused(UNSUPPORTED, "topk * group_size <= fetch <= 2048", lambda: call(topk=5, group_size=3, fetch=14))
            refused(UNSUPPORTED, "fetch <= 2048", lambda: call(topk=5, fetch=2049))
            refused(UNSUPPORTED, "at least 1", lambda: call(topk=0, fetch=8))
            refused(UNSUPPORTED, "at least 1", lambda: call(topk=2, group_size=0, fetch=8))
        L = _lib.lib()                                                       # the C entry itself names the unknown column
        out = np.zeros(64, dtype=np.uint64)
        prm = _lib.GroupParamsT(topk=1, group_size=1, fetch=4)
        o = C.c_void_p(out.ctypes.data)
        assert L.rq_group_results(g._h, o, o, o, 1, b"nope", C.byref(prm), o, o, o, o, o) == INVALID and b"no column named nope" in L.rq_last_error()
        # a filter of another generation, and of another index
        f = g.make_filter(ids=np.arange(100))
        other = big.make_filter(ids=np.arange(100))
        refused(INVALID, "another index", lambda: g.query_batch_grouped(q[:4], 4, 2, "g3", fetch=8, filter=other))
        g.add(x[300:305])
        refused(INVALID, "last mutated", lambda: g.query_batch_grouped(q[:4], 4, 2, "g3", fetch=8, filter=f))
        refused(INVALID, "last mutated", lambda: g.exact_search_grouped(q[:4], 2, "g3", fetch=8, filter=f))
        f.close(), other.close()
    finally:
        g.close()
    # the exact form on a tiered index: the exact search's refusal; the approximate form works there
    ix.set_option("base_device_mb", 1)                                         # n * dim * 4 = 1.5 MB
    try:
        x6, c6, _ = make_data(6000, seed=701)
        t = rq.RaBitQ.build(x6, c6, synth.random_orthogonal(D, seed=77))
    finally:
        ix.set_option("base_device_mb", -1)
    try:
        if not t.n_hbm < t.n:
            pytest.fail("the index was meant to be tiered")
        fill_columns(t, np.arange(6000), ("g50",))
        refused(UNSUPPORTED, "tiered", lambda: t.exact_search_grouped(q[:4], 2, "g50", fetch=8))
        check_query(rq, t, None, q[:20], K, 10, 3, 64, "g50", what="tiered")
    finally:
        t.close()
