"""Diverse search on the GPU: every output array of the diverse entries, bit for bit, against the numpy model of
tests/diverse_model.py applied to the SAME index's plain call at topk = fetch -- so the selection kernel is pinned, whatever the
source returns -- and, behind the exact source, against the model fed by a brute force over all rows.  No tolerance anywhere.

Run on the GPU box:  python -m pytest tests/test_diverse_gpu.py -m gpu -q
"""
import numpy as np
import pytest

import oracle
from tests import diverse_model as M
from tests import synth

pytestmark = pytest.mark.gpu

D, K, N = 64, 16, 3000
INVALID, UNSUPPORTED = -1, -6
TWINS = 20                                   # rows 2 j + 1 == rows 2 j for j < TWINS: pair distance 0, equal distances to every query
# (topk, fetch): both sides of the kernel's boundaries (one wave up to 64, the 256-wide block up to 256, the 2048-wide above), the extremes
SHAPES = [(1, 1), (10, 10), (10, 63), (10, 64), (10, 65), (5, 256), (7, 257), (64, 64), (100, 2048), (2048, 2048)]
NQS = (1, 5, 64, 200)                        # the few-launch query path (<= 64 queries) and the staged one
LAMS = (0.0, 0.3, 0.5, 1.0)


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    import os
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


_DATA = {}


def make_data(n=N, seed=800, d=D):
    """rows (the first TWINS pairs equal), centres (list K - 1 far from every row: it stays empty), 200 queries (the first TWINS are
    the twin rows themselves)"""
    if (n, seed, d) not in _DATA:
        x, centres, _ = synth.mixture(n, d, K - 1, sigma=0.8, seed=seed, centre_scale=0.6)
        centres = np.vstack([centres, np.full((1, d), 1000.0, dtype=np.float32)])
        q, _, _ = synth.mixture(200, d, K - 1, sigma=0.8, seed=seed + 1, centre_scale=0.6)
        t = min(TWINS, n // 2)
        x[1:2 * t:2] = x[0:2 * t:2]
        q[:t] = x[0:2 * t:2]
        _DATA[(n, seed, d)] = (x, centres, q)
    return _DATA[(n, seed, d)]


def build(rq, n=N, seed=800, d=D, **kw):
    x, centres, _ = make_data(n, seed, d)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=77), **kw)
    assert g.n == n and g.k == K
    return g


@pytest.fixture(scope="module")
def big(rq):
    g = build(rq)
    yield g
    g.close()


@pytest.fixture(scope="module")
def wide(rq):
    """dim 192: exact_l2_row's 128- and 64-wide tails run"""
    g = build(rq, 1200, seed=810, d=192)
    yield g
    g.close()


_PLAIN, _ROWS = {}, {}


def plain(g, tag, q, probe, fetch, heur=False, filter=None):
    """the index's plain call at topk = fetch: computed once per (index state, batch, probe, fetch, ranker)"""
    key = (tag, len(q), probe, fetch, heur)
    if tag is None or key not in _PLAIN:
        src = g.query_batch(q, probe, fetch, heuristic_rank=heur, filter=filter)
        if tag is None:
            return src
        _PLAIN[key] = src
    return _PLAIN[key]


def stored(g, tag, live=None):
    """({id: position}, the widened stored rows in position order: what rq_fetch_rows returns) -- once per index state"""
    if tag is None or tag not in _ROWS:
        rows, found = g.fetch(g.map_ids, raw=False)                            # (dim long on an inner-product index too)
        assert np.array_equal(found.astype(bool), np.ones(g.n, dtype=bool) if live is None else live)
        val = (M.posmap_of(g.map_ids, live), np.ascontiguousarray(rows, dtype=np.float32))
        if tag is None:
            return val
        _ROWS[tag] = val
    return _ROWS[tag]


def same(res, src, posmap, base, topk, lam, what, stats=None, fetch=None):
    """every output array equals the model's, bit for bit; the totals"""
    d, i, c = src
    want = M.diversify_rows(d, i, c, posmap, base, topk, lam)
    B = len(c)
    assert res.dist.shape == res.ids.shape == res.div.shape == (B, topk), what
    assert res.dist.dtype == res.div.dtype == np.float32 and res.ids.dtype == res.counts.dtype == np.uint32
    assert np.array_equal(res.counts, want["n"]), (what, "counts", res.counts[:8], want["n"][:8])
    assert np.array_equal(res.ids, want["ids"]), (what, "ids", np.argwhere(res.ids != want["ids"])[:4])
    assert np.array_equal(np.ascontiguousarray(res.dist).view(np.uint32), want["dist_bits"]), (what, "dist")
    assert np.array_equal(np.ascontiguousarray(res.div).view(np.uint32), want["div_bits"]), (what, "div")
    if res.fetched is not None:
        assert np.array_equal(res.fetched, np.minimum(c, fetch if fetch else d.shape[1])), (what, "fetched")
    if stats is not None:
        got = tuple(stats[k] for k in ("candidates", "absent", "skipped", "taken", "pair_distances"))
        assert got == tuple(want[k] for k in ("candidates", "absent", "skipped", "taken", "pair_distances")), (what, stats)
    return want


def sorted_plain(src, topk):
    """the plain rows' first topk pairs in (distance, id) order, padded: what lambda = 1 must return"""
    d, i, c = src
    oi = np.full((len(c), topk), M.PAD_ID, dtype=np.uint32)
    od = np.full((len(c), topk), M.NAN_BITS, dtype=np.uint32)
    for b in range(len(c)):
        n = int(c[b])
        order = np.lexsort((i[b, :n], M.ord32_biased(d[b, :n])))[:topk]
        oi[b, :order.size] = i[b, order]
        od[b, :order.size] = d[b, order].view(np.uint32)
    return od, oi


def check_query(rq, g, tag, q, probe, topk, fetch, lam, heur=False, filter=None, live=None, what=""):
    src = plain(g, tag, q, probe, fetch, heur, filter)
    res = g.query_batch_diverse(q, probe, topk, lam=lam, fetch=fetch, heuristic_rank=heur, filter=filter)
    st = rq.last_diverse_stats()
    assert st["fetch"] == fetch and st["ms_select"] > 0.0
    posmap, base = stored(g, tag, live)
    want = same(res, src, posmap, base, topk, lam, (what, len(q), topk, fetch, lam, heur), stats=st, fetch=fetch)
    if lam == 1.0:                                                             # also: the sorted plain rows, without the model
        od, oi = sorted_plain(src, topk)
        assert np.array_equal(res.ids, oi) and np.array_equal(np.ascontiguousarray(res.dist).view(np.uint32), od), (what, "lambda = 1")
    return want, src, res


# ---- 1. every shape of the kernel, every batch size, every lambda ---------------------------------------------------------------------------
@pytest.mark.parametrize("topk,fetch", SHAPES)
def test_shapes_batches_and_lambdas(rq, big, topk, fetch):
    _, _, q = make_data()
    heavy = fetch > 256                                                        # (the model is a Python loop: the wide shapes take one lambda
    for n_i, nq in enumerate(NQS):                                             #  per batch, 2048 steps over 2048 the first queries of it)
        nq_m = min(nq, 6) if topk * fetch > 300000 else nq
        lams = (LAMS[(n_i + topk) % 4],) if heavy or nq > 64 else LAMS
        src = plain(big, "big", q[:nq], K, fetch)
        assert (src[2] == min(fetch, N)).all()                                # probe = every list: the source fills its rows
        for lam in lams:
            res = big.query_batch_diverse(q[:nq], K, topk, lam=lam, fetch=fetch)
            posmap, base = stored(big, "big")
            cut = lambda a: a[:nq_m]
            sub = rq.DiverseResult(cut(res.dist), cut(res.ids), cut(res.div), cut(res.counts), cut(res.fetched))
            want = same(sub, tuple(cut(a) for a in src), posmap, base, topk, lam, ("shapes", nq, topk, fetch, lam), fetch=fetch)
            assert (want["n"] == topk).all() and (res.counts == topk).all()
            assert np.array_equal(res.fetched, src[2])
            if lam == 1.0:
                od, oi = sorted_plain(src, topk)
                assert np.array_equal(res.ids, oi) and np.array_equal(np.ascontiguousarray(res.dist).view(np.uint32), od)
            if nq >= TWINS:                                                    # c_0: of two rows at the same distance, the smaller id
                assert (res.ids[:TWINS, 0] == 2 * np.arange(TWINS)).all()


@pytest.mark.parametrize("heur", [False, True])
def test_both_rankers_small_probe_and_dim_192(rq, big, wide, heur):
    _, _, q = make_data()
    for topk, fetch, nq in ((10, 64, 64), (7, 257, 12), (20, 200, 40)):
        want, src, _ = check_query(rq, big, "big", q[:nq], 5, topk, fetch, 0.5, heur=heur)
    want, src, _ = check_query(rq, big, "big", q[:70], 1, 10, 256, 0.3, heur=heur)   # one list: rows shorter than fetch
    assert (src[2] < 256).any()
    _, _, q2 = make_data(1200, 810, 192)
    for topk, fetch, lam in ((10, 64, 0.5), (6, 100, 0.3), (5, 300, 0.0)):
        check_query(rq, wide, "wide", q2[:12], K, topk, fetch, lam, heur=heur, what="dim 192")


def test_two_identical_calls_give_identical_bits(rq, big):
    _, _, q = make_data()
    for topk, fetch in ((10, 64), (100, 2048)):
        a = big.query_batch_diverse(q, K, topk, fetch=fetch)
        b = big.query_batch_diverse(q, K, topk, fetch=fetch)
        for name in a.__slots__:
            assert np.array_equal(np.ascontiguousarray(getattr(a, name)).view(np.uint8), np.ascontiguousarray(getattr(b, name)).view(np.uint8)), name


# ---- 2. the selection alone: rq_diversify_results_device -------------------------------------------------------------------------------------
def device_diversify(rq, g, dist, ids, cnt, topk, lam):
    """rq_diversify_results_device over caller-made rows; the outputs are preset to junk: every slot must be written"""
    import torch
    B, F = dist.shape
    td = torch.from_numpy(np.ascontiguousarray(dist)).cuda()
    ti = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32)).cuda()
    tc = torch.from_numpy(np.ascontiguousarray(cnt, dtype=np.uint32).view(np.int32)).cuda()
    od = torch.full((B, topk), 123.0, dtype=torch.float32, device="cuda")
    oi = torch.full((B, topk), 77, dtype=torch.int32, device="cuda")
    ov = torch.full((B, topk), -5.0, dtype=torch.float32, device="cuda")
    on = torch.full((B,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.diversify_results_device(td.data_ptr(), ti.data_ptr(), tc.data_ptr(), B, F, topk, od.data_ptr(), oi.data_ptr(), ov.data_ptr(),
                               on.data_ptr(), lam=lam)
    st = rq.last_diverse_stats()
    return rq.DiverseResult(od.cpu().numpy(), oi.cpu().numpy().view(np.uint32), ov.cpu().numpy(), on.cpu().numpy().view(np.uint32), None), st


def made_rows(rng, map_ids, B, F, absent):
    """B rows of F pairs: stored ids with a few duplicates, a few absent ones, distances with many ties and an inf, counts 0 .. F"""
    ids = np.stack([rng.choice(map_ids, size=F, replace=False) for _ in range(B)]).astype(np.uint32)
    dist = (rng.integers(0, 12, size=(B, F)) / 4).astype(np.float32)
    for b in range(B):
        at = rng.choice(F, size=min(F, len(absent)), replace=False)
        ids[b, at] = absent[:at.size]
        if F >= 8:
            dup = rng.choice(F, size=4, replace=False)
            ids[b, dup[1]], ids[b, dup[3]] = ids[b, dup[0]], ids[b, dup[2]]  # duplicates: separate candidates (one pair at equal distance)
            dist[b, dup[1]] = dist[b, dup[0]]
            dist[b, rng.integers(0, F)] = np.inf
    cnt = rng.integers(0, F + 1, size=B).astype(np.uint32)
    cnt[0], cnt[1 % B] = 0, F
    return dist, ids, cnt


def shuffled(rng, dist, ids, cnt):
    d2, i2 = dist.copy(), ids.copy()
    for b in range(len(cnt)):
        p = rng.permutation(int(cnt[b]))
        d2[b, :cnt[b]], i2[b, :cnt[b]] = dist[b, p], ids[b, p]
    return d2, i2


@pytest.mark.parametrize("topk,F", [(4, 40), (10, 64), (6, 200), (9, 257), (50, 700)])
def test_selection_alone_shuffles_absent_ids_duplicates_empty_rows(rq, big, topk, F):
    rng = np.random.default_rng(F)
    absent = np.array([N, N + 12345, 0xFFFFFFFF, 0xFFFFFFFE, 1 << 31], dtype=np.uint32)   # at and past the directory's top
    dist, ids, cnt = made_rows(rng, big.map_ids, 7, F, absent)
    posmap, base = stored(big, "big")
    for lam in (0.5, 0.0):
        res, st = device_diversify(rq, big, dist, ids, cnt, topk, lam)
        want = same(res, (dist, ids, cnt), posmap, base, topk, lam, ("made rows", F, lam), stats=st)
        assert want["absent"] > 0 and want["skipped"] > 0
        assert res.counts[0] == 0 and (res.ids[0] == M.PAD_ID).all() and np.isnan(res.dist[0]).all() and np.isnan(res.div[0]).all()
        d2, i2 = shuffled(rng, dist, ids, cnt)                                # any order of a row's pairs: identical output
        res2, _ = device_diversify(rq, big, d2, i2, cnt, topk, lam)
        for name in ("dist", "ids", "div", "counts"):
            assert np.array_equal(np.ascontiguousarray(getattr(res, name)).view(np.uint8), np.ascontiguousarray(getattr(res2, name)).view(np.uint8)), name
    res3 = big.diversify_results(dist, ids, cnt, topk, lam=0.3)               # the host form takes the same rows
    same(res3, (dist, ids, cnt), posmap, base, topk, 0.3, ("host form", F))


# ---- 3. filters, removals, relayouts, the hash directory -------------------------------------------------------------------------------------
def test_filters_pending_removals_and_relayouts(rq):
    from rabitq_amd import col as c_
    x, centres, q = make_data()
    g = build(rq)
    try:
        g.create_attr("g50", "u32", fill=0)
        assert g.set_attr("g50", np.arange(N), (np.arange(N) % 50).astype(np.uint32)) == 0
        shapes = ((10, 64), (7, 257))
        rng = np.random.default_rng(5)
        allowed = rng.choice(N, size=900, replace=False)
        with g.make_filter(ids=allowed) as f, g.where(c_("g50") < 20) as w:
            for topk, fetch in shapes:
                _, src, _ = check_query(rq, g, None, q[:20], K, topk, fetch, 0.5, filter=f, what="id filter")
                assert np.isin(src[1][src[1] != M.PAD_ID], allowed).all()
                _, _, res = check_query(rq, g, None, q[:20], K, topk, fetch, 0.5, filter=w, what="where filter")
                assert (res.ids[res.ids != M.PAD_ID] % 50 < 20).all()
            res = g.exact_search_diverse(q[:10], 10, lam=0.3, fetch=64, filter=f)
            posmap, base = stored(g, None)
            same(res, g.exact_search(q[:10], 64, filter=f), posmap, base, 10, 0.3, "exact, id filter", fetch=64)
        # pending removals: the source runs under the live filter; a dead id among supplied pairs is absent
        dead = rng.choice(N, size=700, replace=False).astype(np.uint32)
        assert g.remove(ids=dead, lazy=True) == 700
        live = ~np.isin(g.map_ids, dead)
        for topk, fetch in shapes:
            _, src, _ = check_query(rq, g, None, q[:20], K, topk, fetch, 0.5, live=live, what="pending")
            assert not np.isin(src[1], dead).any()
        dist, ids, cnt = made_rows(rng, g.map_ids, 5, 100, dead[:30])
        res, st = device_diversify(rq, g, dist, ids, cnt, 6, 0.5)
        posmap, base = stored(g, None, live)
        want = same(res, (dist, ids, cnt), posmap, base, 6, 0.5, "dead ids", stats=st)
        assert want["absent"] > 0 and not np.isin(res.ids, dead).any()
        # compact + add + remove: the rows are those of the moved positions
        assert g.compact() == 700 and g.pending_removals == 0
        new = g.add(x[:300] + np.float32(0.01))
        gone = np.arange(1, N, 9)
        gone = gone[~np.isin(gone, dead)]
        assert g.remove(ids=gone) == gone.size
        for topk, fetch in shapes + ((100, 2048),):
            check_query(rq, g, None, q[:6 if fetch > 256 else 20], K, topk, fetch, 0.5, what="relaid out")
        assert np.isin(new, g.map_ids).all()
    finally:
        g.close()


def test_sparse_ids_take_the_hash_directory(rq, big):
    _, _, q = make_data()
    sparse = lambda i: (7 * np.asarray(i, dtype=np.uint64) + (1 << 31)).astype(np.uint32)
    g = rq.RaBitQ.from_arrays(big.base, big.orthogonal, big.centroids, big.offsets, sparse(big.map_ids), big.codes, big.factors)
    try:
        for topk, fetch, nq in ((10, 64, 20), (7, 257, 20), (100, 2048, 5)):
            check_query(rq, g, None, q[:nq], K, topk, fetch, 0.5, what="hash")
        assert rq.last_by_id_stats()["form"] == "hash"
        rng = np.random.default_rng(9)
        absent = np.array([5, (1 << 31) + 1, 0xFFFFFFFF, sparse(N), 0], dtype=np.uint32)     # between the stored ids, and past them
        posmap, base = stored(g, None)
        for F, topk in ((48, 5), (300, 20)):
            dist, ids, cnt = made_rows(rng, g.map_ids, 6, F, absent)
            res, st = device_diversify(rq, g, dist, ids, cnt, topk, 0.5)
            want = same(res, (dist, ids, cnt), posmap, base, topk, 0.5, ("hash, made rows", F), stats=st)
            assert want["absent"] > 0
    finally:
        g.close()


# ---- 4. metrics, row types, a shard, a tiered index --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cosine", "ip", "f16", "u8", "shard", "tiered"])
def test_metrics_row_types_a_shard_and_a_tiered_index(rq, kind):
    from rabitq_amd import index as ix
    x, centres, q = make_data()
    P = synth.random_orthogonal(128 if kind == "ip" else D, seed=79)
    if kind in ("cosine", "ip"):
        g = rq.RaBitQ.build(x, centres, P, metric=kind)
    elif kind == "f16":
        g = rq.RaBitQ.build(x.astype(np.float16), centres, P, rows="f16")
    elif kind == "u8":
        g = rq.RaBitQ.build(np.clip(np.rint(x * 40.0 + 128.0), 0, 255).astype(np.uint8), centres * 40.0 + 128.0, P, rows="u8")
        q = q * np.float32(40.0) + np.float32(128.0)
    elif kind == "tiered":
        ix.set_option("base_device_mb", 1)                                     # n * dim * 4 = 1.5 MB
        try:
            x, centres, _ = make_data(6000, seed=801)
            g = rq.RaBitQ.build(x, centres, P)
        finally:
            ix.set_option("base_device_mb", -1)
        if not g.n_hbm < g.n:
            g.close()
            pytest.fail("the index was meant to be tiered")
    else:
        g = rq.RaBitQ.build(x, centres, P)
    held = [g]
    try:
        if kind == "shard":
            owner, _ = g.partition_lists(2)
            g = g.shard(owner, 0)
            held.append(g)
            assert 0 < g.n < N
        for topk, fetch, lam in ((10, 64, 0.5), (7, 257, 0.3)):
            check_query(rq, g, None, q[:16], K, topk, fetch, lam, what=kind)
        posmap, base = stored(g, None)
        if kind == "tiered":                                                   # the exact form is refused wherever rq_exact_search is
            with pytest.raises(rq.RabitqError) as e:
                g.exact_search_diverse(q[:4], 2, fetch=8)
            assert e.value.status == UNSUPPORTED and "tiered" in str(e.value)
        else:
            res = g.exact_search_diverse(q[:10], 10, lam=0.5, fetch=100)
            same(res, g.exact_search(q[:10], 100), posmap, base, 10, 0.5, (kind, "exact"), fetch=100)
    finally:
        for h in held[::-1]:
            h.close()


# ---- 5. truth ----------------------------------------------------------------------------------------------------------------------------
def test_exact_diverse_over_every_row_against_a_brute_force(rq):
    """n = 1500 < fetch = 2048: every query fetches every row, so the source of the model can be a brute force -- the distance of
    every row (the bits exact_search returns), all ids -- and the pair distances the oracle's over the given rows."""
    n, topk = 1500, 12
    x, _, q = make_data(n)
    g = build(rq, n)
    try:
        nq = 4
        d, i, c = g.exact_search(q[:nq], n)
        assert (c == n).all() and np.array_equal(np.sort(i, axis=1), np.tile(np.arange(n, dtype=np.uint32), (nq, 1)))
        brute_d = np.zeros((nq, 2048), dtype=np.float32)
        brute_i = np.zeros((nq, 2048), dtype=np.uint32)
        for b in range(nq):                                                    # in id order, not in the search's
            brute_d[b, i[b]] = d[b]
            brute_i[b, :n] = np.arange(n)
        base = np.ascontiguousarray(x[:n])                                     # an L2 f32 index stores the rows as given
        assert np.array_equal(brute_d[0, :5].view(np.uint32),
                              np.array([oracle.l2_squared_distance(base[r], q[0]) for r in range(5)], dtype=np.float32).view(np.uint32))
        posmap = {int(v): p for p, v in enumerate(g.map_ids)}
        assert np.array_equal(stored(g, None)[1][[posmap[r] for r in range(n)]], base)
        res = g.exact_search_diverse(q[:nq], topk, lam=0.5, fetch=2048)
        assert (res.fetched == n).all() and (res.counts == topk).all()
        same(res, (brute_d, brute_i, np.full(nq, n, dtype=np.uint32)), {r: r for r in range(n)}, base, topk, 0.5, "brute force")
    finally:
        g.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(rq, big):
    _, _, q = make_data()
    x, _, _ = make_data()

    def refused(status, text, fn):
        with pytest.raises(rq.RabitqError) as e:
            fn()
        assert e.value.status == status and text in str(e.value), (status, text, str(e.value))

    g = build(rq, 300)
    try:
        for call in (lambda **kw: g.query_batch_diverse(q[:4], 4, **kw), lambda **kw: g.exact_search_diverse(q[:4], **kw)):
            refused(UNSUPPORTED, "topk <= fetch <= 2048", lambda: call(topk=9, fetch=8))
            refused(UNSUPPORTED, "topk <= fetch <= 2048", lambda: call(topk=5, fetch=2049))
            refused(UNSUPPORTED, "at least 1", lambda: call(topk=0, fetch=8))
            for lam in (-0.1, 1.1, float("nan")):
                refused(INVALID, "lambda must be in [0, 1]", lambda: call(topk=2, fetch=8, lam=lam))
        refused(INVALID, "lambda", lambda: g.diversify_results(np.zeros((2, 8), np.float32), np.zeros((2, 8), np.uint32), np.zeros(2, np.uint32), 2, lam=2.0))
        refused(UNSUPPORTED, "topk <= fetch", lambda: g.diversify_results(np.zeros((2, 8), np.float32), np.zeros((2, 8), np.uint32), np.zeros(2, np.uint32), 9))
        # a filter of another generation, and of another index
        f = g.make_filter(ids=np.arange(100))
        other = big.make_filter(ids=np.arange(100))
        refused(INVALID, "another index", lambda: g.query_batch_diverse(q[:4], 4, 2, fetch=8, filter=other))
        g.add(x[300:305])
        refused(INVALID, "last mutated", lambda: g.query_batch_diverse(q[:4], 4, 2, fetch=8, filter=f))
        refused(INVALID, "last mutated", lambda: g.exact_search_diverse(q[:4], 2, fetch=8, filter=f))
        f.close(), other.close()
        # the directory is made by the first call after a relayout
        g.query_batch_diverse(q[:4], K, 2, fetch=8)
        assert rq.last_diverse_stats()["directory_built"] == 1
        g.query_batch_diverse(q[:4], K, 2, fetch=8)
        assert rq.last_diverse_stats()["directory_built"] == 0
    finally:
        g.close()
