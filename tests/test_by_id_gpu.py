"""Rows by id on the GPU: rq_locate, rq_fetch_rows, rq_fetch_stored, rq_pair_distances, rq_neighbours_of[_exact] and
the id directory behind them, against numpy on the index's own arrays (tests/by_id_model.py).  Bit for bit everywhere: the only
tolerance in this file is the tie rule of the k-NN graph test, which compares against a float64 brute force.

Run on the GPU box:  python -m pytest tests/test_by_id_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import by_id_model as bm
from tests import synth
from tests.models import ARRAYS, bits

pytestmark = pytest.mark.gpu

N, K = 6000, 16
INVALID, UNSUPPORTED = -1, -6
ABSENT = bm.ABSENT
TWIN_A, TWIN_B = 17, 4321          # two stored rows that are bitwise equal (make_data)


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def ceil64(v):
    return (v + 63) // 64 * 64


_DATA = {}


def make_data(rows, d, n=N, seed=300):
    """-> (x as the build takes it, centres, P is made by the caller, raw f32 queries): a mixture, scaled into the type's range for
    byte rows; rows TWIN_A and TWIN_B are equal."""
    key = (rows, d, n, seed)
    if key not in _DATA:
        xf, centres, _ = synth.mixture(n, d, K, sigma=0.8, seed=seed, centre_scale=0.6)
        qf, _, _ = synth.mixture(64, d, K, sigma=0.8, seed=seed + 1, centre_scale=0.6)
        if n > TWIN_B:
            xf[TWIN_B] = xf[TWIN_A]
        if rows == "u8":
            x, centres, qf = np.clip(np.rint(xf * 40.0 + 128.0), 0, 255).astype(np.uint8), centres * 40.0 + 128.0, qf * 40.0 + 128.0
        elif rows == "i8":
            x, centres, qf = np.clip(np.rint(xf * 40.0), -128, 127).astype(np.int8), centres * 40.0, qf * 40.0
        elif rows == "f16":
            x = xf.astype(np.float16)
        elif rows == "bf16":
            x = (np.ascontiguousarray(xf).view(np.uint32) >> 16).astype(np.uint16)
        else:
            x = xf
        _DATA[key] = (x, centres.astype(np.float32), qf.astype(np.float32))
    return _DATA[key]


def make_index(rq, rows, metric, d, n=N, seed=300):
    x, centres, q = make_data(rows, d, n, seed)
    dim = ceil64(d + 1) if metric == "ip" else ceil64(d)
    P = synth.random_orthogonal(dim, seed=seed + 2)
    g = rq.RaBitQ.build(x, centres, P, metric=metric, rows=None if rows == "f32" else rows)
    assert g.dim == dim and g.n == n and g.row_type == rows and g.metric == metric
    return g, x, centres, P, q


def request(rng, map_ids, m, absent_below_top=()):
    """m ids: stored ones with duplicates, ids at or above top (2^32 - 1 among them), and, where the caller knows some, absent ids
    below top."""
    top = int(map_ids.max()) + 1 if len(map_ids) else 0
    ids = rng.choice(map_ids, size=m, replace=True).astype(np.uint32) if len(map_ids) else np.zeros(m, dtype=np.uint32)
    if m >= 7:
        ids[1] = ids[0]                                                       # a duplicate side by side, one far apart
        ids[m - 1] = ids[0]
        ids[2] = 0xFFFFFFFF
        ids[3] = min(top, 0xFFFFFFFF)
        ids[4] = min(top + 12345, 0xFFFFFFFF)
        if len(absent_below_top):
            ids[5] = absent_below_top[0]
    if m > 100:
        if top < 1 << 32:
            far = rng.integers(top, 1 << 32, size=m // 10, dtype=np.uint64).astype(np.uint32)
            ids[rng.choice(np.arange(7, m - 1), size=far.size, replace=False)] = far
        if len(absent_below_top):
            at = rng.choice(np.arange(7, m - 1), size=min(50, m // 20), replace=False)
            ids[at] = rng.choice(np.asarray(absent_below_top, dtype=np.uint32), size=at.size)
    return ids


def check_locate_fetch(rq, g, ids, live=None, what=""):
    """locate and fetch of `ids` against numpy on the index's arrays; -> the expected positions."""
    map_ids, base = g.map_ids, g.base
    want = bm.locate(map_ids, ids, live)
    got = g.locate(ids)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (what, "locate", np.nonzero(got != want)[0][:5])
    st = rq.last_by_id_stats()
    have = want != ABSENT
    assert (st["found"], st["absent"]) == (int(have.sum()), int((~have).sum())), (what, st)
    assert np.array_equal(g.contains(ids), have), what
    rows, found = g.fetch(ids, raw=False)
    exp = np.zeros((len(ids), g.dim), dtype=np.float32)
    exp[have] = base[want[have]]
    assert rows.shape == exp.shape and rows.dtype == np.float32 and np.array_equal(found, have), what
    assert np.array_equal(bits(rows), bits(exp)), (what, "fetch", np.nonzero((bits(rows) != bits(exp)).reshape(len(ids), -1).any(1))[0][:5])
    st = rq.last_by_id_stats()
    if len(ids) and g.n:
        row_bytes = g.dim * rq._lib.ROW_TYPE_BY_NAME[g.row_type].elem_bytes
        assert st["gather_bytes"] == int(have.sum()) * row_bytes + len(ids) * (g.dim * 4 + 4), (what, st)
    if g.metric == "ip":                                                      # raw=True: the augmented coordinate and the padding are cut off
        cut, _ = g.fetch(ids)
        assert cut.shape == (len(ids), g.ip_params[0]) and np.array_equal(bits(cut), bits(np.ascontiguousarray(exp[:, :g.ip_params[0]]))), what
    if g.row_type == "f32":
        with pytest.raises(rq.RabitqError) as e:                              # as rq_get_array(RQ_ARR_BASE_ROWS) on an f32 index
            g.fetch(ids, stored=True)
        assert e.value.status == INVALID
    else:
        stored = g.base_rows
        srows, sfound = g.fetch(ids, stored=True)
        sexp = np.zeros((len(ids), g.dim), dtype=stored.dtype)
        sexp[have] = stored[want[have]]
        assert srows.dtype == stored.dtype and np.array_equal(sfound, have) and np.array_equal(bits(srows), bits(sexp)), (what, "stored")
    return want


# ---- 1. locate and fetch against numpy: row types x metrics x row lengths x request sizes ----------------------------------------
COMBOS = [("f32", "l2"), ("f32", "cosine"), ("f32", "ip"), ("f16", "l2"), ("f16", "cosine"), ("bf16", "l2"), ("bf16", "cosine"),
          ("u8", "l2"), ("i8", "l2")]


@pytest.mark.parametrize("dim", [64, 128, 192, 320])     # a 64-byte byte row, a padded row (d = 100), a piece count that is no power of two, a row longer than one 64-lane step
@pytest.mark.parametrize("rows,metric", COMBOS)
def test_locate_and_fetch(rq, rows, metric, dim):
    d = 100 if dim == 128 else dim
    if metric == "ip":
        d = min(d, dim - 1)                                                   # dim = ceil64(d + 1)
    g, _, _, _, _ = make_index(rq, rows, metric, d)
    try:
        assert g.dim == dim
        rng = np.random.default_rng(dim + len(rows))
        map_ids = g.map_ids
        for m in (0, 1, 7, 4099):
            check_locate_fetch(rq, g, request(rng, map_ids, m), what=(rows, metric, dim, m))
            st = rq.last_by_id_stats()
            assert st["form"] == "dense" and st["directory_bytes"] == 4 * N and st["longest_chain"] == 0, st   # a built index: ids 0 .. n-1
        whole = np.arange(N, dtype=np.uint32)                                 # every id once, in id order: the inverse of map_ids
        assert np.array_equal(map_ids[g.locate(whole)], whole)
    finally:
        g.close()


# ---- 2. both directory forms, and their rebuild after every relayout -------------------------------------------------------------
def collision_ids(n_after, taken):
    """Ids up to 2^32 - 1 for an index that will hold n_after rows: three that share a home slot, three whose home is the table's
    last slot (their run wraps past its end), and 2^32 - 1 itself."""
    b = bm.hash_bits(n_after)
    cap = 1 << b
    share = bm.colliding_ids(b, 1234, 3, lo=1 << 31, taken=taken)
    wrap = bm.colliding_ids(b, cap - 1, 3, lo=3 << 30, taken=taken)
    ids = np.concatenate([share, wrap, np.array([0xFFFFFFFF], dtype=np.uint32)])
    assert len(set(ids.tolist())) == 7
    return ids, b


def test_hash_form_with_collisions(rq):
    g, x, _, _, _ = make_index(rq, "f32", "l2", 64)
    try:
        rng = np.random.default_rng(9)
        g.locate(np.arange(3, dtype=np.uint32))
        assert rq.last_by_id_stats()["form"] == "dense" and rq.last_by_id_stats()["built"] == 1
        new_ids, b = collision_ids(N + 7, g.map_ids)
        g.add(x[100:107] * np.float32(1.01), ids=new_ids)
        map_ids = g.map_ids
        assert g.n == N + 7 and int(map_ids.max()) == 0xFFFFFFFF
        assert not bm.is_dense(int(map_ids.max()) + 1, g.n)
        want = check_locate_fetch(rq, g, new_ids, what="the colliding ids")
        assert (want != ABSENT).all()
        st = rq.last_by_id_stats()
        assert st["form"] == "hash" and st["directory_bytes"] == 8 << b, st
        assert st["longest_chain"] >= 3, st                                   # three ids on one home slot: cannot pass without the collisions
        slots, chain = bm.build_table(map_ids, b)                             # the model's table: same capacity, same answers
        assert chain.max() >= 3
        occupied = np.nonzero(slots != np.uint64(bm.EMPTY))[0]
        assert occupied[0] <= 1 and occupied[-1] == (1 << b) - 1              # the last slot's run wrapped to the table's start
        for m in (0, 1, 7, 4099):
            ids = request(rng, map_ids, m, absent_below_top=np.array([N + 5, 1 << 31, (1 << 32) - 2], dtype=np.uint32))
            want = check_locate_fetch(rq, g, ids, what=("hash", m))
            assert np.array_equal(bm.table_lookup(slots, ids), want)
            assert rq.last_by_id_stats()["form"] == "hash"
        # ids that collide with the runs but are not stored: the walk ends at an empty slot
        miss = np.concatenate([bm.colliding_ids(b, 1234, 4, lo=1 << 30, hi=1 << 31, taken=map_ids), bm.colliding_ids(b, (1 << b) - 1, 4, lo=1 << 29, hi=1 << 30, taken=map_ids)])
        assert (g.locate(miss) == ABSENT).all()
    finally:
        g.close()


@pytest.mark.parametrize("form", ["dense", "hash"])
def test_directory_is_rebuilt_after_every_relayout(rq, form):
    """A stale directory would return the old layout's positions: after remove, add, merge_from and compact the answers are the new
    layout's, and the first by-id call after each reports a new directory."""
    g, x, centres, P, _ = make_index(rq, "f32", "l2", 64)
    other = rq.RaBitQ.build(x[:500] * np.float32(0.99), centres, P)
    try:
        rng = np.random.default_rng(21)
        if form == "hash":
            g.add(x[:1] * np.float32(1.02), ids=np.array([0xFFFFFFF0], dtype=np.uint32))
        gone = []

        def step(what, built=1):
            map_ids = g.map_ids
            ids = request(rng, map_ids, 777, absent_below_top=np.array(gone, dtype=np.uint32) if gone else ())
            want = bm.locate(map_ids, ids)
            got = g.locate(ids)
            st = rq.last_by_id_stats()
            assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:5])
            assert st["form"] == form and st["built"] == built, (what, st)
            check_locate_fetch(rq, g, ids, what=what)
            assert rq.last_by_id_stats()["built"] == 0, what                  # kept until the next relayout
            return ids, want

        ids0, pos0 = step("built")
        dead = rng.choice(N, size=900, replace=False).astype(np.uint32)
        assert g.remove(ids=dead) == 900
        gone += dead.tolist()
        step("after remove")
        moved = g.locate(ids0)                                                # the same request, the new layout
        assert np.array_equal(moved, bm.locate(g.map_ids, ids0)) and not np.array_equal(moved, pos0)
        back = dead[:300]
        g.add(x[back] * np.float32(1.03), ids=back)
        gone = [i for i in gone if i not in set(back.tolist())]
        step("after add")
        g.merge_from(other, ids=10_000)                                      # (ids that keep the dense form dense)
        assert g.n == N + (1 if form == "hash" else 0) - 900 + 300 + 500
        step("after merge_from")
        lazy = rng.choice(g.map_ids[g.map_ids < 1 << 31], size=400, replace=False).astype(np.uint32)
        assert g.remove(ids=lazy, lazy=True) == 400
        assert (g.locate(lazy) == ABSENT).all() and rq.last_by_id_stats()["built"] == 0   # marking rows dead keeps the directory
        assert g.compact() == 400
        gone += lazy.tolist()
        step("after compact")
    finally:
        g.close()
        other.close()


# ---- 3. other index kinds ------------------------------------------------------------------------------------------------------------
def prepared(rq, g, q):
    """The query as the rerank sees it: transformed and padded to dim."""
    if g.metric == "cosine":
        return rq.normalize(q)
    out = np.zeros((len(q), g.dim), dtype=np.float32)
    out[:, :q.shape[1]] = q
    return out


def rerank(rq, g, q_prepared, pos):
    out = np.empty(len(pos), dtype=np.float32)
    pos = np.ascontiguousarray(pos, dtype=np.uint32)
    q_prepared = np.ascontiguousarray(q_prepared, dtype=np.float32)
    rq._lib.check(rq._lib.lib().rq_rerank(g._h, C.c_void_p(q_prepared.ctypes.data), C.c_void_p(pos.ctypes.data), len(pos), C.c_void_p(out.ctypes.data)))
    return out


def check_distances(rq, g, q, ids, live=None, what=""):
    """distances_to == rq_rerank at locate's positions with the prepared query; +inf for an absent id."""
    got = g.distances_to(q, ids)
    pos = bm.locate(g.map_ids, ids.reshape(-1), live).reshape(ids.shape)
    qp = prepared(rq, g, q)
    want = np.full(ids.shape, np.inf, dtype=np.float32)
    for i in range(len(q)):
        have = pos[i] != ABSENT
        if have.any():
            want[i, have] = rerank(rq, g, qp[i], pos[i, have])
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (what, np.nonzero(bits(got).reshape(-1, 4).any(1) != bits(want).reshape(-1, 4).any(1))[0][:5])
    assert np.isinf(got[pos == ABSENT]).all() and (pos == ABSENT).any() and np.isfinite(got[pos != ABSENT]).all(), what


@pytest.mark.parametrize("kind", ["tiered", "split_rows"])
def test_tiered_and_split_rows(rq, kind):
    from rabitq_amd import index as ix
    x, centres, q = make_data("f32", 128)
    P = synth.random_orthogonal(128, seed=302)
    if kind == "tiered":
        ix.set_option("base_device_mb", 1)                                    # n * dim * 4 = 3 MB
    else:
        ix.set_option("split_rows", 2)
    try:
        g = rq.RaBitQ.build(x, centres, P)
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)
    try:
        assert g.n_hbm < N if kind == "tiered" else g.split_rows
        rng = np.random.default_rng(31)
        for m in (1, 7, 4099):
            check_locate_fetch(rq, g, request(rng, g.map_ids, m), what=(kind, m))      # fetch == rq_get_array(RQ_ARR_BASE) at the position
        ids = request(rng, g.map_ids, 5 * 9).reshape(5, 9)
        check_distances(rq, g, q[:5], ids, what=kind)
        d, i, found = g.neighbours_of(ids[0], 8, 5)                           # the approximate form works on both tiers and on split rows
        rows, f2 = g.fetch(ids[0])
        exp = bm.drop_self(*g.query_batch(rows, 8, 6), ids[0], f2)
        assert np.array_equal(found, f2) and np.array_equal(bits(d), bits(exp[0])) and np.array_equal(i, exp[1])
    finally:
        g.close()


@pytest.mark.parametrize("rows", ["f32", "u8"])
def test_pending_lazy_removals(rq, rows):
    g, _, _, _, q = make_index(rq, rows, "l2", 64)
    try:
        rng = np.random.default_rng(41)
        map_ids = g.map_ids
        ask = request(rng, map_ids, 600)
        before = (g.locate(ask), g.fetch(ask), g.neighbours_of(ask[:80], 8, 6))
        dead = rng.choice(N, size=1500, replace=False).astype(np.uint32)
        dead = dead[~np.isin(dead, ask)]                                       # the asked rows stay live ...
        dead = np.concatenate([dead, ask[10:14]])                              # ... but four of them
        dead = dead[dead < N]
        assert g.remove(ids=dead, lazy=True) == len(np.unique(dead))
        live = ~np.isin(map_ids, dead)
        assert (g.locate(dead) == ABSENT).all() and not g.contains(dead).any()
        r, f = g.fetch(dead)
        assert not f.any() and not r.any()
        st = rq.last_by_id_stats()
        assert st["built"] == 0 and st["found"] == 0 and st["absent"] == len(dead)     # the epoch is not part of the directory's validity
        check_locate_fetch(rq, g, ask, live=live, what="pending")
        now = g.locate(ask)
        keep = ~np.isin(ask, dead)
        assert np.array_equal(now[keep], before[0][keep]) and (now[~keep] == ABSENT).all()      # live ones unchanged
        ids = np.concatenate([ask[:40], dead[:5]]).reshape(5, 9)
        check_distances(rq, g, q[:5], ids, live=live, what="pending")
        d, i, found = g.neighbours_of(dead[:7], 8, 6)
        assert not found.any() and np.isnan(d).all() and (i == ABSENT).all()
        # a live row's neighbours are the plain call's under the live filter: no dead id among them
        d, i, found = g.neighbours_of(ask[:80], 8, 6)
        rws, f2 = g.fetch(ask[:80])
        exp = bm.drop_self(*g.query_batch(rws, 8, 7), ask[:80], f2)
        assert np.array_equal(found, f2) and np.array_equal(bits(d), bits(exp[0])) and np.array_equal(i, exp[1])
        assert not np.isin(i, dead).any()
        if rows != "f32":
            return
        pend = (g.fetch(ask), d, i, found)
        assert g.compact() == len(np.unique(dead))                            # after compact() nothing changes for live ids
        check_locate_fetch(rq, g, ask, what="compacted")
        again = g.fetch(ask)
        assert np.array_equal(bits(again[0]), bits(pend[0][0])) and np.array_equal(again[1], pend[0][1])
        d2, i2, f2 = g.neighbours_of(ask[:80], 8, 6)
        assert np.array_equal(bits(d2), bits(d)) and np.array_equal(i2, i) and np.array_equal(f2, found)
    finally:
        g.close()


def test_shard(rq):
    g, _, _, _, _ = make_index(rq, "f32", "l2", 64)
    owner, _ = g.partition_lists(2)
    s0, s1 = g.shard(owner, 0), g.shard(owner, 1)
    try:
        mine, theirs = s0.map_ids, s1.map_ids
        assert len(mine) and len(theirs) and len(mine) + len(theirs) == N
        assert (s0.locate(theirs) == ABSENT).all()                            # ids are global: the other shard's are absent here
        rng = np.random.default_rng(51)
        ids = np.concatenate([request(rng, mine, 500), theirs[:200]])
        want = check_locate_fetch(rq, s0, ids, what="shard 0")
        assert (want[500:] == ABSENT).all()
        whole, _ = g.fetch(ids[:500])
        part, _ = s0.fetch(ids[:500])
        have = want[:500] != ABSENT
        assert np.array_equal(bits(whole[have]), bits(part[have]))
    finally:
        s0.close(), s1.close(), g.close()


# ---- 4. distances_to -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,metric", [("f32", "l2"), ("f32", "cosine"), ("f32", "ip"), ("u8", "l2")])
def test_distances_to(rq, rows, metric):
    d = 99 if metric == "ip" else 100                                          # padded rows: dim 128
    g, _, _, _, q = make_index(rq, rows, metric, d)
    try:
        rng = np.random.default_rng(61)
        for B, c in ((1, 1), (5, 9), (3, 300)):
            ids = request(rng, g.map_ids, max(B * c, 7))[:B * c].reshape(B, c)
            if B * c == 1:
                check = g.distances_to(q[:1], ids)
                assert np.array_equal(bits(check), bits(rerank(rq, g, prepared(rq, g, q[:1])[0], g.locate(ids[0]))[None, :]))
            else:
                check_distances(rq, g, q[:B], ids, what=(rows, metric, B, c))
        assert g.distances_to(q[:0], np.zeros((0, 4), dtype=np.uint32)).shape == (0, 4)
    finally:
        g.close()


# ---- 5. neighbours_of ------------------------------------------------------------------------------------------------------------------
def expected_neighbours(g, ids, probe, topk, heur, filt, exact):
    rows, found = g.fetch(ids)                                                # [:L]: an inner-product index's rows are cut to its d
    if exact:
        plain = g.exact_search(rows, topk + 1, filter=filt)
    else:
        plain = g.query_batch(rows, probe, topk + 1, heur, filter=filt)
    return bm.drop_self(*plain, ids, found) + (found,)


def check_neighbours(g, ids, probe, topk, heur=False, filt=None, exact=False, what=""):
    d, i, found = g.neighbours_of(ids, probe, topk, filter=filt, heuristic_rank=heur, exact=exact)
    ed, ei, ef = expected_neighbours(g, ids, probe, topk, heur, filt, exact)
    assert np.array_equal(found, ef), what
    assert np.array_equal(i, ei), (what, np.nonzero((i != ei).any(1))[0][:5])
    assert np.array_equal(bits(d), bits(ed)), what
    return d, i, found


@pytest.mark.parametrize("rows,metric", [("f32", "l2"), ("f32", "cosine"), ("f32", "ip"), ("f16", "l2"), ("i8", "l2")])
def test_neighbours_of(rq, rows, metric):
    g, _, _, _, _ = make_index(rq, rows, metric, 63 if metric == "ip" else 64)
    try:
        rng = np.random.default_rng(71)
        map_ids = g.map_ids
        topk, probe = 10, 6
        for m in (1, 70, 2500):                                               # one row; above the small-batch path's 64; a batch whose scan runs on the matrix cores
            ids = rng.choice(map_ids, size=m, replace=False).astype(np.uint32)
            if m >= 70:
                ids[:6] = [TWIN_A, TWIN_B, 0xFFFFFFFF, N + 3, ids[6], TWIN_A]  # the bitwise-equal pair, two absent ids, duplicates
            for heur in (False, True):
                d, i, found = check_neighbours(g, ids, probe, topk, heur, what=(rows, metric, m, heur))
                assert not (i == ids[:, None])[found].any(), (rows, metric, m, heur)  # no row among its own neighbours
                if m >= 70:
                    assert list(found[:6]) == [True, True, False, False, True, True]
                    assert np.isnan(d[2:4]).all() and (i[2:4] == ABSENT).all()
                    if not heur and metric == "l2":                           # the twin is there, at the distance of the row to itself
                        assert TWIN_B in i[0] and TWIN_A in i[1] and d[0][list(i[0]).index(TWIN_B)] == d[1][list(i[1]).index(TWIN_A)]
        # a filter that excludes some of the asked ids themselves: such a row is absent from its own result and the last entry leaves
        ids = rng.choice(map_ids, size=70, replace=False).astype(np.uint32)
        allowed = np.ones(N, dtype=bool)
        allowed[ids[::2]] = False
        allowed[rng.choice(N, size=N // 3, replace=False)] = False
        allowed[ids[1::2]] = True
        with g.make_filter(mask=allowed) as f:
            for heur in (False, True):
                d, i, found = check_neighbours(g, ids, probe, topk, heur, filt=f, what=(rows, metric, "filtered", heur))
                assert found.all() and allowed[i[i != ABSENT]].all()
            plain = g.query_batch(g.fetch(ids)[0], probe, topk + 1, False, filter=f)
            assert not (plain[1][::2] == ids[::2, None]).any()                 # (an excluded row is absent from its own plain result)
            check_neighbours(g, ids, probe, topk, filt=f, exact=True, what=(rows, metric, "filtered exact"))
        # the exact form: ascending by (distance, id), so of the bitwise-equal pair the smaller id comes first in both rows
        ids = np.concatenate([np.array([TWIN_A, TWIN_B, 0xFFFFFFFF], dtype=np.uint32), rng.choice(map_ids, size=67, replace=False).astype(np.uint32)])
        d, i, found = check_neighbours(g, ids, probe, topk, exact=True, what=(rows, metric, "exact"))
        assert not found[2]
        if metric != "ip":                                                    # (an inner-product index's raw query is not its augmented row)
            assert i[0, 0] == TWIN_B and i[1, 0] == TWIN_A and bits(d[0, :1]).tobytes() == bits(d[1, :1]).tobytes()
    finally:
        g.close()


# ---- 6. the k-NN graph against a float64 brute force -----------------------------------------------------------------------------------
def test_knn_graph_exact(rq):
    n, d, topk = 2000, 64, 5
    x, centres, _ = synth.mixture(n, d, K, sigma=0.8, seed=500, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=501)
    g = rq.RaBitQ.build(x, centres, P)
    try:
        ids, nd, ni = g.knn_graph(probe=K, topk=topk, exact=True, chunk=768)   # (three chunks, the last one short)
        assert np.array_equal(ids, np.arange(n, dtype=np.uint32)) and nd.shape == ni.shape == (n, topk)
        x64 = x.astype(np.float64)
        d2 = np.concatenate([((x64[r0:r0 + 100, None, :] - x64[None, :, :]) ** 2).sum(-1) for r0 in range(0, n, 100)])
        np.fill_diagonal(d2, np.inf)
        order = np.argsort(d2, axis=1, kind="stable")[:, :topk + 1]
        near = np.take_along_axis(d2, order, axis=1)
        tied = (near[:, topk] - near[:, topk - 1]) <= 1e-5 * near[:, topk - 1]  # the sixth within 1e-5 relative of the fifth: the set is not defined
        assert tied.mean() <= 0.01, tied.mean()
        bad = [r for r in np.nonzero(~tied)[0] if set(ni[r].tolist()) != set(order[r, :topk].tolist())]
        assert not bad, (len(bad), bad[:5])
        assert (np.diff(nd, axis=1) >= 0).all()                               # ascending, as the exact search returns them
    finally:
        g.close()


# ---- 7. refusals are the plain entry's, and leave the index as it was ------------------------------------------------------------------
def snapshot(g):
    return {name: bits(getattr(g, name)).copy() for name in ARRAYS + ("map_ids",)}


def test_refusals(rq):
    from rabitq_amd import index as ix
    g, x, centres, P, q = make_index(rq, "f32", "l2", 128)
    try:
        ids = np.arange(10, dtype=np.uint32)
        snap, answer = snapshot(g), g.query_batch(q, 8, 10)
        rows, _ = g.fetch(ids)
        with pytest.raises(rq.RabitqError) as e1:
            g.query_batch(rows, 8, 2049)
        for exact in (False, True):
            with pytest.raises(rq.RabitqError) as e2:                         # topk + 1 over the plain limit
                g.neighbours_of(ids, 8, 2048, exact=exact)
            assert e2.value.status == e1.value.status == UNSUPPORTED
        with pytest.raises(rq.RabitqError) as e3:
            g.neighbours_of(ids, 0, 10)                                       # probe == 0: the plain entry's RQ_ERR_INVALID
        with pytest.raises(rq.RabitqError) as e4:
            g.query_batch(rows, 0, 11)
        assert e3.value.status == e4.value.status == INVALID
        d, i, f = check_neighbours(g, ids, 8, 2047, what="topk + 1 == 2048")  # the largest topk the plain entry takes at topk + 1
        assert f.all() and d.shape == (10, 2047) and not (i == ids[:, None]).any()
        for name, b in snapshot(g).items():
            assert np.array_equal(b, snap[name]), name
        again = g.query_batch(q, 8, 10)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(answer, again))
    finally:
        g.close()
    ix.set_option("base_device_mb", 1)
    try:
        t = rq.RaBitQ.build(x, centres, P)
    finally:
        ix.set_option("base_device_mb", -1)
    try:
        assert t.n_hbm < N
        ids = np.arange(10, dtype=np.uint32)
        base, answer = t.base.copy(), t.query_batch(q, 8, 10)
        rows, _ = t.fetch(ids)
        with pytest.raises(rq.RabitqError) as e1:
            t.exact_search(rows, 6)
        with pytest.raises(rq.RabitqError) as e2:                             # the exact form on a tiered index: the exact search's refusal
            t.neighbours_of(ids, 8, 5, exact=True)
        assert e1.value.status == e2.value.status == UNSUPPORTED and "tiered" in str(e2.value)
        assert np.array_equal(bits(t.base), bits(base))
        again = t.query_batch(q, 8, 10)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(answer, again))
    finally:
        t.close()
