"""Attribute columns on the GPU: columns, their values by id, how they follow their rows through every relayout, a
shard and a dump, predicates as filters, and the set algebra of filters -- against the numpy model of tests/attr_model.py.  A
predicate's filter is compared with the id-list filter of the model's id set (rq_filter_create, pinned to the oracle by
tests/test_filtered_gpu.py): same rows, same ids, and bit-identical answers of the query entries.

Run on the GPU box:  python -m pytest tests/test_attr_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import attr_model as M
from tests import synth
from tests.models import bits

pytestmark = pytest.mark.gpu

D, K, N = 64, 8, 3000
INVALID, IO, UNSUPPORTED = -1, -3, -6
SPARSE = lambda i: 7 * np.asarray(i, dtype=np.uint64) + (1 << 31)      # ids far apart: by-id calls take the hash directory


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


_DATA = {}


def make_data(n, seed=500, d=D):
    """rows, centres (list K - 1 far from every row: it stays empty), queries"""
    if (n, seed, d) not in _DATA:
        x, centres, _ = synth.mixture(n, d, K - 1, sigma=0.8, seed=seed, centre_scale=0.6)
        centres = np.vstack([centres, np.full((1, d), 1000.0, dtype=np.float32)])
        q, _, _ = synth.mixture(100, d, K - 1, sigma=0.8, seed=seed + 1, centre_scale=0.6)
        _DATA[(n, seed, d)] = (x, centres, q)
    return _DATA[(n, seed, d)]


def build(rq, n, seed=500, **kw):
    x, centres, _ = make_data(n, seed)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(D, seed=77), **kw)
    off = g.offsets
    assert g.n == n and g.k == K and off[K] == off[K - 1], "list K - 1 is empty"
    return g


def values_by_id(n, seed=1):
    """{column: (dtype, values by id 0 .. n - 1)}: small ranges so that every op selects something, and the edge values.  One column of
    each type, and two more 4-byte ones (v, w) for a predicate over five columns none of which is 8 bytes wide."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 50, size=n).astype(np.uint32)
    i = rng.integers(-20, 20, size=n).astype(np.int32)
    f = (rng.integers(-6, 7, size=n) * 0.5).astype(np.float32)
    U = (rng.integers(0, 53, size=n).astype(np.uint64) + np.uint64(2**32 - 3))
    I = rng.integers(-2**33, 2**33, size=n).astype(np.int64)
    for arr, edge in ((u, [0xFFFFFFFF, 0x80000000, 0]), (i, [-1, -2**31, 2**31 - 1]), (f, [np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan]),
                      (U, [2**64 - 1, 2**63, 2**32, 1]), (I, [-1, -2**63, 2**63 - 1, 2**32 + 1])):
        at = rng.choice(n, size=min(n, 3 * len(edge)), replace=False)
        arr[at] = np.array(edge * 3, dtype=arr.dtype)[:at.size]
    v = rng.integers(0, 100, size=n).astype(np.uint32)                       # (drawn last: the five columns above are what they were)
    w = rng.integers(-3, 4, size=n).astype(np.int32)
    for arr, edge in ((v, [0xFFFFFFFF, 0]), (w, [-2**31, 2**31 - 1])):
        at = rng.choice(n, size=min(n, 3 * len(edge)), replace=False)
        arr[at] = np.array(edge * 3, dtype=arr.dtype)[:at.size]
    return {"u": ("u32", u), "i": ("i32", i), "f": ("f32", f), "U": ("u64", U), "I": ("i64", I), "v": ("u32", v), "w": ("i32", w)}


def fill_columns(g, cols, ids):
    for name, (dtype, vals) in cols.items():
        g.create_attr(name, dtype, fill=0)
        assert g.set_attr(name, ids, vals) == 0


@pytest.fixture(scope="module")
def big(rq):
    g = build(rq, N)
    cols = values_by_id(N)
    fill_columns(g, cols, np.arange(N))
    yield g, cols
    g.close()


def model_ids(cols, expr, ids=None):
    """the ids the model admits for a predicate over values held by id (ids: what row j's id is; default j)"""
    from rabitq_amd import where as W
    terms, prog = W.compile_expr(expr)
    keep = M.where(cols, [(t.column, t.op, t.a, t.b, t.values) for t in terms], prog)
    at = np.nonzero(keep)[0]
    return (at if ids is None else np.asarray(ids)[at]).astype(np.uint32)


def same_answers(g, f, y, queries, what):
    """every query entry answers the same under the two filters: ids, distance bits, counts"""
    for q, probe, topk in ((queries, 4, 10), (queries[:16], K, 5)):          # the staged launches; a batch of <= 64 queries
        a, b = g.query_batch(q, probe, topk, filter=f), g.query_batch(q, probe, topk, filter=y)
        for u, v in zip(a, b):
            assert np.array_equal(bits(u), bits(v)), (what, "query_batch", len(q))
    a, b = g.range_search(queries[:20], 4, 95.0, filter=f), g.range_search(queries[:20], 4, 95.0, filter=y)
    for u, v in zip(a, b):
        assert np.array_equal(bits(u), bits(v)), (what, "range_search")
    a, b = g.exact_search(queries[:8], 10, filter=f), g.exact_search(queries[:8], 10, filter=y)
    for u, v in zip(a, b):
        assert np.array_equal(bits(u), bits(v)), (what, "exact_search")
    return int(a[2].sum())


def predicates():
    from rabitq_amd import col
    u, i, f, U, I, v, w = col("u"), col("i"), col("f"), col("U"), col("I"), col("v"), col("w")
    nan = float("nan")
    return {
        "u_eq": u == 3, "u_ne": u != 3, "u_lt": u < 10, "u_le": u <= 10, "u_gt": u > 40, "u_ge": u >= 40, "u_between": u.between(5, 9),
        "u_in17": u.isin(range(1, 35, 2)), "u_any": u.any_bits(6), "u_all": u.all_bits(6), "u_max": u == 0xFFFFFFFF,
        "u_high": u > 0x7FFFFFFF, "u_empty_between": u.between(7, 6),
        "i_eq_m1": i == -1, "i_lt0": i < 0, "i_ge": i >= -5, "i_between": i.between(-3, 3), "i_in4096": i.isin(range(-2048, 2048)),
        "i_sign_bit": i.all_bits(-2**31), "i_ne_min": i != -2**31, "i_le_min": i <= -2**31, "i_gt": i > 2**31 - 2,
        "f_eq0": f == 0.0, "f_eq_m0": f == -0.0, "f_ne_nan": f != nan, "f_eq_nan": f == nan, "f_lt": f < 1.0, "f_le": f <= -0.0,
        "f_gt_inf": f > np.inf, "f_ge": f >= 2.5, "f_between": f.between(-1.5, 2.0), "f_in": f.isin([nan, 0.0, 2.5]), "f_ne": f != 0.5,
        "f_between_inf": f.between(-np.inf, np.inf),
        "U_eq": U == 2**32 + 1, "U_ge": U >= 2**32, "U_between": U.between(2**32, 2**63), "U_in1": U.isin([2**64 - 1]),
        "U_in": U.isin([2**64 - 1, 2**32, 5]), "U_any": U.any_bits(2**32), "U_lt": U < 2**32, "U_ne": U != 1,
        "I_lt0": I < 0, "I_eq_m1": I == -1, "I_gt": I > 2**32, "I_between": I.between(-2**33, -1), "I_all": I.all_bits(2**32 + 1),
        "I_le_min": I <= -2**63, "I_in": I.isin([-1, 2**63 - 1, 12345]),
        "and2": (u < 10) & (i < 0), "or_not": ~(u < 10) | (f >= 1.0), "nested": ((u == 3) | (i == -1)) & ~((f < 0.0) | (U >= 2**32)),
        "not_not": ~~(I < 0), "and3": (u < 25) & (i >= 0) & (f <= 1.0), "all5": (u < 40) & (i > -15) & (f < 3.0) & (U > 5) & (I != 0),
        "all5_narrow": (u < 40) & (i > -15) & (f < 3.0) & (v != 3) & (w >= -2),         # where_kernel<8, false>: five 4-byte columns
        "xor": ((u < 25) & ~(i < 0)) | (~(u < 25) & (i < 0)), "none": (u < 5) & (u > 45), "every": (u < 5) | ~(u < 5),
    }


@pytest.mark.parametrize("name", sorted(predicates()))
def test_predicate_filter_equals_the_id_list_filter(rq, big, name):
    g, cols = big
    _, _, queries = make_data(N)
    expr = predicates()[name]
    want = model_ids(cols, expr)
    with g.where(expr) as f, g.make_filter(ids=want) as y:
        assert f.rows == y.rows == want.size, (name, f.rows, want.size)
        got = f.ids()
        assert got.dtype == np.uint32 and np.array_equal(np.sort(got), want), name
        mids = g.map_ids
        assert np.array_equal(got, mids[np.isin(mids, want)]), (name, "ids() is in position order")
        returned = same_answers(g, f, y, queries, name)
        assert (returned > 0) == (want.size > 0), name


def test_where_stats_and_the_raw_entry(rq, big):
    """rq_last_where_stats; program == NULL is the AND of all terms; no term admits every row; a program that needs depth 32."""
    from rabitq_amd import _lib, col
    g, cols = big
    with g.where((col("u") < 10) & (col("U") >= 2**32) & (col("u") != 3)) as f:
        st = rq.last_where_stats()
        assert (st["columns"], st["rows"], st["admitted"], st["bytes_read"]) == (2, N, f.rows, N * 12), st
        assert st["ms_eval"] > 0 and st["ms_finish"] > 0
    L = _lib.lib()

    def raw(terms, program):
        arr = (_lib.WhereTermT * max(1, len(terms)))()
        for t, (column, op, a) in zip(arr, terms):
            t.column, t.op, t.a.u64 = column, op, a
        prog = np.asarray(list(program or []) + [0], dtype=np.uint8)
        h = C.c_void_p()
        _lib.check(L.rq_filter_create_where(g._h, arr, len(terms), C.c_void_p(prog.ctypes.data) if program is not None else None,
                                            len(program) if program is not None else 0, C.byref(h)))
        return rq.Filter(g, h)

    names = [a["name"] for a in g.attrs()]
    u, i = names.index("u"), names.index("i")
    uv, iv = cols["u"][1], cols["i"][1]
    with raw([(u, M.LT, 30), (i, M.GE, 0), (u, M.NE, 7)], None) as f:
        assert np.array_equal(np.sort(f.ids()), np.nonzero((uv < 30) & (iv >= 0) & (uv != 7))[0])
    with raw([], None) as f:
        assert f.rows == N and np.array_equal(f.ids(), g.map_ids)
        assert rq.last_where_stats()["columns"] == 0
    terms = [(u, M.EQ, v) for v in range(32)]
    with raw(terms, list(range(32)) + [M.TOK_OR] * 31) as f:                 # 32 pushes, then 31 ORs
        assert np.array_equal(np.sort(f.ids()), np.nonzero(uv < 32)[0])
    with raw(terms, [0] + [t for v in range(1, 32) for t in (v, M.TOK_OR)]) as f:
        assert np.array_equal(np.sort(f.ids()), np.nonzero(uv < 32)[0])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 8191, 8192, 8193, 16385])
def test_bitmap_tail_words(rq, n):
    """n around the 64-position runs: the predicate's bitmap, its complement and the id list at the last words; and around the 8192
    positions of one block of ids(): the smallest sizes at which the id list is joined from two and from three blocks."""
    from rabitq_amd import col
    g = build(rq, n)
    g.create_attr("v", "u64", fill=2**40)
    ids = np.arange(n)
    assert g.set_attr("v", ids[::2], ids[::2]) == 0                          # odd ids keep the fill
    v = np.where(ids % 2 == 0, ids, 2**40).astype(np.uint64)
    assert np.array_equal(g.attr_array("v"), v[g.map_ids])
    for expr, keep in ((col("v") < 2**40, v < 2**40), (col("v") >= n - 1, v >= n - 1), (col("v") == 2**40, v == 2**40)):
        with g.where(expr) as f, ~f as nf, (f | nf) as both, (f & nf) as none:
            assert np.array_equal(np.sort(f.ids()), ids[keep]) and f.rows == keep.sum()
            assert np.array_equal(np.sort(nf.ids()), ids[~keep]) and nf.rows == n - keep.sum()
            assert both.rows == n and none.rows == 0 and none.ids().size == 0
            mids = g.map_ids
            assert np.array_equal(both.ids(), mids) and np.array_equal(f.ids(), mids[keep[mids]]) and np.array_equal(nf.ids(), mids[~keep[mids]])
            assert np.array_equal(f.id_bits(n + 3), np.concatenate([keep, [False] * 3]))
            assert np.array_equal(nf.id_bits(), (~keep)[:nf.id_bits().size]) and not (~keep)[nf.id_bits().size:].any()
    g.close()


def test_sparse_ids_take_the_hash_directory(rq):
    from rabitq_amd import col
    g0 = build(rq, N)
    ids = SPARSE(g0.map_ids).astype(np.uint32)
    g = rq.RaBitQ.from_arrays(g0.base, g0.orthogonal, g0.centroids, g0.offsets, ids, g0.codes, g0.factors)
    g.create_attr("t", "i32", fill=-7)
    rng = np.random.default_rng(3)
    vals = rng.integers(-100, 100, size=N).astype(np.int32)
    all_ids = SPARSE(np.arange(N)).astype(np.uint32)
    ask = np.concatenate([all_ids, [5, 2**31 + 1, 0xFFFFFFFF], all_ids[:10]])          # absent ids; ten ids twice: the last value wins
    new = np.concatenate([vals, [1, 2, 3], vals[:10] + 1000])
    assert g.set_attr("t", ask, new) == 3
    assert rq.last_by_id_stats()["form"] == "hash"
    want = vals.copy()
    want[:10] += 1000
    got, found = g.get_attr("t", ask[:N + 3])
    assert np.array_equal(found, [True] * N + [False] * 3) and np.array_equal(got, np.concatenate([want, [-7] * 3]))
    assert np.array_equal(g.attr_array("t"), want[(g.map_ids.astype(np.int64) - 2**31) // 7])
    with g.where(col("t") >= 1000) as f:
        assert f.rows > 0 and np.array_equal(np.sort(f.ids()), all_ids[want >= 1000])
        assert not f.id_bits(4096).any()                                      # every admitted id is past nbits
    g.close()
    g0.close()


def check_columns(g, m, what, dead=()):
    """get_attr over all live ids (and some that are not there) equals the model; attr_array is aligned with map_ids"""
    live = np.array(sorted(m.ids), dtype=np.uint32)
    gone = np.array(list(dead) + [0xFFFFFFF0, 123456789], dtype=np.uint32)
    assert [a["name"] for a in g.attrs()] == list(m.cols), what
    mids = g.map_ids
    alive = np.isin(mids, live)
    assert alive.sum() == live.size and (len(dead) or alive.all()), what
    for name, (dtype, fill, _) in m.cols.items():
        info = [a for a in g.attrs() if a["name"] == name][0]
        assert info["dtype"] == dtype and bits(np.array([info["fill"]], dtype=M.DTYPES[dtype])).tolist() == bits(np.array([fill])).tolist(), (what, name)
        assert info["bytes"] == g.n * np.dtype(M.DTYPES[dtype]).itemsize
        ask = np.concatenate([live, gone])
        got, found = g.get_attr(name, ask)
        want, wfound = m.get(name, ask)
        assert np.array_equal(found, wfound) and not found[live.size:].any(), (what, name, "found")
        assert np.array_equal(bits(got), bits(want)), (what, name, np.nonzero(got != want)[0][:5])
        arr = g.attr_array(name)
        assert arr.shape == (g.n,) and np.array_equal(bits(arr[alive]), bits(m.array(name, mids[alive]))), (what, name, "attr_array")


def test_columns_follow_their_rows(rq):
    x, centres, _ = make_data(N)
    P = synth.random_orthogonal(D, seed=77)
    g = rq.RaBitQ.build(x[:2000], centres, P)
    m = M.Columns(range(2000))
    rng = np.random.default_rng(11)
    for name, dtype, fill in (("t", "u32", 7), ("w", "f32", -0.0), ("big", "u64", 2**40 + 1)):
        g.create_attr(name, dtype, fill=fill)
        m.create(name, dtype, fill)
    ids = rng.choice(2000, size=1500, replace=False)
    for name, vals in (("t", rng.integers(0, 2**32, size=1500)), ("w", rng.standard_normal(1500).astype(np.float32)),
                       ("big", rng.integers(0, 2**64, size=1500, dtype=np.uint64))):
        assert g.set_attr(name, ids, vals) == 0
        m.set(name, ids, vals)
    check_columns(g, m, "set")
    # add: the new rows hold the fill values; the gather's bytes count the columns
    new = g.add(x[2000:2300])
    m.add(new)
    from rabitq_amd import index as ix
    st = ix.last_mutate_stats()
    assert st["gather_bytes"] == 2 * g.n * (D * 4 + 8 + 16 + 4 + 4) + g.n * 4 + 2 * g.n * (4 + 4 + 8), st
    check_columns(g, m, "add")
    g.set_attr("t", new[:100], np.arange(100))
    m.set("t", new[:100], np.arange(100))
    # eager remove
    out = rng.choice(2300, size=400, replace=False)
    assert g.remove(ids=out) == 400
    m.remove(out)
    check_columns(g, m, "remove", dead=out[:50])
    # lazy remove: the dead ids are absent, the stored rows stay; set skips a dead id
    live = np.array(sorted(m.ids))
    lazy = rng.choice(live, size=300, replace=False)
    assert g.remove(ids=lazy, lazy=True) == 300
    m.remove(lazy)
    assert g.set_attr("t", lazy[:5], [1, 2, 3, 4, 5]) == 5
    check_columns(g, m, "lazy remove", dead=lazy[:50])
    still = [int(v) for v in live[:200] if int(v) in m.ids]                 # values can be set while removals are pending
    assert g.set_attr("w", live[:200], np.full(200, 2.5)) == 200 - len(still)
    m.set("w", still, [2.5] * len(still))
    assert g.compact() == 300
    check_columns(g, m, "compact", dead=lazy[:50])
    # merge_from: a source with column t (its values and its fill), without w and big (dst's fill), with a column only it has
    src = rq.RaBitQ.build(x[2300:2700], centres, P)
    ms = M.Columns(range(400))
    for name, dtype, fill in (("only_src", "i64", -1), ("t", "u32", 99)):
        src.create_attr(name, dtype, fill=fill)
        ms.create(name, dtype, fill)
    src.set_attr("t", np.arange(0, 400, 2), np.arange(200) + 5000)
    ms.set("t", np.arange(0, 400, 2), np.arange(200) + 5000)
    shift = g.merge_from(src, ids=10000)
    m.merge_from(ms, shift)
    check_columns(g, m, "merge (src has t)")
    check_columns(src, ms, "merge source untouched")
    bare = rq.RaBitQ.build(x[2700:2900], centres, P)                          # no column at all
    shift = g.merge_from(bare, ids=20000)
    m.merge_from(M.Columns(range(200)), shift)
    check_columns(g, m, "merge (src without columns)")
    clash = rq.RaBitQ.build(x[2900:3000], centres, P)
    clash.create_attr("w", "i32", fill=1)                                     # f32 in dst
    before = (g.n, g.map_ids.copy(), g.attr_array("w").copy())
    with pytest.raises(rq.RabitqError) as e:
        g.merge_from(clash, ids=30000)
    assert e.value.status == INVALID and "type of column w" in str(e.value)
    assert g.n == before[0] and np.array_equal(g.map_ids, before[1]) and np.array_equal(bits(g.attr_array("w")), bits(before[2]))
    assert clash.n == 100 and clash.attrs()[0]["dtype"] == "i32"
    # extract, copy: the new index has every column
    live = np.array(sorted(m.ids))
    take = rng.choice(live, size=700, replace=False)
    e = g.extract(ids=np.concatenate([take, [999999]]))
    check_columns(e, m.extract(take), "extract")
    c = g.copy()
    check_columns(c, m.copy(), "copy")
    c.set_attr("t", live[:10], np.zeros(10))                                  # the copy's columns are its own
    check_columns(g, m, "after the copy was written")
    # shards: each owned list's slice of every column
    owner, _ = g.partition_lists(2)
    total = 0
    for rank in range(2):
        sh = g.shard(owner, rank)
        mids = sh.map_ids
        total += sh.n
        check_columns(sh, m.extract(mids), f"shard {rank}")
        other = live[~np.isin(live, mids)][:20]
        assert not sh.get_attr("t", other)[1].any()
        sh.close()
    assert total == g.n
    for ix in (e, c, clash, bare, src, g):
        ix.close()


FIVE = ["base.fvecs", "centroids.fvecs", "factors.fvecs", "offsets_ids.ivecs", "orthogonal.fvecs", "x_binary_vec.u64vecs"]


def test_dump_and_load(rq, tmp_path):
    g = build(rq, 1000)
    bare_dir = tmp_path / "bare"
    g.dump_to_dir(str(bare_dir))
    assert sorted(os.listdir(bare_dir)) == FIVE                               # an index without columns: the files it wrote before
    cols = values_by_id(1000, seed=4)
    for name, (dtype, vals) in cols.items():
        g.create_attr(name, dtype, fill={"f": -0.0, "I": -5, "U": 2**64 - 1}.get(name, 3))
        g.set_attr(name, np.arange(0, 1000, 3), vals[::3])
    d = tmp_path / "full"
    g.dump_to_dir(str(d))
    assert sorted(os.listdir(d)) == sorted(FIVE + ["attrs"] + ["attr." + n for n in cols])
    text = open(d / "attrs").read()
    assert text.splitlines()[0] == "u 0 0000000000000003" and text.splitlines()[2] == "f 2 0000000080000000"
    assert text.splitlines()[3] == "U 3 ffffffffffffffff" and text.endswith("\n")
    assert os.path.getsize(d / "attr.u") == 4000 and os.path.getsize(d / "attr.I") == 8000
    assert np.array_equal(np.fromfile(d / "attr.I", dtype="<i8"), g.attr_array("I"))
    back = rq.RaBitQ.load_from_dir(str(d))
    assert back.attrs() == g.attrs() and [a["name"] for a in back.attrs()] == list(cols)
    assert np.array_equal(back.map_ids, g.map_ids)
    for name in cols:
        assert np.array_equal(bits(back.attr_array(name)), bits(g.attr_array(name))), name
    v, f = back.get_attr("f", [1, 5000])                                      # an unset row and an absent id: the fill, -0.0 bit for bit
    assert bits(v).tolist() == bits(np.array([-0.0, -0.0], dtype=np.float32)).tolist() and f.tolist() == [True, False]
    back.close()
    with pytest.raises(rq.RabitqError) as e:                                  # JSON is the debugging format
        g.dump_to_json(str(tmp_path / "x.json"))
    assert e.value.status == UNSUPPORTED

    def broken(change):
        change()
        with pytest.raises(rq.RabitqError) as e:
            rq.RaBitQ.load_from_dir(str(d))
        assert e.value.status == IO, str(e.value)

    full = open(d / "attr.U", "rb").read()
    broken(lambda: open(d / "attr.U", "wb").write(full[:-1]))                 # truncated
    broken(lambda: open(d / "attr.U", "wb").write(full + b"\0"))              # too long
    broken(lambda: os.remove(d / "attr.U"))                                   # missing
    open(d / "attr.U", "wb").write(full)
    for bad in ("u 0 3\n", "u 9 0000000000000003\n", "u-x 0 0000000000000003\n", "u 0 000000000000000g\n", "u 0\n", "u 0 0000000100000003\n",
                text + "u 0 0000000000000003\n", text.rstrip("\n")):
        broken(lambda: open(d / "attrs", "w").write(bad))
    open(d / "attrs", "w").write(text)
    rq.RaBitQ.load_from_dir(str(d)).close()                                   # whole again
    for name in list(cols):
        g.drop_attr(name)
    g.dump_to_dir(str(d))                                                     # a column-less dump into that directory drops `attrs`
    assert "attrs" not in os.listdir(d)
    back = rq.RaBitQ.load_from_dir(str(d))
    assert back.attrs() == [] and back.n == 1000
    back.close()
    g.close()


def test_filter_algebra_and_delete_where(rq):
    from rabitq_amd import col
    g = build(rq, N)
    cols = values_by_id(N, seed=8)
    fill_columns(g, {k: cols[k] for k in ("u", "i")}, np.arange(N))
    u, i = cols["u"][1], cols["i"][1]
    rng = np.random.default_rng(21)
    dead = rng.choice(N, size=500, replace=False)
    assert g.remove(ids=dead, lazy=True) == 500                               # removals pending: no filter admits a dead row
    live = np.ones(N, dtype=bool)
    live[dead] = False
    allow = rng.random(N) < 0.3
    A = set(np.nonzero((u < 20) & live)[0])
    B = set(np.nonzero(allow & live)[0])
    everything = set(np.nonzero(live)[0])
    with g.where(col("u") < 20) as fa, g.make_filter(mask=allow) as fb:      # a predicate and an id allow-list meet
        for f, want in ((fa, A), (fb, B)):
            assert set(f.ids().tolist()) == want
        for made, want in ((fa & fb, A & B), (fa | fb, A | B), (fa - fb, A - B), (fb - fa, B - A), (~fa, everything - A),
                           (~(fa | fb), everything - A - B), (~fa & ~fb, everything - A - B)):
            with made as f:
                assert f.rows == len(want) and set(f.ids().tolist()) == want
                mask = f.id_bits(N)
                assert mask.dtype == bool and set(np.nonzero(mask)[0].tolist()) == want
                assert set(np.nonzero(f.id_bits(1000))[0].tolist()) == {v for v in want if v < 1000}     # ids at or past nbits are left out
        with fa & fb as f, g.make_filter(ids=sorted(A & B)) as y:
            _, _, queries = make_data(N)
            same_answers(g, f, y, queries, "predicate AND allow-list")
        with pytest.raises(TypeError):
            fa & 3
    # delete where: exactly the predicate's rows go (and the pending ones, as with every eager remove)
    with g.where((col("i") < 0) & (col("u") >= 20)) as f:
        gone = (i < 0) & (u >= 20) & live
        assert g.remove(mask=f.id_bits()) == gone.sum()
    assert np.array_equal(np.sort(g.map_ids), np.nonzero(live & ~gone)[0])
    # extract where
    with g.where(col("u").between(3, 5)) as f:
        e = g.extract(mask=f.id_bits())
    assert np.array_equal(np.sort(e.map_ids), np.nonzero(live & ~gone & (u >= 3) & (u <= 5))[0])
    assert np.array_equal(e.attr_array("u"), u[e.map_ids])
    e.close()
    g.close()


def test_filters_outlive_value_changes_not_relayouts(rq):
    from rabitq_amd import col
    g = build(rq, N)
    other = build(rq, 64)
    _, _, queries = make_data(N)
    g.create_attr("t", "u32", fill=0)
    g.set_attr("t", np.arange(N), np.arange(N) % 10)
    f = g.where(col("t") == 3)
    want = np.arange(3, N, 10)
    before = g.query_batch(queries, 4, 10, filter=f)
    g.set_attr("t", np.arange(N), np.zeros(N))                                # values change, positions do not: the filter is the set it selected
    assert np.array_equal(np.sort(f.ids()), want)
    after = g.query_batch(queries, 4, 10, filter=f)
    for a, b in zip(before, after):
        assert np.array_equal(bits(a), bits(b))
    with g.where(col("t") == 3) as now:
        assert now.rows == 0
    g.create_attr("later", "i64", fill=-1)                                    # nor does a new or a dropped column disturb it
    g.drop_attr("later")
    with ~f as nf:
        assert nf.rows == N - want.size
    fo = other.make_filter(ids=[1, 2, 3])
    for call in (lambda: g.query_batch(queries, 4, 10, filter=fo), lambda: rq._lib.check(rq._lib.lib().rq_filter_combine(
            g._h, f._h, fo._h, 0, C.byref(C.c_void_p())))):
        with pytest.raises(rq.RabitqError) as e:
            call()
        assert e.value.status == INVALID and "another index" in str(e.value)
    assert g.remove(ids=[0], lazy=True) == 1                                  # a marking lazy removal: stale, as for the queries
    for call in (lambda: g.query_batch(queries, 4, 10, filter=f), lambda: ~f, lambda: f.ids(), lambda: f.id_bits(N)):
        with pytest.raises(rq.RabitqError) as e:
            call()
        assert e.value.status == INVALID and "marked dead" in str(e.value)
    f.close()
    f = g.where(col("t") == 0)
    assert f.rows == N - 1
    g.add(make_data(N)[0][:5], ids=np.arange(N, N + 5))                       # a relayout
    for call in (lambda: g.query_batch(queries, 4, 10, filter=f), lambda: f & f, lambda: f.ids(), lambda: f.id_bits(N)):
        with pytest.raises(rq.RabitqError) as e:
            call()
        assert e.value.status == INVALID and "last mutated" in str(e.value)
    for h in (f, fo, g, other):
        h.close()


@pytest.mark.parametrize("kind", ["f16", "u8", "split_rows", "tiered"])
def test_every_storage_accepts_columns(rq, kind):
    from rabitq_amd import col
    from rabitq_amd import index as ix
    n = 6000
    x, centres, queries = make_data(n, seed=600)
    P = synth.random_orthogonal(D, seed=78)
    if kind == "f16":
        g = rq.RaBitQ.build(x.astype(np.float16), centres, P, rows="f16")
    elif kind == "u8":
        g = rq.RaBitQ.build(np.clip(np.rint(x * 40.0 + 128.0), 0, 255).astype(np.uint8), centres * 40.0 + 128.0, P, rows="u8")
        queries = queries * 40.0 + 128.0
    else:
        ix.set_option("base_device_mb" if kind == "tiered" else "split_rows", 1 if kind == "tiered" else 2)
        try:
            g = rq.RaBitQ.build(x, centres, P)
        finally:
            ix.set_option("base_device_mb", -1)
            ix.set_option("split_rows", 1)
        assert (g.n_hbm < n) if kind == "tiered" else g.split_rows
    g.create_attr("t", "i32", fill=-1)
    vals = (np.arange(n) % 7).astype(np.int32)
    assert g.set_attr("t", np.arange(n), vals) == 0
    assert np.array_equal(g.attr_array("t"), vals[g.map_ids])
    assert g.remove(ids=np.arange(0, n, 5), lazy=True) == n // 5             # lazy removal works on every storage
    want = np.nonzero((vals >= 5) & (np.arange(n) % 5 != 0))[0]
    with g.where(col("t") >= 5) as f, g.make_filter(ids=want) as y:
        assert f.rows == want.size and np.array_equal(np.sort(f.ids()), want)
        a, b = g.query_batch(queries, 4, 10, filter=f), g.query_batch(queries, 4, 10, filter=y)
        for u, v in zip(a, b):
            assert np.array_equal(bits(u), bits(v)), kind
        assert a[2].sum() > 0
    g.close()


def test_refusals(rq):
    from rabitq_amd import _lib, col
    g = build(rq, 200)
    L = _lib.lib()

    def refused(call, status, text):
        with pytest.raises(rq.RabitqError) as e:
            call()
        assert e.value.status == status and text in str(e.value), str(e.value)

    g.create_attr("f", "f32", fill=1.0)
    g.create_attr("u", "u32")
    refused(lambda: g.create_attr("u", "i64"), INVALID, "already has a column named u")
    refused(lambda: g.create_attr("no-dash", "u32"), INVALID, "[A-Za-z0-9_]")
    refused(lambda: g.create_attr("x" * 32, "u32"), INVALID, "[A-Za-z0-9_]")
    g.create_attr("x" * 31, "u32")
    g.drop_attr("x" * 31)
    refused(lambda: g.drop_attr("nope"), INVALID, "no column named nope")
    refused(lambda: g.set_attr("nope", [1], [1]), INVALID, "no column named nope")
    refused(lambda: g.get_attr("nope", [1]), INVALID, "no column named nope")
    refused(lambda: g.attr_array("nope"), INVALID, "no column named nope")
    refused(lambda: g.where(col("nope") == 1), INVALID, "no column named nope")
    small = np.zeros(10, dtype=np.uint32)
    refused(lambda: _lib.check(L.rq_attr_get_array(g._h, b"u", C.c_void_p(small.ctypes.data), small.nbytes)), INVALID, "too small")
    info = _lib.AttrInfoT()
    refused(lambda: _lib.check(L.rq_attr_info(g._h, 2, C.byref(info))), INVALID, "column index 2 of 2")
    idx = C.c_uint32(99)
    _lib.check(L.rq_attr_index(g._h, b"u", C.byref(idx)))
    assert idx.value == 1
    with pytest.raises(ValueError):
        g.create_attr("bad", "f64")
    with pytest.raises(ValueError):
        g.where(col("u") == -1)                                               # not a value of a u32 column
    with pytest.raises(ValueError):
        g.where(col("u") == 1.5)
    with pytest.raises(ValueError):
        g.set_attr("u", [1, 2], [1, 2, 3])
    # the bit ops are for integer columns; an unknown column index; more than 8 distinct columns
    refused(lambda: g.where(col("f").any_bits(1)), INVALID, "integer columns")
    refused(lambda: g.where(col("f").all_bits(1)), INVALID, "integer columns")
    terms = (_lib.WhereTermT * 9)()
    h = C.c_void_p()
    terms[0].column = 2
    refused(lambda: _lib.check(L.rq_filter_create_where(g._h, terms, 1, None, 0, C.byref(h))), INVALID, "no column 2")
    for j in range(14):
        g.create_attr(f"c{j}", "u32")
    assert len(g.attrs()) == 16
    refused(lambda: g.create_attr("one_more", "u32"), UNSUPPORTED, "16 columns")
    for j in range(9):                                                        # f != 0 (its fill is 1), every other column == 0 (its fill)
        terms[j].column, terms[j].op = j, M.NE if j == 0 else M.EQ
    refused(lambda: _lib.check(L.rq_filter_create_where(g._h, terms, 9, None, 0, C.byref(h))), INVALID, "8 distinct columns")
    _lib.check(L.rq_filter_create_where(g._h, terms, 8, None, 0, C.byref(h)))           # eight are read
    with rq.Filter(g, h) as f:
        assert rq.last_where_stats()["columns"] == 8 and f.rows == 200
    # open tickets do not stand in the way of values
    import torch
    _, _, queries = make_data(N)
    dq = torch.from_numpy(queries).cuda()
    od = torch.empty((100, 5), dtype=torch.float32, device="cuda")
    oi = torch.empty((100, 5), dtype=torch.int32, device="cuda")
    on = torch.empty(100, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ticket = g.query_batch_device_begin(dq.data_ptr(), 100, D, 4, 5, od.data_ptr(), oi.data_ptr(), on.data_ptr())
    try:
        assert g.set_attr("u", [3, 999], [33, 1]) == 1 and g.get_attr("u", [3])[0].tolist() == [33]
    finally:
        g.query_batch_device_end(ticket)
    g.close()
