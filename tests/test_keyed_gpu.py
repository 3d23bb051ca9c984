"""Postings and the keyed exact search on the GPU: rq_postings_* against numpy on the column, rq_exact_search_keyed*
bit for bit against tests/keyed_model.py (the existing exact search under a `where` filter per key), and once against plain f64
numpy on integer data whose squared distances are exact in f32.

Run on the GPU box:  python -m pytest tests/test_keyed_gpu.py -m gpu -q
"""
import os

import numpy as np
import pytest

from tests import byte_model as bm
from tests import exact_scan_cases as xc
from tests import half_model as hm
from tests import synth
from tests.keyed_model import keyed_reference, same_bits

pytestmark = pytest.mark.gpu

N, K, CHUNK = 20000, 32, 1024          # CHUNK: RQ_KEYED_CHUNK_ROWS = RQ_KEYED_SMALL_ROWS of host_keyed.h
INVALID = -1
# key -> rows: the tile (32), four-wave (128) and chunk boundaries, one key of about half the index; the rest go to keys 100 .. 139
SIZES = {1: 1, 2: 31, 3: 32, 4: 33, 5: 127, 6: 128, 7: 129, 8: CHUNK + 1, 9: N // 2}
ABSENT = 77
NO_SEED, NO_PREFILTER = 1, 2


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def tenant_values(n, sizes, seed):
    """One value per id: sizes[key] ids of every key at random places, the others spread over keys 100 .. 139."""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([np.full(c, k, dtype=np.int64) for k, c in sizes.items()])
    vals = np.concatenate([vals, 100 + rng.integers(0, 40, size=n - vals.size)])
    return rng.permutation(vals)


def make_index(rq, n, d, seed, k=K, **kw):
    x, centres, _ = synth.mixture(n, d, k, sigma=0.6, seed=seed, centre_scale=0.8)
    q, _, _ = synth.mixture(200, d, k, sigma=0.6, seed=seed + 1, centre_scale=0.8)
    dim = (d + 63) // 64 * 64
    return rq.RaBitQ.build(x, centres, np.eye(dim, dtype=np.float32) if dim > 256 else synth.random_orthogonal(dim, seed=seed + 2), **kw), q


@pytest.fixture(scope="module")
def world(rq):
    """The 20 000-row index with a u32 tenant column and a second column, its postings, and one reference cache."""
    g, q = make_index(rq, N, 64, 900)
    ids = np.arange(N, dtype=np.uint32)
    g.create_attr("tenant", "u32", fill=0)
    g.set_attr("tenant", ids, tenant_values(N, SIZES, 1))
    g.create_attr("lang", "i32", fill=0)
    g.set_attr("lang", ids, np.random.default_rng(2).integers(-2, 3, size=N))
    post = g.postings("tenant")
    yield dict(g=g, q=q, post=post, ref={})
    post.close(), g.close()


def reference(w, keys, nq, topk):
    """keyed_reference of the world's first nq queries, computed once per (keys, topk)."""
    at = (tuple(int(k) for k in keys), topk)
    if at not in w["ref"]:
        w["ref"][at] = keyed_reference(w["g"], "tenant", w["q"][:nq], keys, topk)
    return w["ref"][at]


def test_postings_equal_numpy_on_the_column(world):
    g, post = world["g"], world["post"]
    col = g.attr_array("tenant")
    values, counts = np.unique(col, return_counts=True)
    assert np.array_equal(post.values, values) and np.array_equal(post.counts, counts.astype(np.uint64))
    assert post.rows == N and post.type.name == "u32"
    for key in list(SIZES) + [100, ABSENT]:
        assert np.array_equal(post.positions(key), np.nonzero(col == key)[0].astype(np.uint32)), key
    assert post.count_of([9, ABSENT, 1]).tolist() == [N // 2, 0, 1]


@pytest.mark.parametrize("per_key", [1, 32, 33])
@pytest.mark.parametrize("topk", [1, 10, 200])
def test_every_segment_size_bit_for_bit(world, per_key, topk):
    """Every boundary size, the absent key among them; 1 / 32 / 33 queries per key (a full tile and a tile + 1); topk 200 is above the
    sizes up to 129.  One call holds all keys: small and large segments, seeded and not, share the launches."""
    keys = np.array([ABSENT] + list(SIZES), dtype=np.uint32) if per_key == 1 else np.repeat(np.array([9, 4, ABSENT, 7, 8, 1], dtype=np.uint32), per_key)
    nq = keys.size
    got = world["g"].exact_search_keyed(world["q"][:nq], keys, topk, by=world["post"])
    want = reference(world, keys, nq, topk)
    assert same_bits(got, want)
    assert np.all(got[2][keys == ABSENT] == 0)
    st = world["g"].last_keyed_stats()
    assert st["prefilter"] == 1 and st["queries_absent"] == int((keys == ABSENT).sum())


@pytest.mark.parametrize("params", [dict(flags=NO_SEED), dict(flags=NO_PREFILTER), dict(cand_per_query=1)], ids=["no_seed", "no_prefilter", "cap1"])
def test_hooks_keep_the_bits(world, params):
    keys = np.array([9] * 33 + [8, 7, 3, ABSENT], dtype=np.uint32)
    got = world["g"].exact_search_keyed(world["q"][:keys.size], keys, 10, by=world["post"], params=params)
    st = world["g"].last_keyed_stats()
    assert same_bits(got, reference(world, keys, keys.size, 10))
    assert st["prefilter"] == (0 if params.get("flags") == NO_PREFILTER else 1)
    assert st["reruns"] > 0 or "cand_per_query" not in params     # (without a bound the large key overflows its slots, too)
    assert st["ms_seed"] == 0 if params.get("flags") else st["ms_seed"] > 0


@pytest.mark.parametrize("tuning", [(0, 0, 1), (64, 0, 2), (100000, 128, 0)], ids=["one_slab", "small_chunks", "one_chunk_low_threshold"])
def test_tuning_keeps_the_bits(world, tuning):
    """The world is dim 64, where the default scan is the double-buffered one: the single slab, 64-row work items (two tiles a block:
    waves without a tile) and one item per key with the matrix pass from 128 rows on give the same bits."""
    from rabitq_amd import _lib
    keys = np.array([9] * 33 + [8, 7, 3, ABSENT], dtype=np.uint32)
    _lib.check(_lib.lib().rq_keyed_tuning(*tuning))
    try:
        got = world["g"].exact_search_keyed(world["q"][:keys.size], keys, 10, by=world["post"])
    finally:
        _lib.check(_lib.lib().rq_keyed_tuning(0, 0, 0))
    assert same_bits(got, reference(world, keys, keys.size, 10)) and world["g"].last_keyed_stats()["prefilter"] == 1


def test_filter_on_a_second_column(world):
    g = world["g"]
    from rabitq_amd import col
    f = g.where(col("lang") >= 1)
    keys = np.array([9, 9, 8, 5, 2, 1, ABSENT], dtype=np.uint32)
    got = g.exact_search_keyed(world["q"][:keys.size], keys, 10, by=world["post"], filter=f)
    assert same_bits(got, keyed_reference(g, "tenant", world["q"][:keys.size], keys, 10, extra=f))


@pytest.mark.parametrize("d", [100, 192, 512])
def test_dimensions(rq, d):
    """100 pads to 128; 192 is the widest tile in this file; at 512 the tiles pass a CU's LDS and the exact-only form runs."""
    g, q = make_index(rq, 6000, d, 910 + d, k=8)
    g.create_attr("t", "u32", fill=0)
    g.set_attr("t", np.arange(6000, dtype=np.uint32), tenant_values(6000, {1: 33, 2: CHUNK + 200}, 3))
    post = g.postings("t")
    keys = np.array([2] * 33 + [1, 100, ABSENT], dtype=np.uint32)
    got = g.exact_search_keyed(q[:keys.size], keys, 10, by=post)
    assert g.last_keyed_stats()["prefilter"] == (1 if d < 512 else 0)
    assert same_bits(got, keyed_reference(g, "t", q[:keys.size], keys, 10))
    post.close(), g.close()


@pytest.mark.parametrize("rows,metric", [("f32", "cosine"), ("f32", "ip"), ("f16", "l2"), ("f16", "cosine"), ("bf16", "l2"), ("bf16", "cosine"),
                                         ("u8", "l2"), ("i8", "l2")])
def test_rows_and_metrics(rq, rows, metric):
    """Every row type x metric an index accepts (f32 x l2 is the world's); the large key takes the matrix pass through the gather of
    that row type."""
    n, d = 5000, 63 if metric == "ip" else 64
    if rows in bm.TYPES:
        b, centres, marks = bm.byte_data(rows, n, d, 8, seed=77)
        x, q = bm.typed(b, rows), bm.byte_queries(rows, b, marks, 40, d, 8, seed=78)
    else:
        x, centres, _ = synth.mixture(n, d, 8, sigma=0.6, seed=77, centre_scale=0.8)
        q, _, _ = synth.mixture(40, d, 8, sigma=0.6, seed=78, centre_scale=0.8)
        if rows != "f32":
            h = hm.narrow(x, rows)
            x = h.view(np.float16) if rows == "f16" else h
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(64, seed=79), metric=metric, **({} if rows == "f32" else {"rows": rows}))
    g.create_attr("t", "u32", fill=0)
    g.set_attr("t", np.arange(n, dtype=np.uint32), tenant_values(n, {1: 33, 2: CHUNK + 100}, 4))
    post = g.postings("t")
    keys = np.array([2] * 33 + [1, 100, ABSENT], dtype=np.uint32)
    got = g.exact_search_keyed(q[:keys.size], keys, 10, by=post)
    assert g.last_keyed_stats()["prefilter"] == 1
    assert same_bits(got, keyed_reference(g, "t", q[:keys.size], keys, 10))
    post.close(), g.close()


@pytest.mark.parametrize("dtype,special", [("i32", [-5, -2**31, 2**31 - 1]), ("u64", [2**32 + 7, 2**64 - 1, 2**63]),
                                           ("i64", [-1, -2**63, 2**40])], ids=["i32", "u64", "i64"])
def test_column_types(rq, dtype, special):
    """Negative keys, keys above 2^32, and the table's empty mark (u64 2^64 - 1 = i64 -1: all ones) as a value."""
    n = 3000
    g, q = make_index(rq, n, 64, 930, k=8)
    np_t = {"i32": np.int32, "u64": np.uint64, "i64": np.int64}[dtype]
    vals = np.array([special[i % 3] if i % 5 else 3 for i in range(n)], dtype=np_t)
    g.create_attr("t", dtype, fill=0)
    g.set_attr("t", np.arange(n, dtype=np.uint32), vals)
    post = g.postings("t")
    col = g.attr_array("t")
    values, counts = np.unique(col, return_counts=True)
    assert np.array_equal(post.values, values) and np.array_equal(post.counts, counts.astype(np.uint64))
    keys = np.array(special + [3, 4], dtype=np_t)
    for key in keys:
        assert np.array_equal(post.positions(key), np.nonzero(col == key)[0].astype(np.uint32)), key
    got = g.exact_search_keyed(q[:5], keys, 10, by=post)
    assert same_bits(got, keyed_reference(g, "t", q[:5], keys, 10)) and got[2][4] == 0
    post.close(), g.close()


def test_margin_family(rq):
    """The data of tests/exact_scan_cases.py on which the bf16 approximation is as wrong as it can be: one key holds every row but a
    few, so the matrix pass decides, and the cut falls inside a class of tied rows."""
    c = xc.margin_case(128)
    n = c["n"]
    g = rq.RaBitQ.build(np.tile(c["x"], (12, 1)), c["centres"], c["P"])       # 12 copies: the key's segment passes the small-segment threshold
    n *= 12
    g.create_attr("t", "u32", fill=5)
    g.set_attr("t", np.arange(0, n, 97, dtype=np.uint32), 6)
    post = g.postings("t")
    keys = np.full(xc.MARGIN_NQ, 5, dtype=np.uint32)
    topk = 12 * xc.cut_inside_class(c["cls"][0], 2)
    got = g.exact_search_keyed(c["q"], keys, topk, by=post)
    assert g.last_keyed_stats()["prefilter"] == 1 and post.count_of([5])[0] >= CHUNK
    assert same_bits(got, keyed_reference(g, "t", c["q"], keys, topk))
    post.close(), g.close()


def test_against_f64_numpy_on_integer_data(rq):
    """Independent of the engine: rows and queries are integers in [-8, 8] at dim 64, so every squared distance is an integer below
    2^24 and exact in f32; the answer is the f64 brute force over the key's rows, ties broken by id."""
    rng = np.random.default_rng(11)
    n, nq, topk = 6000, 40, 10
    x = rng.integers(-8, 9, size=(n, 64)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, 64)).astype(np.float32)
    g = rq.RaBitQ.build(x, x[:8].copy(), np.eye(64, dtype=np.float32))
    vals = tenant_values(n, {1: 5, 2: CHUNK + 300}, 5)
    g.create_attr("t", "u32", fill=0)
    g.set_attr("t", np.arange(n, dtype=np.uint32), vals)
    post = g.postings("t")
    keys = np.array([2] * 33 + [1] * 6 + [ABSENT], dtype=np.uint32)
    dist, ids, cnt = g.exact_search_keyed(q, keys, topk, by=post)
    d64 = ((q.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    for b in range(nq):
        mine = np.nonzero(vals == keys[b])[0]
        order = mine[np.lexsort((mine, d64[b, mine]))][:topk]
        assert cnt[b] == order.size
        assert np.array_equal(ids[b, :cnt[b]], order.astype(np.uint32)) and np.array_equal(dist[b, :cnt[b]].astype(np.float64), d64[b, order])
    post.close(), g.close()


def test_lazy_removals_staleness_and_refusals(rq):
    n = 3000
    g, q = make_index(rq, n, 64, 940, k=8)
    ids = np.arange(n, dtype=np.uint32)
    vals = tenant_values(n, {1: 40, 2: 700}, 6)
    g.create_attr("t", "u32", fill=0)
    g.set_attr("t", ids, vals)
    g.create_attr("f", "f32", fill=0)
    with pytest.raises(rq.RabitqError) as e:                                  # an f32 column has no postings
        g.postings("f")
    assert e.value.status == INVALID
    g.remove(ids=ids[::3], lazy=True)                                         # removals pending before creation: dead rows are not in it
    post = g.postings("t")
    col, live = g.attr_array("t"), np.isin(g.map_ids, ids[::3], invert=True)
    assert post.rows == int(live.sum())
    assert np.array_equal(post.positions(2), np.nonzero((col == 2) & live)[0].astype(np.uint32))
    keys = np.array([2] * 5 + [1, ABSENT], dtype=np.uint32)
    want = keyed_reference(g, "t", q[:7], keys, 10)
    assert same_bits(g.exact_search_keyed(q[:7], keys, 10, by=post), want)
    g.set_attr("t", ids, 1)                                                   # rq_attr_set after creation: the postings keep what they saw
    assert same_bits(g.exact_search_keyed(q[:7], keys, 10, by=post), want)
    g.remove(ids=[1], lazy=True)                                              # a marking lazy removal: stale
    with pytest.raises(rq.RabitqError) as e:
        g.exact_search_keyed(q[:7], keys, 10, by=post)
    assert e.value.status == INVALID
    fresh = g.postings("t")
    g.compact()                                                               # a relayout: stale
    for call in (lambda: g.exact_search_keyed(q[:7], keys, 10, by=fresh), lambda: fresh.count_of([1]), lambda: fresh.positions(1)):
        with pytest.raises(rq.RabitqError) as e:
            call()
        assert e.value.status == INVALID
    post.close(), fresh.close(), g.close()


def test_stale_after_add(rq):
    g, q = make_index(rq, 2000, 64, 950, k=8)
    g.create_attr("t", "u32", fill=3)
    post = g.postings("t")
    assert g.exact_search_keyed(q[:2], [3, 3], 5, by=post)[2].tolist() == [5, 5]
    g.add(q[:2], ids=np.array([2005, 2006], dtype=np.uint32))
    for call in (lambda: g.exact_search_keyed(q[:2], [3, 3], 5, by=post), lambda: post.count_of([3]), lambda: post.positions(3)):
        with pytest.raises(rq.RabitqError) as e:
            call()
        assert e.value.status == INVALID
    post.close(), g.close()
