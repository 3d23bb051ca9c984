"""The keyed exact search on wide, split-row and tiered indexes (rq_exact_search_keyed_tiered*): ids, distance bits and
counts BIT FOR BIT against the CPU model (tests/exact_model.py::index_answer) with allow_mask = (column == key) per query, over the
rows the index was built from.  Nothing is read back from the engine but map_ids.

Run on the GPU box:  python -m pytest tests/test_keyed_tiered_gpu.py -m gpu -q
"""
import numpy as np
import pytest

from tests import exact_model as em
from tests import exact_scan_cases as esc
from tests import half_model as hm
from tests import synth
from tests.test_exact_tiered_gpu import LAYOUTS, host_positions, rq, same, ties_up_case  # noqa: F401  (rq: the module's fixture)

pytestmark = pytest.mark.gpu
INVALID = -1
ALL_LAYOUTS = dict(LAYOUTS, plain=(-1, 0))
N, ABSENT, SMALL = 6000, 77, 1024                  # SMALL: RQ_KEYED_SMALL_ROWS = RQ_KEYED_CHUNK_ROWS of host_keyed.h
# key -> rows: more than two chunks and no multiple of 32; exactly the threshold; just below it (no matrix pass); tiny ones
SIZES = {1: 2101, 2: SMALL, 3: SMALL - 1, 4: 1, 5: 33, 6: 40}
KEYS = np.array([1] * 33 + [2, 3, 4, 5, 6, ABSENT], dtype=np.uint32)   # two query tiles on the large key, one query per other key
CASES = [("plain", d) for d in (512, 576, 768, 2048, 2112)] + [(lay, d) for lay in LAYOUTS for d in (64, 192, 768)]


def build(rq, layout, x, centres, **kw):
    from rabitq_amd import index as ix
    ix.set_option("base_device_mb", ALL_LAYOUTS[layout][0])
    ix.set_option("split_rows", ALL_LAYOUTS[layout][1])
    try:
        g = rq.RaBitQ.build(x, centres, np.eye(x.shape[1], dtype=np.float32), **kw)
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)
    assert (g.n_hbm < g.n) == layout.startswith("tiered") and g.split_rows == (layout in ("split", "tiered", "tiered+split"))
    return g


def with_column(g, col):
    g.create_attr("t", "u32", fill=0)
    g.set_attr("t", np.arange(col.size, dtype=np.uint32), col)
    return g


def reference(oracle, g, x, q, keys, topk, col, extra=None):
    """index_answer per distinct key: the queries of key k under allow_mask = (column == k) [& extra], masks over ids."""
    base = np.ascontiguousarray(x[g.map_ids])
    out = (np.full((len(keys), topk), np.nan, dtype=np.float32), np.full((len(keys), topk), em.NO_ID, dtype=np.uint32), np.zeros(len(keys), dtype=np.uint32))
    for k in np.unique(keys):
        sel = keys == k
        mask = (col == k) if extra is None else (col == k) & extra
        for o, w in zip(out, em.index_answer(oracle, g, q[sel], topk, allow_mask=mask, base=base)):
            o[sel] = w
    return out


def data(d):
    """Rows, queries and the column of dimension d.  Half of the rows of the keys with a matrix pass (1, 2) lie in a FAR cluster which
    the pass must reject: checked here, on the CPU, with the float64 model of the scan -- for every query of the key, a - 4 m > the
    exact distance of EVERY near row of the key (so above any bound a sample with topk near rows gives; 4 m covers the plane scan's
    m' <= 2.04 m and its approximate norm)."""
    x, centres, _ = synth.mixture(N, d, 8, sigma=0.8, seed=61 + d, centre_scale=0.6)
    q, _, _ = synth.mixture(KEYS.size, d, 8, sigma=0.8, seed=161 + d, centre_scale=0.6)
    rng = np.random.default_rng(d)
    col = np.concatenate([np.full(c, k) for k, c in SIZES.items()] + [100 + rng.integers(0, 40, N - sum(SIZES.values()))])
    col = rng.permutation(col).astype(np.uint32)
    far = np.isin(col, (1, 2)) & (rng.random(N) < 0.5)
    x[far] += np.float32(30.0)
    near_pairs = 0
    for k in (1, 2):
        a, m = esc.approx_and_margin(x[far & (col == k)], q[KEYS == k], d)
        T = esc.exact64(x[~far & (col == k)], q[KEYS == k]).max(axis=1)
        assert (a - 4.0 * m > T[:, None]).all()
        near_pairs += int((KEYS == k).sum()) * int((~far & (col == k)).sum())
    plain_pairs = sum(int((KEYS == k).sum()) * c for k, c in SIZES.items() if c < SMALL)
    return dict(x=x, centres=centres, q=q, col=col, may_keep=near_pairs + plain_pairs)


_DATA, _INDEX = {}, {}


@pytest.fixture(scope="module")
def world(rq):
    """(layout, d) -> the index of that layout with its column and postings, and the data of dimension d (made once per dimension)."""
    def get(layout, d):
        if d not in _DATA:
            _DATA[d] = data(d)
        c = _DATA[d]
        if (layout, d) not in _INDEX:
            g = with_column(build(rq, layout, c["x"], c["centres"]), c["col"])
            _INDEX[layout, d] = (g, g.postings("t"))
        return dict(c, g=_INDEX[layout, d][0], post=_INDEX[layout, d][1])
    yield get
    for g, post in _INDEX.values():
        post.close(), g.close()
    _INDEX.clear()
    _DATA.clear()


@pytest.mark.parametrize("layout,d", CASES)
def test_parity(rq, oracle, world, layout, d):
    c = world(layout, d)
    g, topk = c["g"], (1, 10, 300)[CASES.index((layout, d)) % 3]
    got = g.exact_search_keyed_tiered(c["q"], KEYS, topk, by=c["post"])
    st = rq.last_keyed_stats()
    want = reference(oracle, g, c["x"], c["q"], KEYS, topk, c["col"])
    same(got, want)
    assert got[2][-1] == 0 and st["queries_absent"] == 1
    assert st["prefilter"] == (d <= 2048)
    if d <= 2048:
        assert st["rows_gathered"] > 0 and st["candidates"] <= c["may_keep"]       # the pass rejected the far half
    if layout.startswith("tiered"):
        on_host = np.zeros(N, dtype=bool)
        on_host[g.map_ids[host_positions(g)]] = True
        assert g.n_hbm < N and on_host[want[1][want[1] != em.NO_ID]].any()


@pytest.mark.parametrize("layout", ["split", "tiered"])
def test_filter_lazy_removals_and_stale_postings(rq, oracle, world, layout):
    c = world(layout, 192)
    rng = np.random.default_rng(7)
    mask = rng.random(N) < 0.4                                                     # cuts through every key
    f = c["g"].make_filter(mask=mask)
    try:
        same(c["g"].exact_search_keyed_tiered(c["q"], KEYS, 10, by=c["post"], filter=f),
             reference(oracle, c["g"], c["x"], c["q"], KEYS, 10, c["col"], extra=mask))
    finally:
        f.close()
    g = with_column(build(rq, layout, c["x"], c["centres"]), c["col"])            # an index of its own: the removals stay with it
    dead = rng.choice(N, 900, replace=False).astype(np.uint32)
    g.remove(ids=dead, lazy=True)                                                  # before the postings: dead rows are not in them
    post = g.postings("t")
    alive = np.ones(N, dtype=bool)
    alive[dead] = False
    same(g.exact_search_keyed_tiered(c["q"], KEYS, 10, by=post), reference(oracle, g, c["x"], c["q"], KEYS, 10, c["col"], extra=alive))
    g.remove(ids=[int(np.flatnonzero(alive)[0])], lazy=True)                       # a marking removal since: stale
    with pytest.raises(rq.RabitqError) as err:
        g.exact_search_keyed_tiered(c["q"], KEYS, 10, by=post)
    assert err.value.status == INVALID
    post.close(), g.close()


@pytest.mark.parametrize("params", [dict(flags=1), dict(flags=2), dict(flags=3), dict(cand_per_query=1)], ids=["no_seed", "no_prefilter", "both", "cap1"])
def test_hooks_keep_the_bits(rq, oracle, world, params):
    c = world("tiered+split", 768)
    got = c["g"].exact_search_keyed_tiered(c["q"], KEYS, 10, by=c["post"], params=params)
    st = rq.last_keyed_stats()
    same(got, reference(oracle, c["g"], c["x"], c["q"], KEYS, 10, c["col"]))
    assert st["prefilter"] == (0 if params.get("flags", 0) & 2 else 1)
    assert st["reruns"] > 0 or "cand_per_query" not in params


@pytest.mark.parametrize("layout,case", [("split", "margin_case"), ("split", "ties_up"), ("plain", "margin_case")])
def test_margin_worst_cases_inside_a_key(rq, oracle, layout, case):
    """The families of test_exact_tiered_gpu.py::test_margin_worst_cases at dim 768, nine copies so that the key passes the
    small-segment threshold: the matrix pass decides, and the cuts fall inside classes of tied rows."""
    c = esc.margin_case(768) if case == "margin_case" else ties_up_case(768)
    x = np.tile(c["x"], (9, 1))
    col = np.full(len(x), 5, dtype=np.uint32)
    col[::97] = 6
    g = with_column(build(rq, layout, x, c["centres"]), col)
    post = g.postings("t")
    keys = np.full(len(c["q"]), 5, dtype=np.uint32)
    for topk in (10, 200):
        same(g.exact_search_keyed_tiered(c["q"], keys, topk, by=post), reference(oracle, g, x, c["q"], keys, topk, col))
        assert rq.last_keyed_stats()["prefilter"] == 1 and post.count_of([5])[0] >= SMALL
    post.close(), g.close()


def test_non_finite_rows_inside_a_key(rq, oracle):
    """test_exact_tiered_gpu.py::test_non_finite_rows' rows (inf, a NaN plane 0 wraps to -0, an element plane 0 rounds to inf, an
    overflowing norm) among the 1200 rows of one key on a split index."""
    d, n, big = 64, 1200, np.float32(1.5e19)
    x, centres, _ = synth.mixture(n, d, 4, sigma=0.8, seed=5, centre_scale=0.6)
    q, _, _ = synth.mixture(33, d, 4, sigma=0.8, seed=6, centre_scale=0.6)
    x[10, 3] = np.inf
    x[11] = 0.0
    x[11, 5] = np.array([0x7FFF8001], dtype=np.uint32).view(np.float32)[0]
    x[12, 7] = np.array([0x7F7FC000], dtype=np.uint32).view(np.float32)[0]
    x[13] = big
    q[0] = big
    q[0, :4] = np.float32(1.4e19)
    q[1] = 0.0
    col = np.full(n, 5, dtype=np.uint32)
    col[100::97] = 6
    g = with_column(build(rq, "split", x, centres), col)
    post = g.postings("t")
    keys = np.full(33, 5, dtype=np.uint32)
    got = g.exact_search_keyed_tiered(q, keys, 20, by=post)
    same(got, reference(oracle, g, x, q, keys, 20, col))
    assert rq.last_keyed_stats()["prefilter"] == 1
    assert not np.isin(got[1], [10, 11]).any() and got[1][0, 0] == 13 and np.isfinite(got[0][0, 0])
    post.close(), g.close()


@pytest.mark.parametrize("rows,d", [("f32", 128), ("f16", 512)])
def test_forwarded_indexes_give_the_keyed_entry_its_bits(rq, rows, d):
    c = data(d)
    x = c["x"] if rows == "f32" else hm.narrow(c["x"], rows).view(np.float16)
    g = with_column(rq.RaBitQ.build(x, c["centres"], np.eye(d, dtype=np.float32), **({} if rows == "f32" else {"rows": rows})), c["col"])
    post = g.postings("t")
    same(g.exact_search_keyed_tiered(c["q"], KEYS, 10, by=post), g.exact_search_keyed(c["q"], KEYS, 10, by=post))
    assert rq.last_keyed_stats()["prefilter"] == (rows == "f32")                  # (typed rows at dim 512: that entry's exact-only form)
    post.close(), g.close()
