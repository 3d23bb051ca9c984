"""Exact search on split-row and tiered indexes (rq_exact_search_tiered*, rq_exact_range_search_tiered*, include/rabitq_hip.h).

Ids, distance bits and counts are compared BIT FOR BIT with the CPU model (tests/exact_model.py) over the rows the index was built from,
in its cluster order -- nothing is read back from the engine but map_ids.  The model of a dimension is computed once and shared by the
layouts: the layout of the raw vectors changes no answer.

Run on the GPU box:  python -m pytest tests/test_exact_tiered_gpu.py -m gpu -q
"""
import os

import numpy as np
import pytest

from tests import exact_model as em
from tests import exact_scan_cases as esc
from tests import synth

pytestmark = pytest.mark.gpu
UNSUPPORTED = -6
N, K, NQ, TOP = 12000, 24, 40, 300
# layout -> (option base_device_mb, option split_rows): -1 = every row in HBM; 2 / 0 = split rows always / never, 1 = the engine's choice
LAYOUTS = {"split": (-1, 2), "tiered": (1, 1), "tiered+split": (1, 2), "tiered+plain": (1, 0)}
DIMS = (64, 192, 256, 512)


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def build(rq, layout, x, centres, P):
    from rabitq_amd import index as ix
    ix.set_option("base_device_mb", LAYOUTS[layout][0])
    ix.set_option("split_rows", LAYOUTS[layout][1])
    try:
        g = rq.RaBitQ.build(x, centres, P)
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)
    assert (g.n_hbm < g.n) == layout.startswith("tiered") and g.split_rows == (layout != "tiered+plain")
    return g


_DATA, _INDEX = {}, {}


@pytest.fixture(scope="module")
def world(rq, oracle):
    """(layout, d) -> the index of that layout over the mixture of dimension d, its data, and `full`: the model's top-300 of the 40
    queries (and `base`, the rows in cluster order) -- computed once per dimension."""
    def get(layout, d):
        if d not in _DATA:
            x, centres, _ = synth.mixture(N, d, K, sigma=0.8, seed=61 + d, centre_scale=0.6)
            q, _, _ = synth.mixture(NQ, d, K, sigma=0.8, seed=161 + d, centre_scale=0.6)
            _DATA[d] = dict(x=x, centres=centres, P=esc.rotation(d, 62 + d), q=q)
        c = _DATA[d]
        if (layout, d) not in _INDEX:
            _INDEX[layout, d] = build(rq, layout, c["x"], c["centres"], c["P"])
        g = _INDEX[layout, d]
        if "full" not in c:
            c["map_ids"] = g.map_ids.copy()
            c["base"] = np.ascontiguousarray(c["x"][c["map_ids"]])
            c["full"] = em.exact_batch(oracle, c["base"], c["map_ids"], em.transformed_queries(oracle, c["q"], "l2", d), TOP)
        assert np.array_equal(g.map_ids, c["map_ids"])
        return dict(c, g=g)
    yield get
    for g in _INDEX.values():
        g.close()
    _INDEX.clear()
    _DATA.clear()


def same(got, want, topk=None):
    """(dist, ids, counts) equal bit for bit; `want` may be a wider model answer cut at topk"""
    gd, gi, gc = got
    wd, wi, wc = want
    if topk is not None:
        wd, wi, wc = wd[:, :topk], wi[:, :topk], np.minimum(wc, topk)
    assert np.array_equal(gc, wc)
    assert np.array_equal(gi, wi)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def host_positions(g):
    """Positions that are certainly in the host tier: list c keeps floor(len_c B / n) rows in HBM with n_hbm <= B < n_hbm + k."""
    off = np.asarray(g.offsets, dtype=np.int64)
    local = np.arange(g.n) - np.repeat(off[:-1], np.diff(off))
    length = np.repeat(np.diff(off), np.diff(off))
    return local * g.n >= length * (g.n_hbm + g.k)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_parity(rq, world, layout, d):
    c = world(layout, d)
    g = c["g"]
    topk = (1, 10, 300)[(list(LAYOUTS).index(layout) + DIMS.index(d)) % 3]
    same(g.exact_search_tiered(c["q"], topk), c["full"], topk)
    st = rq.last_exact_stats()
    assert st["scan_subtiles"] == esc.expected_rt(d) and st["reruns"] + 1 == st["scan_launches"]
    if g.split_rows:
        assert st["row_bytes_read"] == st["scan_launches"] * N * 2 * d      # the second plane was not scanned
    if layout.startswith("tiered"):
        on_host = np.zeros(N, dtype=bool)
        on_host[c["map_ids"][host_positions(g)]] = True
        assert g.n_hbm < N and on_host[c["full"][1][:, :topk]].any()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_filter_and_lazy_removals(rq, oracle, world, layout):
    c = world(layout, 128)
    rng = np.random.default_rng(7)
    mask = rng.random(N) < 0.125
    qp = em.transformed_queries(oracle, c["q"], "l2", 128)
    f = c["g"].make_filter(mask=mask)
    try:
        same(c["g"].exact_search_tiered(c["q"], 10, filter=f), em.exact_batch(oracle, c["base"], c["map_ids"], qp, 10, mask))
    finally:
        f.close()
    g = build(rq, layout, c["x"], c["centres"], c["P"])     # an index of its own: the removals stay with it
    try:
        dead = rng.choice(N, 700, replace=False)
        dead = np.union1d(dead, c["full"][1][:, 0])          # every query loses its nearest row
        g.remove(ids=dead.astype(np.uint32), lazy=True)
        alive = np.ones(N, dtype=bool)
        alive[dead] = False
        same(g.exact_search_tiered(c["q"], 10), em.exact_batch(oracle, c["base"], c["map_ids"], qp, 10, alive))
    finally:
        g.close()


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_no_seed_and_no_prefilter_change_nothing(rq, world, flags):
    c = world("tiered+split", 128)
    same(c["g"].exact_search_tiered(c["q"], 10, params=dict(flags=flags)), c["full"], 10)
    assert (rq.last_exact_stats()["scan_subtiles"] == 0) == bool(flags & 2)


def ties_up_case(dim):
    """Rows on which plane 0 is as wrong as it can be in the direction that loses answers: every coordinate is +-(1 + 2^-8) 2^j, a TIE
    of two bf16 values that the first plane rounds away from zero (round-to-nearest-even would go down to 1), so |x~|^2 exceeds |x|^2
    by almost 2^-7 of itself; the queries are zero or tiny, so nothing of the product's error offsets it: a - e is 0.93 of m'."""
    n = esc.rows_of(dim)
    rng = np.random.default_rng(9000 + dim)
    sign = np.where(rng.random((n, dim)) < 0.5, -1.0, 1.0).astype(np.float32)
    x = sign * np.float32(1.0 + 2.0 ** -8) * np.exp2(rng.integers(0, 3, n)).astype(np.float32)[:, None]
    q = np.where(rng.random((esc.MARGIN_NQ, dim)) < 0.5, -1.0, 1.0).astype(np.float32) * np.float32(2.0 ** -10)
    q[0] = 0.0
    return dict(x=np.ascontiguousarray(x), centres=rng.standard_normal((esc.K, dim)).astype(np.float32), P=np.eye(dim, dtype=np.float32), q=q)


@pytest.mark.parametrize("case", ["margin_case", "ties_up"])
@pytest.mark.parametrize("d", [128, 768])
def test_margin_worst_cases(rq, oracle, d, case):
    c = esc.margin_case(d) if case == "margin_case" else ties_up_case(d)
    g = build(rq, "split", c["x"], c["centres"], c["P"])
    try:
        base = np.ascontiguousarray(c["x"][g.map_ids])
        for topk in (10, 200):    # (the cuts fall inside classes of tied rows)
            same(g.exact_search_tiered(c["q"], topk), em.exact_batch(oracle, base, g.map_ids, em.transformed_queries(oracle, c["q"], "l2", d), topk))
            assert rq.last_exact_stats()["scan_subtiles"] == esc.expected_rt(d)
    finally:
        g.close()


def test_non_finite_rows(rq, oracle):
    d, big = 64, np.float32(1.5e19)
    x, centres, _ = synth.mixture(300, d, 4, sigma=0.8, seed=5, centre_scale=0.6)
    q, _, _ = synth.mixture(33, d, 4, sigma=0.8, seed=6, centre_scale=0.6)
    x[10, 3] = np.inf
    x[11] = 0.0
    x[11, 5] = np.array([0x7FFF8001], dtype=np.uint32).view(np.float32)[0]     # a NaN that plane 0 wraps to -0: the row looks like zero
    x[12, 7] = np.array([0x7F7FC000], dtype=np.uint32).view(np.float32)[0]     # finite, rounds to inf in plane 0
    x[13] = big                                                                # |x|^2 = 64 x 2.25e38 overflows; beside query 0 e is finite
    q[0] = big
    q[0, :4] = np.float32(1.4e19)
    q[1] = 0.0                                                                 # next to the zero query row 11 would be the nearest
    g = build(rq, "split", x, centres, synth.random_orthogonal(d, seed=8))
    try:
        base = np.ascontiguousarray(x[g.map_ids])
        want = em.exact_batch(oracle, base, g.map_ids, em.transformed_queries(oracle, q, "l2", d), 20)
        got = g.exact_search_tiered(q, 20)
        same(got, want)
        assert not np.isin(got[1], [10, 11]).any() and got[1][0, 0] == 13 and np.isfinite(got[0][0, 0])
    finally:
        g.close()


def test_range_form(rq, oracle, world):
    from tests import exact_range_model as erm
    c = world("tiered+split", 128)
    qp = em.transformed_queries(oracle, c["q"], "l2", 128)
    e = np.stack([oracle.l2_squared_distance_rows(qp[b], c["base"], np.arange(N, dtype=np.uint64)) for b in range(NQ)])
    radius = np.quantile(e, 0.001, axis=1).astype(np.float32)
    radius[3] = 0.0                                            # admits nothing
    lims, dist, ids = c["g"].exact_range_search_tiered(c["q"], radius=radius)
    wl, wd, wi = erm.range_batch(oracle, c["base"], c["map_ids"], qp, radius)
    assert np.array_equal(lims, wl) and np.array_equal(ids, wi) and np.array_equal(dist.view(np.uint32), wd.view(np.uint32))
    assert lims[4] == lims[3] and lims[-1] > NQ and rq.last_exact_stats()["row_bytes_read"] % (N * 2 * 128) == 0
    with pytest.raises(rq.RabitqError) as err:
        c["g"].exact_range_search(c["q"], radius=radius)
    assert err.value.status == UNSUPPORTED


def test_recall_takes_the_tiered_truth(rq, world):
    c = world("tiered+split", 128)
    g = c["g"]
    _, ids, cnt = g.query_batch(c["q"], 8, 10)
    want = g._recall_of(ids, cnt, c["full"][1][:, :10], np.minimum(c["full"][2], 10))
    assert g.recall(c["q"], 8, 10, tiered=True) == want
    assert g.tune_nprobe(c["q"], 10, 2.0, tiered=True)[0] == K     # out of reach: (k, recall at k)
    with pytest.raises(rq.RabitqError) as err:
        g.recall(c["q"], 8, 10)
    assert err.value.status == UNSUPPORTED
