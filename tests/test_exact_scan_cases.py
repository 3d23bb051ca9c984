"""The conditions tests/test_exact_scan_instantiations_gpu.py relies on, checked on the CPU from tests/exact_scan_cases.py, the CPU
models and numpy alone: the tile table follows from the header's LDS formula, the fixtures have the shapes the scan's forms need, the
filters empty exactly the tile they are meant to, and the adversarial fixture drives the scan's bf16 approximation to within a few
percent of the margin the kernel allows -- where a mixture stays in the first sixth of it.  No GPU needed.

Measured here, (a - e) / m over every (query, row) pair of margin_case, smallest .. largest per dim:
    128: 0.9068 .. 0.9420    448: 0.9219 .. 0.9329    768: 0.9176 .. 0.9240    2432: 0.8784 .. 0.8804
and the largest |a - e| / m of the mixture parity_case(128) over the first 200 ranks of its 160 queries: 0.1498 (the zero query and
the query on a stored row included; the single worst pair of 32 000 -- a margin half as wide still covers every one of them)."""
import numpy as np
import pytest

from tests import exact_model as em
from tests import exact_range_model as erm
from tests import exact_scan_cases as xc

RT_TABLE = {64: 4, 192: 4, 256: 2, 448: 2, 512: 1, 2432: 1, 2496: 0}
MARGIN_FLOOR = 0.85          # every pair of the adversarial fixture sits at least this fraction of m above its exact distance
MIXTURE_CEILING = 0.25       # and no answer pair of a mixture comes this close


def test_tile_table_follows_from_the_lds_formula():
    assert xc.DIMS == tuple(sorted(RT_TABLE))
    assert {d: xc.expected_rt(d) for d in xc.DIMS} == RT_TABLE
    # the boundaries are boundaries: one 64-column step further the tile height changes (dims are multiples of 64)
    assert xc.expected_rt(192 + 64) == 2 and xc.expected_rt(448 + 64) == 1 and xc.expected_rt(2432 + 64) == 0
    assert xc.lds_bytes(4, 192) <= xc.LDS_HALF < xc.lds_bytes(4, 256)
    assert xc.lds_bytes(2, 448) <= xc.LDS_HALF < xc.lds_bytes(2, 512)
    assert xc.lds_bytes(1, 2432) == 156544 <= xc.LDS_MAX == 159744 < xc.lds_bytes(1, 2496)
    # the kernel header states the same formula and limits
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rabitq_amd", "csrc", "kernels_exact.h")).read()
    assert "return (size_t)rt * 32 * ((size_t)dim * 2 + 16) + (size_t)rt * 32 * 12;" in src
    assert "#define RQ_EXACT_LDS_MAX (156u * 1024u)" in src and "#define RQ_EXACT_LDS_HALF (64u * 1024u)" in src


@pytest.mark.parametrize("dim", xc.DIMS)
def test_parity_cases_have_the_shapes_the_forms_need(dim):
    c = xc.parity_case(dim)
    tile = xc.tile_rows(dim)
    n = c["n"]
    assert c["x"].shape == (n, dim) and c["centres"].shape == (xc.K, dim) and c["P"].shape == (dim, dim)
    assert n == 3 * tile + 37 and n % 32 == 5                              # three tiles, a full sub-tile, five rows of the next
    assert n <= 421                                                         # the largest index of the GPU file
    assert c["q"].shape == (xc.NQ, dim) and xc.NQ == 160 and xc.NQ_SMALL == 33
    assert xc.NQ // 32 == 5 and xc.NQ_SMALL % 32 == 1                       # five query tiles: wave 0 takes tiles 0 and 4; one + a ragged one
    assert np.array_equal(c["q"][xc.QUERY_IS_ROW], c["x"][7]) and not c["q"][xc.QUERY_IS_ZERO].any()
    if dim >= 512:
        assert np.array_equal(c["P"], np.eye(dim, dtype=np.float32))
    else:
        np.testing.assert_allclose(c["P"].astype(np.float64) @ c["P"].astype(np.float64).T, np.eye(dim), atol=1e-5)


@pytest.mark.parametrize("dim", xc.DIMS)
def test_filters_empty_the_tiles_they_are_meant_to(dim):
    n, tile = xc.rows_of(dim), xc.tile_rows(dim)
    map_ids = np.random.default_rng(dim).permutation(n).astype(np.uint32)    # positions are not ids
    masks = xc.filters(map_ids, n, tile // 32)
    assert sorted(masks) == ["hole", "straddle", "tail", "third"]
    admitted = {name: np.sort(em.admitted_positions(map_ids, m)).astype(np.int64) for name, m in masks.items()}
    blocks = (n + tile - 1) // tile                                          # (RT = 1: the 37 rows behind three tiles are a tile and five rows)
    rows_in = np.bincount(np.arange(n) // tile, minlength=blocks)
    per_tile = {name: np.bincount(p // tile, minlength=blocks) for name, p in admitted.items()}
    assert per_tile["hole"][1] == 0 and np.array_equal(np.delete(per_tile["hole"], 1), np.delete(rows_in, 1))   # one dead tile, live neighbours
    assert not per_tile["tail"][:-1].any() and per_tile["tail"][-1] == rows_in[-1] == (37 if tile > 32 else 5)
    assert admitted["straddle"].tolist() == [30, 31, 32, 33, 34]
    assert sorted(set((admitted["straddle"] >> 5).tolist())) == [0, 1]       # two words of the position bitmap
    assert np.array_equal(np.flatnonzero(masks["third"]), np.arange(0, n, 3)) and np.all(per_tile["third"] > 0)


@pytest.mark.parametrize("rows", ["f16", "bf16", "u8", "i8"])
def test_typed_cases_are_their_widened_rows(rows):
    from tests import byte_model as bm
    from tests import half_model as hm
    c = xc.typed_case(rows, 192)
    assert c["typed"].shape == c["wide"].shape == (xc.rows_of(192), 192) and c["wide"].dtype == np.float32
    assert c["typed"].dtype.itemsize == (1 if rows in bm.TYPES else 2)
    wide = bm.widen(c["typed"], rows) if rows in bm.TYPES else hm.widen(c["typed"], rows)
    assert np.array_equal(wide, c["wide"]) and c["q"].shape == (xc.NQ_SMALL, 192)


def ratios(x, q, dim):
    a, m = xc.approx_and_margin(x, q, dim)
    return (a - xc.exact64(x, q)) / m


def test_the_adversarial_value_rounds_down_by_almost_two_to_the_minus_eight():
    v = np.array([xc.V, np.float32(2.0) * xc.V, -xc.V], dtype=np.float32)
    r = xc.bf16_round(v)
    assert r.tolist() == [1.0, 2.0, -1.0]
    rel = (np.abs(v.astype(np.float64)) - np.abs(r.astype(np.float64))) / np.abs(v.astype(np.float64))
    assert np.all(rel > 2.0 ** -8 * 0.995) and np.all(rel < 2.0 ** -8)
    assert xc.bf16_round(np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])).tolist() == [1.0, 1.0 + 2.0 ** -6]   # ties go to even


@pytest.mark.parametrize("dim", xc.MARGIN_DIMS)
def test_margin_cases_sit_almost_a_whole_margin_above_the_exact_distance(dim):
    """Every (query, row) pair -- so every pair of every answer the GPU test asks for, whatever its radii and topk."""
    c = xc.margin_case(dim)
    assert c["x"].shape == (xc.rows_of(dim), dim) and c["q"].shape == (xc.MARGIN_NQ, dim)
    assert set(np.unique(np.abs(c["x"])).tolist()) == {float(xc.V), float(np.float32(2.0) * xc.V)}
    assert not (c["x"][:, None, :] == c["centres"][None, :, :]).all(axis=2).any()        # no centroid is a row
    assert c["cls"][0].min() == 0 and c["cls"][0].max() == xc.CLASSES - 1 and np.all(np.bincount(c["cls"][0]) >= 4)
    r = ratios(c["x"], c["q"], dim)
    assert r.min() >= MARGIN_FLOOR and r.max() < 1.0, f"dim {dim}: (a - e) / m in [{r.min():.4f}, {r.max():.4f}]"
    print(f"dim {dim}: (a - e) / m in [{r.min():.4f}, {r.max():.4f}]")


def test_a_mixture_stays_far_inside_the_margin(oracle):
    """The same ratio on parity_case(128), over the pairs of the answers the GPU test asks for (radii at the 10th and 200th neighbour,
    topk 10 and 64: the first 200 ranks of every query): why the adversarial fixture is needed."""
    c = xc.parity_case(128)
    n = c["n"]
    full = em.exact_batch(oracle, c["x"], np.arange(n, dtype=np.uint32), c["q"], n)
    assert np.all(full[2] == n)
    r = np.abs(ratios(c["x"], c["q"], 128))
    worst = max(float(r[b, full[1][b, :200]].max()) for b in range(xc.NQ))
    assert worst < MIXTURE_CEILING, f"mixture: |a - e| / m up to {worst:.4f}"
    print(f"mixture, dim 128: |a - e| / m up to {worst:.4f}")


@pytest.mark.parametrize("dim", xc.MARGIN_DIMS)
def test_the_model_ties_the_margin_cases_by_class(oracle, dim):
    """A radius just above class c's distance returns exactly the rows of classes <= c, and a topk picked inside a class cuts it."""
    c = xc.margin_case(dim)
    n, cls = c["n"], c["cls"]
    ids = np.arange(n, dtype=np.uint32)                                      # the answer does not depend on the cluster order
    dist = np.stack([oracle.l2_squared_distance_rows(q, c["x"], ids.astype(np.uint64)) for q in c["q"]])
    v2 = float(xc.V) ** 2
    np.testing.assert_allclose(dist, cls * v2, rtol=1e-5)
    spread = max(float(np.ptp(dist[0][cls[0] == k])) for k in range(1, xc.CLASSES))
    assert spread <= 8 * v2 * 2.0 ** -23, spread                              # the rows of a class tie, to the rounding of the f32 chain
    for k in range(1, xc.CLASSES):
        radii = xc.class_radii(dist, cls, k)
        lims, _, got = erm.range_batch(oracle, c["x"], ids, c["q"], radii)
        assert np.array_equal(np.diff(lims).astype(np.int64), (cls <= k).sum(axis=1)), k
        for b in (0, 1, xc.MARGIN_NQ - 1):
            assert set(got[int(lims[b]):int(lims[b + 1])].tolist()) == set(np.flatnonzero(cls[b] <= k).tolist())
    for k in (2, 5):
        topk = xc.cut_inside_class(cls[0], k)
        d0, i0 = em.exact_one(oracle, c["x"], ids, c["q"][0], topk + 1)
        assert cls[0][i0[topk - 1]] == cls[0][i0[topk]] == k and 1 <= topk < n
