"""The CPU model of the exact range search (tests/exact_range_model.py): it is the prefix of the exact search's whole ranking cut at
the radius, "<" is strict, and the edge radii (NaN, 0, negative, inf, f32::MAX) behave as the header says.  No GPU needed."""
import numpy as np

from tests import exact_model as em
from tests import exact_range_model as erm
from tests import synth


def world(oracle, n=600, d=64, nq=12, seed=11):
    x, _, _ = synth.mixture(n, d, 8, sigma=0.5, seed=seed, centre_scale=0.7)
    q, _, _ = synth.mixture(nq, d, 8, sigma=0.5, seed=seed + 1, centre_scale=0.7)
    q[0] = x[5]
    ids_of = np.random.default_rng(seed).permutation(n).astype(np.uint32)    # positions are not ids
    return x, ids_of, em.transformed_queries(oracle, q, "l2", d)


def same(a, b):
    return all(np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u, v.view(np.uint32) if v.dtype == np.float32 else v)
               for u, v in zip(a, b))


def test_model_is_the_prefix_of_the_whole_ranking(oracle):
    x, ids_of, qp = world(oracle)
    n = len(x)
    full = em.exact_batch(oracle, x, ids_of, qp, n)
    for kth in (1, 10, 300):
        radii = full[0][:, kth - 1].copy()
        got = erm.range_batch(oracle, x, ids_of, qp, radii)
        assert same(got, erm.cut_full(full, radii))
        lims, dist, ids = got
        for b in range(len(qp)):
            seg = slice(int(lims[b]), int(lims[b + 1]))
            m = seg.stop - seg.start
            assert m <= kth - 1 and np.array_equal(ids[seg], full[1][b, :m])     # strictly below the kth distance
            assert np.all(dist[seg] < radii[b])
    mask = np.zeros(n, dtype=bool)
    mask[::3] = True
    got = erm.range_batch(oracle, x, ids_of, qp, 40.0, mask)
    assert same(got, erm.cut_full(em.exact_batch(oracle, x, ids_of, qp, n, mask), 40.0))
    assert set(got[2].tolist()) <= set(np.flatnonzero(mask).tolist())


def test_the_comparison_is_strict(oracle):
    x, ids_of, qp = world(oracle)
    full = em.exact_batch(oracle, x, ids_of, qp, len(x))
    for b in (1, 2):
        e = full[0][b, 4]
        assert full[0][b, 3] < e                                              # (no tie at this place of the fixture)
        d_at, i_at = erm.range_one(oracle, x, ids_of, qp[b], e)
        d_up, i_up = erm.range_one(oracle, x, ids_of, qp[b], np.nextafter(e, np.float32(np.inf)))
        assert full[1][b, 4] not in i_at and i_at.size == 4
        assert i_up.size >= 5 and i_up[4] == full[1][b, 4] and d_up[4] == e
    # the query that sits on a stored row: e = 0 is not below 0, and is below the smallest positive f32
    assert erm.range_one(oracle, x, ids_of, qp[0], 0.0)[0].size == 0
    tiny = erm.range_one(oracle, x, ids_of, qp[0], np.float32(1e-45))
    assert tiny[0].tolist() == [0.0] and tiny[1][0] == ids_of[5]


def test_edge_radii(oracle):
    x, ids_of, qp = world(oracle)
    x = x.copy()
    x[3, 0] = np.nan                       # never returned
    x[4, :] = 3.0e19                       # e = inf: never returned
    n = len(x)
    for r in (np.nan, 0.0, -0.0, -1.0, -np.inf):
        lims, dist, ids = erm.range_batch(oracle, x, ids_of, qp, r)
        assert not lims.any() and dist.size == 0 and ids.size == 0
    with np.errstate(all="ignore"):
        everything = erm.range_batch(oracle, x, ids_of, qp, np.inf)
        assert same(everything, erm.range_batch(oracle, x, ids_of, qp, em.F32_MAX))
        assert np.array_equal(np.diff(everything[0]), np.full(len(qp), n - 2, dtype=np.uint64))
        assert ids_of[3] not in everything[2] and ids_of[4] not in everything[2] and np.all(everything[1] < em.F32_MAX)
        mixed = np.full(len(qp), 30.0, dtype=np.float32)
        mixed[1], mixed[2], mixed[3] = np.nan, np.inf, 0.0
        lims, _, _ = erm.range_batch(oracle, x, ids_of, qp, mixed)
    counts = np.diff(lims)
    assert counts[1] == 0 and counts[3] == 0 and counts[2] == n - 2
    assert lims.dtype == np.uint64 and lims[0] == 0
    empty = erm.pack([])
    assert empty[0].tolist() == [0] and empty[1].size == 0
