"""The CPU model of the centroid trainer (tests/train_model.py) against numbers worked out by hand.  No GPU needed."""
import numpy as np
import pytest

from tests import train_model as tm

F32 = np.float32


@pytest.mark.parametrize("n,ns,seed", [(10, 10, 0), (10, 9, 0), (1000, 64, 3), (1000, 999, 7), (20_000, 2048, 0), (2 ** 32 - 1, 4096, 5),
                                       (2 ** 32 - 1, 3, 1 << 63)])
def test_sample_positions_are_one_per_stratum(n, ns, seed):
    pos = [tm.sample_pos(r, n, ns, seed) for r in range(ns)]
    assert all(a < b for a, b in zip(pos, pos[1:]))                      # distinct and ascending
    for r, p in enumerate(pos):
        assert r * n // ns <= p < (r + 1) * n // ns                     # one per stratum
    assert 0 <= pos[0] and pos[-1] < n
    if ns == n:
        assert pos == list(range(n))                                     # every row in order, whatever the seed
    elif ns > 8 and n >= 2 * ns:                                         # (strata of one row leave a seed no choice)
        assert pos != [tm.sample_pos(r, n, ns, seed + 1) for r in range(ns)]
    assert tm.sample_size(n, 1, ns) == ns and tm.sample_size(5, 2, 0) == 2   # ppc = 0 counts as 1


def test_mix64_known_answers():
    # splitmix64 from state 0: the first two outputs of the published generator
    assert tm.mix64(0) == 0xE220A8397B1DCDAF
    assert tm.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def rows2(*xy, d=64):
    out = np.zeros((len(xy), d), np.float32)
    for i, (x, y) in enumerate(xy):
        out[i, 0], out[i, 1] = x, y
    return out


def test_hand_worked_two_clusters(oracle):
    """6 rows, k = 2, d = 64, only columns 0 and 1 non-zero.  ns = 6 = n.  Start: c0 = row 0 = (0, 0), c1 = row 3 = (10, 0).
    Iteration 0: distances to (c0, c1): row 0 (0, 100), row 1 (4, 64), row 2 (1, 101), row 3 (100, 0), row 4 (144, 4),
    row 5 (109, 9) -> labels 0 0 0 1 1 1, objective (0 + 4 + 1) + (0 + 4 + 9) = 18; c0 = ((0 + 2 + 0) / 3, (0 + 0 + 1) / 3),
    c1 = ((10 + 12 + 10) / 3, (0 + 0 + 3) / 3).  Iteration 1: the same labels -> stop, iters_run = 1."""
    x = rows2((0, 0), (2, 0), (0, 1), (10, 0), (12, 0), (10, 3))
    m = tm.train(oracle, x, 2)
    assert (m.iters_run, m.sample_rows, m.splits) == (1, 6, 0)
    assert m.positions.tolist() == [0, 1, 2, 3, 4, 5]
    assert m.labels.tolist() == [0, 0, 0, 1, 1, 1] and m.counts == [[3, 3]]
    assert m.objective.tolist() == [18.0]
    want = rows2((F32(2) / F32(3), F32(1) / F32(3)), (F32(32) / F32(3), F32(1)))
    assert m.centroids.shape == (2, 64) and np.array_equal(m.centroids.view(np.uint32), want.view(np.uint32))
    assert m.centroids[:, :2].view(np.uint32).tolist() == [[0x3F2AAAAB, 0x3EAAAAAB], [0x412AAAAB, 0x3F800000]]
    # the cap: no iteration -> the start; one iteration -> the same centroids, iters_run = iters
    m0 = tm.train(oracle, x, 2, iters=0)
    assert m0.iters_run == 0 and m0.objective.size == 0 and np.array_equal(m0.centroids, x[[0, 3]])
    m1 = tm.train(oracle, x, 2, iters=1)
    assert m1.iters_run == 1 and np.array_equal(m1.centroids, m.centroids)


def test_hand_worked_split(oracle):
    """6 rows, k = 3, iters = 1.  Start: rows 0, 2, 4 = (0, 2), (0, 2), (100, 0): c1 duplicates c0, and the first minimum sends
    every tie to c0, so cluster 1 is empty.  Labels 0 0 0 0 2 2, distances 0 4 0 16 0 4 -> objective 20 + 0 + 4 = 24;
    c0 = (6 / 4, 8 / 4) = (1.5, 2), c2 = (101, 0).  Split: donor = cluster 0 (4 members); eps = 2^-10:
    c1 = (1.5 (1 + eps), 2 (1 - eps)) = (1.50146484375, 1.998046875), c0 = (1.5 (1 - eps), 2 (1 + eps)) = (1.49853515625,
    2.001953125); counts 4 0 2 -> 2 2 2."""
    x = rows2((0, 2), (2, 2), (0, 2), (4, 2), (100, 0), (102, 0))
    m = tm.train(oracle, x, 3, iters=1)
    assert (m.iters_run, m.splits) == (1, 1) and m.counts == [[4, 0, 2]]
    assert m.labels.tolist() == [0, 0, 0, 0, 2, 2] and m.objective.tolist() == [24.0]
    want = rows2((1.49853515625, 2.001953125), (1.50146484375, 1.998046875), (101, 0))
    assert np.array_equal(m.centroids.view(np.uint32), want.view(np.uint32))
    # (ns >= k, so while a cluster is empty another holds two members: the "donor has fewer than two" rule never fires in a run)
    y = rows2((1, 0), (1, 0), (5, 0))
    m = tm.train(oracle, y, 3, iters=1)
    assert m.counts == [[2, 0, 1]] and m.splits == 1
    z = rows2((1, 0), (1, 0), (1, 0), (1, 0))
    m = tm.train(oracle, z, 4, iters=1)                                   # 4 0 0 0 -> 2 2 0 0 -> 1 2 1 0 -> 1 1 1 1: every empty is served
    assert m.counts == [[4, 0, 0, 0]] and m.splits == 3


def test_refusals_and_metrics(oracle):
    x = rows2((0, 0), (2, 0), (0, 1))
    with pytest.raises(ValueError):
        tm.train(oracle, x, 4)                                            # n < k
    bad = x.copy()
    bad[1, 5] = np.nan
    with pytest.raises(ValueError):
        tm.train(oracle, bad, 2)
    # inner product: k x (d + 1) columns, the centroids of the augmented rows; cosine: of the normalised rows
    rng = np.random.default_rng(3)
    w = rng.standard_normal((40, 70)).astype(np.float32)
    ip = tm.train(oracle, w, 3, metric="ip")
    assert ip.centroids.shape == (3, 71)
    from tests import cosine_model, ip_model
    S = ip_model.auto_bound(oracle, w)
    l2 = tm.train(oracle, ip_model.augment_rows(oracle, w, S), 3)
    assert np.array_equal(ip.centroids, l2.centroids[:, :71]) and not l2.centroids[:, 71:].any()
    cs = tm.train(oracle, w, 3, metric="cosine")
    assert np.array_equal(cs.centroids, tm.train(oracle, cosine_model.normalize_rows(oracle, w), 3).centroids[:, :70])
    with pytest.raises(ValueError):
        tm.train(oracle, w, 3, metric="ip", max_sq_norm=1.0)              # a sample row above the bound
