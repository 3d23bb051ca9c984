"""The model of diverse search (tests/diverse_model.py) against itself and against hand cases: the incremental form and the one
that recomputes div from the full matrix of pair distances agree, and the contract's corner cases come out as the header says.
No GPU needed (D is oracle.l2_squared_distance_rows)."""
import numpy as np
import pytest

from tests import diverse_model as M

INF_BITS = 0x7F800000


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def f32(b):
    return np.array(b, dtype=np.uint32).view(np.float32)


def same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("seed", range(6))
def test_the_two_forms_agree_on_random_inputs(seed):
    rng = np.random.default_rng(seed)
    n, dim, B, F = 60, 64, 5, 24
    base = rng.standard_normal((n, dim)).astype(np.float32)
    base[1::7] = base[0:-1:7][:len(base[1::7])]                                # twins: pair distance 0
    posmap = {int(i): p for p, i in enumerate(rng.permutation(n) + 100)}
    ids = np.stack([rng.choice(np.arange(95, 100 + n), size=F, replace=False) for _ in range(B)]).astype(np.uint32)   # 5 absent ids
    dist = (rng.integers(0, 9, size=(B, F)) / 4).astype(np.float32)          # many ties
    dist[2, 3] = np.inf
    cnt = np.array([F, 0, F, 7, F - 1], dtype=np.uint32)
    for lam in (0.0, 0.3, 0.5, 1.0):
        for topk in (1, 5, F):
            a = M.diversify_rows(dist, ids, cnt, posmap, base, topk, lam, select=M.select_incremental)
            b = M.diversify_rows(dist, ids, cnt, posmap, base, topk, lam, select=M.select_from_matrix)
            same(a, b)
            assert a["n"][1] == 0 and (a["ids"][1] == M.PAD_ID).all()
            assert a["candidates"] == int(cnt.sum()) and a["taken"] == int(a["n"].sum())
            if lam == 1.0:                                                      # the source's first topk candidates in (distance, id) order
                for r in range(B):
                    c, _, _ = M.candidates(dist[r], ids[r], cnt[r], posmap)
                    assert list(a["ids"][r, :a["n"][r]]) == [x[1] for x in c[:topk]]
            if topk == 1:
                for r in range(B):
                    c, _, _ = M.candidates(dist[r], ids[r], cnt[r], posmap)
                    assert a["n"][r] == min(1, len(c)) and (not c or a["ids"][r, 0] == c[0][1])


def twin_case():
    """A (rel 1.0), A' (rel 1.1, D(A, A') = 0), B (rel 2.0, D = 10 to both)"""
    base = np.zeros((3, 64), dtype=np.float32)
    base[2, 0] = np.float32(3.0)
    base[2, 1] = np.float32(1.0)                                                # 9 + 1 = 10, exactly
    posmap = {10: 0, 11: 1, 12: 2}
    dist = np.array([[1.0, 1.1, 2.0]], dtype=np.float32)
    ids = np.array([[10, 11, 12]], dtype=np.uint32)
    return base, posmap, dist, ids


def test_twins_are_separated_by_diversity_and_not_by_relevance():
    base, posmap, dist, ids = twin_case()
    cnt = np.array([3], dtype=np.uint32)
    r = M.diversify_rows(dist, ids, cnt, posmap, base, 3, 0.5)
    assert list(r["ids"][0]) == [10, 12, 11] and r["n"][0] == 3                 # A, B, A'
    assert list(r["div_bits"][0]) == [INF_BITS, bits([10.0])[0], bits([0.0])[0]]
    assert np.array_equal(r["dist_bits"][0], bits([1.0, 2.0, 1.1]))
    assert r["pair_distances"] == 2 + 1
    r = M.diversify_rows(dist, ids, cnt, posmap, base, 3, 1.0)
    assert list(r["ids"][0]) == [10, 11, 12]                                    # A, A', B
    for perm in ([2, 0, 1], [1, 2, 0]):                                         # any order of a row's pairs
        p = M.diversify_rows(dist[:, perm], ids[:, perm], cnt, posmap, base, 3, 0.5)
        assert list(p["ids"][0]) == [10, 12, 11]


def test_short_empty_absent_and_non_finite():
    base, posmap, dist, ids = twin_case()
    r = M.diversify_rows(dist, ids, np.array([0], dtype=np.uint32), posmap, base, 2, 0.5)                # cnt = 0
    assert r["n"][0] == 0 and (r["ids"] == M.PAD_ID).all() and (r["dist_bits"] == M.NAN_BITS).all() and (r["div_bits"] == M.NAN_BITS).all()
    r = M.diversify_rows(dist, ids, np.array([2], dtype=np.uint32), posmap, base, 3, 0.5)                # cnt < topk
    assert r["n"][0] == 2 and list(r["ids"][0]) == [10, 11, M.PAD_ID] and r["div_bits"][0, 2] == M.NAN_BITS
    r = M.diversify_rows(dist, np.array([[10, 99, 12]], dtype=np.uint32), np.array([3], dtype=np.uint32), posmap, base, 3, 0.5)
    assert r["absent"] == 1 and r["n"][0] == 2 and list(r["ids"][0]) == [10, 12, M.PAD_ID]              # an absent id
    for bad in (np.inf, -np.inf, np.nan):                                      # a non-finite distance
        d = dist.copy()
        d[0, 1] = bad
        r = M.diversify_rows(d, ids, np.array([3], dtype=np.uint32), posmap, base, 3, 0.5)
        assert r["skipped"] == 1 and r["absent"] == 0 and list(r["ids"][0]) == [10, 12, M.PAD_ID], bad
    d = dist.copy()
    d[0, 1] = np.inf                                                           # absent AND not finite: counted as absent
    r = M.diversify_rows(d, np.array([[10, 99, 12]], dtype=np.uint32), np.array([3], dtype=np.uint32), posmap, base, 3, 0.5)
    assert (r["absent"], r["skipped"]) == (1, 0)
    r = M.diversify_rows(dist, ids, np.array([9], dtype=np.uint32), posmap, base, 3, 0.5)                # a larger cnt is cut at fetch
    assert r["candidates"] == 3 and r["n"][0] == 3


def test_duplicate_ids_are_separate_candidates():
    base, posmap, _, _ = twin_case()
    dist = np.array([[1.0, 1.0, 2.0, 1.0]], dtype=np.float32)
    ids = np.array([[10, 10, 12, 10]], dtype=np.uint32)
    r = M.diversify_rows(dist, ids, np.array([4], dtype=np.uint32), posmap, base, 4, 0.5)
    assert r["n"][0] == 4 and list(r["ids"][0]) == [10, 12, 10, 10]            # the copies tie on score: place decides
    assert list(r["div_bits"][0]) == [INF_BITS, bits([10.0])[0], 0, 0]


def test_tied_scores_are_decided_by_place_and_lambda_zero_is_diversity_alone():
    base = np.zeros((4, 64), dtype=np.float32)
    base[1, 0], base[2, 1], base[3, 0] = 2.0, 2.0, 1.0                          # D(0,1) = D(0,2) = 4, D(0,3) = 1, D(1,2) = 8
    posmap = {0: 0, 1: 1, 2: 2, 3: 3}
    ids = np.array([[0, 1, 2, 3]], dtype=np.uint32)
    dist = np.array([[0.5, 1.0, 1.0, 1.0]], dtype=np.float32)
    cnt = np.array([4], dtype=np.uint32)
    r = M.diversify_rows(dist, ids, cnt, posmap, base, 2, 0.5)
    assert list(r["ids"][0]) == [0, 1]                                          # 1 and 2 tie (rel 1, div 4): the earlier place
    r = M.diversify_rows(dist, ids[:, [0, 2, 1, 3]], cnt, posmap, base, 2, 0.5)
    assert list(r["ids"][0]) == [0, 1]                                          # ... which is the smaller id, however the row arrives
    r = M.diversify_rows(np.array([[0.5, 3.0, 2.0, 1.0]], dtype=np.float32), ids, cnt, posmap, base, 4, 0.0)
    assert list(r["ids"][0]) == [0, 2, 1, 3]                                    # lambda = 0: rel only orders the candidates; 1 and 2 tie on
    assert list(r["div_bits"][0]) == [INF_BITS] + list(bits([4.0, 4.0, 1.0]))   # div 4, place (by rel) decides; then D(1, 2) = 8 > 4 keeps 1
    assert M.score_key(np.float32(1.0), np.float32(0.0), np.float32(1.0), M.INF, 3) == (int(M.ord32_biased(f32([M.NAN_BITS])[0])) << 32) | 3
