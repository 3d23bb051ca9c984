"""The numpy model of MaxSim by postings (tests/maxsim_keyed_model.py) on hand cases -- no GPU."""
import numpy as np
import pytest

from tests import maxsim_keyed_model as M


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(33)
    base = rng.standard_normal((40, 64)).astype(np.float32)
    base[20:24] = base[10:14]                                  # the rows of key 3 equal the rows of key -5
    col = np.full(40, 9, dtype=np.int64)
    col[10:14], col[20:24], col[30] = -5, 3, 7                 # key 7: a one-row document
    return base, rng.standard_normal((2, 5, 64)).astype(np.float32), col


def test_scores_on_hand_cases(data):
    base, tok, col = data
    segs = M.segments(col)
    keys = np.array([[7, 100, 9, 9, -5], [3, -5, 7, 7, 7]], dtype=np.int64)
    sb, rows = M.scores(tok, [5, 2], keys, [5, 2], segs, base)
    assert rows.tolist() == [[1, 0, 31, 31, 4], [4, 4, 0, 0, 0]]
    assert sb[0, 1] == M.NAN_BITS and (sb[1, 2:] == M.NAN_BITS).all()           # an absent key; slots past counts
    assert sb[0, 2] == sb[0, 3] and sb[1, 0] == sb[1, 1]                        # a duplicate; equal rows under two keys
    one = ((base[30].astype(np.float64) - tok[0].astype(np.float64)) ** 2).sum()   # one row: every token's minimum is that row
    assert abs(float(sb[0, :1].view(np.float32)[0]) - one) <= 1e-5 * one
    assert abs(float(sb[0, 4:5].view(np.float32)[0]) - M.chamfer_f64(tok[0], 5, base, segs[-5])) <= 1e-5 * one


def test_search_orders_a_tie_by_signed_key_and_a_nan_token_poisons_the_sum(data):
    base, tok, col = data
    posmap = {i: i for i in range(40)}
    src = np.tile(np.array([10, 21, 30, 0], dtype=np.uint32), (10, 1))         # every token found rows of keys -5, 3, 7 and 9
    db, keys, cnt, ncand = M.search(tok, [5, 0], src, np.full(10, 4), 3, posmap, col, M.segments(col), base)
    assert cnt.tolist() == [3, 0] and ncand.tolist() == [4, 0] and (db[1] == M.NAN_BITS).all() and (keys[1] == 0).all()
    at = keys[0].tolist().index(-5)
    assert keys[0, at + 1] == 3 and db[0, at] == db[0, at + 1]                 # the tie: -5 before 3, the i64 order
    now = col.copy()
    now[10] = 77                                                               # the live column routes row 10 to a key without a segment
    assert M.search(tok, [5, 0], src[:, :1], np.full(10, 1), 3, posmap, now, M.segments(col), base)[3].tolist() == [0, 0]
    bad = tok.copy()
    bad[0, 1, 3] = np.nan
    db, _, cnt, _ = M.search(bad, [5, 0], src, np.full(10, 4), 4, posmap, col, M.segments(col), base)
    assert cnt[0] == 4 and (db[0] == M.NAN_BITS).all()
