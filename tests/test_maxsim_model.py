"""The numpy model of multi-vector search (tests/maxsim_model.py) against a plain f64 Chamfer sum, its ordering rules, and the
identities behind RaBitQ.maxsim_similarity -- no GPU."""
import numpy as np
import pytest

from tests import maxsim_model as M


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(31)
    base = rng.standard_normal((200, 64)).astype(np.float32)
    tok = rng.standard_normal((3, 5, 64)).astype(np.float32)
    return base, tok, {i: i for i in range(200) if i % 7 != 3}


def test_model_equals_the_f64_sum(data):
    base, tok, posmap = data
    cand = np.array([[0, 3, 9, 3, 50], [1, 2, 19, 0, 0], [4, 4, 4, 4, 4]], dtype=np.uint32)
    sb, rows = M.scores(tok, [5, 2, 0], cand, [5, 3, 5], 10, posmap, base)
    for b, nt in enumerate((5, 2, 0)):
        for c in range(5):
            pos = M.doc_positions(posmap, cand[b, c], 10)
            if c >= (5, 3, 5)[b] or not pos:
                assert sb[b, c] == M.NAN_BITS and rows[b, c] == 0
                continue
            ref = M.chamfer_f64(tok[b], nt, base, pos)
            assert rows[b, c] == len(pos) and abs(float(sb[b, c:c + 1].view(np.float32)[0]) - ref) <= 1e-5 * abs(ref)
    assert (sb[2] == 0).all() and sb[0, 1] == sb[0, 3]       # no token: +0.0; a duplicate is scored independently, equally


def test_search_orders_by_score_then_document(data):
    base, tok, posmap = data
    src = np.tile(np.arange(0, 200, 7, dtype=np.uint32)[:20], (15, 1))
    db, docs, cnt, ncand = M.search(tok, [5, 0, 3], src, np.full(15, 20), 10, 4, posmap, base)
    assert cnt.tolist() == [4, 0, 4] and ncand.tolist() == [14, 0, 14] and (docs[1] == M.PAD_DOC).all() and (db[1] == M.NAN_BITS).all()
    d0 = db[0].view(np.float32)
    assert (np.diff(d0) >= 0).all()


def test_similarity_identities(data):
    """cosine: sum max cos = T - chamfer / 2; ip (rows augmented to squared norm S): sum max <x, q> = (T S + sum |q|^2 - chamfer) / 2"""
    base, tok, _ = data
    x, q = base[:10].astype(np.float64), tok[0].astype(np.float64)
    xn, qn = x / np.linalg.norm(x, axis=1, keepdims=True), q / np.linalg.norm(q, axis=1, keepdims=True)
    ch = ((xn[None] - qn[:, None]) ** 2).sum(axis=2).min(axis=1).sum()
    assert abs((5 - ch / 2) - (qn @ xn.T).max(axis=1).sum()) < 1e-9
    S = float((x ** 2).sum(axis=1).max())
    xa = np.hstack([x, np.sqrt(S - (x ** 2).sum(axis=1))[:, None]])
    qa = np.hstack([q, np.zeros((5, 1))])
    ch = ((xa[None] - qa[:, None]) ** 2).sum(axis=2).min(axis=1).sum()
    assert abs((5 * S + (q ** 2).sum() - ch) / 2 - (q @ x.T).max(axis=1).sum()) < 1e-9
