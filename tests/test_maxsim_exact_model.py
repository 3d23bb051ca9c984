"""CPU checks of the model of exact multi-vector search (tests/maxsim_exact_model.py) on the GPU cases' own inputs: the restated
bounds enclose the score, the ranking agrees with a plain f64 Chamfer sum where scores are well separated, and the planted case of
tests/test_maxsim_exact_gpu.py leaves at most half of the (query, document) pairs by the model's own L / U."""
import numpy as np

from tests import maxsim_exact_model as M
from tests.maxsim_model import chamfer_f64
from tests.test_maxsim_exact_gpu import KEY, LENS, corpus, planted_tokens


def scored(tok, n_tok):
    """every document of the l2 corpus (the stored rows of an f32 l2 index are the rows as given) -> keys, scores, L, U"""
    x, _, doc, _ = corpus("l2")
    segs = M.segments(np.array([KEY["u32"](int(j)) for j in doc]))
    keys = sorted(segs)
    s = np.array([M.chamfer(tok, n_tok, x, segs[k]) for k in keys], dtype=np.float64)
    lu = np.array([M.bounds(tok, n_tok, x, segs[k]) for k in keys])
    return keys, segs, x, s, lu[:, 0], lu[:, 1]


def test_bounds_enclose_the_score_and_the_ranking_is_the_f64_one():
    tok = planted_tokens()[1][1]
    keys, segs, x, s, L, U = scored(tok, 5)
    assert (L <= s).all() and (s <= U).all() and (U - L < 0.2 * np.median(s)).all()
    got = M.search(tok[None], None, len(keys), segs, x, np.uint32)
    ref = np.array([chamfer_f64(tok, 5, x, segs[k]) for k in keys])
    order = np.argsort(ref)
    apart = np.diff(ref[order]) > 1e-4 * ref[order][1:]          # neighbours in the f64 order that f32 rounding cannot swap
    model = [keys.index(int(k)) for k in got[1][0]]
    assert got[2][0] == len(LENS) and all(model.index(order[i]) < model.index(order[i + 1]) for i in np.flatnonzero(apart))


def test_the_planted_case_prunes_by_the_models_own_bounds():
    left = 0
    for b, n_tok in enumerate((5, 3, 1)):
        _, _, _, _, L, U = scored(planted_tokens()[1][b], n_tok)
        left += int((L <= np.sort(U)[0]).sum())                   # topk = 1: tau is the smallest U
    assert 3 <= left <= 3 * len(LENS) // 2
