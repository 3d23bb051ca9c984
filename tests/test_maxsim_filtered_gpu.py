"""The exact multi-vector search under a filter: exact_search_maxsim(..., filter=f) against
tests/maxsim_exact_model.py fed the numpy restriction of the segments, bit for bit, and against the same search by p.restrict(f)."""
import numpy as np
import pytest

from tests import maxsim_exact_model as M
from tests.test_maxsim_exact_gpu import tokens, bits, rq  # noqa: F401
from tests.test_postings_restrict_gpu import restricted

pytestmark = pytest.mark.gpu
_TOKENS = {}


@pytest.mark.parametrize("fname", ["half", "whole", "rows", "none"])
@pytest.mark.parametrize("kind,T,nq,topk,ctype", [("l2", 5, 3, 10, "u32"), ("l2_128", 33, 3, 10, "i64"), ("u8", 5, 3, 10, "u32")])
def test_filtered_search_equals_the_model(rq, kind, T, nq, topk, ctype, fname):
    w, f, segs = restricted(rq, kind, fname)
    g, p = w["g"], w["post"][ctype]
    if kind not in _TOKENS:
        _TOKENS[kind] = tokens(rq, kind, w, nq, T)
    raw, prep = _TOKENS[kind]
    want = M.search(prep, None, topk, segs[ctype], w["base"], g.attr_array("doc_" + ctype).dtype)
    with p.restrict(f) as q:
        got = [g.exact_search_maxsim(raw, topk, by=q)]
    for pre in (True, False):
        got.append(g.exact_search_maxsim(raw, topk, by=p, filter=f, prefilter=pre))
        assert rq.last_maxsim_exact_stats()["documents"] == len(segs[ctype])
    for res in got:
        assert np.array_equal(res.counts, want[2]) and res.docs.dtype == want[1].dtype, (fname, res.counts)
        assert np.array_equal(res.docs, want[1]), (fname, "keys", np.argwhere(res.docs != want[1])[:4])
        assert np.array_equal(bits(res.dist), want[0]), (fname, "dist", np.argwhere(bits(res.dist) != want[0])[:4])
    assert int(want[2].max()) == min(topk, len(segs[ctype]))
    if fname == "none":
        assert not got[1].counts.any() and (bits(got[1].dist) == M.NAN_BITS).all()
