"""Restricted postings on the GPU: p.restrict(f) against plain numpy on tests.maxsim_keyed_model.segments -- every
segment cut down to its admitted positions, the emptied ones dropped -- on the corpus of tests/test_maxsim_exact_gpu.py (2983 rows:
a chunk boundary of 2048 postings falls inside a document)."""
import numpy as np
import pytest

from tests.test_maxsim_exact_gpu import KEY, LENS, N, corpus, index, tokens, bits, rq  # noqa: F401

pytestmark = pytest.mark.gpu

FILTERS = ["half", "whole", "rows", "all", "none"]
_MADE = {}


def restricted(rq, kind, fname):
    """-> (the index's dict, the filter, {column type: the numpy restriction of its segments}); made once per (kind, filter)"""
    if (kind, fname) not in _MADE:
        w = index(rq, kind)
        g, doc, segs = w["g"], corpus(kind)[2], w["segs"]["u32"]
        ids = {"half": np.arange(0, N, 2),                                    # a cut inside every tile
               "whole": np.flatnonzero(np.isin(doc, [1, 4, 6, 9, 10, 20])),   # whole documents, one of the twins 6 / 7
               "rows": g.map_ids[[segs[KEY["u32"](3)][-1], segs[KEY["u32"](5)][-1]]],   # the 33rd row of document 3, the last of 5
               "all": np.arange(N), "none": np.empty(0, dtype=np.int64)}[fname]
        adm = np.isin(g.map_ids, ids)
        f = g.make_filter(mask=np.isin(np.arange(N), ids))
        _MADE[kind, fname] = w, f, {t: cut(s, adm) for t, s in w["segs"].items()}
    return _MADE[kind, fname]


def cut(segs, adm):
    return {v: [p for p in pos if adm[p]] for v, pos in segs.items() if adm[pos].any()}


def same(q, want, keys):
    assert q.values.tolist() == sorted(want) and q.rows == sum(map(len, want.values()))
    assert q.count_of(keys).tolist() == [len(want.get(int(k), [])) for k in keys]
    for v, pos in want.items():
        assert np.array_equal(q.positions(v), np.array(pos, dtype=np.uint32)), v


@pytest.mark.parametrize("ctype", ["u32", "i64"])
@pytest.mark.parametrize("fname", FILTERS)
def test_restrict_equals_numpy(rq, fname, ctype):
    w, f, want = restricted(rq, "l2", fname)
    p = w["post"][ctype]
    with p.restrict(f) as q:
        same(q, want[ctype], p.values)
        assert q.type == p.type and q.column == p.column
        if fname == "all":
            assert np.array_equal(q.values, p.values) and np.array_equal(q.counts, p.counts)
        if fname == "none":
            assert q.values.size == 0 and q.rows == 0


def test_every_row_its_own_document(rq):
    """2983 segments, more than one block of the segment pass, every third id admitted"""
    g = index(rq, "l2")["g"]
    g.create_attr("own", "u32", fill=0)
    g.set_attr("own", np.arange(N, dtype=np.uint32), 5 * np.arange(N))
    with g.postings("own") as p, p.restrict(g.make_filter(ids=np.arange(0, N, 3))) as q:
        same(q, {5 * int(i): [pos] for pos, i in enumerate(g.map_ids) if i % 3 == 0}, p.values)


def test_keyed_search_by_restricted_postings(rq):
    w, f, _ = restricted(rq, "l2", "half")
    g, p = w["g"], w["post"]["u32"]
    qv = tokens(rq, "l2", w, 2, 4)[0].reshape(8, -1)
    keys = [KEY["u32"](j) for j in (0, 3, 5, 5, 6, 7, 20, 47)]
    with p.restrict(f) as q:
        a, b = g.exact_search_keyed(qv, keys, 5, by=q), g.exact_search_keyed(qv, keys, 5, by=p, filter=f)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[2].max() == 5
