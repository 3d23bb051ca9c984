"""Exact multi-vector search on the GPU: dist bits, keys and counts of rq_exact_search_maxsim against
tests/maxsim_exact_model.py fed the same index's widened rows and column, with the bound pass and without it."""
import numpy as np
import pytest

from tests import exact_scan_cases as X
from tests import maxsim_exact_model as M
from tests import synth
from tests.test_maxsim_gpu import bits, rq  # noqa: F401  (the same library fixture and bit view)

pytestmark = pytest.mark.gpu

K = 8
# document lengths: a short tile, an exact tile, a tile plus one row, many tiles (the position prefetch), twins (6 and 7), the rest
LENS = [1, 31, 32, 33, 100, 700, 3, 3] + [52] * 40
N = sum(LENS)
KEY = {"u32": lambda j: 7 * j + 3, "i64": lambda j: j - 5}
_INDEX = {}


def corpus(kind):
    """-> (x, centres, doc of every id, d): document j owns LENS[j] ids of a random permutation; documents 6 and 7 hold equal rows"""
    d = {"l2_128": 128, "l2_100": 100}.get(kind, 64)
    x, centres, _ = synth.mixture(N, d, K, sigma=0.8, seed=700 + d, centre_scale=0.6)
    doc = np.empty(N, dtype=np.int64)
    doc[np.random.default_rng(23).permutation(N)] = np.repeat(np.arange(len(LENS)), LENS)
    x[doc == 7] = x[doc == 6]
    return x, centres, doc, d


def index(rq, kind):
    """-> dict(g, d, base, post, segs, col): built once per kind"""
    if kind in _INDEX:
        return _INDEX[kind]
    if kind == "margin":           # rows and tokens on which bf16 is as wrong as it can be; documents of 8 rows
        c = X.margin_case(64)
        x, centres, d, doc = c["x"], c["centres"], 64, np.arange(len(c["x"])) // 8
        g = rq.RaBitQ.build(x, centres, c["P"])
    else:
        x, centres, doc, d = corpus(kind)
        P = synth.random_orthogonal(-(-(d + (kind == "ip")) // 64) * 64, seed=78)
        if kind == "wild":
            x[np.flatnonzero(doc == 2)[0], 3] = np.nan
        if kind == "f16":
            g = rq.RaBitQ.build(x.astype(np.float16), centres, P)
        elif kind == "u8":
            g = rq.RaBitQ.build(np.clip(np.rint(x * 40.0 + 128.0), 0, 255).astype(np.uint8), centres * 40.0 + 128.0, P, rows="u8")
        else:
            g = rq.RaBitQ.build(x, centres, P, **({"metric": kind} if kind in ("cosine", "ip") else {}))
    post, segs = {}, {}
    for t, key in KEY.items():
        g.create_attr("doc_" + t, t, fill=0)
        g.set_attr("doc_" + t, np.arange(g.n, dtype=np.uint32), np.array([key(int(j)) for j in doc]))
        post[t], segs[t] = g.postings("doc_" + t), M.segments(g.attr_array("doc_" + t))
    rows, found = g.fetch(g.map_ids, raw=False)
    assert found.all()
    _INDEX[kind] = dict(g=g, d=d, base=np.ascontiguousarray(rows, dtype=np.float32), post=post, segs=segs)
    return _INDEX[kind]


def tokens(rq, kind, w, nq, T):
    """-> (raw nq x T x d, prepared nq x T x dim); query 0 asks with rows of the twin documents, so both lead its result and tie"""
    d = w["d"]
    if kind == "margin":
        t = X.margin_case(64)["q"][:nq * T]
    else:
        t, _, _ = synth.mixture(nq * T, d, K, sigma=0.8, seed=811 + d, centre_scale=0.6)
        t[:T] = corpus(kind)[0][corpus(kind)[2] == 6][np.arange(T) % 3]
        if kind == "u8":
            t = t * np.float32(40.0) + np.float32(128.0)
    prep = np.zeros((nq * T, w["g"].dim), dtype=np.float32)
    prep[:, :d] = rq.normalize(t)[:, :d] if kind == "cosine" else t
    return np.ascontiguousarray(t.reshape(nq, T, d)), prep.reshape(nq, T, w["g"].dim)


def check(rq, kind, T, nq, topk, ctype, tok=None, image_in_lds=1):
    """both forms equal the model bit for bit -> (the model's result, the stats of the run with the bound pass)"""
    w = index(rq, kind)
    g, p = w["g"], w["post"][ctype]
    if nq == "chunk+1":            # one query more than a chunk of the bound pass holds: a second chunk with one query
        g.exact_search_maxsim(np.zeros((1, T, w["d"]), dtype=np.float32), 1, by=p)
        nq = rq.last_maxsim_exact_stats()["chunk_queries"] + 1
    raw, prep = tokens(rq, kind, w, nq, T) if tok is None else tok
    n_tokens = np.array([T, max(T - 2, 1), 1][:nq] + [T] * max(nq - 3, 0), dtype=np.uint32) if T > 1 else None
    want = M.search(prep, n_tokens, topk, w["segs"][ctype], w["base"], g.attr_array("doc_" + ctype).dtype)
    for pre in (True, False):
        res = g.exact_search_maxsim(raw, topk, by=p, n_tokens=n_tokens, prefilter=pre)
        st = rq.last_maxsim_exact_stats()
        assert np.array_equal(res.counts, want[2]) and res.docs.dtype == want[1].dtype, (kind, pre, res.counts)
        assert np.array_equal(res.docs, want[1]), (kind, pre, "keys", np.argwhere(res.docs != want[1])[:4])
        assert np.array_equal(bits(res.dist), want[0]), (kind, pre, "dist", np.argwhere(bits(res.dist) != want[0])[:4])
        assert st["prefilter"] == int(pre) and st["documents"] == len(w["segs"][ctype]) and st["survivors"] >= int(want[2].sum())
        if pre:
            assert st["image_in_lds"] == image_in_lds and st["query_chunks"] == -(-nq // st["chunk_queries"])
            stats = st
    return want, stats


@pytest.mark.parametrize("kind,T,nq,topk,ctype", [
    ("l2", 5, "chunk+1", 10, "u32"), ("l2", 33, 3, 1, "i64"), ("l2_128", 33, 3, 10, "u32"), ("l2_128", 5, "chunk+1", 10, "i64"),
    ("l2_100", 1, 1, 100, "i64"), ("f16", 5, 3, 10, "u32"), ("f16", 33, 1, 10, "u32"), ("u8", 5, 3, 10, "i64"), ("u8", 33, 1, 10, "u32"),
    ("cosine", 5, 3, 10, "u32"), ("ip", 5, 3, 10, "i64"), ("margin", 16, 2, 10, "u32")])
def test_search_equals_the_model(rq, kind, T, nq, topk, ctype):
    want, stats = check(rq, kind, T, nq, topk, ctype)
    if kind not in ("margin", "ip"):   # the twins tie for every query and lead query 0: the smaller key first (i64: 1 before 2)
        assert topk == 1 or want[0][0, 0] == want[0][0, 1]
        assert want[1][0, :2].tolist() == [KEY[ctype](6), KEY[ctype](7)][:topk]
    if topk == 100:                # more than the postings hold: every document, padding behind
        assert want[2][0] == len(LENS) and (want[0][0, len(LENS):] == M.NAN_BITS).all()


def test_image_read_through_the_l2(rq):
    """dim 128, T = 65: not even two queries' images fit beside the waves' regions, so the bound pass reads them from workspace memory"""
    check(rq, "l2_128", 65, 3, 10, "u32", image_in_lds=0)


def test_nan_row_and_nan_token(rq):
    w = index(rq, "wild")
    raw, prep = tokens(rq, "wild", w, 3, 5)
    raw[1, 2, 5] = prep[1, 2, 5] = np.nan
    want, _ = check(rq, "wild", 5, 3, 10, "u32", tok=(raw, prep))
    assert (want[0][1, :10] == M.NAN_BITS).all() and want[2][1] == 10   # a NaN token: every sum is the one NaN, the keys ascend


def test_the_bound_pass_prunes(rq):
    """query b's tokens are rows of document b: tests/test_maxsim_exact_model.py shows on the CPU that the model's own L / U leave at
    most half of the (query, document) pairs; the engine's float32 bounds differ from those by roundings the margin's slack covers"""
    w = index(rq, "l2")
    raw, prep = planted_tokens()
    want, stats = check(rq, "l2", 5, 3, 1, "u32", tok=(raw, prep))
    assert stats["survivors"] < 3 * len(LENS)


def planted_tokens():
    x, _, doc, _ = corpus("l2")
    t = np.stack([x[doc == j][np.arange(5) % LENS[j]] for j in (4, 5, 8)])
    return t, t.copy()


def test_maxsim_recall_is_the_pooled_fraction(rq):
    w = index(rq, "l2")
    g, p = w["g"], w["post"]["u32"]
    raw, _ = tokens(rq, "l2", w, 3, 5)
    truth, got = g.exact_search_maxsim(raw, 10, by=p), g.query_batch_maxsim(raw, 1, 10, fetch=4, by=p)
    hit = sum(len(set(got.docs[b, :got.counts[b]]) & set(truth.docs[b, :truth.counts[b]])) for b in range(3))
    assert g.maxsim_recall(raw, 1, 10, by=p, fetch=4) == hit / int(truth.counts.sum()) and 0 < hit
    with pytest.raises(rq.RabitqError):
        g.maxsim_recall(raw, 1, 10, by=p, filter=g.make_filter(ids=np.arange(4, dtype=np.uint32)))
