"""Multi-vector search on the GPU: every output of rq_maxsim_scores and rq_query_batch_maxsim, bit for bit, against
the numpy model of tests/maxsim_model.py fed the same index's widened rows (the end-to-end entry also the same index's plain call
at topk = fetch), with and without the matrix-core pass; one check against a plain f64 Chamfer sum at rtol 1e-5.

Run on the GPU box:  python -m pytest tests/test_maxsim_gpu.py -m gpu -q
"""
import numpy as np
import pytest

from tests import maxsim_model as M
from tests import synth

pytestmark = pytest.mark.gpu

K, N, B = 16, 4000, 4
INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def rq():
    import os
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


_INDEX = {}


def index(rq, kind):
    """-> (index, raw token length, live mask by position or None): built once per kind, closed with the process"""
    if kind in _INDEX:
        return _INDEX[kind]
    d = {"l2_192": 192, "l2_100": 100, "l2_512": 512}.get(kind, 64)
    dim = -(-(d + (kind == "ip")) // 64) * 64
    x, centres, _ = synth.mixture(N, d, K, sigma=0.8, seed=900 + d, centre_scale=0.6)
    P, live = synth.random_orthogonal(dim, seed=78), None
    if kind == "f16":
        g = rq.RaBitQ.build(x.astype(np.float16), centres, P)
    elif kind == "u8":
        g = rq.RaBitQ.build(np.clip(np.rint(x * 40.0 + 128.0), 0, 255).astype(np.uint8), centres * 40.0 + 128.0, P, rows="u8")
    elif kind in ("cosine", "ip"):
        g = rq.RaBitQ.build(x, centres, P, metric=kind)
    elif kind == "holes":      # stride 40: a third of the ids never added (id % 3 == 2 outside 800 .. 1199; 1200 .. 1239), some removed:
        g = rq.RaBitQ.build(x[:400], centres, P)   # documents of 1 row (12), of 33 rows (20) and without a live row (30, 50)
        ids = np.array([i for i in range(400, N) if (i % 3 != 2 or 800 <= i < 1200) and not 1200 <= i < 1240], dtype=np.uint32)
        g.add(x[ids], ids=ids)
        dead = np.concatenate([np.arange(481, 520), np.arange(800, 840)[[1, 3, 6, 9, 10, 12, 15]], np.arange(2000, 2040)])
        g.remove(ids=np.intersect1d(dead, g.map_ids).astype(np.uint32), lazy=True)
        live = ~np.isin(g.map_ids, dead)
    elif kind == "sparse":     # ids far above 4 n + 65536: the directory is the hash table
        g = rq.RaBitQ.build(x[:64], centres, P)
        g.add(x[64:], ids=np.arange(64, N, dtype=np.uint32) + np.uint32(1 << 28))
    elif kind == "margin":     # one large common vector plus differences below bf16 resolution; document 0 (stride 64): 64 equal rows
        rng = np.random.default_rng(5)
        x = (np.full((1024, 64), 12.0) + rng.standard_normal((1024, 64)) * 1e-3).astype(np.float32)
        x[:64] = x[0]
        g = rq.RaBitQ.build(x, centres + 12.0, P)
    elif kind == "twins":      # rows 32 .. 63 equal rows 0 .. 31: documents 0 and 1 (stride 32) tie for every query
        x[32:64] = x[:32]
        g = rq.RaBitQ.build(x, centres, P)
    elif kind == "wild":       # a row with an inf element
        x = x[:512].copy()
        x[37, 3] = np.inf
        g = rq.RaBitQ.build(x, centres, P)
    else:
        g = rq.RaBitQ.build(x, centres, P)
    rows, found = g.fetch(g.map_ids, raw=False)
    assert np.array_equal(found, np.ones(g.n, dtype=bool) if live is None else live)
    _INDEX[kind] = (g, d, M.posmap_of(g.map_ids, live), np.ascontiguousarray(rows, dtype=np.float32))
    return _INDEX[kind]


def tokens(rq, kind, g, d, T, seed=7):
    """-> (raw tokens B x T x d, the prepared ones B x T x dim)"""
    t, _, _ = synth.mixture(B * T, d, K, sigma=0.8, seed=900 + d + seed, centre_scale=0.6)
    if kind == "u8":
        t = t * np.float32(40.0) + np.float32(128.0)
    if kind == "twins":        # the first query asks with the twin rows themselves: both documents are among its candidates
        t[:T] = synth.mixture(N, d, K, sigma=0.8, seed=900 + d, centre_scale=0.6)[0][:T]
    if kind == "margin":
        t = (12.0 + np.random.default_rng(seed).standard_normal((B * T, d)) * 1e-3).astype(np.float32)
    prep = np.zeros((B * T, g.dim), dtype=np.float32)
    prep[:, :d] = rq.normalize(t)[:, :d] if kind == "cosine" else t
    return t.reshape(B, T, d), prep.reshape(B, T, g.dim)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_scores(rq, kind, T, S, docs, n_tokens=None, counts=None, tok=None, fits=True):
    """both forms of the scoring equal the model bit for bit -> the stats of the prefiltered run, the scores, the prepared tokens
    (fits: the matrix pass's tiles fit in LDS at this dim and T; where they do not, the call must run exact-only by itself)"""
    g, d, posmap, base = index(rq, kind)
    raw, prep = tokens(rq, kind, g, d, T) if tok is None else tok
    want_s, want_r = M.scores(prep, n_tokens, docs, counts, S, posmap, base)
    stats = {}
    for pre in (False, True):
        s, r = g.maxsim_scores(raw, docs, S, n_tokens=n_tokens, counts=counts, prefilter=pre)
        stats = rq.last_maxsim_stats()
        assert np.array_equal(r, want_r), (kind, pre, "rows", np.argwhere(r != want_r)[:4])
        assert np.array_equal(bits(s), want_s), (kind, pre, "score", np.argwhere(bits(s) != want_s)[:4])
        assert stats["prefilter"] == int(pre and fits) and stats["rows_gathered"] == int(want_r.sum())
    return stats, want_s.view(np.float32), prep


def some_docs(top_id, S, seed=3):
    """B x 14 document numbers: ten random ones, the last (partly empty) document, two beyond the stored ids, a duplicate"""
    rng = np.random.default_rng(seed)
    last = (top_id - 1) // S
    rows = [np.concatenate([rng.integers(0, last, 10), [last, last + 1, 0xFFFFFFFF]]) for _ in range(B)]
    return np.array([np.append(r, r[2]) for r in rows], dtype=np.uint32)


# dim 64 / 192 (an odd number of 64-wide chunks) / 100 padded to 128; T 1 / 32 / 33 (second token tile mostly padding); stride 1 / 32 /
# 40 (second row tile partly empty); row types and metrics, not crossed.  The two forms the host picks by itself: T 256 (the f32 tokens
# do not fit beside the tiles and are read from global memory) and dim 512 (the tiles do not fit: exact-only without the flag)
SCORE_CASES = [("l2", 1, 1), ("l2", 32, 32), ("l2", 33, 40), ("l2_192", 32, 40), ("l2_100", 33, 32), ("f16", 32, 40), ("u8", 33, 32),
               ("cosine", 32, 40), ("ip", 33, 32), ("holes", 33, 40), ("sparse", 32, 32), ("l2", 256, 32), ("l2_512", 32, 40)]


@pytest.mark.parametrize("kind,T,S", SCORE_CASES)
def test_scores_equal_the_model(rq, kind, T, S):
    g = index(rq, kind)[0]
    top = int(g.map_ids.max()) + 1
    docs = some_docs(top, S)
    if kind == "sparse":
        docs[:, :10] += np.uint32((1 << 28) // S)
    if kind == "holes":
        docs[:, :4] = [12, 20, 30, 50]
    n_tokens = np.array([T, 0, 1, max(T - 13, 1)], dtype=np.uint32) if T > 1 else None
    counts = np.array([14, 11, 14, 0], dtype=np.uint32)
    stats, want, _ = check_scores(rq, kind, T, S, docs, n_tokens, counts, fits=kind != "l2_512")
    assert stats["tokens_in_lds"] == int(T < 256) or kind != "l2"        # dim 64: staged up to T 33, read from global memory at T 256
    if n_tokens is not None:                 # no token: +0.0 for every document that has a row
        assert (bits(want[1, :10])[np.isfinite(want[1, :10])] == 0).all()
    if kind == "l2" and T == 32:             # benign data: the matrix pass decides most pairs
        assert 0 < stats["exact_distances"] < stats["pairs"] and stats["list_overflows"] == 0


@pytest.mark.parametrize("kind", ["l2", "cosine"])
def test_scores_against_a_plain_f64_sum(rq, kind):
    g, d, posmap, base = index(rq, kind)
    docs = some_docs(N, 40)[:, :11]
    _, got, prep = check_scores(rq, kind, 33, 40, docs)
    for b in range(B):
        for c in range(11):
            ref = M.chamfer_f64(prep[b], 33, base, M.doc_positions(posmap, docs[b, c], 40))
            assert abs(float(got[b, c]) - ref) <= 1e-5 * abs(ref), (kind, b, c, got[b, c], ref)
    sim = g.maxsim_similarity(got, tokens(rq, kind, g, d, 33)[0])
    if kind == "cosine":                     # sum max cos, straight from the normalised rows and tokens
        pos = M.doc_positions(posmap, docs[0, 0], 40)
        ref = (prep[0].astype(np.float64) @ base[pos].astype(np.float64).T).max(axis=1).sum()
        assert abs(sim[0, 0] - ref) <= 1e-4, (sim[0, 0], ref)
    else:
        assert np.array_equal(sim, -got.astype(np.float64))


def test_margin_data_and_list_overflow(rq):
    docs = np.tile(np.arange(40, 54, dtype=np.uint32), (B, 1))               # two rows a document: the approximate arg-min is a coin toss,
    stats, _, _ = check_scores(rq, "margin", 32, 2, docs)                      # both rows are kept and the exact distance decides
    assert stats["exact_distances"] == stats["pairs"] and stats["list_overflows"] == 0
    stats, _, _ = check_scores(rq, "margin", 32, 64, np.zeros((B, 2), dtype=np.uint32))   # 64 equal rows: every row is kept
    assert stats["list_overflows"] > 0 and stats["exact_distances"] >= stats["pairs"]


def test_inf_row_and_nan_token(rq):
    g, d, _, _ = index(rq, "wild")
    raw, prep = tokens(rq, "wild", g, d, 33)
    raw[1, 2, 5] = prep[1, 2, 5] = np.nan
    check_scores(rq, "wild", 33, 32, np.tile(np.arange(16, dtype=np.uint32), (B, 1)), tok=(raw, prep))


@pytest.mark.parametrize("kind,T,S,fetch", [("l2", 32, 32, 16), ("l2_100", 33, 40, 20), ("holes", 33, 40, 20), ("u8", 1, 1, 64),
                                            ("cosine", 32, 40, 64), ("ip", 32, 32, 30), ("sparse", 33, 32, 16), ("twins", 32, 32, 16)])
def test_search_equals_the_model_on_the_plain_call(rq, kind, T, S, fetch):
    g, d, posmap, base = index(rq, kind)
    raw, prep = tokens(rq, kind, g, d, T, seed=11)
    n_tokens = np.array([T, max(T - 7, 1), 0, T], dtype=np.uint32)
    _, src_ids, src_cnt = g.query_batch(raw.reshape(B * T, d), 4, fetch)
    want = M.search(prep, n_tokens, src_ids, src_cnt, S, 10, posmap, base)
    for pre in (True, False):
        res = g.query_batch_maxsim(raw, 4, 10, S, fetch=fetch, n_tokens=n_tokens, prefilter=pre)
        assert np.array_equal(res.counts, want[2]) and np.array_equal(res.candidates, want[3]), (kind, pre, res.counts, res.candidates)
        assert np.array_equal(res.docs, want[1]), (kind, pre, "docs")
        assert np.array_equal(bits(res.dist), want[0]), (kind, pre, "dist")
    assert want[2][2] == 0 and want[2][0] == 10 and rq.last_maxsim_stats()["ms_source"] > 0.0
    # (a query without tokens has no candidate, so "all candidates tie" never reaches the selection from n_tokens = 0; the twins do it)
    if kind == "twins":                      # equal rows, equal sums: the selection orders the tie by document number
        assert want[1][0, :2].tolist() == [0, 1] and want[0][0, 0] == want[0][0, 1]


# (dim > 4096 is refused as well, but no index of that width can be built: every constructor refuses it first)
@pytest.mark.parametrize("what", ["source", "topk0", "topk", "stride0", "stride", "tokens", "shard", "tiered", "split_rows"])
def test_refusals(rq, what):
    from rabitq_amd import index as ix
    g, d, _, _ = index(rq, "l2")
    tok = np.zeros((2, 300 if what == "tokens" else 33, d), dtype=np.float32)
    held = []
    if what == "shard":
        g = g.shard(g.partition_lists(2)[0], 0)
        held.append(g)
    if what in ("tiered", "split_rows"):     # split_rows: every row in HBM, so the tier check passes and the split-row check refuses
        ix.set_option(*(("base_device_mb", 1) if what == "tiered" else ("split_rows", 2)))
        try:
            x, centres, _ = synth.mixture(6000, 64, K, sigma=0.8, seed=964, centre_scale=0.6)
            g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(64, seed=78))
        finally:
            ix.set_option("base_device_mb", -1)
            ix.set_option("split_rows", 1)
        held.append(g)
        assert g.n_hbm < g.n if what == "tiered" else (g.split_rows and g.n_hbm == g.n)
    kw = {"source": dict(topk=10, doc_stride=32, fetch=63), "topk0": dict(topk=0, doc_stride=32, fetch=8),
          "topk": dict(topk=2049, doc_stride=32, fetch=8), "stride0": dict(topk=10, doc_stride=0, fetch=8),
          "stride": dict(topk=10, doc_stride=4097, fetch=8)}.get(what, dict(topk=10, doc_stride=32, fetch=8))
    try:
        with pytest.raises(rq.RabitqError) as e:
            g.query_batch_maxsim(tok, 4, **kw)
        assert e.value.status == (INVALID if what in ("stride0", "stride", "tokens") else UNSUPPORTED), str(e.value)
        assert what not in ("tiered", "split_rows") or what.split("_")[0] in str(e.value)
        if what in ("shard", "tiered", "split_rows", "stride0", "tokens"):
            with pytest.raises(rq.RabitqError) as e:
                g.maxsim_scores(tok, np.zeros((2, 3), dtype=np.uint32), kw["doc_stride"])
            assert e.value.status == (INVALID if what in ("stride0", "tokens") else UNSUPPORTED), str(e.value)
    finally:
        for h in held:
            h.close()
