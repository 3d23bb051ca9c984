"""Multi-vector search over documents named by a column, on the GPU: every output of rq_maxsim_scores_keyed and
rq_query_batch_maxsim_keyed, bit for bit, against the numpy model of tests/maxsim_keyed_model.py fed the same index's widened rows
and column (the end-to-end entry also the same index's plain call at topk = fetch), with and without the matrix-core pass; against
the stride form where both can name the same documents; one check against a plain f64 Chamfer sum at rtol 1e-5."""
import numpy as np
import pytest

from tests import maxsim_keyed_model as M
from tests import synth
from tests import test_maxsim_gpu as G
from tests.diverse_model import posmap_of
from tests.test_maxsim_gpu import bits, rq  # noqa: F401  (the same library fixture and bit view)

pytestmark = pytest.mark.gpu

K, B = 16, 4
# segment lengths on both sides of one tile, of two position loads and of the 128-entry ring; 300 spans more than two look-aheads
LENS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300] + [40] * 40
N = sum(LENS)
INVALID, UNSUPPORTED = -1, -6
# the key of document j: u32; i64 with negative keys and -1 (j = 4); u64 keys that differ in the high word only
KEY = {"u32": lambda j: 7 * j + 3, "i64": lambda j: j - 5, "u64": lambda j: ((j + 1) << 32) | 5}
ABSENT = {"u32": 5, "i64": -77, "u64": 5}


_INDEX = {}


def doc_of_id(seed=17):
    """document j owns LENS[j] ids of a random permutation: its rows lie in many lists -> the document number of every id"""
    doc = np.empty(N, dtype=np.int64)
    doc[np.random.default_rng(seed).permutation(N)] = np.repeat(np.arange(len(LENS)), LENS)
    return doc


def index(rq, kind):
    """-> dict(g, d, posmap, base, post {column type: postings}, segs {column type: the model's segments}): built once per kind"""
    if kind in _INDEX:
        return _INDEX[kind]
    d = {"l2_128": 128, "l2_192": 192, "l2_100": 100, "l2_512": 512}.get(kind, 64)
    dim = -(-(d + (kind == "ip")) // 64) * 64
    x, centres, _ = synth.mixture(N, d, K, sigma=0.8, seed=900 + d, centre_scale=0.6)
    P, doc = synth.random_orthogonal(dim, seed=78), doc_of_id()
    col = {t: np.array([KEY[t](int(j)) for j in doc]) for t in KEY}
    if kind == "f16":
        g = rq.RaBitQ.build(x.astype(np.float16), centres, P)
    elif kind == "u8":
        g = rq.RaBitQ.build(np.clip(np.rint(x * 40.0 + 128.0), 0, 255).astype(np.uint8), centres * 40.0 + 128.0, P, rows="u8")
    elif kind in ("cosine", "ip"):
        g = rq.RaBitQ.build(x, centres, P, metric=kind)
    elif kind == "stride":     # what the stride form can name as well: contiguous ids, doc = id // 40
        g = rq.RaBitQ.build(x, centres, P)
        col = {"u32": np.arange(N) // 40}
    elif kind == "margin":     # one large common vector plus differences below bf16 resolution; key 0: 64 equal rows
        rng = np.random.default_rng(5)
        x = (np.full((1024, 64), 12.0) + rng.standard_normal((1024, 64)) * 1e-3).astype(np.float32)
        x[:64] = x[0]
        g = rq.RaBitQ.build(x, centres + 12.0, P)
        col = {"u32": np.where(np.arange(1024) < 64, 0, np.arange(1024))}
    elif kind == "wild":       # two-row documents, a row with an inf element
        x = x[:512].copy()
        x[37, 3] = np.inf
        g = rq.RaBitQ.build(x, centres, P)
        col = {"u32": np.arange(512) // 2}
    elif kind == "twins":      # the two rows of document 1, here keyed 3, equal the one row of key -5 (j = 0): the two tie for every query
        x[doc == 1] = x[doc == 0]
        col["i64"] = np.where(doc == 1, 3, np.where(doc == 8, -4, col["i64"]))
        g = rq.RaBitQ.build(x, centres, P)
    else:
        g = rq.RaBitQ.build(x, centres, P)
    ids = np.arange(g.n, dtype=np.uint32)
    for t, v in col.items():
        g.create_attr("doc_" + t, t, fill=0)
        g.set_attr("doc_" + t, ids, v)
    rows, found = g.fetch(g.map_ids, raw=False)
    assert found.all()
    post = {t: g.postings("doc_" + t) for t in col}
    _INDEX[kind] = dict(g=g, d=d, posmap=posmap_of(g.map_ids), base=np.ascontiguousarray(rows, dtype=np.float32), post=post,
                        segs={t: M.segments(g.attr_array("doc_" + t)) for t in col})
    return _INDEX[kind]


def tokens(rq, kind, g, d, T, seed=7):
    """-> (raw tokens B x T x d, the prepared ones B x T x dim): test_maxsim_gpu's; twins: the first query asks with the twin row itself"""
    raw, prep = G.tokens(rq, "l2" if kind == "twins" else kind, g, d, T, seed)
    if kind == "twins":
        raw[0] = prep[0] = synth.mixture(N, d, K, sigma=0.8, seed=900 + d, centre_scale=0.6)[0][doc_of_id() == 0]
    return raw, prep


def some_keys(ctype, seed=3):
    """B x 14 keys: six of the twelve edge documents (all twelve over queries 0 and 3), five random ones, two absent keys, a duplicate"""
    rng = np.random.default_rng(seed)
    rows = [[KEY[ctype](j) for j in list(range(6 * (b % 2), 6 * (b % 2) + 6)) + list(rng.integers(12, len(LENS), 5))] for b in (0, 1, 2, 1)]
    return np.array([r + [ABSENT[ctype], KEY[ctype](1000), r[2]] for r in rows])


def check_scores(rq, kind, T, ctype, keys, n_tokens=None, counts=None, tok=None, fits=True):
    """both forms of the scoring equal the model bit for bit -> the stats of the prefiltered run, the scores, the prepared tokens"""
    w = index(rq, kind)
    raw, prep = tokens(rq, kind, w["g"], w["d"], T) if tok is None else tok
    want_s, want_r = M.scores(prep, n_tokens, keys, counts, w["segs"][ctype], w["base"])
    stats = {}
    for pre in (False, True):
        s, r = w["g"].maxsim_scores(raw, keys, n_tokens=n_tokens, counts=counts, prefilter=pre, by=w["post"][ctype])
        stats = rq.last_maxsim_stats()
        assert np.array_equal(r, want_r), (kind, pre, "rows", np.argwhere(r != want_r)[:4])
        assert np.array_equal(bits(s), want_s), (kind, pre, "score", np.argwhere(bits(s) != want_s)[:4])
        assert stats["prefilter"] == int(pre and fits) and stats["rows_gathered"] == int(want_r.sum())
    return stats, want_s.view(np.float32), prep


@pytest.mark.parametrize("kind,T,ctype", [
    ("l2", 1, "u32"), ("l2", 32, "i64"), ("l2", 33, "u64"), ("l2_128", 32, "u32"), ("l2_192", 32, "i64"), ("l2_100", 33, "u32"),
    ("f16", 32, "u32"), ("u8", 33, "i64"), ("cosine", 32, "u64"), ("ip", 33, "u32"), ("l2", 256, "u32"), ("l2_512", 32, "u32")])
def test_scores_equal_the_model(rq, kind, T, ctype):
    n_tokens = np.array([T, 0, 1, max(T - 13, 1)], dtype=np.uint32) if T > 1 else None
    counts = np.array([14, 11, 0, 14], dtype=np.uint32)
    stats, want, _ = check_scores(rq, kind, T, ctype, some_keys(ctype), n_tokens, counts, fits=kind != "l2_512")
    assert np.isnan(want[0, 11:13]).all() and bits(want[0, 2:3]) == bits(want[0, 13:14])   # the absent keys; the duplicate
    if n_tokens is not None:                 # no token: +0.0 for every document that has a row
        assert (bits(want[1, :11]) == 0).all()
    if kind == "l2" and T == 32:             # benign data: the matrix pass decides most pairs
        assert 0 < stats["exact_distances"] < stats["pairs"] and stats["list_overflows"] == 0


def test_scores_and_search_equal_the_stride_form(rq):
    w = index(rq, "stride")
    g, p = w["g"], w["post"]["u32"]
    raw, _ = tokens(rq, "stride", g, w["d"], 33)
    docs = np.tile(np.array([0, 1, 17, 63, 64, 65, 17], dtype=np.uint32), (B, 1))     # 64: the partly filled last document; 65: none
    for pre in (True, False):
        a, b = g.maxsim_scores(raw, docs, by=p, prefilter=pre), g.maxsim_scores(raw, docs, 40, prefilter=pre)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[1][0].tolist() == [40, 40, 40, 40, 15, 0, 40]
        ra, rb = g.query_batch_maxsim(raw, 4, 10, fetch=16, by=p, prefilter=pre), g.query_batch_maxsim(raw, 4, 10, 40, fetch=16, prefilter=pre)
        assert np.array_equal(ra.counts, rb.counts) and np.array_equal(ra.candidates, rb.candidates) and ra.counts[0] == 10
        held = np.arange(10)[None, :] < ra.counts[:, None]
        assert np.array_equal(bits(ra.dist), bits(rb.dist)) and np.array_equal(ra.docs[held], rb.docs[held]) and ra.docs.dtype == np.uint32


@pytest.mark.parametrize("kind", ["l2", "cosine"])
def test_scores_against_a_plain_f64_sum(rq, kind):
    w = index(rq, kind)
    keys = some_keys("u32")[:, :11]
    _, got, prep = check_scores(rq, kind, 33, "u32", keys)
    for b in range(B):
        for c in range(11):
            ref = M.chamfer_f64(prep[b], 33, w["base"], w["segs"]["u32"][int(keys[b, c])])
            assert abs(float(got[b, c]) - ref) <= 1e-5 * abs(ref), (kind, b, c, got[b, c], ref)


def test_margin_data_and_list_overflow(rq):
    stats, _, _ = check_scores(rq, "margin", 32, "u32", np.zeros((B, 2), dtype=np.uint32))   # 64 equal rows: every row is kept
    assert stats["list_overflows"] > 0 and stats["exact_distances"] >= stats["pairs"]


def test_two_row_documents_inf_row_and_nan_token(rq):
    w = index(rq, "wild")
    raw, prep = tokens(rq, "wild", w["g"], w["d"], 33)
    raw[1, 2, 5] = prep[1, 2, 5] = np.nan
    check_scores(rq, "wild", 33, "u32", np.tile(np.arange(10, 26, dtype=np.uint32), (B, 1)), tok=(raw, prep))   # (key 18: the inf row)


def check_search(rq, w, kind, T, ctype, fetch, post, segs, flt=None):
    g = w["g"]
    raw, prep = tokens(rq, kind, g, w["d"], T, seed=11)
    n_tokens = np.array([T, max(T - 7, 1), 0, T], dtype=np.uint32)
    _, src_ids, src_cnt = g.query_batch(raw.reshape(B * T, w["d"]), 4, fetch, filter=flt)
    want = M.search(prep, n_tokens, src_ids, src_cnt, 10, w["posmap"], g.attr_array("doc_" + ctype), segs, w["base"])
    for pre in (True, False):
        res = g.query_batch_maxsim(raw, 4, 10, fetch=fetch, n_tokens=n_tokens, prefilter=pre, by=post, filter=flt)
        assert np.array_equal(res.counts, want[2]) and np.array_equal(res.candidates, want[3]), (kind, pre, res.counts, res.candidates)
        assert res.docs.dtype == want[1].dtype and np.array_equal(res.docs, want[1]), (kind, pre, "keys")
        assert np.array_equal(bits(res.dist), want[0]), (kind, pre, "dist")
    assert want[2][2] == 0 and want[2][0] > 1 and rq.last_maxsim_stats()["ms_source"] > 0.0
    return want


@pytest.mark.parametrize("kind,T,ctype,fetch", [("l2", 32, "u32", 16), ("l2_100", 33, "i64", 20), ("u8", 1, "u64", 64),
                                                ("cosine", 32, "u32", 64), ("twins", 32, "i64", 16)])
def test_search_equals_the_model_on_the_plain_call(rq, kind, T, ctype, fetch):
    w = index(rq, kind)
    flt = w["g"].make_filter(ids=np.arange(0, N, 3, dtype=np.uint32)) if kind == "cosine" else None   # cosine: under an id filter
    want = check_search(rq, w, kind, T, ctype, fetch, w["post"][ctype], w["segs"][ctype], flt)
    if kind == "twins":                      # equal rows, equal sums: the selection orders the tie by the i64 order, -5 before 3
        assert want[1][0, :2].tolist() == [-5, 3] and want[0][0, 0] == want[0][0, 1]


def test_the_live_column_routes_and_the_snapshot_scores(rq):
    w = index(rq, "l2_128")
    g, col = w["g"], w["g"].attr_array("doc_i64")
    try:   # after the postings were made: rows of key 7 become key 8's, rows of key 9 take a key the postings do not hold
        g.set_attr("doc_i64", g.map_ids[col == 7], 8)
        g.set_attr("doc_i64", g.map_ids[col == 9], 1 << 40)
        want = check_search(rq, w, "l2_128", 32, "i64", 16, w["post"]["i64"], w["segs"]["i64"])
        assert not np.isin(want[1], [7, 9, 1 << 40]).any()
    finally:
        g.set_attr("doc_i64", g.map_ids, col)


def test_device_keys_give_the_host_forms_bits(rq):
    import torch
    w = index(rq, "l2")
    g, p, T = w["g"], w["post"]["i64"], 33
    raw, _ = tokens(rq, "l2", g, w["d"], T)
    keys, counts = some_keys("i64"), np.array([14, 11, 0, 14], dtype=np.uint32)
    want = g.maxsim_scores(raw, keys, counts=counts, by=p)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t, k, c = dev(raw), dev(keys.astype(np.int64)), dev(counts.view(np.int32))
    s, r = torch.empty(keys.shape, dtype=torch.float32, device="cuda"), torch.empty(keys.shape, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.maxsim_scores_device(t.data_ptr(), 0, B, T, w["d"], k.data_ptr(), c.data_ptr(), keys.shape[1], out_score_ptr=s.data_ptr(),
                           out_rows_ptr=r.data_ptr(), by=p)
    assert np.array_equal(bits(s.cpu().numpy()), bits(want[0])) and np.array_equal(r.cpu().numpy().view(np.uint32), want[1])


@pytest.mark.parametrize("what", ["add", "lazy_remove", "foreign", "both", "source", "shard", "tiered", "split_rows"])
def test_refusals(rq, what):
    from rabitq_amd import index as ix
    x, centres, _ = synth.mixture(6000, 64, K, sigma=0.8, seed=964, centre_scale=0.6)
    if what in ("tiered", "split_rows"):     # split_rows: every row in HBM, so the tier check passes and the split-row check refuses
        ix.set_option(*(("base_device_mb", 1) if what == "tiered" else ("split_rows", 2)))
    try:
        g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(64, seed=78))
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)
    held = [g]
    try:
        g.create_attr("doc", "u32", fill=1)
        if what == "shard":
            g = g.shard(g.partition_lists(2)[0], 0)
            held.append(g)
        p = index(rq, "l2")["post"]["u32"] if what == "foreign" else g.postings("doc")
        held += [p] if what != "foreign" else []
        if what == "add":
            g.add(x[:2], ids=np.array([7000, 7001], dtype=np.uint32))
        if what == "lazy_remove":
            g.remove(ids=[1], lazy=True)
        tok, keys = np.zeros((2, 33, 64), dtype=np.float32), np.ones((2, 3), dtype=np.uint32)
        calls = [lambda: g.query_batch_maxsim(tok, 4, 10, 40 if what == "both" else None, fetch=63 if what == "source" else 8, by=p),
                 lambda: g.maxsim_scores(tok, keys, 40 if what == "both" else None, by=p)]
        for call in calls[:1 if what == "source" else 2]:
            with pytest.raises(ValueError if what == "both" else rq.RabitqError) as e:
                call()
            assert what == "both" or e.value.status == (INVALID if what in ("add", "lazy_remove", "foreign") else UNSUPPORTED), str(e.value)
    finally:
        for h in held[::-1]:
            h.close()
