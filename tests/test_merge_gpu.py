"""rq_merge_from / rq_extract: merging two indexes over the same rotation and centroids, and copying a sub-index out of one, give
canonical(S) -- the index a fresh build of the live rows S produces -- bit for bit: the arrays, rq_info, rq_dump_dir's files and
the ids, distance bits, counts and counters of the query entry points.  No comparison here has a tolerance.

Run on the GPU box:  python -m pytest tests/test_merge_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import synth
from tests.models import ARRAYS, Live, bits
from tests.test_mutable_gpu import assert_same_arrays, assert_same_queries, check

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6
KEEP, SHIFT, APPEND = 0, 1, 2


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def snap(g):
    return [bits(getattr(g, a)).copy() for a in ARRAYS + ("map_ids",)] + [bits(np.array([g.n, g.max_list_len, g.k, g.dim]))]


def unchanged(g, before, what):
    g._refresh()
    for u, v in zip(before, snap(g)):
        assert np.array_equal(u, v), what


def same_dumps(a, b, tmp_path, what):
    a.dump_to_dir(tmp_path / "a")
    b.dump_to_dir(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names and names == sorted(os.listdir(tmp_path / "b")), what
    for name in names:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), (what, name)


def with_ids(rq, b, ids, **kw):
    """The index b with its map_ids replaced (rq_from_arrays takes the arrays as they are)."""
    return rq.RaBitQ.from_arrays(b.base, b.orthogonal, b.centroids, b.offsets, np.asarray(ids, dtype=np.uint32), b.codes, b.factors, **kw)


def raw_merge(rq, dst, src, mode, shift=0):
    from rabitq_amd import _lib
    L = _lib.lib()
    out = C.c_uint32(0xDEAD)
    st = L.rq_merge_from(dst._h, src._h, mode, shift, C.byref(out))
    return st, out.value, L.rq_last_error().decode()


# ---- 1. halves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(64, 16), (100, 64), (128, 16), (192, 8), (768, 8)])
def test_merge_of_halves_equals_rebuild(rq, d, k, tmp_path):
    n = 2000 if d == 768 else 4000
    dim = (d + 63) // 64 * 64
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=d + k, centre_scale=0.6)
    P = synth.random_orthogonal(dim, seed=d + 3)
    queries, _, _ = synth.mixture(100, d, k, sigma=0.8, seed=d + 5, centre_scale=0.6)
    n0 = n // 2 - 37
    A, B, whole = rq.RaBitQ.build(x[:n0], centres, P), rq.RaBitQ.build(x[n0:], centres, P), rq.RaBitQ.build(x, centres, P)
    b_before = snap(B)
    want_b = B.query_batch(queries, 4, 10)
    assert A.merge_from(B, "append") == n0
    st = rq.index.last_mutate_stats()
    assert st["rows_before"] == n0 and st["rows_after"] == n and st["ms_assign"] == 0 and st["gather_bytes"] > 0, st
    ids = np.arange(n, dtype=np.uint32)
    assert_same_arrays(A, whole, ids, (d, k))
    same_dumps(A, whole, tmp_path, (d, k))
    assert_same_queries(rq, A, whole, ids, queries, (1, k), what=(d, k))
    unchanged(B, b_before, "src after the merge")
    for u, v in zip(want_b, B.query_batch(queries, 4, 10)):
        assert np.array_equal(bits(u), bits(v))
    for g in (A, B, whole):
        g.close()


# ---- 2. round trip -----------------------------------------------------------------------------------------------------------
def test_extract_and_merge_round_trip(rq):
    d, k, n = 128, 16, 4001
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=7, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=8)
    queries, _, _ = synth.mixture(100, d, k, sigma=0.8, seed=9, centre_scale=0.6)
    G = rq.RaBitQ.build(x, centres, P)
    g_before = snap(G)
    all_ids = np.arange(n, dtype=np.uint32)
    E, O = G.extract(ids=all_ids[::2]), G.extract(mask=(all_ids % 2 == 1))
    st = rq.index.last_mutate_stats()
    assert st["rows_before"] == n and st["rows_after"] == O.n == n // 2 and st["ms_assign"] == 0 and st["gather_bytes"] > 0, st
    unchanged(G, g_before, "src after extract")
    for part, sel in ((E, all_ids[::2]), (O, all_ids[1::2])):
        check(rq, part, Live(sel, x[sel]), centres, P, queries, (k,), "extract")
    assert E.merge_from(O, "keep") == 0
    assert_same_arrays(E, G, all_ids, "round trip")
    assert np.array_equal(E.map_ids, G.map_ids)
    assert_same_queries(rq, E, G, all_ids, queries, (2, k), what="round trip")
    c = G.copy()
    assert_same_arrays(c, G, all_ids, "copy")
    assert_same_queries(rq, c, G, all_ids, queries[:40], (k,), what="copy")
    # no bit set: a valid empty index
    for empty in (G.extract(ids=[n + 5]), G.extract(mask=np.zeros(0, dtype=bool)), G.extract(ids=np.zeros(0, np.int64))):
        assert (empty.n, empty.k, empty.dim, empty.max_list_len) == (0, k, d, 0)
        assert not empty.offsets.any() and np.array_equal(bits(empty.centroids), bits(G.centroids))
        dist, ids, cnt = empty.query_batch(queries, k, 10)
        assert not cnt.any()
        # merging into it gives the source back
        assert empty.merge_from(G, "keep") == 0
        assert_same_arrays(empty, G, all_ids, "into empty")
        empty.close()
    e2 = G.extract(ids=[n + 5])
    assert e2.merge_from(G, "append") == 0           # an empty dst holds no id: the shift is 0
    assert_same_arrays(e2, G, all_ids, "append into empty")
    for g in (G, E, O, c, e2):
        g.close()


# ---- 3. ties and edges ---------------------------------------------------------------------------------------------------------
def test_ties_and_edges(rq):
    """The identity rotation makes distances exact.  The same rows in both indexes (equal key words: the id decides, with the src
    copy after the dst copy and before it), NaN / inf rows on both sides (list 0, key f32::MAX), lists empty on one side and filled
    on the other, one list past 8192 rows only after the merge, and the end of the id space."""
    d, k = 128, 16
    rng = np.random.default_rng(5)
    centres = np.zeros((k, d), np.float32)
    for c in range(k):
        centres[c, c % d] = 4.0 if c % 2 == 0 else -4.0
        centres[c, (c // 2) + 32] = 1.0
    P = np.eye(d, dtype=np.float32)
    bad = np.stack([np.full(d, np.nan, np.float32), np.full(d, np.inf, np.float32)])
    u = rng.integers(0, 6, size=2000)                   # dst: lists 0-5 and 3 (big); nothing in 6-15
    xa = (centres[u] + 0.5 * rng.standard_normal((2000, d))).astype(np.float32)
    big_a = (centres[3] + 0.5 * rng.standard_normal((5000, d))).astype(np.float32)
    xd = np.concatenate([xa, bad, big_a]).astype(np.float32)
    v = rng.integers(8, k, size=1500)                   # src: lists 8-15 and 3 (big); nothing in 0-2, 4-7 but the copies
    xb = (centres[v] + 0.5 * rng.standard_normal((1500, d))).astype(np.float32)
    big_b = (centres[3] + 0.5 * rng.standard_normal((4000, d))).astype(np.float32)
    xs = np.concatenate([xa[[5, 17, 17, 1999]], bad[::-1], xb, big_a[:3], big_b]).astype(np.float32)
    nd, ns = len(xd), len(xs)
    queries = (centres[rng.integers(0, k, 64)] + 0.5 * rng.standard_normal((64, d))).astype(np.float32)
    D, S = rq.RaBitQ.build(xd, centres, P), rq.RaBitQ.build(xs, centres, P)
    od, os_ = np.diff(D.offsets.astype(np.int64)), np.diff(S.offsets.astype(np.int64))
    assert od[3] <= 8192 and os_[3] <= 8192 and od[3] + os_[3] > 8192
    assert (od[8:] == 0).all() and (os_[8:] > 0).all() and ((od > 0) & (os_ == 0)).any()

    # the src copies sort after the dst copies (appended ids)
    g = D.copy()
    assert g.merge_from(S, "append") == nd
    live = Live(np.arange(nd), xd)
    live.add(nd + np.arange(ns), xs)
    check(rq, g, live, centres, P, queries, (2, k), "src after dst")
    assert g.offsets[4] - g.offsets[3] > 8192
    g.close()

    # ... and before them: dst under large ids, src's kept
    g = with_ids(rq, D, D.map_ids.astype(np.int64) + 100000)
    assert g.merge_from(S, "keep") == 0
    live = Live(100000 + np.arange(nd), xd)
    live.add(np.arange(ns), xs)
    check(rq, g, live, centres, P, queries[:40], (k,), "src before dst")
    g.close()

    # the end of the id space: a largest new id of 2^32 - 1 is accepted, one more is not
    small = rq.RaBitQ.build(xs[:50], centres, P)
    g = D.copy()
    before, s_before = snap(g), snap(small)
    top = (1 << 32) - 50                                # 49 + top == 2^32 - 1
    st, _, msg = raw_merge(rq, g, small, SHIFT, top + 1)
    assert st == UNSUPPORTED and msg
    unchanged(g, before, "id space: dst")
    unchanged(small, s_before, "id space: src")
    assert g.merge_from(small, top) == top
    live = Live(np.arange(nd), xd)
    live.add(top + np.arange(50), xs[:50])
    assert int(g.map_ids.max()) == 0xFFFFFFFF
    check(rq, g, live, centres, P, queries[:40], (k,), "largest id")
    cp = g.copy()                                       # every id, 2^32 - 1 among them: no bitmap is made
    assert cp.n == g.n and np.array_equal(cp.map_ids, g.map_ids) and np.array_equal(bits(cp.base), bits(g.base))
    cp.close()
    st, _, msg = raw_merge(rq, g, small, APPEND)        # dst now holds 2^32 - 1: nothing can be appended
    assert st == UNSUPPORTED and msg
    for x_ in (g, small, D, S):
        x_.close()


# ---- 4. metrics ------------------------------------------------------------------------------------------------------------------
def test_cosine_merge_equals_build_of_the_original_rows(rq):
    d, k, n = 100, 16, 3000
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=41, centre_scale=0.6)
    P = synth.random_orthogonal(128, seed=42)
    queries, _, _ = synth.mixture(100, d, k, sigma=0.8, seed=43, centre_scale=0.6)
    n0 = 1234
    A, B = rq.RaBitQ.build(x[:n0], centres, P, metric="cosine"), rq.RaBitQ.build(x[n0:], centres, P, metric="cosine")
    whole = rq.RaBitQ.build(x, centres, P, metric="cosine")
    assert A.merge_from(B) == n0 and A.metric == "cosine"
    ids = np.arange(n, dtype=np.uint32)
    assert_same_arrays(A, whole, ids, "cosine")
    assert_same_queries(rq, A, whole, ids, queries, (2, k), what="cosine")
    sub = whole.extract(ids=ids[::3])
    assert sub.metric == "cosine"
    part = rq.RaBitQ.build(x[::3], centres, P, metric="cosine")
    assert_same_arrays(sub, part, ids[::3], "cosine extract")
    l2 = rq.RaBitQ.build(x[n0:], centres, P)
    before = snap(A)
    st, _, msg = raw_merge(rq, A, l2, APPEND)
    assert st == INVALID and "metric" in msg
    unchanged(A, before, "l2 into cosine")
    for g in (A, B, whole, sub, part, l2):
        g.close()


def test_inner_product_merge_equals_build_with_the_same_bound(rq):
    d, k, n = 64, 16, 3000
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=51, centre_scale=0.6)
    P = synth.random_orthogonal(128, seed=52)
    queries, _, _ = synth.mixture(100, d, k, sigma=0.8, seed=53, centre_scale=0.6)
    S = float(np.float32((x.astype(np.float64) ** 2).sum(1).max() * 1.25))
    n0 = 1777
    A = rq.RaBitQ.build(x[:n0], centres, P, metric="ip", max_sq_norm=S)
    B = rq.RaBitQ.build(x[n0:], centres, P, metric="ip", max_sq_norm=S)
    whole = rq.RaBitQ.build(x, centres, P, metric="ip", max_sq_norm=S)
    assert A.dim == 128 and A.merge_from(B) == n0
    assert A.metric == "ip" and A.ip_params == whole.ip_params
    ids = np.arange(n, dtype=np.uint32)
    assert_same_arrays(A, whole, ids, "ip")
    assert_same_queries(rq, A, whole, ids, queries, (2, k), what="ip")
    other = rq.RaBitQ.build(x[n0:], centres, P, metric="ip", max_sq_norm=float(np.nextafter(np.float32(S), np.float32(np.inf))))
    before, o_before = snap(A), snap(other)
    st, _, msg = raw_merge(rq, A, other, APPEND)
    assert st == INVALID and msg
    unchanged(A, before, "ip S: dst")
    unchanged(other, o_before, "ip S: src")
    for g in (A, B, whole, other):
        g.close()


# ---- 5. gather shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128, 192, 320, 768, 4096])
def test_gather_shapes(rq, dim):
    """Sub-groups of 16, 32 and 64 lanes (48 of them used at dim 192), rows longer than one wave's step, the largest dim; one
    output row, and row counts that are no multiple of what a wave handles (16, 8 or 4 rows per step)."""
    k, n = 8, 701
    x, centres, _ = synth.mixture(n, dim, k, sigma=0.8, seed=dim, centre_scale=0.6)
    P = synth.random_orthogonal(dim, seed=dim + 1) if dim <= 320 else np.eye(dim, dtype=np.float32)[::-1].copy()
    G = rq.RaBitQ.build(x, centres, P)
    ids = np.arange(n, dtype=np.uint32)
    c = G.copy()
    assert_same_arrays(c, G, ids, ("copy", dim))
    assert np.array_equal(c.map_ids, G.map_ids)
    for sel in (ids[::3], ids[5:6]):                   # 234 rows; 1 row
        sub = G.extract(ids=sel)
        want = rq.RaBitQ.build(x[sel], centres, P)
        assert_same_arrays(sub, want, sel, ("extract", dim, sel.size))
        sub.close()
        want.close()
    back = G.extract(ids=ids[::3])
    rest = G.extract(mask=(ids % 3 != 0))
    assert back.merge_from(rest, "keep") == 0          # the two-source gather at this shape
    assert_same_arrays(back, G, ids, ("merge", dim))
    assert np.array_equal(back.map_ids, G.map_ids)
    for g in (G, c, back, rest):
        g.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_indexes_unchanged(rq):
    import torch
    from rabitq_amd import _lib
    d, k = 128, 16
    x, centres, _ = synth.mixture(3000, d, k, sigma=0.8, seed=31, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=32)
    queries, _, _ = synth.mixture(50, d, k, sigma=0.8, seed=33, centre_scale=0.6)
    A, B = rq.RaBitQ.build(x[:2000], centres, P), rq.RaBitQ.build(x[2000:], centres, P)
    a_before, b_before = snap(A), snap(B)

    def refused(dst, src, status, mode=APPEND, shift=0, contains=None, what=""):
        befores = [(g, snap(g)) for g in (dst, src)]
        st, _, msg = raw_merge(rq, dst, src, mode, shift)
        assert st == status and msg, (what, st, msg)
        if contains is not None:
            assert contains in msg, (what, msg)
        for g, before in befores:
            unchanged(g, before, what)
        return msg

    cent = B.centroids.copy()
    cent.view(np.uint32)[3, 7] ^= 1                                          # one centroid float, one bit
    other = rq.RaBitQ.from_arrays(B.base, B.orthogonal, cent, B.offsets, B.map_ids, B.codes, B.factors)
    assert str(3 * d + 7) in refused(A, other, INVALID, contains="centroids", what="centroid bit")
    other.close()
    rot = B.orthogonal.copy()
    rot[d - 1, d - 1] = np.float32(np.nan)                                   # (bit patterns: a NaN differs from the number it replaced)
    other = rq.RaBitQ.from_arrays(B.base, rot, B.centroids, B.offsets, B.map_ids, B.codes, B.factors)
    assert str(d * d - 1) in refused(A, other, INVALID, contains="rotation", what="P element")
    other.close()
    other = rq.RaBitQ.build(x[2000:], centres[:8], P)
    refused(A, other, INVALID, contains="differ in k", what="k")
    other.close()
    other = rq.RaBitQ.build(x[2000:, :64], centres[:, :64], synth.random_orthogonal(64, seed=34))
    refused(A, other, INVALID, contains="dim", what="dim")
    refused(other, A, INVALID, contains="dim", what="dim, reversed")
    other.close()
    other = rq.RaBitQ.build(x[2000:], centres, P, metric="cosine")
    refused(A, other, INVALID, contains="metric", what="l2 against cosine")
    other.close()
    half = rq.RaBitQ.build(x[2000:].astype(np.float16), centres, P)
    assert half.row_type == "f16"
    refused(A, half, UNSUPPORTED, what="f16 src")
    refused(half, A, UNSUPPORTED, what="f16 dst")
    half.close()
    owner = np.zeros(k, dtype=np.uint32)
    owner[k // 2:] = 1
    sh = B.shard(owner, 0)
    refused(A, sh, UNSUPPORTED, what="shard src")
    refused(sh, A, UNSUPPORTED, what="shard dst")
    sh.close()
    refused(A, A, INVALID, what="dst == src")
    with pytest.raises(ValueError):
        A.merge_from(A)
    refused(A, B, INVALID, mode=KEEP, contains="1000", what="overlapping ids")   # B's ids 0 .. 999 are all in A
    overlap = with_ids(rq, B, B.map_ids.astype(np.int64) * 5)                     # 0, 5, .. 4995: the 400 below 2000 are in A
    refused(A, overlap, INVALID, mode=KEEP, contains="400", what="partly overlapping ids")
    refused(A, overlap, INVALID, mode=SHIFT, shift=5, contains="399", what="shifted ids that collide")
    overlap.close()
    refused(A, B, INVALID, mode=7, what="id_mode 7")
    with pytest.raises(_lib.RabitqError) as e:
        A.merge_from(B, "keep")
    assert e.value.status == INVALID and "1000" in str(e.value)

    # a list out of the build's order (rq_from_arrays takes what it is given): merging refuses it, extraction keeps the order it has
    offs = B.offsets.astype(np.int64)
    c = int(np.argmax(np.diff(offs)))
    order = np.arange(B.n)
    order[offs[c]], order[offs[c] + 1] = offs[c] + 1, offs[c]
    arrs = [B.base[order], B.orthogonal, B.centroids, B.offsets, B.map_ids[order], B.codes[order], B.factors[order]]
    ooo = rq.RaBitQ.from_arrays(*arrs)
    refused(A, ooo, UNSUPPORTED, contains="build's order", what="out-of-order src")
    refused(ooo, A, UNSUPPORTED, contains="build's order", what="out-of-order dst")
    cp = ooo.copy()
    assert_same_arrays(cp, ooo, np.arange(B.n, dtype=np.uint32), "copy of an out-of-order index")
    assert np.array_equal(cp.map_ids, ooo.map_ids)
    refused(A, cp, UNSUPPORTED, contains="build's order", what="the copy is out of order too")
    cp.close()
    ooo.close()

    # an open _begin ticket on either side
    qd = torch.from_numpy(np.ascontiguousarray(np.tile(queries, (40, 1)))).cuda()
    nq = qd.shape[0]
    od = torch.empty((nq, 10), device="cuda", dtype=torch.float32)
    oi = torch.empty((nq, 10), device="cuda", dtype=torch.int32)
    on = torch.empty((nq,), device="cuda", dtype=torch.int32)
    for holder, what in ((A, "ticket on dst"), (B, "ticket on src")):
        t = holder.query_batch_device_begin(qd.data_ptr(), nq, d, 4, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        st, _, msg = raw_merge(rq, A, B, APPEND)
        holder.query_batch_device_end(t)
        assert st == INVALID and "ticket" in msg, what
    unchanged(A, a_before, "after every refusal: dst")
    unchanged(B, b_before, "after every refusal: src")
    assert A.merge_from(B) == 2000 and A.n == 3000                                # and the pair still merges
    A.close()
    B.close()


# ---- 7. life after a merge -------------------------------------------------------------------------------------------------------
def test_life_after_a_merge(rq):
    from rabitq_amd import _lib
    L = _lib.lib()
    d, k = 128, 16
    x, centres, _ = synth.mixture(4000, d, k, sigma=0.8, seed=61, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=62)
    queries, _, _ = synth.mixture(64, d, k, sigma=0.8, seed=63, centre_scale=0.6)
    A, B = rq.RaBitQ.build(x[:1500], centres, P), rq.RaBitQ.build(x[1500:3000], centres, P)

    def filtered(f):
        return L.rq_query_batch_filtered(A._h, f._h, queries.ctypes.data, 5, d, 4, 10, 0, np.empty((5, 10), np.float32).ctypes.data,
                                         np.empty((5, 10), np.uint32).ctypes.data, np.empty(5, np.uint32).ctypes.data)

    empty = B.extract(ids=[1 << 20])
    with A.make_filter(ids=np.arange(0, 1500, 2)) as f:
        before = snap(A)
        assert A.merge_from(empty) == 1500                                      # nothing changes: the filter stays valid
        unchanged(A, before, "empty src")
        assert filtered(f) == 0
        assert A.merge_from(B) == 1500
        assert filtered(f) == INVALID                                           # made before the merge
    empty.close()
    live = Live(np.arange(3000), x[:3000])
    got = A.add(x[3000:3500])
    st = rq.index.last_mutate_stats()
    assert st["ms_keys"] == 0 and st["ms_assign"] > 0, st                       # the merge left dst's key cache valid
    live.add(got, x[3000:3500])
    check(rq, A, live, centres, P, queries, (k,), "add after merge")
    gone = np.arange(100, 3100, 6)
    assert A.remove(ids=gone) == 500
    st = rq.index.last_mutate_stats()
    assert st["ms_keys"] == 0, st
    live.remove(gone)
    check(rq, A, live, centres, P, queries, (4,), "remove after merge")
    A.close()
    B.close()
