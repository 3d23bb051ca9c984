"""The row bookkeeping around the search core -- relayout, lazy removal, rows by id, attribute columns and predicate filters, grouped
search -- on an index of 2.2M rows, where every capped launch of those kernels takes a second trip through its grid-stride loop and
the id list of a filter is joined from 269 blocks (tests/scale_cases.py holds the table of kernels, caps and sizes, and
tests/test_scale_cases.py holds that table to the launch sites).  Every assertion is exact: integers and bit patterns against numpy.
A mutated index is compared with a fresh build of the same rows, as tests/test_mutable_gpu.py::test_scale_2m does; the build itself
is pinned to the oracle elsewhere.

Still uncovered at this size: bitmap_grid (4096 blocks x 256 words: 33.5M positions), fetch_gather_kernel and merge_gather_kernel
(2^20 blocks) and arrays past 4 GiB, which need indexes of tens of millions of rows; bits_differ_kernel past one trip (k * dim >
1 048 576); typed, tiered and split-row indexes at this size (their by-id paths differ in the gather alone).

Run on the GPU box:  python -m pytest tests/test_bookkeeping_scale_gpu.py -m gpu -q --durations=0
"""
import os

import numpy as np
import pytest

from tests import by_id_model as BM
from tests import group_model as GM
from tests import scale_cases as S
from tests import synth
from tests.models import bits

pytestmark = pytest.mark.gpu

D, K, NA, NB, N = S.D, S.K, S.NA, S.NB, S.N
INVALID = -1
SIGMA = 0.9
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


# ---- the indexes -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows(rq):
    """(x N x D and the K centres, both on the device; the rotation; 200 queries on the host)"""
    x, cd = synth.device_mixture(N, D, K, SIGMA, "cuda", centre_scale=1.0)
    q = synth.device_queries(cd, 200, SIGMA, "cuda", seed=53).cpu().numpy()
    return x, cd, synth.random_orthogonal(D, seed=51), q


def build_half(rq, rows, first, n, lacks=()):
    """rows [first, first + n) under the ids 0 .. n - 1, the columns set from the values of id + first"""
    x, cd, P, _ = rows
    g = rq.RaBitQ.build_device(x[first:].data_ptr(), n, D, cd.data_ptr(), K, orthogonal=P)
    ids = np.arange(n, dtype=np.uint32)
    for name, (dtype, _) in S.COLUMNS.items():
        if name not in lacks:
            g.create_attr(name, dtype, fill=S.FILLS[name])
            assert g.set_attr(name, ids, S.column_values(name, ids.astype(np.uint64) + np.uint64(first))) == 0
    return g


@pytest.fixture(scope="module")
def A(rq, rows):
    g = build_half(rq, rows, 0, NA)
    yield g
    g.close()


@pytest.fixture(scope="module")
def B(rq, rows):
    g = build_half(rq, rows, NA, NB, lacks=(S.B_LACKS,))
    yield g
    g.close()


@pytest.fixture(scope="module")
def Cn(rq, rows):
    """the canonical answer: a fresh build of all rows (no columns)"""
    x, cd, P, _ = rows
    g = rq.RaBitQ.build_device(x.data_ptr(), N, D, cd.data_ptr(), K, orthogonal=P)
    yield g
    g.close()


@pytest.fixture(scope="module")
def G(rq, A, B):
    """(A's copy with B merged in, the shift applied, its map_ids, its columns in position order as the model has them)"""
    g = A.copy()
    shift = g.merge_from(B, ids="append")
    mids = g.map_ids
    cols = {name: (dtype, S.merged_values(name, mids)) for name, (dtype, _) in S.COLUMNS.items()}
    yield g, shift, mids, cols
    g.close()


class DeviceWords:
    """An array of the library's in device memory as 32-bit words, for torch (the CUDA array interface)."""

    def __init__(self, ptr, nbytes):
        assert ptr and nbytes % 4 == 0
        self.__cuda_array_interface__ = {"shape": (nbytes // 4,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def device_words(g, which):
    import torch
    return torch.as_tensor(DeviceWords(*g.device_ptr(which)), device="cuda")


def request(rng, stored, m, absent_lo, absent_hi, absent=150_000, repeats=100_000):
    """m ids in random order: draws of `stored` (with replacement), `repeats` of them once more, `absent` ids of [absent_lo, absent_hi)"""
    draws = rng.choice(stored, size=m - absent - repeats)
    ids = np.concatenate([draws, draws[:repeats], rng.integers(absent_lo, absent_hi, size=absent, dtype=np.uint64).astype(np.uint32)])
    return rng.permutation(ids).astype(np.uint32)


def locate_model(map_ids, ids, live=None):
    """by_id_model.locate, asked in ascending order of the ids (the same answers; its bisection then walks the memory forwards)"""
    order = np.argsort(ids, kind="stable")
    out = np.empty(ids.size, dtype=np.uint32)
    out[order] = BM.locate(map_ids, ids[order], live)
    return out


# ---- 1. merge --------------------------------------------------------------------------------------------------------------------------
# (the four tests before the merge ask for one fixture each, so that --durations shows every fixture's set-up by itself; the first
# set-up also pays for the start of the runtime)
def test_rows_are_made_on_the_device(rq, rows):
    x, cd, P, q = rows
    assert x.is_cuda and tuple(x.shape) == (N, D) and tuple(cd.shape) == (K, D) and P.shape == (D, D) and q.shape == (200, D)
    assert x.is_contiguous() and bool(x.isfinite().all())


def half_holds_its_columns(g, first, n, lacks=()):
    mids = g.map_ids
    assert g.n == n and np.array_equal(np.sort(mids), np.arange(n, dtype=np.uint32))
    assert [a["name"] for a in g.attrs()] == [c for c in S.COLUMNS if c not in lacks]
    for a in g.attrs():                                                       # attr_fill and the three passes of set_attr at n = m > 1 048 576
        want = S.column_values(a["name"], mids.astype(np.uint64) + np.uint64(first))
        assert np.array_equal(bits(g.attr_array(a["name"])), bits(want)), a["name"]


def test_first_half_holds_its_columns(rq, A):
    half_holds_its_columns(A, 0, NA)


def test_second_half_holds_its_columns(rq, B):
    half_holds_its_columns(B, NA, NB, lacks=(S.B_LACKS,))


def test_canonical_build_holds_every_row(rq, Cn):
    off = Cn.offsets
    assert Cn.n == N and Cn.k == K and off[0] == 0 and off[K] == N and (np.diff(off.astype(np.int64)) > 0).all() and Cn.attrs() == []


def test_merge_past_every_cap(rq, B, Cn, G):
    import torch
    from rabitq_amd import index as ix
    g, shift, mids, cols = G
    assert shift == NA and g.n == Cn.n == N and g.pending_removals == 0
    for which in (ix.ARR_OFFSETS, ix.ARR_MAP_IDS, ix.ARR_CODES, ix.ARR_FACTORS, ix.ARR_BASE):
        a, b = device_words(g, which), device_words(Cn, which)
        assert a.shape == b.shape and a.numel() > 0 and torch.equal(a, b), which
    assert device_words(g, ix.ARR_BASE).numel() == N * D and np.array_equal(np.sort(mids), np.arange(N, dtype=np.uint32))
    assert [a["name"] for a in g.attrs()] == list(S.COLUMNS)
    for name, (_, want) in cols.items():
        got = g.attr_array(name)
        assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), (name, np.nonzero(bits(got) != bits(want))[0][:5])
    late = mids >= NA
    assert late.sum() == NB and (g.attr_array(S.B_LACKS)[late] == S.FILLS[S.B_LACKS]).all()
    assert not (cols[S.B_LACKS][1][~late] == S.FILLS[S.B_LACKS]).all()
    # colliding ids: refused with the count, dst untouched -- five ids of src's 1.1M collide, then all of them
    u_before = g.attr_array("u")
    for ids, hits in ((N - 5, 5), ("keep", NB)):
        with pytest.raises(rq.RabitqError) as e:
            g.merge_from(B, ids=ids)
        assert e.value.status == INVALID and f"{hits} of the ids of src are already in dst" in str(e.value), str(e.value)
    assert g.n == N and np.array_equal(g.map_ids, mids) and np.array_equal(g.attr_array("u"), u_before)
    assert torch.equal(device_words(g, ix.ARR_BASE), device_words(Cn, ix.ARR_BASE))


# ---- 2. / 3. the directory ---------------------------------------------------------------------------------------------------------------
def test_dense_directory(rq, G):
    g0, _, mids, _ = G
    g = g0.copy()                                                             # a new index: its first by-id call builds the directory
    try:
        assert np.array_equal(g.map_ids, mids)
        rng = np.random.default_rng(81)
        ids = request(rng, mids, S.M_IDS, N, 2**32)
        ids[:3] = [N, 2**32 - 1, N - 1]                                       # top, the largest id there is, the largest stored
        got = g.locate(ids)
        st = rq.last_by_id_stats()
        want = locate_model(mids, ids)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
        assert (st["form"], st["built"]) == ("dense", 1) and st["found"] + st["absent"] == S.M_IDS, st
        assert st["found"] == (want != BM.ABSENT).sum() == (ids < N).sum() and st["directory_bytes"] == 4 * N
        assert (want[ids < N] >= 2_097_152).any()
        assert np.array_equal(g.locate(ids[:1000]), want[:1000]) and rq.last_by_id_stats()["built"] == 0
    finally:
        g.close()


def test_fetch_rows_of_the_large_directory(rq, rows, G):
    """fetch returns the source rows, those at positions past 2 097 152 among them"""
    import torch
    g, _, mids, _ = G
    x = rows[0]
    rng = np.random.default_rng(87)
    sample = np.concatenate([rng.choice(mids[2_097_152:], 5000), rng.choice(N, 4990), [N + 7] * 10]).astype(np.uint32)
    got_rows, found = g.fetch(sample)
    assert rq.last_by_id_stats()["form"] == "dense"
    src = x[torch.from_numpy(np.minimum(sample, N - 1).astype(np.int64)).cuda()].cpu().numpy()
    src[sample >= N] = 0.0
    assert np.array_equal(found, sample < N) and np.array_equal(bits(got_rows), bits(src))


def test_hash_directory(rq, A):
    mids = S.HASH_ID(A.map_ids).astype(np.uint32)
    g = rq.RaBitQ.from_arrays(A.base, A.orthogonal, A.centroids, A.offsets, mids, A.codes, A.factors)
    try:
        assert g.n == NA
        rng = np.random.default_rng(82)
        draws = S.HASH_ID(rng.integers(0, NA, size=S.M_IDS - 400_000)).astype(np.uint32)
        between = (S.HASH_ID(rng.integers(0, NA, size=200_000)) + rng.integers(1, 7, size=200_000).astype(np.uint64)).astype(np.uint32)
        ids = rng.permutation(np.concatenate([draws, draws[:50_000], between, rng.integers(0, 2**31, size=100_000).astype(np.uint32),
                                              rng.integers(int(mids.max()) + 1, 2**32, size=50_000, dtype=np.uint64).astype(np.uint32)]))
        assert ids.size == S.M_IDS > 2_097_152
        got = g.locate(ids)
        st = rq.last_by_id_stats()
        want = locate_model(mids, ids)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
        assert (st["form"], st["built"]) == ("hash", 1) and st["longest_chain"] >= 1 and st["directory_bytes"] == 8 << 22, st
        assert st["found"] + st["absent"] == S.M_IDS and st["found"] == (want != BM.ABSENT).sum() == S.M_IDS - 350_000
        assert (want[want != BM.ABSENT] >= 1_048_576).any()
    finally:
        g.close()


# ---- 4. set and get ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,fill", [("i32", -123), ("u64", 2**40 + 1)])
def test_column_set_and_get(rq, G, dtype, fill):
    g, _, mids, _ = G
    np_t = np.dtype({"i32": np.int32, "u64": np.uint64}[dtype])
    g.create_attr("scratch", dtype, fill=fill)
    try:
        assert (g.attr_array("scratch") == np_t.type(fill)).all() and g.attr_array("scratch").shape == (N,)
        rng = np.random.default_rng(83)
        ids = request(rng, N, S.M_IDS, N, 2**32, repeats=215_000)             # a tenth of the ids a second time, and the draws' own repeats
        vals = rng.integers(0, 2**63, size=S.M_IDS, dtype=np.uint64).astype(np_t)          # (every request another value)
        assert g.set_attr("scratch", ids, vals) == 150_000
        uniq, last, absent = S.set_last_wins(ids, vals, ids < N)
        assert absent == 150_000 and uniq.size < S.M_IDS - 150_000 - 215_000
        by_id = np.full(N, fill, dtype=np_t)
        by_id[uniq] = last
        got = g.attr_array("scratch")
        assert np.array_equal(got, by_id[mids]), np.nonzero(got != by_id[mids])[0][:5]
        ask = request(np.random.default_rng(84), N, S.M_IDS, N, 2**32)
        v, found = g.get_attr("scratch", ask)
        st = rq.last_by_id_stats()
        assert np.array_equal(found, ask < N) and np.array_equal(v, np.where(ask < N, by_id[np.minimum(ask, N - 1)], np_t.type(fill)))
        assert st["found"] == (ask < N).sum() and st["absent"] == 150_000
    finally:
        g.drop_attr("scratch")


# ---- 5. predicates ---------------------------------------------------------------------------------------------------------------------
def keep_of(cols, name):
    """the model's admitted positions of predicate `name`, and what has to hold of the model alone for the test to mean something"""
    keep = S.where_fast(cols, S.predicates()[name])
    n = keep.size
    assert 0.01 < keep.mean() < 0.99, (name, keep.mean())
    for part in (keep[2_097_152:], keep[n - n % 64:]):                        # past one trip of where_kernel's grid; the last, partial run
        assert part.size and part.any() and not part.all(), name
    return keep


_OTHER = {}


@pytest.mark.parametrize("name", sorted(S.NS_OF))
def test_predicates(rq, G, name):
    g, _, mids, cols = G
    keep = keep_of(cols, name)
    if "keep" not in _OTHER:
        _OTHER["keep"] = keep_of(cols, "ns2_wide")
    other = _OTHER["keep"]
    with g.where(S.predicates()[name]) as f:
        st = rq.last_where_stats()
        assert st["rows"] == N and st["admitted"] == f.rows == keep.sum(), (name, st)
        ns, wide = S.NS_OF[name]
        assert (1 if st["columns"] <= 1 else 2 if st["columns"] <= 2 else 4 if st["columns"] <= 4 else 8) == ns
        assert (st["bytes_read"] > 4 * N * st["columns"]) == wide
        got = f.ids()
        assert got.dtype == np.uint32 and np.array_equal(got, mids[keep]), (name, "ids() in position order over 269 blocks")
        mask = np.zeros(N + 3, dtype=bool)
        mask[mids[keep]] = True
        assert np.array_equal(f.id_bits(N + 3), mask), name
        with g.where(S.predicates()["ns2_wide"]) as o:
            for made, want in ((~f, ~keep), (f & o, keep & other), (f | o, keep | other), (f - o, keep & ~other)):
                with made as c:
                    assert c.rows == want.sum() and np.array_equal(c.ids(), mids[want]), name


@pytest.mark.parametrize("name", S.ANSWERS)
def test_predicate_answers_equal_the_id_list_filters(rq, rows, G, name):
    g, _, mids, cols = G
    q = rows[3]
    keep = keep_of(cols, name)
    with g.where(S.predicates()[name]) as f, g.make_filter(ids=mids[keep]) as y:
        assert f.rows == y.rows == keep.sum()
        admitted = mids[keep]
        for nq in (64, 200):                                                  # the few-launch path and the staged launches
            a, b = g.query_batch(q[:nq], 4, 10, filter=f), g.query_batch(q[:nq], 4, 10, filter=y)
            for u, v in zip(a, b):
                assert np.array_equal(bits(u), bits(v)), (name, "query_batch", nq)
            assert (a[2] == 10).all() and np.isin(a[1], admitted).all(), (name, "query_batch", nq)
        a, b = g.range_search(q[:20], 4, 80.0, filter=f), g.range_search(q[:20], 4, 80.0, filter=y)
        for u, v in zip(a, b):
            assert np.array_equal(bits(u), bits(v)), (name, "range_search")
        assert a[0][-1] == a[2].size > 0 and np.isin(a[2], admitted).all(), (name, "range_search")
        a, b = g.exact_search(q[:8], 10, filter=f), g.exact_search(q[:8], 10, filter=y)
        for u, v in zip(a, b):
            assert np.array_equal(bits(u), bits(v)), (name, "exact_search")
        assert (a[2] == 10).all() and np.isin(a[1], admitted).all(), (name, "exact_search")


# ---- 6. the id list cut short ----------------------------------------------------------------------------------------------------------------
def test_ids_device_cut_short(rq, G):
    import torch
    g, _, mids, cols = G
    keep = keep_of(cols, S.HALF)
    want = mids[keep]
    rows_n = int(keep.sum())
    assert 0.45 * N < rows_n < 0.55 * N
    with g.where(S.predicates()[S.HALF]) as f:
        assert f.rows == rows_n
        for cap in (0, 1, 8191, 8192, 8193, rows_n - 1, rows_n, rows_n + 5):
            out = torch.full((rows_n + 64,), SENTINEL - 2**32, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert f.ids_device(out.data_ptr(), cap) == rows_n, cap
            got = out.cpu().numpy().view(np.uint32)
            cut = min(cap, rows_n)
            assert np.array_equal(got[:cut], want[:cut]), (cap, np.nonzero(got[:cut] != want[:cut])[0][:5])
            assert (got[cut:] == SENTINEL).all(), (cap, "a slot past the cut was written")


# ---- 7. pending removals, compaction, an add --------------------------------------------------------------------------------------------
# (three tests, each on its own copy with its own removals, so that none takes longer than test_scale_2m)
def with_pending_removals(G):
    """-> (a copy of G with DEAD rows marked dead, the dead ids, alive by position, ids to ask for: the dead, 200 000 draws, two absent)"""
    g0, _, mids, _ = G
    g = g0.copy()
    rng = np.random.default_rng(85)
    dead = rng.choice(N, size=S.DEAD, replace=False).astype(np.uint32)
    alive_id = np.ones(N, dtype=bool)
    alive_id[dead] = False
    assert g.remove(ids=dead, lazy=True) == S.DEAD and g.live_n == N - S.DEAD and g.n == N
    ask = np.concatenate([dead, rng.choice(N, size=200_000), [N, 2**32 - 1]]).astype(np.uint32)
    return g, dead, alive_id[mids], ask


def test_pending_removals(rq, G):
    _, _, mids, cols = G
    g, dead, alive, ask = with_pending_removals(G)
    try:
        want = locate_model(mids, ask, live=alive)
        got = g.locate(ask)
        assert np.array_equal(got, want) and (want[:S.DEAD] == BM.ABSENT).all() and (want[S.DEAD:] != BM.ABSENT).sum() > 190_000
        v, found = g.get_attr("I", ask)
        there = want != BM.ABSENT
        assert np.array_equal(found, there) and (v[~there] == S.FILLS["I"]).all()
        assert np.array_equal(v[there], S.merged_values("I", ask[there]))
        keep = keep_of(cols, S.HALF)
        with g.where(S.predicates()[S.HALF]) as f, ~f as nf:                  # no dead row under a predicate, none under its complement
            assert f.rows == (keep & alive).sum() and np.array_equal(f.ids(), mids[keep & alive])
            assert nf.rows == (~keep & alive).sum() and np.array_equal(nf.ids(), mids[~keep & alive])
            assert f.rows + nf.rows == N - S.DEAD
    finally:
        g.close()


def test_compaction(rq, G):
    """the columns follow their rows past one trip of the gather, the directory is made again"""
    _, _, mids, cols = G
    g, dead, alive, ask = with_pending_removals(G)
    try:
        assert not g.contains(dead[:100]).any() and rq.last_by_id_stats()["built"] == 1
        assert g.compact() == S.DEAD and g.n == S.N_COMPACT == g.live_n and g.pending_removals == 0
        mids2 = g.map_ids
        assert np.array_equal(mids2, mids[alive])                             # the live rows keep their order
        for name in S.COLUMNS:
            assert np.array_equal(bits(g.attr_array(name)), bits(cols[name][1][alive])), (name, "after compact")
        got = g.locate(ask)
        st = rq.last_by_id_stats()
        assert (st["form"], st["built"]) == ("dense", 1) and np.array_equal(got, locate_model(mids2, ask)), st
        assert (got[:S.DEAD] == BM.ABSENT).all()
        cols2 = {name: (dtype, vals[alive]) for name, (dtype, vals) in cols.items()}
        with g.where(S.predicates()["ns8_narrow"]) as f:
            k2 = keep_of(cols2, "ns8_narrow")
            assert rq.last_where_stats()["rows"] == S.N_COMPACT and np.array_equal(f.ids(), mids2[k2])
    finally:
        g.close()


def test_add_after_removals(rq, rows, G):
    """an add with removals pending compacts first; the new rows hold every column's fill, the old rows keep their values"""
    _, _, mids, cols = G
    x = rows[0]
    g, dead, alive, _ = with_pending_removals(G)
    try:
        first = g.add_device(x.data_ptr(), S.ADDED, D)                        # (copies of the first rows under new ids)
        assert first == int(mids[alive].max()) + 1 and g.n == S.N_COMPACT + S.ADDED and g.pending_removals == 0
        mids3 = g.map_ids
        new = mids3 >= first
        assert new.sum() == S.ADDED and np.array_equal(mids3[~new], mids[alive])
        assert np.array_equal(np.sort(mids3[new]), np.arange(first, first + S.ADDED, dtype=np.uint32))
        for name in S.COLUMNS:
            got = g.attr_array(name)
            assert np.array_equal(bits(got[~new]), bits(cols[name][1][alive])), (name, "after add")
            assert np.array_equal(bits(got[new]), bits(np.full(S.ADDED, S.FILLS[name], dtype=got.dtype))), (name, "fill of the new rows")
    finally:
        g.close()


# ---- 8. grouped search ---------------------------------------------------------------------------------------------------------------------
def same_groups(res, src, values_of, topk, gs, fetch, what):
    d, i, c = src
    want = GM.group_rows(d, i, c, S.keymap_for(i, values_of), topk, gs)
    assert res.ids.shape == (len(c), topk, gs) and np.array_equal(res.counts, want["n"]), what
    assert np.array_equal(res.ids, want["ids"]), (what, np.argwhere(res.ids != want["ids"])[:4])
    assert np.array_equal(np.ascontiguousarray(res.dist).view(np.uint32), want["dist_bits"]), what
    assert np.array_equal(GM.key_image(res.keys), want["keys"]) and np.array_equal(res.group_counts, want["group_n"]), what
    assert np.array_equal(res.fetched, np.minimum(c, fetch)) and want["absent"] == 0 and want["kept"] > 0, what


@pytest.mark.parametrize("nq,topk,gs,fetch,col", [(64, 10, 3, 64, "u"), (200, 10, 3, 64, "I"), (64, 100, 2, 2048, "I"), (200, 100, 2, 2048, "u")])
def test_grouped_search(rq, rows, G, nq, topk, gs, fetch, col):
    g, _, mids, _ = G
    q = rows[3][:nq]
    values_of = lambda ids: S.merged_values(col, ids)
    src = g.query_batch(q, 4, fetch)
    res = g.query_batch_grouped(q, 4, topk, col, group_size=gs, fetch=fetch)
    assert (src[2] > 0).all() and (src[1][src[1] != GM.PAD_ID] >= 1_048_576).any()     # rows of the merged-in half among the candidates
    same_groups(res, src, values_of, topk, gs, fetch, (nq, topk, gs, fetch, col))
    held = res.ids != GM.PAD_ID                                               # independent of the model: a group's members hold its key
    assert np.array_equal(GM.key_image(values_of(res.ids[held])), np.broadcast_to(GM.key_image(res.keys)[:, :, None], res.ids.shape)[held])


def test_grouped_exact_search(rq, rows, G):
    g, _, mids, _ = G
    q = rows[3][:20]
    src = g.exact_search(q, 64)
    res = g.exact_search_grouped(q, 10, "u", group_size=3, fetch=64)
    same_groups(res, src, lambda ids: S.merged_values("u", ids), 10, 3, 64, "exact")


# ---- 9. neighbours_of past one trip of drop_self_kernel ----------------------------------------------------------------------------------
def test_neighbours_of_many_ids(rq):
    n = S.N_NEIGH
    x, centres, _ = synth.mixture(n, D, K, sigma=0.8, seed=900, centre_scale=0.6)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(D, seed=77))
    try:
        rng = np.random.default_rng(86)
        ids = rng.integers(0, n, size=S.M_NEIGH).astype(np.uint32)            # every stored id about ninety times
        gone = rng.random(S.M_NEIGH) < 0.05
        ids[gone] = rng.integers(n, 2**32, size=int(gone.sum()), dtype=np.uint64).astype(np.uint32)
        d, i, found = g.neighbours_of(ids, 1, 3)
        st = rq.last_by_id_stats()
        assert st["found"] + st["absent"] == S.M_NEIGH and st["absent"] == gone.sum()
        fetched, f2 = g.fetch(ids)
        assert np.array_equal(f2, ~gone) and np.array_equal(found, f2)
        plain = g.query_batch(fetched, 1, 4)
        ed, ei = S.drop_self_fast(*plain, ids, f2)
        assert np.array_equal(i, ei), np.nonzero((i != ei).any(1))[0][:5]
        assert np.array_equal(bits(d), bits(ed))
        assert (i[gone] == BM.ABSENT).all() and np.isnan(d[gone]).all() and (i[~gone, 0] != BM.ABSENT).all()
        assert (i[~gone] != ids[~gone, None]).all()                           # no row is its own neighbour (no two rows are equal)
        at = np.arange(262_144, S.M_NEIGH, 97)                                # rows of the second trip, by the per-row model
        sd, si = BM.drop_self(plain[0][at], plain[1][at], plain[2][at], ids[at], f2[at])
        assert np.array_equal(i[at], si) and np.array_equal(bits(d[at]), bits(sd))
    finally:
        g.close()
