"""Filtered queries (rq_filter_create / rq_query_batch*_filtered): a query restricted to an allow-list of ids returns exactly
what the unfiltered query returns on the SUB-INDEX -- the same rotation, centroids and k, every list keeping only its admitted
rows in stored order.  Every check is bit for bit: ids, distance bits, counts, status and the process counters, against the
engine's unfiltered query on RaBitQ.from_arrays of the removed-rows arrays and against the CPU oracle's view of them.

Run on the GPU box:  python -m pytest tests/test_filtered_gpu.py -m gpu -q
"""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import synth
from tests.models import bits, sub_arrays

pytestmark = pytest.mark.gpu

# scan implementation x gate of the matrix-core scan (as in test_gpu_parity.py): VALU, bf16 threshold MFMA, additive bound
SCAN_VARIANTS = [(1, 0), (2, 1), (2, 2)]


@pytest.fixture(scope="module")
def rq():
    import os
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def check_same(rq, gidx, filt, sidx, queries, probe, topk, heur, what=""):
    """filtered on the full index == unfiltered on the sub-index: results and counters."""
    rq.metrics_reset()
    a = gidx.query_batch(queries, probe, topk, heur, filter=filt)
    ma = rq.metrics()
    rq.metrics_reset()
    b = sidx.query_batch(queries, probe, topk, heur)
    mb = rq.metrics()
    assert np.array_equal(a[2], b[2]), (what, "counts", np.nonzero(a[2] != b[2])[0][:5])
    for qi in range(len(queries)):
        n = int(a[2][qi])
        assert np.array_equal(a[1][qi, :n], b[1][qi, :n]), (what, qi, a[1][qi, :n], b[1][qi, :n])
        assert np.array_equal(bits(a[0][qi, :n]), bits(b[0][qi, :n])), (what, qi)
    assert (ma["rough"], ma["precise"], ma["query"]) == (mb["rough"], mb["precise"], mb["query"]), (what, ma, mb)
    return a, ma


def check_oracle(rq, oracle, gidx, filt, sub, queries, probe, topk, heur):
    """filtered on the full index == the oracle on the sub-index (per query, counters summed)."""
    ov = oracle.OracleIndex.view(gidx.dim, *sub)
    try:
        rq.metrics_reset()
        d, ids, cnt = gidx.query_batch(queries, probe, topk, heur, filter=filt)
        m = rq.metrics()
        tot_r = tot_p = 0
        for qi, q in enumerate(queries):
            oracle.metrics_reset()
            od, oi = ov.query(q, probe, topk, heur)
            om = oracle.metrics()
            tot_r += om["rough"]
            tot_p += om["precise"]
            n = int(cnt[qi])
            assert n == oi.size and np.array_equal(ids[qi, :n], oi), (qi, ids[qi, :n], oi)
            assert np.array_equal(bits(d[qi, :n]), bits(od)), qi
        assert (m["rough"], m["precise"], m["query"]) == (tot_r, tot_p, len(queries))
    finally:
        ov.close()


def filters_of(gidx, n, rng):
    """name -> bool mask over ids: everything, one id, random 50 % and 1 %, and whole lists (correlated with the clustering)."""
    mids, offs = gidx.map_ids, gidx.offsets.astype(np.int64)
    out = {"all": np.ones(n, dtype=bool)}
    one = np.zeros(n, dtype=bool)
    one[int(mids[offs[1] if gidx.k > 1 and offs[1] < n else 0])] = True
    out["one"] = one
    out["half"] = rng.random(n) < 0.5
    out["pct1"] = rng.random(n) < 0.01
    lists = np.zeros(n, dtype=bool)
    for c in range(0, gidx.k, 4):   # a quarter of the lists, whole
        lists[mids[offs[c]:offs[c + 1]]] = True
    out["lists"] = lists
    return out


@pytest.mark.parametrize("d,k,impl,gate", [(64, 12, 1, 0), (64, 12, 2, 1), (64, 12, 2, 2), (128, 16, 1, 0), (128, 16, 2, 1),
                                           (128, 16, 2, 2), (768, 6, 0, 0), (960, 6, 0, 0),
                                           (1024, 5, 2, 0)])   # dim 1024: the matrix-core ring beyond 64 KiB of LDS
def test_filtered_equals_sub_index(rq, oracle, d, k, impl, gate):
    """Every filter shape, heap and heuristic rankers, small (<= 64) and large (>= 256) batches, the scan variants at dim 64 /
    128, the wide matrix-core instantiations (dim 768; dim 1024 on the matrix cores everywhere) and the generic-W scan (dim 960).
    Sparse filters leave some queries of the heuristic ranker with nothing (RQ_ERR_EMPTY for the batch): the batch still has to
    match the sub-index's query by query."""
    from rabitq_amd import index as ix
    n = 6000 if d <= 128 else (2500 if d < 1024 else 1500)
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=d + k, centre_scale=0.6)
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=d + 1)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=d + 2, centre_scale=0.6)
    queries[3] = x[5]
    rng = np.random.default_rng(d)
    ix.set_option("scan_impl", impl)
    ix.set_option("scan_gate", gate)
    try:
        for name, allowed in filters_of(gidx, n, rng).items():
            sub = sub_arrays(gidx, allowed)
            sidx = rq.RaBitQ.from_arrays(*sub)
            with gidx.make_filter(mask=allowed) as f:
                assert f.rows == int(allowed.sum())
                for nq, probe, topk, heur in ((300, k, 10, False), (300, 4, 50, False), (40, k, 10, False), (1, k, 10, False),
                                              (300, k, 10, True)):
                    check_same(rq, gidx, f, sidx, queries[:nq], probe, topk, heur, (name, nq, probe, topk, heur))
                if name in ("half", "lists") and d <= 128 and impl != 2:
                    check_oracle(rq, oracle, gidx, f, sub, queries[:40], k, 10, False)
            sidx.close()
        # the id form and the mask form are the same filter
        allowed = filters_of(gidx, n, np.random.default_rng(d))["half"]
        with gidx.make_filter(ids=np.nonzero(allowed)[0]) as fi, gidx.make_filter(mask=allowed) as fm:
            a = gidx.query_batch(queries[:64], k, 10, filter=fi)
            b = gidx.query_batch(queries[:64], k, 10, filter=fm)
            for u, v in zip(a, b):
                assert np.array_equal(bits(u), bits(v))
    finally:
        ix.set_option("scan_impl", 0)
        ix.set_option("scan_gate", 0)
    gidx.close()


def test_all_admitted_equals_unfiltered_and_query_entry(rq):
    """A filter that admits everything is the unfiltered call (counters included); query(filter=) is the one-query batch."""
    from rabitq_amd import index as ix
    n, d, k = 8000, 128, 20
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=3, centre_scale=0.6)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=4))
    queries, _, _ = synth.mixture(512, d, k, sigma=0.8, seed=5, centre_scale=0.6)
    with gidx.make_filter(ids=np.arange(n)) as f:
        assert f.rows == n
        for nq, heur in ((512, False), (512, True), (20, False)):
            rq.metrics_reset()
            a = gidx.query_batch(queries[:nq], 8, 10, heur, filter=f)
            ma = rq.metrics()
            rq.metrics_reset()
            b = gidx.query_batch(queries[:nq], 8, 10, heur)
            mb = rq.metrics()
            for u, v in zip(a, b):
                assert np.array_equal(bits(u), bits(v))
            assert (ma["rough"], ma["precise"], ma["query"]) == (mb["rough"], mb["precise"], mb["query"])
        for q in queries[:5]:
            assert gidx.query(q, 8, 10, filter=f) == gidx.query(q, 8, 10)
        # the profile's matrix-core pair count reads the stream lengths (not the admitted rows) on a filtered pass as well
        ix.set_option("scan_impl", 2)
        ix.set_profiling(1)
        try:
            gidx.query_batch(queries, 8, 10, filter=f)
            pf = ix.last_profile()
            gidx.query_batch(queries, 8, 10)
            pu = ix.last_profile()
        finally:
            ix.set_profiling(0)
            ix.set_option("scan_impl", 0)
        assert pf["matrix_launches"] > 0 and pf["matrix_pairs"] == pu["matrix_pairs"]
    gidx.close()


def test_nothing_admitted(rq):
    """An empty filter: no results for the heap ranker, RQ_ERR_EMPTY for the heuristic one (the sub-index's status), no
    rough / precise counts.  A one-id filter: the heuristic ranker returns that id or reports RQ_ERR_EMPTY, as the sub-index."""
    from rabitq_amd import _lib
    n, d, k = 5000, 64, 10
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=11, centre_scale=0.6)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=12))
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=13, centre_scale=0.6)
    for f in (gidx.make_filter(ids=np.array([], dtype=np.int64)), gidx.make_filter(mask=np.zeros(n, dtype=bool))):
        assert f.rows == 0
        for nq in (300, 3):
            rq.metrics_reset()
            _, _, cnt = gidx.query_batch(queries[:nq], k, 10, filter=f)
            assert not cnt.any()
            m = rq.metrics()
            assert (m["rough"], m["precise"], m["query"]) == (0, 0, nq)
        with pytest.raises(_lib.RabitqError) as e:
            gidx.query(queries[0], k, 10, heuristic_rank=True, filter=f)
        assert e.value.status == _lib.RQ_ERR_EMPTY
        f.close()
    allowed = np.zeros(n, dtype=bool)
    allowed[int(gidx.map_ids[0])] = True
    sidx = rq.RaBitQ.from_arrays(*sub_arrays(gidx, allowed))
    with gidx.make_filter(mask=allowed) as f:
        for q in queries[:8]:
            try:
                want = sidx.query(q, k, 10, heuristic_rank=True)
            except _lib.RabitqError as e:
                assert e.status == _lib.RQ_ERR_EMPTY
                with pytest.raises(_lib.RabitqError) as e2:
                    gidx.query(q, k, 10, heuristic_rank=True, filter=f)
                assert e2.value.status == _lib.RQ_ERR_EMPTY
                continue
            assert gidx.query(q, k, 10, heuristic_rank=True, filter=f) == want
    sidx.close()
    gidx.close()


def test_filter_rows_and_validation(rq):
    """rq_filter_rows = the popcount over map_ids; ids >= nbits are not admitted; a filter of another index, nbits > 2^32, a
    NULL bitmap with nbits > 0 and a NULL index are RQ_ERR_INVALID."""
    from rabitq_amd import _lib
    L = _lib.lib()
    n, d, k = 4000, 64, 8
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=21, centre_scale=0.6)
    a = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=22))
    b = rq.RaBitQ.build(x[:3000], centres, synth.random_orthogonal(d, seed=22))
    rng = np.random.default_rng(0)
    ids = rng.integers(0, n + 500, size=1700)
    mask = np.zeros(n + 500, dtype=bool)
    mask[ids] = True
    with a.make_filter(ids=ids) as f:
        assert f.rows == int(mask[a.map_ids].sum())
        q = x[:4]
        d_ = np.zeros((4, 10), np.float32)
        i_ = np.zeros((4, 10), np.uint32)
        c_ = np.zeros(4, np.uint32)
        st = L.rq_query_batch_filtered(b._h, f._h, q.ctypes.data, 4, d, 4, 10, 0, d_.ctypes.data, i_.ctypes.data,
                                       c_.ctypes.data)
        assert st == -1  # RQ_ERR_INVALID: the filter belongs to another index
        st = L.rq_query_batch_filtered(None, f._h, q.ctypes.data, 4, d, 4, 10, 0, d_.ctypes.data, i_.ctypes.data,
                                       c_.ctypes.data)
        assert st == -1
    words = np.zeros(4, np.uint32)
    out = C.c_void_p()
    assert L.rq_filter_create(a._h, words.ctypes.data, (1 << 32) + 1, 0, C.byref(out)) == -1
    assert L.rq_filter_create(a._h, None, 10, 0, C.byref(out)) == -1
    assert L.rq_filter_create(None, words.ctypes.data, 10, 0, C.byref(out)) == -1
    with a.make_filter(ids=np.arange(n)) as f:
        assert f.rows == n
    a.close()
    b.close()


def test_device_bitmap_filter(rq):
    """make_filter_device (the bitmap in device memory) and query_batch_device(filter=)."""
    import torch
    n, d, k = 6000, 128, 12
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=31, centre_scale=0.6)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=32))
    allowed = np.random.default_rng(1).random(n) < 0.3
    words, nbits = rq.pack_filter_bits(mask=allowed)
    dev_words = torch.from_numpy(words.view(np.int32).copy()).cuda()
    queries, _, _ = synth.mixture(400, d, k, sigma=0.8, seed=33, centre_scale=0.6)
    with gidx.make_filter_device(dev_words.data_ptr(), nbits) as fd, gidx.make_filter(mask=allowed) as fh:
        assert fd.rows == fh.rows == int(allowed.sum())
        dq = torch.from_numpy(queries).cuda()
        od = torch.zeros((400, 10), dtype=torch.float32, device="cuda")
        oi = torch.zeros((400, 10), dtype=torch.int32, device="cuda")
        on = torch.zeros(400, dtype=torch.int32, device="cuda")
        gidx.query_batch_device(dq.data_ptr(), 400, d, k, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr(), filter=fd)
        torch.cuda.synchronize()
        hd, hi, hn = gidx.query_batch(queries, k, 10, filter=fh)
        assert np.array_equal(on.cpu().numpy().view(np.uint32), hn)
        for qi in range(400):
            m = int(hn[qi])
            assert np.array_equal(oi.cpu().numpy()[qi, :m].view(np.uint32), hi[qi, :m])
            assert np.array_equal(bits(od.cpu().numpy()[qi, :m]), bits(hd[qi, :m]))
    gidx.close()


def test_filtered_overflow_rerun_and_arena_stages(rq, oracle):
    """One list and a large topk: the filtered pass overflows its survivor buffers and re-runs the affected queries (with the
    filter); then every large batch through the survivor arena (survivor_segments = 2)."""
    from rabitq_amd import index as ix
    n, d = 24000, 64
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    gidx = rq.RaBitQ.build(x, np.zeros((1, d), np.float32), synth.random_orthogonal(d, seed=3))
    allowed = rng.random(n) < 0.5
    sub = sub_arrays(gidx, allowed)
    sidx = rq.RaBitQ.from_arrays(*sub)
    queries = rng.standard_normal((6, d)).astype(np.float32) * 0.2
    with gidx.make_filter(mask=allowed) as f:
        check_oracle(rq, oracle, gidx, f, sub, queries, 1, 2000, False)
        assert ix.last_profile()["retries"] > 0, "the test no longer exercises the overflow path"
        check_same(rq, gidx, f, sidx, queries, 1, 1000, True, "heuristic")
    sidx.close()
    gidx.close()
    n, d, k = 30000, 128, 16
    x, centres, _ = synth.mixture(n, d, k, sigma=1.0, seed=41, centre_scale=0.5)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=42))
    queries, _, _ = synth.mixture(600, d, k, sigma=1.0, seed=43, centre_scale=0.5)
    allowed = np.random.default_rng(2).random(n) < 0.5
    sidx = rq.RaBitQ.from_arrays(*sub_arrays(gidx, allowed))
    ix.set_option("survivor_segments", 2)
    try:
        with gidx.make_filter(mask=allowed) as f:
            for topk, heur in ((100, False), (10, False), (50, True)):
                check_same(rq, gidx, f, sidx, queries, k, topk, heur, ("arena", topk, heur))
                assert ix.last_profile()["segmented_passes"] >= 1
    finally:
        ix.set_option("survivor_segments", 1)
    sidx.close()
    gidx.close()


def test_filter_learns_its_own_survivor_capacity(rq):
    """A filtered call whose survivors overflow the default buffers teaches the FILTER a larger capacity, not the index: later
    unfiltered large batches keep the uniform buffers, later filtered ones size their final stage per query."""
    from rabitq_amd import index as ix
    n, d = 24000, 64
    rng = np.random.default_rng(8)
    x = rng.standard_normal((n, d)).astype(np.float32)
    gidx = rq.RaBitQ.build(x, np.zeros((1, d), np.float32), synth.random_orthogonal(d, seed=9))
    queries = rng.standard_normal((300, d)).astype(np.float32) * 0.2
    allowed = rng.random(n) < 0.5
    sidx = rq.RaBitQ.from_arrays(*sub_arrays(gidx, allowed))
    gidx.query_batch(queries, 1, 10)
    assert ix.last_profile()["segmented_passes"] == 0
    with gidx.make_filter(mask=allowed) as f:
        check_same(rq, gidx, f, sidx, queries[:6], 1, 2000, False, "overflow")
        gidx.query_batch(queries[:6], 1, 2000, filter=f)
        gidx.query_batch(queries, 1, 10)
        assert ix.last_profile()["segmented_passes"] == 0, "a filtered call resized the index's unfiltered passes"
        check_same(rq, gidx, f, sidx, queries, 1, 10, False, "after")
        gidx.query_batch(queries, 1, 10, filter=f)
        assert ix.last_profile()["segmented_passes"] == 1, "the filter did not keep what its passes learnt"
    sidx.close()
    gidx.close()


def test_filtered_call_of_several_passes(rq):
    """More than 65 536 queries: several passes, overlapped (and one after the other), every pass filtered."""
    from rabitq_amd import index as ix
    n, d, k = 20000, 64, 32
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=51, centre_scale=0.6)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=52))
    queries, _, _ = synth.mixture(70000, d, k, sigma=0.8, seed=53, centre_scale=0.6)
    allowed = np.random.default_rng(3).random(n) < 0.3
    sidx = rq.RaBitQ.from_arrays(*sub_arrays(gidx, allowed))
    with gidx.make_filter(mask=allowed) as f:
        for overlap in (1, 0):
            ix.set_option("pass_overlap", overlap)
            try:
                check_same(rq, gidx, f, sidx, queries, 6, 10, False, ("passes", overlap))
            finally:
                ix.set_option("pass_overlap", 1)
    sidx.close()
    gidx.close()


@pytest.mark.parametrize("kind", ["tiered", "split_rows"])
def test_filtered_tiered_and_split_rows(rq, kind):
    """Raw vectors partly in pinned host memory (base_device_mb = 1), and split rows: the rerank is unchanged by the filter."""
    from rabitq_amd import index as ix
    n, d, k = 12000, 128, 24
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=61, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=62)
    plain = rq.RaBitQ.build(x, centres, P)
    allowed = np.random.default_rng(4).random(n) < 0.4
    sub = sub_arrays(plain, allowed)
    sidx = rq.RaBitQ.from_arrays(*sub)
    if kind == "tiered":
        ix.set_option("base_device_mb", 1)
    else:
        ix.set_option("split_rows", 2)
    try:
        gidx = rq.RaBitQ.build(x, centres, P)
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)
    assert (gidx.n_hbm < n) if kind == "tiered" else gidx.split_rows
    queries, _, _ = synth.mixture(400, d, k, sigma=0.8, seed=63, centre_scale=0.6)
    with gidx.make_filter(mask=allowed) as f:
        for nq, heur in ((400, False), (400, True), (16, False)):
            check_same(rq, gidx, f, sidx, queries[:nq], 8, 10, heur, (kind, nq, heur))
    sidx.close()
    gidx.close()
    plain.close()


def test_filtered_and_unfiltered_queries_concurrently(rq):
    """Filtered (two filters) and unfiltered queries from several threads on one handle: every result as when run alone."""
    n, d, k = 20000, 128, 32
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=71, centre_scale=0.6)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=72))
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=73, centre_scale=0.6)
    rng = np.random.default_rng(5)
    filts = [None, gidx.make_filter(mask=rng.random(n) < 0.5), gidx.make_filter(mask=rng.random(n) < 0.05)]
    want = [gidx.query_batch(queries, 8, 10, filter=f) for f in filts]
    errors = []

    def worker(t):
        try:
            for it in range(6):
                j = (t + it) % 3
                got = gidx.query_batch(queries, 8, 10, filter=filts[j])
                for u, v in zip(got, want[j]):
                    if not np.array_equal(bits(u), bits(v)):
                        errors.append((t, it, j))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:5]
    for f in filts[1:]:
        f.close()
    gidx.close()


def test_large_batch_stages_at_scale(rq):
    """2M x 128, 1024 lists, 8192 queries, nprobe 64, 10 % admitted: filtered on the full index == unfiltered on the sub-index,
    both on the GPU (the matrix-core stages, cluster-major grouping and the full-chip rerank all run)."""
    n, d, k = 2_000_000, 128, 1024
    x, centres, _ = synth.mixture(n, d, k, sigma=0.5, seed=81, centre_scale=1.0)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=82))
    del x
    queries, _, _ = synth.mixture(8192, d, k, sigma=0.5, seed=83, centre_scale=1.0)
    allowed = np.random.default_rng(6).random(n) < 0.1
    sidx = rq.RaBitQ.from_arrays(*sub_arrays(gidx, allowed))
    with gidx.make_filter(mask=allowed) as f:
        assert f.rows == int(allowed.sum())
        _, m = check_same(rq, gidx, f, sidx, queries, 64, 10, False, "2M")
        assert m["rough"] > 0
    sidx.close()
    gidx.close()
