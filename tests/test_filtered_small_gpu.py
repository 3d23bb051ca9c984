"""Filtered batches of <= 64 queries on the few-launch path (the FILT instantiations of sb_query_kernel, option
"small_batch_filtered") and filtered tickets (rq_query_batch_device_begin_filtered).  As everywhere: a filtered query is the
unfiltered query on the sub-index, bit for bit -- ids, order, distance bits, out_n, status and the rough / precise / query
counters -- and the path taken never changes a result.  Every case asserts that the small-batch path was really taken.

Run on the GPU box:  python -m pytest tests/test_filtered_small_gpu.py -m gpu -q
"""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import cosine_model as cm
from tests import scan_cases, synth
from tests.models import bits, sub_arrays
from tests.test_filtered_gpu import check_oracle, check_same, filters_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rq():
    import os
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


@pytest.fixture(autouse=True)
def restore_options():
    from rabitq_amd import index as ix
    yield
    for name, v in (("small_batch_filtered", 1), ("small_batch_span", 2560), ("scan_impl", 0), ("small_batch", 0)):
        ix.set_option(name, v)


def mixture_index(rq, n, d, k):
    """The indexes of test_small_batch_path_matches_oracle: a duplicated centroid (a tie in the probe selection) and an empty list."""
    x, centres, _ = synth.mixture(n, d, k, sigma=0.9, seed=n + d, centre_scale=0.6)
    if k > 4:
        centres[3] = centres[1]
        centres[k - 1] += 50.0
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=d + 7)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(64, d, k, sigma=0.9, seed=n + d + 1, centre_scale=0.6)
    queries[1] = x[11]
    return x, gidx, queries


@pytest.fixture(scope="module")
def big(rq):
    """80 000 x 128, 32 lists: more than 1 MiB of stream behind a query's block, so the final stage is a launch of its own."""
    x, gidx, queries = mixture_index(rq, 80_000, 128, 32)
    yield {"x": x, "gidx": gidx, "queries": queries, "n": 80_000, "d": 128, "k": 32}
    gidx.close()


def call(rq, idx, q, probe, topk, heur, filt=None):
    """One host-entry call -> (dist, ids, counts, status, (rough, precise, query), last_profile())."""
    from rabitq_amd import _lib
    from rabitq_amd import index as ix
    q = np.ascontiguousarray(q, dtype=np.float32)
    B = q.shape[0]
    d = np.full((B, topk), np.nan, dtype=np.float32)
    ids = np.full((B, topk), 0xFFFFFFFF, dtype=np.uint32)
    cnt = np.zeros(B, dtype=np.uint32)
    rq.metrics_reset()
    st = _lib.lib().rq_query_batch_filtered(idx._h, filt._h if filt is not None else None, q.ctypes.data, B, q.shape[1], probe, topk,
                                            int(heur), d.ctypes.data, ids.ctypes.data, cnt.ctypes.data)
    assert st in (0, _lib.RQ_ERR_EMPTY), (st, _lib.lib().rq_last_error())
    m = rq.metrics()
    return d, ids, cnt, st, (m["rough"], m["precise"], m["query"]), ix.last_profile()


def same(a, b, what):
    assert a[3] == b[3], (what, "status", a[3], b[3])
    assert np.array_equal(a[2], b[2]), (what, "counts", np.nonzero(a[2] != b[2])[0][:5])
    for qi in range(len(a[2])):
        n = int(a[2][qi])
        assert np.array_equal(a[1][qi, :n], b[1][qi, :n]), (what, qi, a[1][qi, :n], b[1][qi, :n])
        assert np.array_equal(bits(a[0][qi, :n]), bits(b[0][qi, :n])), (what, qi)
    assert a[4] == b[4], (what, "counters", a[4], b[4])


def shape_parity(rq, oracle, gidx, queries, n, d, k):
    from rabitq_amd import index as ix
    cfgs = [(1, min(k, 64), 10, False), (2, min(k, 32), 10, False), (64, min(k, 64), 10, False), (33, 5, 63, False),
            (16, min(k, 8), 256, False), (5, 1, 1, False), (20, min(k, 16), 10, True), (1, min(k, 6), 100, True)]
    filters = filters_of(gidx, n, np.random.default_rng(d))
    filters["none"] = np.zeros(n, dtype=bool)
    empty_batches = 0
    for name, allowed in filters.items():
        sub = sub_arrays(gidx, allowed)
        sidx = rq.RaBitQ.from_arrays(*sub)
        with gidx.make_filter(mask=allowed) as f:
            assert f.rows == int(allowed.sum())
            for nq, probe, topk, heur in cfgs:
                what = (name, nq, probe, topk, heur)
                q = queries[:nq]
                ix.set_option("small_batch_filtered", 2)
                a = call(rq, gidx, q, probe, topk, heur, f)
                assert a[5]["small_batch_passes"] == 1, (what, "the filtered batch did not take the small-batch path")
                ix.set_option("small_batch_filtered", 0)
                b = call(rq, gidx, q, probe, topk, heur, f)
                assert b[5]["small_batch_passes"] == 0, what
                same(a, b, (what, "small-batch path vs staged path"))
                same(a, call(rq, sidx, q, probe, topk, heur), (what, "filtered vs the sub-index"))   # (its status included)
                empty_batches += a[3] != 0
                if d <= 128 and name in ("half", "lists"):
                    ix.set_option("small_batch_filtered", 2)
                    try:
                        check_oracle(rq, oracle, gidx, f, sub, q, probe, topk, heur)
                    except RuntimeError as e:   # the oracle reports a reference panic (heuristic ranker without a candidate)
                        if "reference panics" not in str(e):
                            raise
                        continue
                    assert ix.last_profile()["small_batch_passes"] == 1, what
        sidx.close()
    assert empty_batches >= 2   # (the empty filter's heuristic batches at the least: RQ_ERR_EMPTY, the sub-index's status)


@pytest.mark.parametrize("n,d,k", [(3000, 64, 9), (5000, 100, 8), (9000, 256, 20), (30_000, 768, 12), (6000, 1024, 5)])
def test_parity_over_shapes(rq, oracle, n, d, k):
    """Every filter shape (and one that admits nothing) x eight batch shapes on the small-batch path: equal to the sub-index's
    unfiltered query and to the staged path; the oracle at d <= 128.  Streams that end inside the block, a padded dim, W = 12 with
    a final stage of its own."""
    _, gidx, queries = mixture_index(rq, n, d, k)
    try:
        shape_parity(rq, oracle, gidx, queries, n, d, k)
    finally:
        gidx.close()


def test_parity_with_a_separate_final_stage(rq, oracle, big):
    """The same on 80 000 x 128: the block hands its thresholds and work records to the filtered scan of the rest."""
    shape_parity(rq, oracle, big["gidx"], big["queries"], big["n"], big["d"], big["k"])


def test_final_stage_decides_answers(rq, oracle, big):
    """probe = k on 80 000 x 128, half of the rows admitted.  The queries are means of four rows from four different lists, so a
    query's neighbours are spread over those lists and most lie behind the block's part of the stream (two lists' worth at this
    density): at least half of the 64 queries return a row outside their nearest list -- asserted on the reference side first, from
    the oracle's sub-index alone (the mixture's own queries find all ten neighbours in their nearest list: 1 of 64 would pass)."""
    from rabitq_amd import index as ix
    gidx, x, n, k = big["gidx"], big["x"], big["n"], big["k"]
    offs, mids = gidx.offsets.astype(np.int64), gidx.map_ids
    rng = np.random.default_rng(5)
    full_lists = np.nonzero(np.diff(offs) > 0)[0]
    queries = np.stack([x[[mids[rng.integers(offs[c], offs[c + 1])] for c in rng.choice(full_lists, 4, replace=False)]].mean(0)
                        for _ in range(64)]).astype(np.float32)
    allowed = filters_of(gidx, n, np.random.default_rng(128))["half"]
    sub = sub_arrays(gidx, allowed)
    ov = oracle.OracleIndex.view(gidx.dim, *sub)
    full = oracle.OracleIndex.view(gidx.dim, *sub_arrays(gidx, np.ones(n, dtype=bool)))
    try:
        answers = [ov.query(q, k, 10, False)[1] for q in queries]
        outside, final = scan_cases.spread(ov, queries, answers, full)
        print("queries with an answer outside the nearest list:", int(outside.sum()), "behind the longest list's length:", int(final.sum()))
        assert outside.sum() >= 32, "the fixture no longer exercises the final stage"
    finally:
        ov.close(), full.close()
    ix.set_option("small_batch_filtered", 2)
    with gidx.make_filter(mask=allowed) as f:
        check_oracle(rq, oracle, gidx, f, sub, queries, k, 10, False)
        p = ix.last_profile()
        assert p["small_batch_passes"] == 1 and p["scan_launches"] >= 1


def test_overflow_behind_the_block_and_hints_stay_apart(rq, oracle):
    """One list of 60 000 rows, admitted: the stored positions [20 000, 30 000) only.  The block (15 360 positions at this density)
    sees no admitted row and hands over with the threshold at f32::MAX; the final stage passes all 10 000 admitted rows, more than
    the default survivor capacity of 4096: the queries are re-run by the staged filtered pass.  Afterwards the index's own hints
    are untouched (an unfiltered batch stays on the small-batch path) and the filtered call repeats bit for bit (the filter has
    learnt a capacity of 16 384: still the small-batch path's, no overflow)."""
    from rabitq_amd import index as ix
    n, d = 60_000, 128
    rng = np.random.default_rng(17)
    x = rng.standard_normal((n, d)).astype(np.float32)
    gidx = rq.RaBitQ.build(x, np.zeros((1, d), np.float32), synth.random_orthogonal(d, seed=18))
    queries = rng.standard_normal((6, d)).astype(np.float32) * 0.2
    allowed = np.zeros(n, dtype=bool)
    allowed[gidx.map_ids[20_000:30_000]] = True
    sub = sub_arrays(gidx, allowed)
    sidx = rq.RaBitQ.from_arrays(*sub)
    ix.set_option("small_batch_filtered", 2)
    try:
        with gidx.make_filter(mask=allowed) as f:
            check_oracle(rq, oracle, gidx, f, sub, queries, 1, 10, False)
            p = ix.last_profile()
            assert p["small_batch_passes"] == 1
            assert p["retries"] > 0, "the test no longer exercises the overflow behind the block"
            first = call(rq, gidx, queries, 1, 10, False, f)
            same(first, call(rq, sidx, queries, 1, 10, False), "after the overflow, against the sub-index")
            # hints stay apart
            u = call(rq, gidx, queries, 1, 10, False)
            assert u[5]["small_batch_passes"] == 1 and u[5]["retries"] == 0
            same(call(rq, gidx, queries, 1, 10, False, f), first, "the filtered call repeated")
            check_same(rq, gidx, f, sidx, queries, 1, 10, False, "repeated, against the sub-index")
    finally:
        sidx.close()
        gidx.close()


def test_knobs_do_not_change_results(rq, big):
    """small_batch_span (where the block's part ends) and scan_impl (the final stage's engine) on filtered small batches."""
    from rabitq_amd import index as ix
    gidx, queries, n, k = big["gidx"], big["queries"], big["n"], big["k"]
    fl = filters_of(gidx, n, np.random.default_rng(128))
    ix.set_option("small_batch_filtered", 2)
    for name in ("half", "pct1"):
        with gidx.make_filter(mask=fl[name]) as f:
            for nq in (1, 40):
                base = None
                try:
                    for span in (256, 2560, 20000):
                        for impl in (1, 2):
                            ix.set_option("small_batch_span", span)
                            ix.set_option("scan_impl", impl)
                            got = call(rq, gidx, queries[:nq], k, 10, False, f)
                            assert got[5]["small_batch_passes"] == 1, (name, nq, span, impl)
                            if base is None:
                                base = got
                            same(got, base, (name, nq, span, impl))
                finally:
                    ix.set_option("small_batch_span", 2560)
                    ix.set_option("scan_impl", 0)


def test_cosine_index(rq, oracle):
    """A cosine index's filtered small batch = the L2 index of the normalised rows asked the normalised queries, same filter."""
    from rabitq_amd import index as ix
    n, d, k = 6000, 128, 12
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=91, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=92)
    queries, _, _ = synth.mixture(64, d, k, sigma=0.8, seed=93, centre_scale=0.6)
    queries *= np.float32(2.5)
    g = rq.RaBitQ.build(x, centres, P, metric="cosine")
    l2 = rq.RaBitQ.build(cm.normalize_rows(oracle, x), cm.pad64(centres), P)
    nqs = cm.normalize_rows(oracle, queries)
    allowed = np.random.default_rng(9).random(n) < 0.5
    ix.set_option("small_batch_filtered", 2)
    try:
        with g.make_filter(mask=allowed) as fc, l2.make_filter(mask=allowed) as fl:
            for nq in (1, 64):
                a = call(rq, g, queries[:nq], k, 10, False, fc)
                assert a[5]["small_batch_passes"] == 1
                same(a, call(rq, l2, nqs[:nq], k, 10, False, fl), ("cosine", nq))
    finally:
        g.close(), l2.close()


class Dev:
    """Queries and outputs in device memory for the device entries."""

    def __init__(self, q, topk):
        import torch
        self.torch = torch
        self.q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda()
        self.nq, self.len, self.topk = q.shape[0], q.shape[1], topk
        self.od = torch.full((self.nq, topk), float("nan"), dtype=torch.float32, device="cuda")
        self.oi = torch.full((self.nq, topk), -1, dtype=torch.int32, device="cuda")
        self.on = torch.zeros(self.nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def args(self, probe):
        return (self.q.data_ptr(), self.nq, self.len, probe, self.topk, self.od.data_ptr(), self.oi.data_ptr(), self.on.data_ptr())

    def result(self):
        self.torch.cuda.synchronize()
        return self.od.cpu().numpy(), self.oi.cpu().numpy().view(np.uint32), self.on.cpu().numpy().view(np.uint32)


def same_dev(a, b, what):
    assert np.array_equal(a[2], b[2]), (what, "counts")
    for qi in range(len(a[2])):
        n = int(a[2][qi])
        assert np.array_equal(a[1][qi, :n], b[1][qi, :n]) and np.array_equal(bits(a[0][qi, :n]), bits(b[0][qi, :n])), (what, qi)


def test_filtered_tickets(rq):
    """begin_filtered / end = the synchronous filtered call on the small route (1, 64 queries) and the staged one (300); three tickets
    in flight on one index; a NULL filter is the unfiltered _begin; rq_add is refused under a filtered ticket; a filter made before a
    mutation is refused by _begin_filtered."""
    from rabitq_amd import _lib
    from rabitq_amd import index as ix
    L = _lib.lib()
    n, d, k = 20_000, 128, 32
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=71, centre_scale=0.6)
    g = rq.RaBitQ.build(x[:n - 100], centres, synth.random_orthogonal(d, seed=72))
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=73, centre_scale=0.6)
    rng = np.random.default_rng(5)
    f1, f2 = g.make_filter(mask=rng.random(n) < 0.5), g.make_filter(mask=rng.random(n) < 0.1)

    def sync(nq, filt):
        dv = Dev(queries[:nq], 10)
        rq.metrics_reset()
        g.query_batch_device(*dv.args(8), filter=filt)
        return dv.result(), rq.metrics(), ix.last_profile()["small_batch_passes"]

    try:
        for nq, small in ((1, 1), (64, 1), (300, 0)):
            want, mw, passes = sync(nq, f1)
            assert passes == small, nq
            dv = Dev(queries[:nq], 10)
            rq.metrics_reset()
            t = g.query_batch_device_begin(*dv.args(8), filter=f1)
            g.query_batch_device_end(t)
            same_dev(dv.result(), want, ("ticket", nq))
            assert rq.metrics() == mw and ix.last_profile()["small_batch_passes"] == small, nq
        # three in flight: two filters and none
        flights = [(f1, 64), (f2, 40), (None, 64)]
        want = [sync(nq, f)[0] for f, nq in flights]
        dvs = [Dev(queries[:nq], 10) for _, nq in flights]
        tickets = [g.query_batch_device_begin(*dv.args(8), filter=f) for dv, (f, _) in zip(dvs, flights)]
        for t in tickets:
            g.query_batch_device_end(t)
        for dv, w, fl in zip(dvs, want, flights):
            same_dev(dv.result(), w, ("in flight", fl[1]))
        # filter == NULL through the new entry: the existing _begin
        dv, dn = Dev(queries[:64], 10), Dev(queries[:64], 10)
        t = C.c_void_p()
        a = dv.args(8)
        _lib.check(L.rq_query_batch_device_begin_filtered(g._h, None, a[0], a[1], a[2], a[3], a[4], 0, a[5], a[6], a[7], C.byref(t)))
        g.query_batch_device_end(t)
        g.query_batch_device_end(g.query_batch_device_begin(*dn.args(8)))
        same_dev(dv.result(), dn.result(), "NULL filter")
        same_dev(dv.result(), want[2], "NULL filter, against the synchronous call")
        # rq_add under an open filtered ticket
        dv = Dev(queries[:64], 10)
        t = g.query_batch_device_begin(*dv.args(8), filter=f1)
        row, first = np.ascontiguousarray(x[n - 1:n]), C.c_uint32()
        assert L.rq_add(g._h, row.ctypes.data, 1, d, None, 0, C.byref(first)) == -1
        g.query_batch_device_end(t)
        same_dev(dv.result(), want[0], "ticket around a refused rq_add")
        # a filter made before a mutation
        g.add(x[n - 100:])
        t = C.c_void_p()
        a = dv.args(8)
        assert L.rq_query_batch_device_begin_filtered(g._h, f1._h, a[0], a[1], a[2], a[3], a[4], 0, a[5], a[6], a[7], C.byref(t)) == -1
        assert not t.value
        with g.make_filter(mask=rng.random(n) < 0.5) as f3:
            g.query_batch_device_end(g.query_batch_device_begin(*dv.args(8), filter=f3))
    finally:
        f1.close(), f2.close()
        g.close()


def test_small_and_staged_filtered_queries_concurrently(rq):
    """Four threads on one handle: filtered batches of 1 and 64 (small-batch path), an unfiltered query, a filtered batch of 300
    (staged launches); every result as when run alone."""
    n, d, k = 20_000, 128, 32
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=71, centre_scale=0.6)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=72))
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=73, centre_scale=0.6)
    rng = np.random.default_rng(6)
    fa, fb = g.make_filter(mask=rng.random(n) < 0.5), g.make_filter(mask=rng.random(n) < 0.05)
    jobs = [(fa, 1), (fb, 64), (None, 1), (fa, 300)]
    want = [g.query_batch(queries[:nq], 8, 10, filter=f) for f, nq in jobs]
    errors = []

    def worker(t):
        f, nq = jobs[t]
        try:
            for it in range(30):
                got = g.query_batch(queries[:nq], 8, 10, filter=f)
                for u, v in zip(got, want[t]):
                    if not np.array_equal(bits(u), bits(v)):
                        errors.append((t, it))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:5]
    fa.close(), fb.close()
    g.close()
