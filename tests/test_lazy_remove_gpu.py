"""Lazy removal (rq_remove_lazy / rq_compact / rq_pending_removals) on the GPU.  The contract: an index with pending
removals D answers every query entry that has a filtered form as the same index after rq_remove(D) would -- ids in order, distance
bits, counts, status, the rough / precise / query counters -- and rq_compact turns it into that index.  Every case is held against
a twin built from the same arrays with the eager remove of the same ids, and, where the helper exists, against the CPU oracle's
view of sub_arrays(oidx, live mask).  Bit for bit everywhere: no tolerance appears in this file.

Run on the GPU box:  python -m pytest tests/test_lazy_remove_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import scan_cases as sc
from tests import synth
from tests.models import ARRAYS, Live, bits, check_oracle, compare_with_oracle, run_range, same_range, sub_arrays
from tests.test_scan_instantiations_gpu import CONFIGS

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def topk_run(rq, idx, queries, probe, topk, heur=False, **kw):
    rq.metrics_reset()
    out = idx.query_batch(queries, probe, topk, heur, **kw)
    m = rq.metrics()
    return out, (m["rough"], m["precise"], m["query"])


def same_topk(a, b, what="", ids=None):
    """a, b: topk_run results; ids: translation of b's ids."""
    (da, ia, ca), ma = a
    (db, ib, cb), mb = b
    assert np.array_equal(ca, cb), (what, "counts", np.nonzero(ca != cb)[0][:5])
    for qi in range(len(ca)):
        n = int(ca[qi])
        want = ib[qi, :n] if ids is None else ids[ib[qi, :n]]
        assert np.array_equal(ia[qi, :n], want), (what, qi, ia[qi, :n], want)
        assert np.array_equal(bits(da[qi, :n]), bits(db[qi, :n])), (what, qi)
    assert ma == mb, (what, "counters", ma, mb)


def same_arrays(g, c, what=""):
    assert (g.n, g.max_list_len, g.k, g.dim) == (c.n, c.max_list_len, c.k, c.dim), what
    for name in ARRAYS + ("map_ids",):
        assert np.array_equal(bits(getattr(g, name)), bits(getattr(c, name))), (what, name)


def snapshot(g):
    return {name: bits(getattr(g, name)).copy() for name in ARRAYS + ("map_ids",)}, g.n, g.pending_removals


def unchanged(g, snap, what=""):
    arrays, n, pending = snap
    g._refresh()
    assert (g.n, g.pending_removals) == (n, pending), what
    for name, b in arrays.items():
        assert np.array_equal(bits(getattr(g, name)), b), (what, name)


def pair(rq, x, centres, P, dead_ids):
    """-> (the index with dead_ids removed lazily, its twin with them removed eagerly)"""
    lazy, twin = rq.RaBitQ.build(x, centres, P), rq.RaBitQ.build(x, centres, P)
    marked = lazy.remove(ids=dead_ids, lazy=True)
    removed = twin.remove(ids=dead_ids)
    assert marked == removed == lazy.pending_removals == lazy.n - twin.n, (marked, removed, lazy.pending_removals)
    assert lazy.live_n == twin.n
    return lazy, twin


# ---- 1. both scan kernels through the plain entry ---------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("W", [1, 2, 4])
def test_plain_entry_on_both_scan_kernels(rq, oracle, W, impl):
    from rabitq_amd import index as ix
    x, centres, P, queries = sc.make_case(W)
    oidx = oracle.OracleIndex.build(x, centres, P)
    masks = sc.make_filters(oidx.map_ids, oidx.offsets)
    try:
        ix.set_option("scan_impl", impl)
        ix.set_option("scan_gate", 1)
        for name, live in masks.items():
            lazy, twin = pair(rq, x, centres, P, np.nonzero(~live)[0])
            try:
                for probe, topk, heur in CONFIGS:
                    what = (W, impl, name, probe, topk, heur)
                    got = topk_run(rq, lazy, queries, probe or lazy.k, topk, heur)
                    pr = ix.last_profile()
                    same_topk(got, topk_run(rq, twin, queries, probe or twin.k, topk, heur), what)
                    assert pr["small_batch_passes"] == 0 and pr["scan_launches"] > 0, (what, pr)
                    assert (pr["matrix_launches"] > 0) if impl == 2 else (pr["matrix_launches"] == 0), (what, pr)
                    compare_with_oracle(rq, oracle, oidx, lazy, queries, probe or lazy.k, topk, heur, filter=(None, live))
            finally:
                lazy.close()
                twin.close()
    finally:
        ix.set_option("scan_impl", 0)
        ix.set_option("scan_gate", 0)
        oidx.close()


# ---- 2. small batches -------------------------------------------------------------------------------------------------------
def test_small_batches(rq, oracle):
    from rabitq_amd import index as ix
    n, d, k = 8000, 128, 20
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=101, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=102)
    queries, _, _ = synth.mixture(64, d, k, sigma=0.8, seed=103, centre_scale=0.6)
    live = np.random.default_rng(104).random(n) >= 0.05
    lazy, twin = pair(rq, x, centres, P, np.nonzero(~live)[0])
    oidx = oracle.OracleIndex.build(x, centres, P)
    try:
        for nq in (1, 40, 64):
            for heur in (False, True):
                got = topk_run(rq, lazy, queries[:nq], 8, 10, heur)
                pr = ix.last_profile()
                same_topk(got, topk_run(rq, twin, queries[:nq], 8, 10, heur), (nq, heur))
                assert pr["small_batch_passes"] >= 1, (nq, heur, pr)
            compare_with_oracle(rq, oracle, oidx, lazy, queries[:nq], 8, 10, False, filter=(None, live))
    finally:
        oidx.close()
        lazy.close()
        twin.close()


# ---- 3. accumulation, compaction ----------------------------------------------------------------------------------------------
def test_accumulation_and_compact(rq, tmp_path):
    n, d, k = 5000, 64, 12
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=111, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=112)
    queries, _, _ = synth.mixture(200, d, k, sigma=0.8, seed=113, centre_scale=0.6)
    lazy, twin = rq.RaBitQ.build(x, centres, P), rq.RaBitQ.build(x, centres, P)
    first = np.concatenate([np.arange(0, n, 3), np.arange(n + 50, n + 90)])           # with ids the index never held
    second = np.concatenate([np.arange(0, n, 2), np.array([n, 7 * n, (1 << 32) - 1])])
    assert lazy.pending_removals == 0 and lazy.live_n == n
    m1 = lazy.remove(ids=first, lazy=True)
    assert m1 == len(np.arange(0, n, 3)) == lazy.pending_removals
    allowed = np.random.default_rng(114).random(n) < 0.5
    f = lazy.make_filter(mask=allowed)
    assert lazy.remove(ids=np.arange(0, n, 6), lazy=True) == 0                          # all dead already: nothing changes ...
    assert lazy.remove(ids=np.arange(n, n + 10), lazy=True) == 0
    assert lazy.pending_removals == m1
    lazy.query_batch(queries[:70], k, 10, filter=f)                                     # ... and the earlier filter stays valid
    f.close()
    m2 = lazy.remove(ids=second, lazy=True)
    union = np.union1d(np.arange(0, n, 3), np.arange(0, n, 2))
    assert m2 == union.size - m1 and lazy.pending_removals == m1 + m2 == union.size
    assert lazy.n == n and lazy.live_n == n - union.size
    assert twin.remove(ids=union) == union.size
    for probe, topk, heur, nq in ((k, 10, False, 200), (4, 100, False, 200), (3, 10, True, 200), (k, 10, False, 30)):
        same_topk(topk_run(rq, lazy, queries[:nq], probe, topk, heur), topk_run(rq, twin, queries[:nq], probe, topk, heur),
                  (probe, topk, heur, nq))
    before = lazy.make_filter(mask=allowed)
    assert lazy.compact() == union.size
    assert lazy.pending_removals == 0 and lazy.live_n == lazy.n == twin.n
    with pytest.raises(rq._lib.RabitqError) as e:                                       # the relayout bumped the generation
        lazy.query_batch(queries[:4], k, 10, filter=before)
    assert e.value.status == INVALID
    before.close()
    same_arrays(lazy, twin, "compacted")
    st = rq.index.last_mutate_stats()
    assert st["rows_before"] == n and st["rows_after"] == twin.n and st["gather_bytes"] > 0
    lazy.dump_to_dir(tmp_path / "lazy")
    twin.dump_to_dir(tmp_path / "twin")
    names = sorted(os.listdir(tmp_path / "twin"))
    assert names == sorted(os.listdir(tmp_path / "lazy"))
    for name in names:
        assert (tmp_path / "lazy" / name).read_bytes() == (tmp_path / "twin" / name).read_bytes(), name
    after = lazy.make_filter(mask=allowed)
    assert lazy.compact() == 0                                                          # nothing pending: the generation stays
    same_topk(topk_run(rq, lazy, queries, k, 10, filter=after), topk_run(rq, twin, queries, k, 10, filter=twin.make_filter(mask=allowed)))
    after.close()
    same_topk(topk_run(rq, lazy, queries, k, 10), topk_run(rq, twin, queries, k, 10), "after compact")
    lazy.close()
    twin.close()


# ---- 4. caller's filters ------------------------------------------------------------------------------------------------------
def test_callers_filters(rq, oracle):
    n, d, k = 6000, 64, 10
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=121, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=122)
    queries, _, _ = synth.mixture(150, d, k, sigma=0.8, seed=123, centre_scale=0.6)
    rng = np.random.default_rng(124)
    live = rng.random(n) >= 0.3
    allowed = rng.random(n) < 0.4
    lazy, twin = pair(rq, x, centres, P, np.nonzero(~live)[0])
    oidx = oracle.OracleIndex.build(x, centres, P)
    stale = lazy.make_filter(mask=allowed)
    fl, ft = lazy.make_filter(mask=allowed), twin.make_filter(mask=allowed)
    try:
        assert fl.rows == ft.rows == int((allowed & live).sum())
        for nq, probe, topk, heur in ((150, k, 10, False), (150, 3, 10, True), (20, k, 10, False)):
            same_topk(topk_run(rq, lazy, queries[:nq], probe, topk, heur, filter=fl),
                      topk_run(rq, twin, queries[:nq], probe, topk, heur, filter=ft), (nq, probe, topk, heur))
        compare_with_oracle(rq, oracle, oidx, lazy, queries, k, 10, False, filter=(fl, allowed & live))
        more = np.nonzero(live)[0][:100]
        assert lazy.remove(ids=more, lazy=True) == 100 and twin.remove(ids=more) == 100
        live[more] = False
        for entry in (lambda: lazy.query_batch(queries[:8], k, 10, filter=stale), lambda: lazy.range_search(queries[:8], k, 1.0, filter=stale),
                      lambda: lazy.exact_search(queries[:8], 10, filter=stale)):
            with pytest.raises(rq._lib.RabitqError) as e:
                entry()
            assert e.value.status == INVALID and "rq_remove_lazy" in str(e.value), e.value
        with lazy.make_filter(mask=allowed) as f2, twin.make_filter(mask=allowed) as t2:
            assert f2.rows == t2.rows == int((allowed & live).sum())
            same_topk(topk_run(rq, lazy, queries, k, 10, filter=f2), topk_run(rq, twin, queries, k, 10, filter=t2), "fresh filter")
    finally:
        for f in (stale, fl, ft):
            f.close()
        oidx.close()
        lazy.close()
        twin.close()


# ---- 5. every entry that has a filtered form, with filter=None ------------------------------------------------------------------
def device_topk(idx, queries, probe, topk, ticket):
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).cuda()
    nq, L = qd.shape
    od = torch.empty((nq, topk), device="cuda", dtype=torch.float32)
    oi = torch.empty((nq, topk), device="cuda", dtype=torch.int32)
    on = torch.empty((nq,), device="cuda", dtype=torch.int32)
    if ticket:
        t = idx.query_batch_device_begin(qd.data_ptr(), nq, L, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        idx.query_batch_device_end(t)
    else:
        idx.query_batch_device(qd.data_ptr(), nq, L, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
    torch.cuda.synchronize()
    return od.cpu().numpy(), oi.cpu().numpy().view(np.uint32), on.cpu().numpy().view(np.uint32)


def test_every_filtered_form_entry(rq):
    n, d, k = 6000, 64, 12
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=131, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=132)
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=133, centre_scale=0.6)
    live = np.random.default_rng(134).random(n) >= 0.25
    lazy, twin = pair(rq, x, centres, P, np.nonzero(~live)[0])
    try:
        radii = np.sort(((x[live][None, :400] - queries[:, None, :]) ** 2).sum(axis=2), axis=1)[:, 15].astype(np.float32)
        (got, mg, _), (want, mw, _) = run_range(rq, lazy, queries, 6, radii), run_range(rq, twin, queries, 6, radii)
        same_range(got, want, "range_search")
        assert (mg["rough"], mg["precise"], mg["query"]) == (mw["rough"], mw["precise"], mw["query"])
        for a, b in zip(lazy.exact_search(queries, 10), twin.exact_search(queries, 10)):
            assert np.array_equal(bits(a), bits(b)), "exact_search"
        same_range(lazy.exact_range_search(queries, radii), twin.exact_range_search(queries, radii), "exact_range_search")
        for nq in (300, 24):
            ga, ta = lazy.query_batch_adaptive(queries[:nq], 8, 10, ratio=1.6), twin.query_batch_adaptive(queries[:nq], 8, 10, ratio=1.6)
            assert np.array_equal(ga[3], ta[3]) and np.array_equal(ga[2], ta[2]), ("adaptive", nq)
            for qi in range(nq):
                m = int(ga[2][qi])
                assert np.array_equal(ga[1][qi, :m], ta[1][qi, :m]) and np.array_equal(bits(ga[0][qi, :m]), bits(ta[0][qi, :m])), ("adaptive", nq, qi)
        for ticket in (False, True):
            for nq in (300, 16):
                (da, ia, na), (db, ib, nb) = device_topk(lazy, queries[:nq], 6, 10, ticket), device_topk(twin, queries[:nq], 6, 10, ticket)
                assert np.array_equal(na, nb), ("device", ticket, nq)
                for qi in range(nq):
                    m = int(na[qi])
                    assert np.array_equal(ia[qi, :m], ib[qi, :m]) and np.array_equal(bits(da[qi, :m]), bits(db[qi, :m])), ("device", ticket, nq, qi)
        for q in queries[:5]:
            for heur in (False, True):
                a, b = lazy.query(q, 6, 10, heur), twin.query(q, 6, 10, heur)
                assert [(np.float32(dd).tobytes(), i) for dd, i in a] == [(np.float32(dd).tobytes(), i) for dd, i in b]
        # the entries that read no row answer as before
        assert np.array_equal(lazy.probe_counts(queries[:50], 8, 1.6), twin.probe_counts(queries[:50], 8, 1.6))
    finally:
        lazy.close()
        twin.close()


def test_call_of_several_passes(rq):
    """More than 65 536 queries (test_filtered_call_of_several_passes' shape): every pass runs under the live filter."""
    n, d, k = 20000, 64, 32
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=51, centre_scale=0.6)
    queries, _, _ = synth.mixture(70000, d, k, sigma=0.8, seed=53, centre_scale=0.6)
    live = np.random.default_rng(3).random(n) < 0.3
    lazy, twin = pair(rq, x, centres, synth.random_orthogonal(d, seed=52), np.nonzero(~live)[0])
    try:
        same_topk(topk_run(rq, lazy, queries, 6, 10), topk_run(rq, twin, queries, 6, 10), "passes")
    finally:
        lazy.close()
        twin.close()


# ---- 6. mutation on top -------------------------------------------------------------------------------------------------------
def test_mutation_on_top(rq):
    n, d, k = 4000, 64, 10
    x, centres, _ = synth.mixture(n + 600, d, k, sigma=0.8, seed=141, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=142)
    queries, _, _ = synth.mixture(120, d, k, sigma=0.8, seed=143, centre_scale=0.6)
    dead = np.arange(5, n, 4)                                                  # (n - 1 = 3999 is not dead: the next id is n on both)
    new = x[n:]

    def fresh():
        return pair(rq, x[:n], centres, P, dead)

    def same(lazy, twin, what):
        assert lazy.pending_removals == 0, what
        same_arrays(lazy, twin, what)
        same_topk(topk_run(rq, lazy, queries, k, 10), topk_run(rq, twin, queries, k, 10), what)

    lazy, twin = fresh()                                                        # add, default ids
    got = lazy.add(new[:300])
    st = rq.index.last_mutate_stats()                                          # the compaction's relayout and the add's, added up
    assert np.array_equal(got, twin.add(new[:300]))
    assert st["rows_before"] == n and st["rows_after"] == twin.n and st["gather_bytes"] > rq.index.last_mutate_stats()["gather_bytes"]
    same(lazy, twin, "add")
    lazy.close(), twin.close()
    lazy, twin = fresh()                                                        # add with explicit ids, some dead but still stored
    ids = np.concatenate([dead[:200], np.arange(n + 10, n + 110)]).astype(np.uint32)
    assert np.array_equal(lazy.add(new[:300], ids), twin.add(new[:300], ids))
    same(lazy, twin, "add explicit")
    lazy.close(), twin.close()
    lazy, twin = fresh()                                                        # an id that is still live is refused, nothing is lost
    with pytest.raises(rq._lib.RabitqError) as e:
        lazy.add(new[:2], np.array([0, 5], dtype=np.uint32))
    assert e.value.status == INVALID
    lazy._refresh()
    assert lazy.live_n == twin.n
    same_topk(topk_run(rq, lazy, queries, k, 10), topk_run(rq, twin, queries, k, 10), "refused add")
    lazy.close(), twin.close()
    lazy, twin = fresh()                                                        # eager remove on a pending index
    more = np.arange(0, n, 7)
    assert lazy.remove(ids=more) == twin.remove(ids=more)
    same(lazy, twin, "eager remove")
    lazy.close(), twin.close()
    lazy, twin = fresh()                                                        # lazy update
    upd = np.concatenate([np.arange(0, 400, 4), np.arange(n + 5, n + 25)]).astype(np.uint32)
    lazy.update(upd, new[:upd.size], lazy=True)
    twin.update(upd, new[:upd.size])
    same(lazy, twin, "update")
    lazy.close(), twin.close()
    lazy, twin = fresh()                                                        # extract / copy: keep = requested AND live
    snap = snapshot(lazy)
    want = np.random.default_rng(144).random(n) < 0.5
    for a, b, what in ((lazy.extract(mask=want), twin.extract(mask=want), "extract"), (lazy.copy(), twin.copy(), "copy")):
        same(a, b, what)
        a.close(), b.close()
    unchanged(lazy, snap, "extract / copy")
    other = rq.RaBitQ.build(new, centres, P)                                    # merge_from with a pending dst
    assert lazy.merge_from(other, "append") == twin.merge_from(other, "append")
    same(lazy, twin, "merge_from, pending dst")
    lazy.close(), twin.close()
    lazy, twin = fresh()                                                        # merge_from with a pending src
    dst = rq.RaBitQ.build(new, centres, P)
    s_lazy, s_dst = snapshot(lazy), snapshot(dst)
    with pytest.raises(rq._lib.RabitqError) as e:
        dst.merge_from(lazy, "append")
    assert e.value.status == UNSUPPORTED
    unchanged(lazy, s_lazy, "pending src")
    unchanged(dst, s_dst, "dst of a pending src")
    same_topk(topk_run(rq, lazy, queries, k, 10), topk_run(rq, twin, queries, k, 10), "pending src")
    for g in (lazy, twin, dst, other):
        g.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(rq, tmp_path):
    import torch
    n, d, k = 3000, 64, 8
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=151, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=152)
    queries, _, _ = synth.mixture(100, d, k, sigma=0.8, seed=153, centre_scale=0.6)
    lazy, twin = pair(rq, x, centres, P, np.arange(0, n, 5))
    snap = snapshot(lazy)
    want = topk_run(rq, lazy, queries, k, 10)
    qd = torch.from_numpy(queries).cuda()
    pc = torch.zeros((100, 4), dtype=torch.int32, device="cuda")
    pd = torch.zeros((100, 4), dtype=torch.float32, device="cuda")
    thr = torch.full((100,), float(np.finfo(np.float32).max), dtype=torch.float32, device="cuda")
    od = torch.empty((100, 10), device="cuda", dtype=torch.float32)
    oi = torch.empty((100, 10), device="cuda", dtype=torch.int32)
    on = torch.empty((100,), device="cuda", dtype=torch.int32)
    lazy.coarse_topk_device(qd.data_ptr(), 100, d, 0, k, 4, pc.data_ptr(), pd.data_ptr())      # (reads no row: accepted)
    owner, _ = lazy.partition_lists(2)
    refused = {
        "dump_to_dir": lambda: lazy.dump_to_dir(tmp_path / "dump"),
        "dump_to_json": lambda: lazy.dump_to_json(tmp_path / "dump.json"),
        "shard": lambda: lazy.shard(owner, 0),
        "probed": lambda: lazy.query_batch_device_probed(qd.data_ptr(), 100, d, pc.data_ptr(), pd.data_ptr(), 4, 10, od.data_ptr(), oi.data_ptr(),
                                                         on.data_ptr()),
        "seeded": lambda: lazy.query_batch_device_seeded(qd.data_ptr(), 100, d, pc.data_ptr(), pd.data_ptr(), 4, 10, thr.data_ptr(), od.data_ptr(),
                                                         oi.data_ptr(), on.data_ptr()),
    }
    for name, call in refused.items():
        with pytest.raises(rq._lib.RabitqError) as e:
            call()
        assert e.value.status == UNSUPPORTED and "rq_compact" in str(e.value), (name, e.value)
        unchanged(lazy, snap, name)
    assert not os.path.exists(tmp_path / "dump.json")
    t = lazy.query_batch_device_begin(qd.data_ptr(), 100, d, k, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr())
    try:
        with pytest.raises(rq._lib.RabitqError) as e:                            # an open ticket
            lazy.remove(ids=np.array([1, 2, 3]), lazy=True)
        assert e.value.status == INVALID
    finally:
        lazy.query_batch_device_end(t)
    unchanged(lazy, snap, "open ticket")
    same_topk(topk_run(rq, lazy, queries, k, 10), want, "after the refusals")
    same_topk(want, topk_run(rq, twin, queries, k, 10), "twin")
    lazy.close()
    shard = twin.shard(twin.partition_lists(2)[0], 0)                            # a shard refuses lazy removal
    s = snapshot(shard)
    with pytest.raises(rq._lib.RabitqError) as e:
        shard.remove(ids=np.array([1, 2, 3]), lazy=True)
    assert e.value.status == UNSUPPORTED
    unchanged(shard, s, "shard")
    shard.close()
    twin.close()


# ---- 8. everything dead -------------------------------------------------------------------------------------------------------
def test_everything_dead(rq):
    from rabitq_amd import _lib
    n, d, k = 5000, 64, 10
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=11, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=12)
    g = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=13, centre_scale=0.6)
    assert g.remove(mask=np.ones(n, dtype=bool), lazy=True) == n
    assert g.pending_removals == n and g.live_n == 0 and g.n == n
    for nq in (300, 3):
        rq.metrics_reset()
        _, _, cnt = g.query_batch(queries[:nq], k, 10)
        assert not cnt.any()
        m = rq.metrics()
        assert (m["rough"], m["precise"], m["query"]) == (0, 0, nq)
    with pytest.raises(_lib.RabitqError) as e:
        g.query(queries[0], k, 10, heuristic_rank=True)
    assert e.value.status == _lib.RQ_ERR_EMPTY
    assert g.query(queries[0], k, 10) == []
    assert not g.query_batch_adaptive(queries[:50], k, 10, ratio=1.6)[2].any()
    assert not device_topk(g, queries[:50], k, 10, True)[2].any() and not device_topk(g, queries[:50], k, 10, False)[2].any()
    assert int(g.range_search(queries[:50], k, 1e9)[0][-1]) == 0
    assert not g.exact_search(queries[:50], 10)[2].any()
    assert int(g.exact_range_search(queries[:50], 1e9)[0][-1]) == 0
    with g.make_filter(mask=np.ones(n, dtype=bool)) as f:
        assert f.rows == 0
    assert g.compact() == n
    assert (g.n, g.pending_removals, g.max_list_len) == (0, 0, 0)
    assert np.array_equal(g.add(x[:500]), np.arange(500, dtype=np.uint32))
    c = rq.RaBitQ.build(x[:500], centres, P)
    same_arrays(g, c, "added to the emptied index")
    same_topk(topk_run(rq, g, queries, k, 10), topk_run(rq, c, queries, k, 10))
    g.close()
    c.close()


# ---- 9. indexes that cannot relayout ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f16", "tiered", "split_rows"])
def test_indexes_that_cannot_relayout(rq, kind):
    from rabitq_amd import index as ix
    rng = np.random.default_rng(161)
    rows = None
    if kind in ("u8", "f16"):
        n, d, k = 2000, 64, 8
        xf, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=162, centre_scale=0.6)
        if kind == "u8":
            x = np.clip(np.rint(xf * 40.0 + 128.0), 0, 255).astype(np.uint8)
            centres = (centres * 40.0 + 128.0).astype(np.float32)
            queries = (synth.mixture(100, d, k, sigma=0.8, seed=163, centre_scale=0.6)[0] * 40.0 + 128.0).astype(np.float32)
            rows = "u8"
        else:
            x = xf.astype(np.float16)
            queries = synth.mixture(100, d, k, sigma=0.8, seed=163, centre_scale=0.6)[0]
    else:
        n, d, k = 12000, 128, 24
        x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=61, centre_scale=0.6)
        queries, _, _ = synth.mixture(400, d, k, sigma=0.8, seed=63, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=164)
    if kind == "tiered":
        ix.set_option("base_device_mb", 1)
    elif kind == "split_rows":
        ix.set_option("split_rows", 2)
    try:
        g = rq.RaBitQ.build(x, centres, P, rows=rows)
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)
    if kind == "tiered":
        assert g.n_hbm < n
    elif kind == "split_rows":
        assert g.split_rows
    else:
        assert g.row_type == kind
    with pytest.raises(rq._lib.RabitqError) as e:                                # the eager removal is refused on these indexes
        g.remove(ids=np.array([1]))
    assert e.value.status == UNSUPPORTED
    live = rng.random(n) >= 0.4
    dead = np.nonzero(~live)[0]
    assert g.remove(ids=dead[: dead.size // 2], lazy=True) == dead.size // 2
    assert g.remove(ids=dead, lazy=True) == dead.size - dead.size // 2
    assert g.pending_removals == dead.size and g.live_n == int(live.sum())
    ids = np.nonzero(live)[0].astype(np.uint32)
    c = rq.RaBitQ.build(x[live], centres, P, rows=rows)                         # a fresh build of the live rows, ids translated
    try:
        for nq, probe, heur in ((len(queries), 8, False), (len(queries), 8, True), (16, 8, False)):
            same_topk(topk_run(rq, g, queries[:nq], probe, 10, heur), topk_run(rq, c, queries[:nq], probe, 10, heur), (kind, nq, heur), ids=ids)
        snap = snapshot(g) if kind not in ("tiered", "split_rows") else None
        with pytest.raises(rq._lib.RabitqError) as e:
            g.compact()
        assert e.value.status == UNSUPPORTED
        g._refresh()
        assert g.pending_removals == dead.size and g.n == n
        if snap:
            unchanged(g, snap, kind)
        same_topk(topk_run(rq, g, queries, 8, 10), topk_run(rq, c, queries, 8, 10), (kind, "after the refused compact"), ids=ids)
    finally:
        g.close()
        c.close()


# ---- 10. a seeded sequence ----------------------------------------------------------------------------------------------------
def test_seeded_sequence(rq, oracle):
    n0, d, k = 3000, 64, 10
    x, centres, _ = synth.mixture(n0 + 12 * 150, d, k, sigma=0.8, seed=171, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=172)
    queries, _, _ = synth.mixture(70, d, k, sigma=0.8, seed=173, centre_scale=0.6)
    rng = np.random.default_rng(174)
    g = rq.RaBitQ.build(x[:n0], centres, P)
    live = Live(np.arange(n0), x[:n0])
    next_row, ops = n0, []

    def check_queries(what):
        ids, rows = live.sorted()
        o = oracle.OracleIndex.build(rows, centres, P)
        try:
            compare_with_oracle(rq, oracle, o, g, queries, k, 10, False, ids=ids)
            compare_with_oracle(rq, oracle, o, g, queries[:20], 4, 10, False, ids=ids)
        finally:
            o.close()
        assert g.live_n == len(live.rows), what

    try:
        for step in range(12):
            op = ("lazy", "lazy", "eager", "add", "compact", "swap")[int(rng.integers(0, 6))] if step else "lazy"
            ops.append(op)
            held = np.array(sorted(live.rows), dtype=np.int64)
            relayout = op != "lazy"
            if op in ("lazy", "eager"):
                pick = np.concatenate([rng.choice(held, size=min(120, held.size), replace=False), rng.integers(0, 6000, size=30)])
                want = int(np.isin(np.unique(pick), held).sum())
                pending = g.pending_removals
                assert g.remove(ids=pick, lazy=(op == "lazy")) == want, (step, op)
                live.remove(pick)
                assert g.pending_removals == (pending + want if op == "lazy" else 0), (step, op)
            elif op == "add":
                rows = x[next_row:next_row + 150]
                next_row += 150
                reuse = np.array([i for i in range(0, 6000, 37) if i not in live.rows][:20], dtype=np.uint32)   # dead or never held
                if step % 2 and reuse.size:
                    ids = np.concatenate([reuse, np.arange(100000 + step * 1000, 100000 + step * 1000 + 150 - reuse.size)]).astype(np.uint32)
                    got = g.add(rows, ids)
                else:
                    got = g.add(rows)
                live.add(got, rows)
            elif op == "compact":
                pending = g.pending_removals
                assert pending == g.n - len(live.rows), (step, ops)
                assert g.compact() == pending, (step, ops)
            else:                                                              # extract nine in ten of the live rows and go on with the extract
                keep = held[rng.random(held.size) < 0.9]
                h = g.extract(ids=keep)
                live.remove(np.setdiff1d(held, keep))
                g.close()
                g = h
            if relayout:
                assert g.pending_removals == 0, (step, ops)
                check_oracle(oracle, g, live, centres, P, (step, ops))
            check_queries((step, ops))
    finally:
        print("operations:", ops)
        g.close()
