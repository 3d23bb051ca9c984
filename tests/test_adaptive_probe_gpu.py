"""Adaptive probing (rq_probe_rule_t, rq_query_batch*_adaptive, rq_probe_counts_device): a query cut to n lists returns exactly what
the same entry returns with probe = n -- ids, distance bits, counts and the rough / precise counters -- and n is what the rule
(tests/adaptive_model.py, its only statement here) derives from the CPU oracle's coarse distances.

Worlds (tests/adaptive_model.py; tests/test_adaptive_model.py shows on the CPU that the rules cut them unevenly):
    d128   20 000 x 128,   64 lists, probe 32        d100   5 000 x 100, 16 lists, probe 16 (generic quantisation kernel, padded queries)
    k1024  30 000 x  64, 1024 lists, probe 64        d768   4 000 x 768, 64 lists, probe 24
A plain call of <= 64 queries takes the few-launch path and an adaptive call never does, so the identity of small groups also sets
the two paths against each other.

Run on the GPU box:  python -m pytest tests/test_adaptive_probe_gpu.py -m gpu -q
"""
import ctypes as C

import numpy as np
import pytest

from tests import adaptive_model as am
from tests import synth
from tests.models import bits

pytestmark = pytest.mark.gpu

INF = float("inf")
_worlds = {}


@pytest.fixture(scope="module")
def rq():
    import os
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def get_world(rq, oracle, name):
    """The world's GPU index, oracle index, queries (2048: the first 600 are the model test's), the oracle's coarse distances of the
    first 600 -- built once, never changed."""
    if name not in _worlds:
        x, centres, P, q, w = am.world(name, nq=2048)
        g = rq.RaBitQ.build(x, centres, P)
        o = oracle.OracleIndex.build(x, centres, P)
        _, dist = am.oracle_coarse(o, q[:600], w["probe"])
        _worlds[name] = dict(g=g, o=o, q=q, w=w, dist=dist, m=min(w["probe"], w["k"]))
    return _worlds[name]


def u32(dist):
    """the bit patterns of an array of f32 distances, same shape"""
    return np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32)


def same_rows(a, b, what):
    """(dist, ids, counts) of two calls over the same queries: counts, and every row up to its count, byte for byte."""
    assert np.array_equal(a[2], b[2]), (what, "counts", np.nonzero(a[2] != b[2])[0][:5])
    live = np.arange(a[1].shape[1])[None, :] < np.asarray(a[2], dtype=np.int64)[:, None]
    assert np.array_equal(a[1][live], b[1][live]), (what, "ids", np.nonzero(((a[1] != b[1]) & live).any(axis=1))[0][:5])
    da, db = u32(a[0]), u32(b[0])
    assert np.array_equal(da[live], db[live]), (what, "dist", np.nonzero(((da != db) & live).any(axis=1))[0][:5])


def counters(rq):
    m = rq.metrics()
    return m["rough"], m["precise"], m["query"]


def check_identity(rq, g, queries, probe, topk, heur, what, filt=None, **rule):
    """One adaptive call; its nprobe output split into groups of equal n; every group against the plain (or filtered) entry with
    probe = n.  The counters of the adaptive call equal the sum over the groups.  -> nprobe."""
    rq.metrics_reset()
    d, ids, cnt, npr = g.query_batch_adaptive(queries, probe, topk, heuristic_rank=heur, filter=filt, **rule)
    got = counters(rq)
    assert npr.min() >= 1 and npr.max() <= min(probe, g.k), (what, npr.min(), npr.max())
    rq.metrics_reset()
    for n in np.unique(npr):
        sel = np.nonzero(npr == n)[0]
        want = g.query_batch(queries[sel], int(n), topk, heur, filter=filt)
        same_rows((d[sel], ids[sel], cnt[sel]), want, (what, "n", int(n), "queries", sel[:4]))
    assert got == counters(rq), (what, got, counters(rq))
    return npr


# ---- counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(am.WORLDS))
def test_counts_equal_the_model_on_the_oracles_distances(rq, oracle, name):
    """probe_counts (the cut kernel behind the staged and the wave selection; behind the pre-filtered ranking for 2048 queries)
    against the model fed with the oracle's coarse distances, with and without caps."""
    wd = get_world(rq, oracle, name)
    g, q, w, dist, m = wd["g"], wd["q"], wd["w"], wd["dist"], wd["m"]
    caps = np.random.default_rng(5).integers(0, m + 3, size=600).astype(np.uint32)      # 0 and > m: clamped
    for ratio, min_probe in w["rules"] + ((INF, 1), (1.0, 1), (0.0, 4)):
        want = am.probe_counts(dist, ratio, min_probe)
        assert np.array_equal(g.probe_counts(q[:600], w["probe"], ratio, min_probe), want), (name, ratio, min_probe)
        assert np.array_equal(g.probe_counts(q[:600], w["probe"], ratio, min_probe, caps), am.probe_counts(dist, ratio, min_probe, caps))
        # the same rows inside a batch that takes the pre-filtered coarse ranking (>= 2048 queries, >= 64 lists): its rows' distances
        # are the exact ones too
        assert np.array_equal(g.probe_counts(q, w["probe"], ratio, min_probe)[:600], want), (name, ratio, min_probe, "2048")
    assert np.array_equal(g.probe_counts(q[:1], w["probe"], w["rules"][0][0]), am.probe_counts(dist[:1], w["rules"][0][0]))
    # probe beyond the number of lists: m = k columns
    if w["k"] <= 64:
        _, dk = am.oracle_coarse(wd["o"], q[:50], 10 * w["k"])
        assert np.array_equal(g.probe_counts(q[:50], 10 * w["k"], 1.8), am.probe_counts(dk, 1.8))


# ---- identity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(am.WORLDS))
def test_identity_with_the_plain_entry(rq, oracle, name):
    """Batches of 1, 70, 300 and 2048 queries (staged small form, large form, pre-filtered coarse ranking), both rankers, topk 1 /
    10 / 100; the adaptive call's nprobe equals probe_counts'."""
    wd = get_world(rq, oracle, name)
    g, q, w = wd["g"], wd["q"], wd["w"]
    (ratio, min_probe), (ratio2, min_probe2) = w["rules"]
    for nq, topk, heur in ((1, 10, False), (70, 10, False), (70, 10, True), (300, 10, False), (300, 10, True), (300, 1, False),
                           (300, 1, True), (300, 100, False), (300, 100, True), (2048, 10, False), (2048, 10, True)):
        npr = check_identity(rq, g, q[:nq], w["probe"], topk, heur, (name, nq, topk, heur), ratio=ratio, min_probe=min_probe)
        assert np.array_equal(npr, g.probe_counts(q[:nq], w["probe"], ratio, min_probe)), (name, nq)
        if nq == 300:
            assert len(np.unique(npr)) >= 4 and npr.min() == min_probe and npr.max() == wd["m"]
    check_identity(rq, g, q[:300], w["probe"], 10, False, (name, "second rule"), ratio=ratio2, min_probe=min_probe2)


def test_many_passes_equal_chunks(rq, oracle):
    """70 000 queries in one call (more than 65 536: several passes, two in flight) against the same queries in chunks of 5 000."""
    wd = get_world(rq, oracle, "d128")
    g, w = wd["g"], wd["w"]
    rng = np.random.default_rng(9)
    q = wd["q"][rng.integers(0, 2048, size=70_000)] + 0.02 * rng.standard_normal((70_000, w["d"])).astype(np.float32)
    ratio, min_probe = w["rules"][0]
    caps = rng.integers(1, w["probe"] + 1, size=70_000).astype(np.uint32)
    for heur, mp in ((False, None), (True, caps)):
        rq.metrics_reset()
        whole = g.query_batch_adaptive(q, w["probe"], 10, ratio, min_probe, mp, heur)
        got = counters(rq)
        rq.metrics_reset()
        for i0 in range(0, 70_000, 5_000):
            s = slice(i0, i0 + 5_000)
            part = g.query_batch_adaptive(q[s], w["probe"], 10, ratio, min_probe, None if mp is None else mp[s], heur)
            same_rows([a[s] for a in whole[:3]], part[:3], ("chunk", i0, heur))
            assert np.array_equal(whole[3][s], part[3]), ("nprobe", i0)
        assert got == counters(rq)
        assert len(np.unique(whole[3])) >= 4
    # the last chunk once more against the plain entry: the passes behind the first one cut their own rows
    s = slice(65_536, 70_000)
    for n in np.unique(whole[3][s])[:6]:
        sel = np.nonzero(whole[3][s] == n)[0] + 65_536
        same_rows([a[sel] for a in whole[:3]], g.query_batch(q[sel], int(n), 10, True), ("tail", int(n)))


# ---- oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(am.WORLDS))
def test_oracle_with_the_cut_probe(rq, oracle, name):
    """200 queries: every row equals oracle.query(q, n_i, topk), the rq_metrics deltas equal the oracle's sums."""
    wd = get_world(rq, oracle, name)
    g, o, q, w = wd["g"], wd["o"], wd["q"][:200], wd["w"]
    ratio, min_probe = w["rules"][0]
    want_n = am.probe_counts(wd["dist"][:200], ratio, min_probe)
    for heur in (False, True):
        rq.metrics_reset()
        d, ids, cnt, npr = g.query_batch_adaptive(q, w["probe"], 10, ratio, min_probe, None, heur)
        got = counters(rq)
        assert np.array_equal(npr, want_n)
        tot_r = tot_p = 0
        for b in range(200):
            oracle.metrics_reset()
            od, oi = o.query(q[b], int(npr[b]), 10, heur)
            om = oracle.metrics()
            tot_r, tot_p = tot_r + om["rough"], tot_p + om["precise"]
            n = int(cnt[b])
            assert n == oi.size and np.array_equal(ids[b, :n], oi), (name, heur, b, int(npr[b]))
            assert np.array_equal(bits(d[b, :n]), bits(od)), (name, heur, b)
        assert got == (tot_r, tot_p, 200), (name, heur, got, tot_r, tot_p)


# ---- no cut, caps, NaN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d128", "k1024"])
def test_no_cut_equals_the_plain_call(rq, oracle, name):
    wd = get_world(rq, oracle, name)
    g, q, w = wd["g"], wd["q"], wd["w"]
    for nq, heur, rule in ((40, False, dict(ratio=INF)), (300, False, dict(ratio=INF)), (300, True, dict(ratio=INF)),
                           (2048, False, dict(ratio=INF)), (300, False, dict(ratio=1.0, min_probe=wd["m"])),
                           (300, False, dict(ratio=0.0, min_probe=10_000))):
        rq.metrics_reset()
        a = g.query_batch_adaptive(q[:nq], w["probe"], 10, heuristic_rank=heur, **rule)
        ma = counters(rq)
        rq.metrics_reset()
        b = g.query_batch(q[:nq], w["probe"], 10, heur)
        same_rows(a[:3], b, (name, nq, heur, rule))
        assert ma == counters(rq)
        assert (a[3] == wd["m"]).all()


def test_caps_and_nan(rq, oracle):
    wd = get_world(rq, oracle, "d128")
    g, w, m, dist = wd["g"], wd["w"], wd["m"], wd["dist"]
    q = wd["q"][:300].copy()
    rng = np.random.default_rng(12)
    caps = rng.integers(1, m + 1, size=300).astype(np.uint32)
    npr = check_identity(rq, g, q, w["probe"], 10, False, "caps alone", ratio=INF, max_probe=caps)
    assert np.array_equal(npr, caps)                                               # per-query nprobe
    ratio, _ = w["rules"][0]
    npr = check_identity(rq, g, q, w["probe"], 10, True, "caps with a ratio", ratio=ratio, min_probe=3, max_probe=caps)
    assert np.array_equal(npr, am.probe_counts(dist[:300], ratio, 3, caps))
    assert (npr < caps).any() and (npr == caps).any()
    # a scalar cap; caps beyond m and 0 are clamped
    wild = caps.copy()
    wild[::3], wild[1::3] = 0, 1000
    assert np.array_equal(g.probe_counts(q, w["probe"], INF, 1, wild), np.clip(wild, 1, m))
    assert (g.query_batch_adaptive(q[:50], w["probe"], 10, INF, 1, 5)[3] == 5).all()
    # a query row holding a NaN: every coarse distance is NaN, the prefix is empty at every ratio -> min_probe; the other rows are not
    # affected
    q[7, 3] = np.nan
    q[150] = np.nan
    for r in (ratio, INF):
        npr = g.query_batch_adaptive(q, w["probe"], 10, r, 2)[3]
        assert npr[7] == 2 and npr[150] == 2, (r, npr[7], npr[150])
        assert np.array_equal(np.delete(npr, [7, 150]), np.delete(am.probe_counts(dist[:300], r, 2), [7, 150]))
        assert np.array_equal(g.probe_counts(q, w["probe"], r, 2), npr)


# ---- filters ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d128", "d100"])
def test_filtered(rq, oracle, name):
    """A random half of the ids, and whole lists (a filter correlated with the clustering: most probed lists admit nothing), against
    the filtered plain entry."""
    wd = get_world(rq, oracle, name)
    g, q, w = wd["g"], wd["q"], wd["w"]
    n = w["n"]
    rng = np.random.default_rng(3)
    half = rng.random(n) < 0.5
    lists = np.zeros(n, dtype=bool)
    mids, offs = g.map_ids, g.offsets.astype(np.int64)
    for c in range(0, g.k, 4):
        lists[mids[offs[c]:offs[c + 1]]] = True
    ratio, min_probe = w["rules"][0]
    for fname, mask in (("half", half), ("lists", lists)):
        with g.make_filter(mask=mask) as f:
            for nq, heur in ((40, False), (300, False), (300, True)):
                npr = check_identity(rq, g, q[:nq], w["probe"], 10, heur, (name, fname, nq, heur), filt=f, ratio=ratio, min_probe=min_probe)
                assert np.array_equal(npr, am.probe_counts(wd["dist"][:nq], ratio, min_probe))     # the cut does not look at the filter


# ---- metrics and row types ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cosine", "ip", "f16", "u8", "split_rows"])
def test_metrics_and_row_types(rq, kind):
    from rabitq_amd import index as ix
    w = am.WORLDS["d100"]
    x, centres, P, q, _ = am.world("d100", nq=300)
    x, q = x[:3000], q.copy()
    try:
        if kind == "cosine":
            g = rq.RaBitQ.build(x, centres / np.linalg.norm(centres, axis=1, keepdims=True), P, metric="cosine")
        elif kind == "ip":
            g = rq.RaBitQ.build(x, centres, P, metric="ip")
        elif kind == "f16":
            g = rq.RaBitQ.build(x.astype(np.float16), centres, P, rows="f16")
        elif kind == "u8":
            to_u8 = lambda a: np.clip(np.rint(a * 24.0 + 128.0), 0, 255)
            g = rq.RaBitQ.build(to_u8(x).astype(np.uint8), to_u8(centres).astype(np.float32), P, rows="u8")
            q = (q * 24.0 + 128.0).astype(np.float32)
        else:
            ix.set_option("split_rows", 2)
            g = rq.RaBitQ.build(x, centres, P)
            assert g.split_rows
        for heur in (False, True):
            npr = check_identity(rq, g, q, w["probe"], 10, heur, (kind, heur), ratio=1.5, min_probe=1)
            assert len(np.unique(npr)) >= 3, (kind, np.unique(npr))      # (an uneven cut on this index too)
        g.close()
    finally:
        ix.set_option("split_rows", 1)


# ---- overflow re-runs -----------------------------------------------------------------------------------------------------------------
def test_overflow_reruns_see_the_cut_lists(rq):
    """40 000 rows around the origin in 4 lists (each far beyond the default survivor capacity of 4096), topk 2000: behind the first
    stage [0, 2000) the heap ranker's threshold is the worst of everything seen, the rest of the nearest list survives it, overflows
    and the queries are run again -- with the lists the cut left them, not the ranked ones.  (The heuristic ranker's thresholds are
    tighter on such data and need not overflow: its leg checks the identity and prints its retries.)"""
    from rabitq_amd import index as ix
    n, d = 40_000, 64
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    centres = (0.25 * rng.standard_normal((4, d))).astype(np.float32)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=3))
    assert np.diff(g.offsets.astype(np.int64)).min() > 4096
    q = (0.2 * rng.standard_normal((6, d))).astype(np.float32)
    caps = np.array([1, 2, 3, 4, 2, 3], dtype=np.uint32)
    for heur in (False, True):
        g2 = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=3))       # (a fresh index: no capacity learnt yet)
        a = g2.query_batch_adaptive(q, 4, 2000, INF, 1, caps, heur)
        retries = ix.last_profile()["retries"]
        print(f"overflow world: heuristic_rank={heur} retries={retries}")
        if not heur:
            assert retries > 0, "the test no longer exercises the overflow path"
        assert np.array_equal(a[3], caps)
        for b in range(6):
            same_rows([v[b:b + 1] for v in a[:3]], g.query_batch(q[b:b + 1], int(caps[b]), 2000, heur), ("overflow", heur, b))
        g2.close()
    g2 = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=3))
    npr = check_identity(rq, g2, q, 4, 2000, False, "overflow, ratio rule", ratio=1.1, min_probe=1)
    assert len(np.unique(npr)) >= 2, npr
    g2.close()
    g.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_index_as_it_was(rq, oracle):
    from rabitq_amd import _lib
    wd = get_world(rq, oracle, "d100")
    g, w = wd["g"], wd["w"]
    q = np.ascontiguousarray(wd["q"][:20])
    L = _lib.lib()
    before = g.query_batch_adaptive(q, w["probe"], 10, 1.6)
    d = np.zeros((20, 10), np.float32)
    ids = np.zeros((20, 10), np.uint32)
    cnt = np.zeros(20, np.uint32)
    npr = np.zeros(20, np.uint32)
    ad = lambda a: C.c_void_p(a.ctypes.data)

    def call(rule, dist=d, idp=ids, cp=cnt, qp=q):
        return L.rq_query_batch_adaptive(g._h, None, ad(qp) if qp is not None else None, 20, q.shape[1], w["probe"], 10, 0,
                                         C.byref(rule) if rule is not None else None, ad(dist) if dist is not None else None,
                                         ad(idp) if idp is not None else None, ad(cp) if cp is not None else None, ad(npr))

    ok = lambda **kw: _lib.ProbeRuleT(**dict(dict(min_probe=1, ratio=1.6, reserved=0, max_probe=None), **kw))
    bad_size = ok()
    bad_size.struct_size = 16
    for what, rule in (("struct_size", bad_size), ("nan ratio", ok(ratio=float("nan"))), ("negative ratio", ok(ratio=-1.0)),
                       ("-inf ratio", ok(ratio=-INF)), ("min_probe 0", ok(min_probe=0)), ("reserved", ok(reserved=1)), ("null rule", None)):
        assert call(rule) == -1, what
        assert L.rq_last_error()
    assert call(ok(), dist=None) == -1 and call(ok(), idp=None) == -1 and call(ok(), cp=None) == -1 and call(ok(), qp=None) == -1
    with pytest.raises(rq.RabitqError) as e:
        g.query_batch_adaptive(q, w["probe"], 10, ratio=float("nan"))
    assert e.value.status == -1
    with pytest.raises(rq.RabitqError) as e:
        g.probe_counts(q, w["probe"], 1.6, min_probe=0)
    assert e.value.status == -1
    with pytest.raises(rq.RabitqError) as e:
        g.query_batch_adaptive(q, 0, 10, 1.6)                                     # what the plain entry refuses
    assert e.value.status == -1
    assert call(ok(ratio=0.0)) == 0 and call(ok(ratio=INF)) == 0 and call(ok(ratio=-0.0)) == 0
    after = g.query_batch_adaptive(q, w["probe"], 10, 1.6)
    same_rows(before[:3], after[:3], "after the refusals")
    assert np.array_equal(before[3], after[3])
    same_rows(g.query_batch(q, w["probe"], 10), g.query_batch_adaptive(q, w["probe"], 10)[:3], "plain after the refusals")


# ---- the device entry -----------------------------------------------------------------------------------------------------------------
def test_device_entry_and_null_nprobe(rq, oracle):
    import torch
    wd = get_world(rq, oracle, "d128")
    g, w = wd["g"], wd["w"]
    q = wd["q"][:300]
    ratio, min_probe = w["rules"][0]
    want = g.query_batch_adaptive(q, w["probe"], 10, ratio, min_probe)
    dq = torch.from_numpy(q).cuda()
    dd = torch.zeros((300, 10), dtype=torch.float32, device="cuda")
    di = torch.zeros((300, 10), dtype=torch.int32, device="cuda")
    dn = torch.zeros(300, dtype=torch.int32, device="cuda")
    dp = torch.zeros(300, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for out_np in (dp.data_ptr(), None):
        g.query_batch_adaptive_device(dq.data_ptr(), 300, q.shape[1], w["probe"], 10, dd.data_ptr(), di.data_ptr(), dn.data_ptr(), out_np,
                                      ratio=ratio, min_probe=min_probe)
        got = (dd.cpu().numpy(), di.cpu().numpy().view(np.uint32), dn.cpu().numpy().view(np.uint32))
        n = want[2]
        assert np.array_equal(got[2], n)
        for b in range(300):
            assert np.array_equal(got[1][b, :n[b]], want[1][b, :n[b]]) and np.array_equal(bits(got[0][b, :n[b]]), bits(want[0][b, :n[b]])), b
    assert np.array_equal(dp.cpu().numpy().view(np.uint32), want[3])


# ---- planning -------------------------------------------------------------------------------------------------------------------------
def test_cut_passes_plan_as_caller_lists_and_plain_calls_as_before(rq, oracle, capfd):
    """The plan trace (scan_debug bit 16384): a cut pass never takes the few-launch path nor the placed final stage, and its reach
    bounds are off (qn_slots = nprobe); the same plain calls still take them."""
    import re
    from rabitq_amd import index as ix
    wd = get_world(rq, oracle, "d128")
    g, q, w = wd["g"], wd["q"], wd["w"]

    def plan_of(fn):
        capfd.readouterr()
        ix.set_option("scan_debug", 16384)
        try:
            fn()
        finally:
            ix.set_option("scan_debug", 0)
        err = capfd.readouterr().err
        m = re.search(r"plan: pass nq=(\d+) nprobe=(\d+) large=(\d) small=(\d) will_list=(\d) placed=(\d) fin_additive=\d qn_slots=(\d+)", err)
        assert m, err
        return dict(zip(("nq", "nprobe", "large", "small", "will_list", "placed", "qn_slots"), map(int, m.groups())))

    p = plan_of(lambda: g.query_batch(q[:40], w["probe"], 10))
    assert p["small"] == 1
    p = plan_of(lambda: g.query_batch_adaptive(q[:40], w["probe"], 10, 1.6))
    assert (p["small"], p["placed"], p["qn_slots"]) == (0, 0, w["probe"]), p
    plain = plan_of(lambda: g.query_batch(q, w["probe"], 10))
    cut = plan_of(lambda: g.query_batch_adaptive(q, w["probe"], 10, 1.6))
    assert (cut["small"], cut["placed"], cut["qn_slots"]) == (0, 0, w["probe"]), cut
    assert plain["nq"] == cut["nq"] == 2048 and plain["small"] == 0
    print("plain plan", plain, "| cut plan", cut)


# ---- tune_probe_ratio -----------------------------------------------------------------------------------------------------------------
def test_tune_probe_ratio(rq, oracle):
    wd = get_world(rq, oracle, "d128")
    g, w, m = wd["g"], wd["w"], wd["m"]
    q = wd["q"][:300]
    _, eids, ecnt = g.exact_search(q, 10)

    def recall_at(ratio, min_probe):
        _, ids, cnt, npr = g.query_batch_adaptive(q, w["probe"], 10, ratio, min_probe)
        return g._recall_of(ids, cnt, eids, ecnt), float(npr.mean())

    full, _ = recall_at(INF, 1)
    for target, min_probe in ((0.9, 1), (min(full, 0.99), 2)):
        ratio, rec, mean = g.tune_probe_ratio(q, w["probe"], 10, target, min_probe)
        print(f"tune_probe_ratio: target {target:.3f} min_probe {min_probe} -> ratio {ratio:.4f} recall {rec:.4f} mean nprobe {mean:.2f} (no cut: {full:.4f}, m {m})")
        assert (rec, mean) == recall_at(ratio, min_probe)                          # the recall it reports is the recall at that ratio
        assert mean <= m
        assert ratio == INF or rec >= target
        if full >= target:
            assert rec >= target
    ratio, rec, mean = g.tune_probe_ratio(q, w["probe"], 10, 1.01)                 # out of reach: (inf, the recall without a cut, m)
    assert (ratio, mean) == (INF, float(m)) and rec == full
