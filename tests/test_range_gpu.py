"""Range search (rq_range_search*): for query b with radius r_b, every row u of its probed lists with
rough(b, u) < r_b and accurate(b, u) < r_b -- the reference's ranker (src/rerank.rs:83-92) with its threshold held at r_b and no
bound on the number kept -- per query ascending by (Ord32(distance), id).  No tolerance anywhere: offsets, ids, distance bits and
the process counters are compared with an answer built here from the CPU oracle's stage functions (rotate_query, coarse_rank,
query_prep, scan_cluster, l2_squared_distance), with the plain query, with sub-indexes, fresh builds, split calls and shards.

Run on the GPU box:  python -m pytest tests/test_range_gpu.py -m gpu -q
"""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import synth
from tests.models import FMAX, Ref, run_range as run, same_range as same, sub_arrays

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def rq():
    import os
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def kth_radii(gidx, queries, probe, scales, topk=10):
    """radii = each query's own 10th plain distance x a scale (cycled over the queries)."""
    d, _, n = gidx.query_batch(queries, probe, topk)
    assert (n == topk).all()
    kth = d.max(axis=1)
    return (kth * np.asarray(scales, dtype=np.float32)[np.arange(len(queries)) % len(scales)]).astype(np.float32), d


def per_query(res):
    lims, dist, ids = res
    return [(dist[int(lims[b]):int(lims[b + 1])], ids[int(lims[b]):int(lims[b + 1])]) for b in range(lims.size - 1)]


SHAPES = {  # name -> n, d, k, probe
    "d128": (30_000, 128, 24, 8),
    "d100": (6_000, 100, 12, 6),
    "d64": (6_000, 64, 12, 12),
}


def make(rq, shape, seed=11):
    n, d, k, probe = SHAPES[shape]
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=seed, centre_scale=0.6)
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=seed + 1)
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=seed + 2, centre_scale=0.6)
    return x, centres, P, queries, probe


@pytest.mark.parametrize("shape", ["d128", "d100", "d64"])
def test_oracle_parity(rq, oracle, shape):
    """1. The oracle's answer on the suite's shapes: batches of 1, 40 and 300 (both sides of the small / large-batch switch; the 300
    batch's stage runs on the matrix cores under scan_impl 0), again under scan_impl 1 and 2, under rerank_shadow 0 / 1 / 2 and on a
    tiered split-row build (base_device_mb) -- every variant bit-identical to the oracle, counters included."""
    from rabitq_amd import index as ix
    x, centres, P, queries, probe = make(rq, shape)
    n, d = x.shape
    oidx = oracle.OracleIndex.build(x, centres, P)
    ref = Ref(oracle, oidx)
    gidx = rq.RaBitQ.build(x, centres, P)
    radii, _ = kth_radii(gidx, queries, probe, [0.9, 1.0, 1.15, 1.4, 2.0])
    want = {nq: ref.answer(queries[:nq], probe, radii[:nq]) for nq in (1, 40, 300)}
    print(shape, "results per query (300):", np.diff(want[300][0].astype(np.int64)).mean(), "max", np.diff(want[300][0].astype(np.int64)).max())
    assert want[300][0][-1] > 3000

    def check(g, what):
        for nq in (1, 40, 300):
            got, m, pr = run(rq, g, queries[:nq], probe, radii[:nq])
            same(got, want[nq][:3], (shape, what, nq))
            assert (m["rough"], m["precise"], m["query"], m["miss"]) == (want[nq][3]["rough"], want[nq][3]["precise"], nq, 0), (what, nq, m, want[nq][3])
            # the profile: every candidate below its radius got an exact distance (or a shadow-row proof) once; the rows scanned are the
            # probed lists' -- and, for the queries that were run again, theirs a second time
            assert pr["rerank_candidates"] == want[nq][3]["precise"], (what, nq, pr)
            assert pr["scan_candidates"] == want[nq][3]["rough"] if pr["retries"] == 0 else pr["scan_candidates"] > want[nq][3]["rough"], (what, nq, pr)
            assert pr["scan_launches"] >= 1 + (pr["retries"] > 0), (what, nq, pr)
        return pr

    try:
        pr = check(gidx, "default")
        assert pr["matrix_launches"] > 0, pr       # 300 queries, scan_impl 0: the stage ran on the matrix cores
        for impl in (1, 2):
            ix.set_option("scan_impl", impl)
            pr = check(gidx, f"scan_impl {impl}")
            assert (pr["matrix_launches"] > 0) == (impl == 2), (impl, pr)
        ix.set_option("scan_impl", 0)
        gidx.close()
        for shadow in (0, 1, 2):
            ix.set_option("rerank_shadow", shadow)
            g = rq.RaBitQ.build(x, centres, P)
            pr = check(g, f"rerank_shadow {shadow}")
            if shadow:
                assert pr["rerank_shadow_rejects"] > 0, (shadow, pr)
            g.close()
        ix.set_option("rerank_shadow", 2)
        ix.set_option("base_device_mb", max(1, (n * ((d + 63) // 64 * 64) * 4 * 4 // 5) >> 20))   # tiered: split rows, list tails in host memory
        g = rq.RaBitQ.build(x, centres, P)
        assert g.split_rows and g.n_hbm < g.n
        check(g, "tiered split rows")
        g.close()
    finally:
        ix.set_option("scan_impl", 0)
        ix.set_option("rerank_shadow", 2)
        ix.set_option("base_device_mb", -1)
        oidx.close()


def test_mixed_radii(rq, oracle):
    """2. One batch whose radii are 0, negative, NaN, +inf, f32::MAX, below the query's best distance, exactly its 10th distance
    (strict: the 10th itself is out) and loose ones.  The conditions on the inputs are asserted on the oracle's answer, so the test
    cannot pass vacuously: a quarter of the queries empty, a quarter with more than 100 results, and the gate leaves something out."""
    x, centres, P, queries, probe = make(rq, "d128", seed=21)
    queries = queries[:96]
    oidx = oracle.OracleIndex.build(x, centres, P)
    ref = Ref(oracle, oidx)
    gidx = rq.RaBitQ.build(x, centres, P)
    d10, _, n10 = gidx.query_batch(queries, probe, 10)
    assert (n10 == 10).all()
    kth, best = d10.max(axis=1), d10.min(axis=1)
    radii = np.empty(96, dtype=np.float32)
    kinds = ["zero", "neg", "nan", "below", "kth", "loose", "looser", "loosest"]
    for b in range(96):
        kind = kinds[b % 8]
        radii[b] = {"zero": 0.0, "neg": -1.5, "nan": np.nan, "below": best[b] * np.float32(0.99), "kth": kth[b],
                    "loose": kth[b] * np.float32(1.6), "looser": kth[b] * np.float32(2.0), "loosest": kth[b] * np.float32(3.0)}[kind]
    radii[90], radii[91] = np.inf, FMAX
    want = ref.answer(queries, probe, radii)
    counts = np.diff(want[0].astype(np.int64))
    print("mixed radii: results per query", counts.tolist())
    assert (counts == 0).sum() >= 24 and (counts > 100).sum() >= 24, counts
    gated = sum(ref.gated_rows(queries[b], probe, radii[b]) for b in range(96) if kinds[b % 8] in ("kth", "loose") and b < 48)
    print("rows with accurate < r <= rough (first 48 queries, tight radii):", gated)
    assert gated >= 1
    for b in range(96):   # strictness: the 10th distance itself is excluded, everything closer is not lost by it
        if kinds[b % 8] == "kth" and b not in (90, 91):
            assert counts[b] <= 9
    nrows = int(ref.rows(queries[90], probe)[0].size)
    assert counts[90] == nrows and counts[91] == int(ref.rows(queries[91], probe)[0].size)   # +inf / f32::MAX: every probed row
    got, m, pr = run(rq, gidx, queries, probe, radii)
    same(got, want[:3], "mixed")
    assert (m["rough"], m["precise"], m["query"]) == (want[3]["rough"], want[3]["precise"], 96), (m, want[3])
    # a scalar radius is the same radius for every query
    got = gidx.range_search(queries[:8], probe, float(kth[5]))
    same(got, ref.answer(queries[:8], probe, np.full(8, kth[5], np.float32))[:3], "scalar")
    gidx.close()
    oidx.close()


def test_beyond_every_uniform_capacity(rq, oracle):
    """3. 80 000 rows in 16 lists, probe 16: three queries with radius f32::MAX among many tight ones return every row (more than
    RQ_MAX_CAP_HINT = 32 768 each), one returns a few thousand; all equal the oracle, and the profile shows the re-runs."""
    n, d, k, nq = 80_000, 64, 16, 120
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=31, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=32)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=33, centre_scale=0.6)
    oidx = oracle.OracleIndex.build(x, centres, P)
    ref = Ref(oracle, oidx)
    gidx = rq.RaBitQ.build(x, centres, P)
    radii, _ = kth_radii(gidx, queries, k, [1.0, 1.1, 1.3])
    radii[[7, 60, 119]] = FMAX
    exact = ((x - queries[40]) ** 2).sum(axis=1)
    radii[40] = np.partition(exact, 6000)[6000]          # a segment for the one-block LDS sort
    want = ref.answer(queries, k, radii)
    counts = np.diff(want[0].astype(np.int64))
    assert (counts[[7, 60, 119]] == n).all() and n > 32768 and 2048 < counts[40] <= 16384, counts[[7, 40, 60, 119]]
    got, m, pr = run(rq, gidx, queries, k, radii)
    same(got, want[:3], "beyond capacity")
    assert (m["rough"], m["precise"], m["query"]) == (want[3]["rough"], want[3]["precise"], nq), (m, want[3])
    print("beyond capacity: retries", pr["retries"], "scan launches", pr["scan_launches"], "total results", int(got[0][-1]))
    assert pr["retries"] >= 3, pr
    # all queries loose at once: every one is re-run (80 000 candidates each is beyond what a pass remembers: both calls re-run
    # them all -- test_learnt_capacity covers the needs that are remembered), and the answer is the same both times
    loose = np.full(nq, FMAX, dtype=np.float32)
    a, _, pra = run(rq, gidx, queries[:16], k, loose[:16])
    b, _, prb = run(rq, gidx, queries[:16], k, loose[:16])
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert (np.diff(a[0].astype(np.int64)) == n).all() and pra["retries"] == 16 and prb["retries"] == 16
    gidx.close()
    oidx.close()


def test_consistent_with_plain_query(rq, oracle):
    """4. The index and queries of test_seeded_probed_query with its own seeds as radii, nextafter(10th distance) * 1.0001: every
    returned entry is one of the plain top-10 (same distance bits) or has a distance not above the plain 10th; the plain entries
    missing from the range answer (estimate not below the radius) number at most nq * 10 / 50.
    One more kind of entry is legitimate and is counted apart: a row whose exact distance lies in the band (10th distance, radius)
    -- the radius is the 10th distance nudged UP, so the 11th neighbour can fall inside it.  On these inputs the reference's own
    gate (CPU oracle) gives 30 missing entries (cap 60), no entry outside the plain answer at or below the 10th distance, and 9 in
    the band."""
    n, d, k, probe, topk, nq = 30_000, 128, 24, 8, 10, 300
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=81, centre_scale=0.6)
    idx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=82))
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=83, centre_scale=0.6)
    wd, wi, wn = idx.query_batch(queries, probe, topk)
    assert (wn == topk).all()
    kth = wd.max(axis=1)
    radii = (np.nextafter(kth, np.float32(np.inf)) * np.float32(1.0001)).astype(np.float32)
    got, m, pr = run(rq, idx, queries, probe, radii)
    missing = band = 0
    for b, (gd, gi) in enumerate(per_query(got)):
        plain = {int(i): wd[b, e].tobytes() for e, i in enumerate(wi[b])}
        assert np.array_equal(np.lexsort((gi, gd.view(np.int32))), np.arange(gd.size)), b     # ascending by (distance, id)
        for dist, i in zip(gd, gi):
            if (int(i) in plain and dist.tobytes() == plain[int(i)]) or dist <= kth[b]:
                continue
            assert kth[b] < dist < radii[b], (b, int(i), dist, kth[b], radii[b])
            band += 1
        missing += sum(1 for i in plain if i not in set(gi.tolist()))
    print("plain top-10 entries missing from the range answer:", missing, "of", nq * topk, "| entries between the 10th distance and the radius:", band)
    assert missing <= nq * topk // 50, missing
    assert band <= nq // 10, band
    assert pr["retries"] == 0 and m["query"] == nq
    idx.close()


@pytest.mark.parametrize("name", ["half", "pct1", "empty", "full"])
def test_filters(rq, oracle, name):
    """5. The filtered range answer = the unfiltered one with the non-admitted ids removed = the oracle's on the sub-index;
    rough counts the admitted rows of the probed lists, precise the admitted candidates below the radius."""
    x, centres, P, queries, probe = make(rq, "d64", seed=41)
    n = x.shape[0]
    nq = 80
    queries = queries[:nq]
    gidx = rq.RaBitQ.build(x, centres, P)
    radii, _ = kth_radii(gidx, queries, probe, [1.0, 1.3, 2.0, 4.0])
    rng = np.random.default_rng(5)
    allowed = {"half": rng.random(n) < 0.5, "pct1": rng.random(n) < 0.01, "empty": np.zeros(n, bool), "full": np.ones(n, bool)}[name]
    plain, _, _ = run(rq, gidx, queries, probe, radii)
    sub = sub_arrays(gidx, allowed)
    ov = oracle.OracleIndex.view(gidx.dim, *sub)
    want = Ref(oracle, ov).answer(queries, probe, radii)
    with gidx.make_filter(mask=allowed) as f:
        got, m, pr = run(rq, gidx, queries, probe, radii, filter=f)
    same(got, want[:3], name)
    assert (m["rough"], m["precise"], m["query"]) == (want[3]["rough"], want[3]["precise"], nq), (name, m, want[3])
    cut_l, cut_d, cut_i = [0], [], []
    for gd, gi in per_query(plain):
        keep = allowed[gi]
        cut_d.append(gd[keep]), cut_i.append(gi[keep]), cut_l.append(cut_l[-1] + int(keep.sum()))
    same(got, (np.array(cut_l, np.uint64), np.concatenate(cut_d), np.concatenate(cut_i)), name + " (cut)")
    if name == "empty":
        assert got[0][-1] == 0 and m["rough"] == 0
    if name == "full":
        same(got, plain, "full == unfiltered")
    ov.close()
    gidx.close()


def test_after_add_and_remove(rq):
    """6. After add / remove the range answers equal those of a fresh build of the live rows (its ids j = the j-th smallest live
    id), and a filter made before the mutation is refused."""
    n, d, k, probe = 6_000, 64, 12, 6
    x, centres, _ = synth.mixture(n + 1500, d, k, sigma=0.8, seed=51, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=52)
    queries, _, _ = synth.mixture(100, d, k, sigma=0.8, seed=53, centre_scale=0.6)
    g = rq.RaBitQ.build(x[:n], centres, P)
    old = g.make_filter(ids=np.arange(0, n, 2))
    rng = np.random.default_rng(9)
    gone = rng.choice(n, 900, replace=False)
    assert g.remove(ids=gone) == 900
    new_ids = g.add(x[n:])
    kept = np.setdiff1d(np.arange(n), gone)
    ids_all = np.concatenate([kept, new_ids.astype(np.int64)])     # (the new ids follow the largest id still held, not n)
    rows_all = np.concatenate([x[kept], x[n:]])
    order = np.argsort(ids_all)
    live = ids_all[order]
    assert np.unique(live).size == live.size
    fresh = rq.RaBitQ.build(rows_all[order], centres, P)
    radii, _ = kth_radii(fresh, queries, probe, [1.0, 1.5, 3.0])
    a = g.range_search(queries, probe, radii)
    b = fresh.range_search(queries, probe, radii)
    same(a, (b[0], b[1], live[b[2]].astype(np.uint32)), "after mutation")
    assert a[0][-1] > 1000
    with pytest.raises(rq.RabitqError) as e:
        g.range_search(queries, probe, radii, filter=old)
    assert e.value.status == -1
    old.close()
    with g.make_filter(ids=live[::3]) as f:
        c = g.range_search(queries, probe, radii, filter=f)
        assert 0 < c[0][-1] < a[0][-1] and np.isin(c[2], live[::3]).all()
    fresh.close()
    g.close()


def test_more_queries_than_a_pass_and_two_threads(rq):
    """7. 70 000 queries (two passes) equal the same queries in two calls; two threads calling range_search_device and
    query_batch_device on one index concurrently both get their single-threaded answers."""
    import torch
    dev = torch.device("cuda", 0)
    n, d, k, probe, nq = 6_000, 64, 12, 4, 70_000
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=61, centre_scale=0.6)
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=62))
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=63, centre_scale=0.6)
    kth, _ = kth_radii(g, queries[:2000], probe, [1.0])
    radii = np.full(nq, np.median(kth), dtype=np.float32) * np.linspace(0.5, 1.6, nq, dtype=np.float32)
    one = g.range_search(queries, probe, radii)
    h = 33_000
    a, b = g.range_search(queries[:h], probe, radii[:h]), g.range_search(queries[h:], probe, radii[h:])
    same(one, (np.concatenate([a[0], b[0][1:] + a[0][-1]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]])), "two calls")
    counts = np.diff(one[0].astype(np.int64))
    print("70 000 queries: total", int(one[0][-1]), "empty", int((counts == 0).sum()), "max", int(counts.max()))
    assert one[0][-1] > nq and (counts == 0).any()

    m = 4096
    q = torch.from_numpy(queries[:m]).to(dev)
    r = torch.from_numpy(radii[:m] * np.float32(1.5)).to(dev)
    od = torch.empty((m, 10), device=dev)
    oi = torch.zeros((m, 10), device=dev, dtype=torch.int32)
    on = torch.zeros(m, device=dev, dtype=torch.int32)
    torch.cuda.synchronize()

    def range_call():
        with g.range_search_device(q.data_ptr(), m, d, probe, r.data_ptr()) as res:
            return res.to_host()

    def topk_call():
        g.query_batch_device(q.data_ptr(), m, d, probe, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        torch.cuda.synchronize()
        return od.cpu().numpy().copy(), oi.cpu().numpy().copy(), on.cpu().numpy().copy()

    want_r, want_t = range_call(), topk_call()
    out, errs = {}, []

    def worker(name, fn, reps):
        try:
            out[name] = [fn() for _ in range(reps)]
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)

    ts = [threading.Thread(target=worker, args=("r", range_call, 6)), threading.Thread(target=worker, args=("t", topk_call, 1))]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for res in out["r"]:
        same(res, want_r, "concurrent range")
    for u, v in zip(out["t"][0], want_t):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    g.close()


def test_shards_unite_to_the_full_answer(rq):
    """8. The union over the shards of a 4-way partition (rq_shard_index: original ids) equals the full index's answer."""
    x, centres, P, queries, probe = make(rq, "d128", seed=71)
    g = rq.RaBitQ.build(x, centres, P)
    radii, _ = kth_radii(g, queries, probe, [1.0, 1.3, 2.0])
    full = g.range_search(queries, probe, radii)
    owner, _ = g.partition_lists(4)
    parts = []
    for rank in range(4):
        s = g.shard(owner, rank)
        parts.append(per_query(s.range_search(queries, probe, radii)))
        s.close()
    lims, dist, ids = [0], [], []
    for b in range(len(queries)):
        d = np.concatenate([p[b][0] for p in parts])
        i = np.concatenate([p[b][1] for p in parts])
        order = np.lexsort((i, d.view(np.int32)))
        dist.append(d[order]), ids.append(i[order]), lims.append(lims[-1] + d.size)
    same(full, (np.array(lims, np.uint64), np.concatenate(dist), np.concatenate(ids)), "shards")
    assert full[0][-1] > 3000
    g.close()


def test_lifetime_and_errors(rq):
    """9. The result's device arrays are readable (by torch) until it is freed; NULL arguments, probe == 0, a wrong len and another
    index's filter give the documented statuses and leave *out NULL; an empty batch is an empty result."""
    import torch
    from rabitq_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    x, centres, P, queries, probe = make(rq, "d64", seed=91)
    d = x.shape[1]
    g = rq.RaBitQ.build(x, centres, P)
    other = rq.RaBitQ.build(x[:2000], centres, P)
    radii, _ = kth_radii(g, queries, probe, [1.5])
    want = g.range_search(queries, probe, radii)
    q = torch.from_numpy(queries).to(dev)
    r = torch.from_numpy(radii).to(dev)
    torch.cuda.synchronize()
    res = g.range_search_device(q.data_ptr(), len(queries), d, probe, r.data_ptr())
    assert (res.nq, res.total) == (len(queries), int(want[0][-1])) and res.total > 0
    pl, pd, pi = res.device_ptrs()
    host = res.to_host()
    same(host, want, "device entry")
    tl = torch.empty(res.nq + 1, dtype=torch.int64, device=dev)
    td = torch.empty(res.total, dtype=torch.float32, device=dev)
    ti = torch.empty(res.total, dtype=torch.int32, device=dev)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for dst, src, nbytes in ((tl, pl, (res.nq + 1) * 8), (td, pd, res.total * 4), (ti, pi, res.total * 4)):
        assert hip.hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(src), nbytes, 3) == 0   # device to device
    torch.cuda.synchronize()
    assert np.array_equal(tl.cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(td.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(ti.cpu().numpy().view(np.uint32), want[2])
    res.close()
    res.close()                                  # idempotent
    L.rq_range_result_free(None)                 # a no-op
    empty = g.range_search(queries[:0], probe, np.zeros(0, np.float32))
    assert empty[0].tolist() == [0] and empty[1].size == 0 and empty[2].size == 0

    def call(idx_h, filt_h, qp, nq, ln, pb, rp, with_out=True):
        h = C.c_void_p(0xDEAD)
        st = L.rq_range_search_device(idx_h, filt_h, C.c_void_p(qp), nq, ln, pb, C.c_void_p(rp), C.byref(h) if with_out else None)
        return st, h.value

    qp, rp, nq = q.data_ptr(), r.data_ptr(), len(queries)
    assert call(g._h, None, qp, nq, d, probe, rp, with_out=False)[0] == -1
    assert call(None, None, qp, nq, d, probe, rp) == (-1, None)
    assert call(g._h, None, 0, nq, d, probe, rp) == (-1, None)
    assert call(g._h, None, qp, nq, d, probe, 0) == (-1, None)
    assert call(g._h, None, qp, nq, d, 0, rp) == (-1, None)            # probe == 0: the reference panics
    assert call(g._h, None, qp, nq, d + 64, probe, rp) == (-2, None)   # does not pad to the index's dim
    with other.make_filter(ids=np.arange(100)) as f:
        assert call(g._h, f._h, qp, nq, d, probe, rp) == (-1, None)
    h = C.c_void_p(0xDEAD)
    assert L.rq_range_search(None, None, None, 1, d, probe, None, C.byref(h)) == -1 and h.value is None
    nqv, tot = C.c_uint32(), C.c_uint64()
    assert L.rq_range_result_info(None, C.byref(nqv), C.byref(tot)) == -1
    same(g.range_search(queries, probe, radii), want, "after the refused calls")
    other.close()
    g.close()


def test_range_calls_leave_the_top_k_path_as_it_was(rq):
    """A range call must not change how later top-k calls on the index run: the matrix-core scan's gate is chosen per index from
    what its passes observe (the additive gate is given up for good once too many sub-tile steps take the exact path), and a
    range stage under loose radii -- every candidate a survivor -- is exactly what that rule would react to.  The plain query's
    profile (additive-gate launches among its matrix-core launches) and its results are the same before and after range calls
    with radius f32::MAX."""
    from rabitq_amd import index as ix
    n, d, k, nq = 60_000, 64, 16, 600
    x, centres, _ = synth.mixture(n, d, k, sigma=0.3, seed=101, centre_scale=1.0)     # well separated lists: a tight gate
    g = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=102))
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.3, seed=103, centre_scale=1.0)
    g.query_batch(queries, k, 10)
    before = g.query_batch(queries, k, 10)
    pb = ix.last_profile()
    # the plain call runs its final stage under the additive gate and keeps it from call to call on its own (else the check
    # below would say nothing about range calls)
    assert pb["matrix_launches"] > 0 and pb["matrix_additive_launches"] > 0, pb
    assert not (pb["matrix_subtile_steps"] >= 4096 and pb["matrix_exact_steps"] * 32 > pb["matrix_subtile_steps"]), pb
    for _ in range(2):
        lims, _, _ = g.range_search(queries, k, FMAX)
        pr = ix.last_profile()
        assert int(lims[-1]) == nq * n
        assert pr["matrix_subtile_steps"] >= 4096 and pr["matrix_exact_steps"] * 32 > pr["matrix_subtile_steps"], pr   # the rule's own condition
    after = g.query_batch(queries, k, 10)
    pa = ix.last_profile()
    assert (pa["matrix_launches"], pa["matrix_additive_launches"]) == (pb["matrix_launches"], pb["matrix_additive_launches"]), (pb, pa)
    for u, v in zip(before, after):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    g.close()


def test_learnt_capacity(rq, oracle):
    """Most queries of a call admit more candidates than the default buffers hold (between 4 096 and RQ_MAX_CAP_HINT = 32 768),
    two admit every row (far beyond it): the first call re-runs them, the index remembers the capacity the ordinary ones needed
    -- the outliers do not decide it -- and the second call re-runs only the two outliers.  Both answers equal the oracle's."""
    n, d, k, nq = 60_000, 64, 16, 64
    probe = k
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=111, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=112)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=113, centre_scale=0.6)
    oidx = oracle.OracleIndex.build(x, centres, P)
    g = rq.RaBitQ.build(x, centres, P)
    # (on the CPU oracle: with the 10th distance x 1.5, 57 of the 64 queries have between 4 096 and 32 768 candidates, at most 20 964)
    radii, _ = kth_radii(g, queries, probe, [1.5])
    radii[[5, 50]] = FMAX            # 60 000 candidates each
    want = Ref(oracle, oidx).answer(queries, probe, radii)
    cand = want[3]["precise"]
    a, ma, pa = run(rq, g, queries, probe, radii)
    b, mb, pb = run(rq, g, queries, probe, radii)
    print("learnt capacity: candidates per query", cand / nq, "retries", pa["retries"], "then", pb["retries"])
    same(a, want[:3], "first call")
    same(b, want[:3], "second call")
    assert pa["retries"] >= nq // 2, pa
    assert pb["retries"] == 2, pb
    for m in (ma, mb):
        assert (m["rough"], m["precise"], m["query"]) == (want[3]["rough"], want[3]["precise"], nq), (m, want[3])
    g.close()
    oidx.close()
