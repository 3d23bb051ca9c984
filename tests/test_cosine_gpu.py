"""Cosine metric (RQ_METRIC_COSINE): an index that normalises its rows and its queries on the GPU.

The contract (include/rabitq_hip.h): a cosine index of (base, centroids, P) equals, bit for bit, the L2 index of (N(base), centroids,
P), and a raw query q returns exactly what that L2 index returns for N(q) -- ids in order, distance bits, counts, status, counters.
N is modelled on the CPU in tests/cosine_model.py from the oracle's vector_dot_product.  Every check is bit-exact except the last
but one (test_meaning_against_float64), whose tolerance is derived there.

Run on the GPU box:  python -m pytest tests/test_cosine_gpu.py -m gpu -q
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import cosine_model as cm
from tests import synth
from tests.models import ARRAYS, Live, Ref, bits, run_range, same_range, sub_arrays

pytestmark = pytest.mark.gpu

GOLDEN = {os.path.basename(p)[:-4]: p for p in sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))}
FILES = ["base.fvecs", "centroids.fvecs", "factors.fvecs", "offsets_ids.ivecs", "orthogonal.fvecs", "x_binary_vec.u64vecs"]


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def raw_rows(n, d, k, seed):
    """Mixture rows with per-row lengths spread over six orders of magnitude: a cosine index must not care."""
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=seed, centre_scale=0.6)
    rng = np.random.default_rng(seed + 1000)
    scale = np.exp2(rng.integers(-10, 11, size=(n, 1))).astype(np.float32) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    return np.ascontiguousarray(x * scale), centres


@pytest.fixture(scope="module")
def big(rq, oracle):
    """The 20 000 x 128 / 32-list index: raw rows, centroids of the normalised mixture, the cosine oracle."""
    n, d, k = 20_000, 128, 32
    x, centres = raw_rows(n, d, k, seed=31)
    centres = cm.normalize_rows(oracle, centres)
    P = synth.random_orthogonal(d, seed=32)
    q, _ = raw_rows(4096, d, k, seed=33)
    nx, nq = cm.normalize_rows(oracle, x), cm.normalize_rows(oracle, q)
    oidx = oracle.OracleIndex.build(nx, centres, P)
    yield dict(x=x, centres=centres, P=P, q=q, nx=nx, nq=nq, oidx=oidx, d=d, k=k)
    oidx.close()


def same_arrays(g, o, what=""):
    assert (g.n, g.k, g.dim) == (o.n, o.k, o.dim), what
    for name in ARRAYS + ("map_ids",):
        assert np.array_equal(bits(getattr(g, name)), bits(getattr(o, name))), (what, name)


def oracle_answers(oracle, oidx, nqueries, probe, topk, heur, ids=None):
    """-> per query (dist, ids) of the oracle on normalised queries (None where the reference panics), rough, precise."""
    out, tr, tp = [], 0, 0
    for q in nqueries:
        oracle.metrics_reset()
        try:
            od, oi = oidx.query(q, probe, topk, heur)
        except Exception:
            od, oi = np.zeros(0, np.float32), np.zeros(0, np.uint32)
        m = oracle.metrics()
        tr, tp = tr + m["rough"], tp + m["precise"]
        out.append((od, oi if ids is None else ids[oi]))
    return out, tr, tp


def check_topk(rq, gidx, queries, want, probe, topk, heur, what="", filter=None):
    from rabitq_amd import index as ix
    ans, tr, tp = want
    rq.metrics_reset()
    d, gids, cnt = gidx.query_batch(queries, probe, topk, heur, filter=filter)
    m = rq.metrics()
    for b, (od, oi) in enumerate(ans):
        n = int(cnt[b])
        assert n == oi.size, (what, b, n, oi.size)
        assert np.array_equal(gids[b, :n], oi), (what, b)
        assert np.array_equal(bits(d[b, :n]), bits(od)), (what, b)
    assert (m["rough"], m["precise"], m["query"]) == (tr, tp, len(ans)), (what, m, tr, tp)
    return ix.last_profile()


# ---- 1. the normalisation on its own -----------------------------------------------------------------------------------
def families(d, rng):
    f = np.float32
    rows = [rng.standard_normal((37, d)).astype(f),
            (rng.standard_normal((9, d)) * 1e-3).astype(f), (rng.standard_normal((9, d)) * 1e6).astype(f),
            np.zeros((3, d), f), np.full((2, d), -0.0, f),
            (rng.standard_normal((5, d)) * 1e-25).astype(f),           # s underflows to zero (a subnormal s has a normal root)
            (rng.standard_normal((5, d)) * 1e-23).astype(f),           # s subnormal
            (rng.standard_normal((5, d)) * 1e-19 / np.sqrt(d)).astype(f),   # s near FLT_MIN: both sides of the is_normal test
            (rng.standard_normal((5, d)) * 3e19).astype(f),            # s overflows to inf
            (rng.standard_normal((5, d)) * 1.5e19 / np.sqrt(d)).astype(f)]  # s near FLT_MAX: both sides again
    x = np.concatenate(rows)
    special = rng.standard_normal((6, d)).astype(f)
    special[0, d // 2] = np.inf
    special[1, 0] = -np.inf
    special[2, d - 1] = np.nan
    special[3, 1], special[3, 2] = np.nan, np.inf
    special[4, ::3] = -0.0
    special[5, :] = 0.0
    special[5, d - 1] = 3.0
    return np.ascontiguousarray(np.concatenate([x, special]))


@pytest.mark.parametrize("d", [64, 100, 128, 256, 768, 1024, 4096])
def test_normalize_matches_the_model(rq, oracle, d):
    import torch
    x = families(d, np.random.default_rng(d))
    want = cm.normalize_rows(oracle, x)
    nrm2 = np.array([oracle.vector_dot_product(r, r) for r in cm.pad64(x)], dtype=np.float32)
    with np.errstate(all="ignore"):
        ident = ~(np.isfinite(np.sqrt(nrm2)) & (np.sqrt(nrm2) >= cm.FLT_MIN))
    assert ident.sum() >= 15 and (~ident).sum() >= 60, (ident.sum(), (~ident).sum())   # the families hit both branches
    got = rq.normalize(x)
    assert got.shape == want.shape
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (d, bad[:10], ident[bad[:10]])
    # device pointers: aligned, and rows starting 4 bytes off a 16-byte boundary (the scalar load / store path)
    dev = torch.device("cuda", 0)
    dim = want.shape[1]
    for off in (0, 1):
        src = torch.zeros(x.size + 4, device=dev)
        src[off:off + x.size] = torch.from_numpy(x.reshape(-1)).to(dev)
        dst = torch.full((want.size + 4,), 7.0, device=dev)
        torch.cuda.synchronize()
        rq.ops.normalize_device(src[off:].data_ptr(), x.shape[0], d, dst[off:].data_ptr())
        out = dst.cpu().numpy()
        assert np.array_equal(out[off:off + want.size].view(np.uint32), want.reshape(-1).view(np.uint32)), (d, off)
        assert (out[:off] == 7.0).all() and (out[off + want.size:] == 7.0).all()      # nothing written outside n x dim
    assert rq.normalize(np.zeros((0, d), np.float32)).shape == (0, dim)


# ---- 2. build ----------------------------------------------------------------------------------------------------------
def read_dir(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path))}


@pytest.mark.parametrize("name", ["d64_k3", "d128_k16", "d768_k4", "d100pad_identity"])
def test_golden_shapes(rq, oracle, name, tmp_path):
    """Arrays, rq_info, the dump's files and the golden query configurations (both rankers) against the cosine oracle."""
    g = np.load(GOLDEN[name])
    rng = np.random.default_rng(3)
    x = np.ascontiguousarray(g["base_in"] * np.exp2(rng.integers(-6, 7, size=(g["base_in"].shape[0], 1))).astype(np.float32))
    cents, P, queries = g["centroids_in"], g["orthogonal"], np.ascontiguousarray(g["queries"] * np.float32(3.7))
    oidx = cm.cosine_oracle(oracle, x, cents, P)
    gidx = rq.RaBitQ.build(x, cents, P, metric="cosine")
    l2 = rq.RaBitQ.build(cm.normalize_rows(oracle, x), cm.pad64(cents), P)
    try:
        assert gidx.metric == "cosine" and l2.metric == "l2"
        same_arrays(gidx, oidx, name)
        assert (gidx.n, gidx.k, gidx.dim, gidx.max_list_len, gidx.n_hbm, gidx.split_rows) == (l2.n, l2.k, l2.dim, l2.max_list_len, l2.n_hbm, l2.split_rows)
        nq = cm.normalize_rows(oracle, queries)
        ci = 0
        while f"q{ci}_cfg" in g:
            probe, topk, heur = (int(v) for v in g[f"q{ci}_cfg"])
            check_topk(rq, gidx, queries, oracle_answers(oracle, oidx, nq, probe, topk, bool(heur)), probe, topk, bool(heur), (name, ci))
            ci += 1
        assert ci == 4
        gidx.dump_to_dir(str(tmp_path / "cos"))
        l2.dump_to_dir(str(tmp_path / "l2"))
        oidx.dump_to_dir(str(tmp_path / "ora"))
        cos, l2f, ora = read_dir(tmp_path / "cos"), read_dir(tmp_path / "l2"), read_dir(tmp_path / "ora")
        assert sorted(l2f) == FILES and sorted(cos) == sorted(FILES + ["metric"]) and cos["metric"] == b"cosine\n"
        for f in FILES:
            assert cos[f] == ora[f] == l2f[f], (name, f)
    finally:
        gidx.close(), l2.close(), oidx.close()


def test_build_paths_store_the_normalised_rows(rq, oracle, big):
    """rq_build_metric, the streamed builder with several chunk sizes, a tiered index and split rows: every array is the oracle's."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    x, centres, P, oidx, d, k = big["x"], big["centres"], big["P"], big["oidx"], big["d"], big["k"]
    n = x.shape[0]
    g = rq.RaBitQ.build(x, centres, P, metric="cosine")
    same_arrays(g, oidx, "rq_build_metric")
    assert np.array_equal(bits(g.base), bits(big["nx"][oidx.map_ids]))
    g.close()
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(centres).to(dev)
    torch.cuda.synchronize()
    g = rq.RaBitQ.build_device(xd.data_ptr(), n, d, cd.data_ptr(), k, P, metric="cosine")
    same_arrays(g, oidx, "rq_build_device_metric")
    g.close()
    for chunk in (n, 7777, 1000):
        b = rq.RaBitQ.builder(n, d, cd.data_ptr(), k, P, metric="cosine")
        starts = list(range(0, n, chunk))
        for i0 in starts:
            b.assign_chunk(xd[i0:i0 + chunk].data_ptr(), i0, min(chunk, n - i0))
        b.order()
        for i0 in reversed(starts):
            b.place_chunk(xd[i0:i0 + chunk].data_ptr(), i0, min(chunk, n - i0))
        g = b.finish()
        assert g.metric == "cosine"
        same_arrays(g, oidx, f"builder chunk {chunk}")
        g.close()
    try:
        ix.set_option("base_device_mb", max(1, (n * d * 4 * 4 // 5) >> 20))
        g = rq.RaBitQ.build(x, centres, P, metric="cosine")
        assert g.n_hbm < g.n and g.split_rows, (g.n_hbm, g.n, g.split_rows)
        same_arrays(g, oidx, "tiered")
        want = oracle_answers(oracle, oidx, big["nq"][:300], 6, 10, False)
        check_topk(rq, g, big["q"][:300], want, 6, 10, False, "tiered")
        g.close()
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 2)
        g = rq.RaBitQ.build(x, centres, P, metric="cosine")
        assert g.split_rows and g.n_hbm == g.n
        same_arrays(g, oidx, "split_rows 2")
        check_topk(rq, g, big["q"][:300], want, 6, 10, False, "split rows")
        g.close()
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)


def test_d100_pads_then_normalises(rq, oracle):
    x, centres = raw_rows(3000, 100, 8, seed=41)
    P = synth.random_orthogonal(128, seed=42)
    q, _ = raw_rows(70, 100, 8, seed=43)
    oidx = cm.cosine_oracle(oracle, x, centres, P)
    g = rq.RaBitQ.build(x, centres, P, metric="cosine")
    same_arrays(g, oidx, "d100")
    nq = cm.normalize_rows(oracle, q)
    for m in (1, 64, 70):
        for heur in (False, True):
            check_topk(rq, g, q[:m], oracle_answers(oracle, oidx, nq[:m], 4, 10, heur), 4, 10, heur, ("d100", m, heur))
    g.close(), oidx.close()


# ---- 3. queries --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gbig(rq, big):
    g = rq.RaBitQ.build(big["x"], big["centres"], big["P"], metric="cosine")
    yield g
    g.close()


@pytest.mark.parametrize("heur", [False, True])
def test_query_batches_against_the_cosine_oracle(rq, oracle, big, gbig, heur):
    from rabitq_amd import index as ix
    probe, topk = 6, 10
    want_all = oracle_answers(oracle, big["oidx"], big["nq"], probe, topk, heur)

    def cut(m):
        ans = want_all[0][:m]
        if m == len(want_all[0]):
            return want_all
        sub = oracle_answers(oracle, big["oidx"], big["nq"][:m], probe, topk, heur)
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(ans, sub[0]))
        return sub

    for m in (1, 32, 64):
        pr = check_topk(rq, gbig, big["q"][:m], cut(m), probe, topk, heur, ("small", m))
        assert pr["small_batch_passes"] > 0, (m, pr)           # batches of <= 64 still take the small-batch path
    pr = check_topk(rq, gbig, big["q"][:300], cut(300), probe, topk, heur, "300")
    assert pr["small_batch_passes"] == 0
    try:
        for impl in (1, 2):
            ix.set_option("scan_impl", impl)
            pr = check_topk(rq, gbig, big["q"], want_all, probe, topk, heur, ("4096", impl))
            assert (pr["matrix_launches"] > 0) == (impl == 2), (impl, pr)
    finally:
        ix.set_option("scan_impl", 0)
    # a query scaled by a power of two is the same query
    d0, i0, n0 = gbig.query_batch(big["q"][:300], probe, topk, heur)
    for s in (1024.0, 2.0 ** -9):
        d1, i1, n1 = gbig.query_batch(np.ascontiguousarray(big["q"][:300] * np.float32(s)), probe, topk, heur)
        assert np.array_equal(n0, n1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)), s


def test_filter_range_and_tickets(rq, oracle, big, gbig):
    import torch
    dev = torch.device("cuda", 0)
    probe, topk, m = 6, 10, 300
    q, nq, oidx = big["q"][:m], big["nq"][:m], big["oidx"]
    # filter: the oracle's view of the sub-index
    allowed = np.random.default_rng(7).random(gbig.n) < 0.3
    ov = oracle.OracleIndex.view(oidx.dim, *sub_arrays(oidx, allowed))
    with gbig.make_filter(mask=allowed) as filt:
        for heur in (False, True):
            for mm in (40, m):
                check_topk(rq, gbig, q[:mm], oracle_answers(oracle, ov, nq[:mm], probe, topk, heur), probe, topk, heur, ("filtered", heur, mm),
                           filter=filt)
        # range, radii in 2 - 2 cos units, strict <: each query's own 10th distance x a scale, and a plain 0.5 (cos > 0.75)
        d10, _, n10 = gbig.query_batch(q, probe, topk)
        assert (n10 == topk).all() and d10.max() < 4.0 + 1e-3
        radii = (d10.max(axis=1) * np.array([0.9, 1.0, 1.2, 1.6], np.float32)[np.arange(m) % 4]).astype(np.float32)
        radii[::7] = 0.5
        ref = Ref(oracle, oidx)
        for mm in (1, 40, m):
            want = ref.answer(nq[:mm], probe, radii[:mm])
            got, met, _ = run_range(rq, gbig, q[:mm], probe, radii[:mm])
            same_range(got, want[:3], ("range", mm))
            assert (met["rough"], met["precise"], met["query"]) == (want[3]["rough"], want[3]["precise"], mm)
        assert want[0][-1] > 1000
        wantf = Ref(oracle, ov).answer(nq, probe, radii)
        got, met, _ = run_range(rq, gbig, q, probe, radii, filter=filt)
        same_range(got, wantf[:3], "range filtered")
        assert (met["rough"], met["precise"]) == (wantf[3]["rough"], wantf[3]["precise"])
    ov.close()
    # _begin / _end: two batches in flight
    want = oracle_answers(oracle, oidx, nq, probe, topk, False)
    qd = [torch.from_numpy(q).to(dev), torch.from_numpy(np.ascontiguousarray(q[::-1])).to(dev)]
    outs = [(torch.empty((m, topk), device=dev), torch.zeros((m, topk), device=dev, dtype=torch.int32), torch.zeros(m, device=dev, dtype=torch.int32))
            for _ in qd]
    torch.cuda.synchronize()
    rq.metrics_reset()
    tickets = [gbig.query_batch_device_begin(t.data_ptr(), m, big["d"], probe, topk, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
               for t, o in zip(qd, outs)]
    for t in tickets:
        gbig.query_batch_device_end(t)
    met = rq.metrics()
    assert (met["rough"], met["precise"], met["query"]) == (2 * want[1], 2 * want[2], 2 * m)
    for o, order in zip(outs, (np.arange(m), np.arange(m)[::-1])):
        gd, gi, gn = o[0].cpu().numpy(), o[1].cpu().numpy().view(np.uint32), o[2].cpu().numpy()
        for b, src in enumerate(order):
            od, oi = want[0][src]
            assert gn[b] == oi.size and np.array_equal(gi[b, :oi.size], oi) and np.array_equal(bits(gd[b, :oi.size]), bits(od)), b


def test_probed_seeded_coarse_and_sharded_equal_the_l2_twin(rq, oracle, big, gbig):
    """The entry points the oracle has no counterpart for, by the contract itself: the cosine index on raw queries == the L2 index
    of the model's N(base) on the model's N(q).  Both indexes are the engine's; the normalised inputs are the CPU model's."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    probe, topk, d = 6, 10, big["d"]
    twin = rq.RaBitQ.build(big["nx"], big["centres"], big["P"])
    try:
        for m in (40, 300):
            q, nq = big["q"][:m], big["nq"][:m]
            y0, cl0, cd0 = rq.ops.coarse_rank(gbig, q, probe)              # rq_coarse_rank normalises too
            y1, cl1, cd1 = rq.ops.coarse_rank(twin, nq, probe)
            assert np.array_equal(bits(y0), bits(y1)) and np.array_equal(cl0, cl1) and np.array_equal(bits(cd0), bits(cd1))
            for o, ycl in zip(range(m), cl0):                                # ... and is the oracle's ranking of N(q)
                ocl, ocd = big["oidx"].coarse_rank(big["oidx"].rotate_query(nq[o]), probe)
                assert np.array_equal(ocl, ycl) and np.array_equal(bits(ocd), bits(cd0[o]))
            pc, pdd = torch.from_numpy(cl0.view(np.int32)).to(dev), torch.from_numpy(cd0).to(dev)

            def call(idx, queries, fn, *extra):
                qd = torch.from_numpy(np.ascontiguousarray(queries)).to(dev)
                od = torch.full((m, topk), -1.0, device=dev)
                oi = torch.zeros((m, topk), device=dev, dtype=torch.int32)
                on = torch.zeros(m, device=dev, dtype=torch.int32)
                torch.cuda.synchronize()
                rq.metrics_reset()
                fn(idx, qd, od, oi, on, *extra)
                met = rq.metrics()
                return od.cpu().numpy(), oi.cpu().numpy(), on.cpu().numpy(), (met["rough"], met["precise"], met["query"])

            def same(a, b, what):
                assert np.array_equal(a[2], b[2]), what
                for r in range(m):
                    n = int(a[2][r])
                    assert np.array_equal(a[1][r, :n], b[1][r, :n]) and np.array_equal(bits(a[0][r, :n]), bits(b[0][r, :n])), (what, r)
                assert a[3] == b[3], (what, a[3], b[3])

            # coarse top-k over a list range
            ck = [torch.zeros((m, probe), device=dev, dtype=torch.int32) for _ in range(2)]
            cdist = [torch.zeros((m, probe), device=dev) for _ in range(2)]
            for j, (idx, queries) in enumerate(((gbig, q), (twin, nq))):
                qd = torch.from_numpy(np.ascontiguousarray(queries)).to(dev)
                torch.cuda.synchronize()
                idx.coarse_topk_device(qd.data_ptr(), m, d, 3, 29, probe, ck[j].data_ptr(), cdist[j].data_ptr())
            assert torch.equal(ck[0], ck[1]) and torch.equal(cdist[0].view(torch.int32), cdist[1].view(torch.int32))

            probed = lambda idx, qd, od, oi, on: idx.query_batch_device_probed(qd.data_ptr(), m, d, pc.data_ptr(), pdd.data_ptr(), probe, topk,
                                                                               od.data_ptr(), oi.data_ptr(), on.data_ptr())
            a, b = call(gbig, q, probed), call(twin, nq, probed)
            same(a, b, ("probed", m))
            plain = gbig.query_batch(q, probe, topk)
            assert np.array_equal(a[1].view(np.uint32)[a[2] > 0], plain[1][a[2] > 0])
            # seeded: thresholds in 2 - 2 cos units -- just above each query's k-th distance, and below its best for every third
            thr = np.nextafter(plain[0].max(axis=1), np.float32(np.inf)) * np.float32(1.0001)
            thr[::3] = plain[0].min(axis=1)[::3]
            t = torch.from_numpy(np.ascontiguousarray(thr, np.float32)).to(dev)
            seeded = lambda idx, qd, od, oi, on: idx.query_batch_device_seeded(qd.data_ptr(), m, d, pc.data_ptr(), pdd.data_ptr(), probe, topk,
                                                                               t.data_ptr(), od.data_ptr(), oi.data_ptr(), on.data_ptr())
            a, b = call(gbig, q, seeded), call(twin, nq, seeded)
            same(a, b, ("seeded", m))
            assert (a[2][::3] == 0).all() and (a[2][1::3] > 0).all()
            # the sharded step, one rank (no communicator), plain and with the shared-threshold path forced
            for shared in (1, 2):
                ix.set_option("shared_thresholds", shared)
                sharded = lambda idx, qd, od, oi, on: idx.query_batch_sharded_device(0, 1, 1000, qd.data_ptr(), m, d, probe, topk, od.data_ptr(),
                                                                                     oi.data_ptr(), on.data_ptr())
                a, b = call(gbig, q, sharded), call(twin, nq, sharded)
                same(a, b, ("sharded", m, shared))
                for r in range(m):
                    order = np.lexsort((plain[1][r], plain[0][r]))
                    assert np.array_equal(a[1][r].view(np.uint32), plain[1][r][order] + 1000), r
        # a shard carved from a cosine index is a cosine index
        owner, _ = gbig.partition_lists(2)
        sh = gbig.shard(owner, 1)
        tw = twin.shard(owner, 1)
        assert sh.metric == "cosine" and tw.metric == "l2"
        a, b = sh.query_batch(big["q"][:100], probe, topk), tw.query_batch(big["nq"][:100], probe, topk)
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
        sh.close(), tw.close()
    finally:
        ix.set_option("shared_thresholds", 1)
        twin.close()


# ---- 4. mutation -------------------------------------------------------------------------------------------------------
def test_add_remove_equal_a_fresh_cosine_build(rq, oracle):
    n, d, k, probe, topk = 6000, 128, 12, 4, 10
    pool, centres = raw_rows(n + 3000, d, k, seed=51)
    centres = cm.normalize_rows(oracle, centres)
    P = synth.random_orthogonal(d, seed=52)
    q, _ = raw_rows(120, d, k, seed=53)
    nq = cm.normalize_rows(oracle, q)
    g = rq.RaBitQ.build(pool[:n], centres, P, metric="cosine")
    live = Live(np.arange(n), pool[:n])
    rng = np.random.default_rng(54)

    def check(what):
        ids, rows = live.sorted()
        o = cm.cosine_oracle(oracle, rows, centres, P)
        fresh = rq.RaBitQ.build(rows, centres, P, metric="cosine")
        try:
            assert g.metric == "cosine" and (g.n, g.k) == (o.n, o.k), what
            for name in ARRAYS:
                assert np.array_equal(bits(getattr(g, name)), bits(getattr(o, name))), (what, name)
                assert np.array_equal(bits(getattr(g, name)), bits(getattr(fresh, name))), (what, "fresh", name)
            assert np.array_equal(g.map_ids, ids[o.map_ids]), what
            for heur in (False, True):
                check_topk(rq, g, q, oracle_answers(oracle, o, nq, probe, topk, heur, ids=ids), probe, topk, heur, (what, heur))
        finally:
            o.close(), fresh.close()

    got = g.add(pool[n:n + 1500])                                   # host rows, default ids
    live.add(got, pool[n:n + 1500])
    check("add 1500")
    drop = rng.choice(n + 1500, size=2000, replace=False)
    assert g.remove(ids=drop) == 2000
    live.remove(drop)
    check("remove 2000")
    import torch
    rows = torch.from_numpy(pool[n + 1500:n + 3000]).to(torch.device("cuda", 0))   # device rows, explicit ids (some re-used)
    new_ids = np.concatenate([drop[:700], np.arange(20_000, 20_800)]).astype(np.uint32)
    rng.shuffle(new_ids)
    idd = torch.from_numpy(new_ids.view(np.int32)).to(rows.device)
    torch.cuda.synchronize()
    g.add_device(rows.data_ptr(), 1500, d, idd.data_ptr())
    live.add(new_ids, pool[n + 1500:n + 3000])
    check("add_device 1500 with ids")
    g.update(new_ids[:50], pool[:50] * np.float32(-3.0))
    live.remove(new_ids[:50])
    live.add(new_ids[:50], pool[:50] * np.float32(-3.0))
    check("update 50")
    g.close()


# ---- 5. persistence ----------------------------------------------------------------------------------------------------
def test_round_trips_keep_the_metric(rq, oracle, tmp_path):
    from rabitq_amd import _lib
    x, centres = raw_rows(1500, 100, 6, seed=61)
    P = synth.random_orthogonal(128, seed=62)
    q, _ = raw_rows(80, 100, 6, seed=63)
    g = rq.RaBitQ.build(x, centres, P, metric="cosine")
    l2 = rq.RaBitQ.build(x, centres, P)
    want = g.query_batch(q, 3, 10)
    g.dump_to_dir(str(tmp_path / "cos"))
    l2.dump_to_dir(str(tmp_path / "l2"))
    assert sorted(os.listdir(tmp_path / "l2")) == FILES                                 # an L2 dump: exactly the crate's files, nothing more
    assert sorted(os.listdir(tmp_path / "cos")) == sorted(FILES + ["metric"])
    assert open(tmp_path / "cos" / "metric", "rb").read() == b"cosine\n"
    g.dump_to_json(str(tmp_path / "cos.json"))
    l2.dump_to_json(str(tmp_path / "l2.json"))
    assert '"metric":"cosine"' in open(tmp_path / "cos.json").read() and "metric" not in open(tmp_path / "l2.json").read()
    o = oracle.OracleIndex.load_from_dir(str(tmp_path / "cos"))                        # the reference's loader reads the five files
    assert np.array_equal(bits(o.base), bits(g.base))
    o.close()
    for load, path, metric in ((rq.RaBitQ.load_from_dir, tmp_path / "cos", "cosine"), (rq.RaBitQ.load_from_json, tmp_path / "cos.json", "cosine"),
                               (rq.RaBitQ.load_from_dir, tmp_path / "l2", "l2"), (rq.RaBitQ.load_from_json, tmp_path / "l2.json", "l2")):
        h = load(str(path))
        assert h.metric == metric, path
        src = g if metric == "cosine" else l2
        for name in ARRAYS + ("map_ids",):
            assert np.array_equal(bits(getattr(h, name)), bits(getattr(src, name))), (path, name)
        got = h.query_batch(q, 3, 10)
        ref = want if metric == "cosine" else l2.query_batch(q, 3, 10)
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[1], ref[1]) and np.array_equal(bits(got[0]), bits(ref[0])), path
        h.close()
    assert not np.array_equal(want[1], l2.query_batch(q, 3, 10)[1])                     # (the metric matters on these rows)
    # from_arrays(metric=...) marks the index and takes the arrays as they are
    h = rq.RaBitQ.from_arrays(g.base, g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors, metric="cosine")
    assert h.metric == "cosine" and np.array_equal(bits(h.base), bits(g.base))
    got = h.query_batch(q, 3, 10)
    assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
    h.close()
    # a dump directory re-used for an L2 index loses the sixth file; unknown contents are refused
    l2.dump_to_dir(str(tmp_path / "cos"))
    assert sorted(os.listdir(tmp_path / "cos")) == FILES
    open(tmp_path / "l2" / "metric", "w").write("dot\n")
    with pytest.raises(rq.RabitqError) as e:
        rq.RaBitQ.load_from_dir(str(tmp_path / "l2"))
    assert e.value.status == -3
    # unknown metric ids are refused by every *_metric entry
    L = _lib.lib()
    h = C.c_void_p()
    xs, cs = np.ascontiguousarray(x), np.ascontiguousarray(centres)
    assert L.rq_build_metric(xs.ctypes.data, 1500, 100, cs.ctypes.data, 6, None, 0, 2, C.byref(h)) == -1
    assert L.rq_build_device_metric(xs.ctypes.data, 1500, 100, cs.ctypes.data, 6, None, 0, 7, C.byref(h)) == -1
    assert L.rq_builder_create_metric(1500, 100, cs.ctypes.data, 6, None, 0, 0, 2, C.byref(h)) == -1
    assert L.rq_build_from_path_metric(b"/nonexistent/b", b"/nonexistent/c", None, 0, 2, C.byref(h)) == -1
    with pytest.raises(rq.RabitqError) as e:
        rq.RaBitQ.from_arrays(g.base, g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors, metric=2)
    assert e.value.status == -1
    g.close(), l2.close()


# ---- 6. meaning --------------------------------------------------------------------------------------------------------
def test_meaning_against_float64(rq, big, gbig):
    """Each returned distance against 2 - 2 cos computed in float64 from the ORIGINAL, un-normalised vectors.
    rtol 1e-5 is the relative tolerance of the f64 checks in tests/test_gpu_parity.py (the f32 rerank's own error).  The absolute
    floor covers what the normalisation adds: each unit vector is off by at most e = (dim/8 + 3) * 2^-24 relative, so
    N(x) - N(q) is off by at most 2e in norm, and |a|^2 with |a| <= 2 moves by at most 2 * 2 * 2e + (2e)^2 < 8.1 e; for dim 128
    that is 9.2e-6 -- the floor for distances near zero, where a relative tolerance says nothing."""
    dim = gbig.dim
    e = cm.unit_error_bound(dim)
    atol = 8.1 * e
    assert atol < 1e-5
    x64, q64 = big["x"].astype(np.float64), big["q"][:1000].astype(np.float64)
    xu = x64 / np.linalg.norm(x64, axis=1)[:, None]
    qu = q64 / np.linalg.norm(q64, axis=1)[:, None]
    # near-zero distances as well: queries that are rows of the index, scaled
    qs = np.ascontiguousarray(np.concatenate([big["q"][:1000], big["x"][:200] * np.float32(0.37)]))
    qu = np.concatenate([qu, xu[:200]])
    d, ids, cnt = gbig.query_batch(qs, 6, 10)
    assert (cnt == 10).all()
    want = 2.0 - 2.0 * np.einsum("bkd,bd->bk", xu[ids.astype(np.int64)], qu)
    err = np.abs(d.astype(np.float64) - want)
    print("meaning: max abs err", err.max(), "max err / (atol + rtol * want)", (err / (atol + 1e-5 * np.abs(want))).max(), "min distance", d.min())
    assert (d[1000:].min(axis=1) < 1e-5).all()                   # every self-query found itself at (almost) zero
    assert (err <= atol + 1e-5 * np.abs(want)).all()
    sim = rq.cosine_similarity(d)
    assert np.abs(sim - np.einsum("bkd,bd->bk", xu[ids.astype(np.int64)], qu)).max() <= (atol + 4e-5) / 2
