"""Inner-product metric (RQ_METRIC_IP): an index that augments its rows on the GPU and answers maximum inner product search.

The contract (include/rabitq_hip.h): an IP index of (base, centroids, P, S) equals, bit for bit, the L2 index of (A(base; S),
centroids zero-extended to dim = ceil64(d + 1), P), and a raw query q of d floats returns exactly what that L2 index returns for
q zero-padded to dim -- ids in order, distance bits, counts, status, counters.  A is modelled on the CPU in tests/ip_model.py from
the oracle's vector_dot_product.  Every check is bit-exact except test_meaning_against_float64, whose tolerance is derived there,
and the merged-shards comparison, which uses the rule of tests/test_sharded_gpu.py.

Run on the GPU box:  python -m pytest tests/test_ip_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ip_model as im
from tests import synth
from tests.models import ARRAYS, Live, Ref, bits, run_range, same_range, sub_arrays
from tests.test_ip_abi import planted_case

pytestmark = pytest.mark.gpu
F32 = np.float32
FILES = ["base.fvecs", "centroids.fvecs", "factors.fvecs", "offsets_ids.ivecs", "orthogonal.fvecs", "x_binary_vec.u64vecs"]


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def raw_rows(n, d, k, seed):
    """Mixture rows whose norms are spread over +-3 octaves: what an inner-product index exists for."""
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=seed, centre_scale=0.6)
    scale = np.exp2(np.random.default_rng(seed + 1000).uniform(-3.0, 3.0, size=(n, 1))).astype(F32)
    return np.ascontiguousarray(x * scale), np.ascontiguousarray(centres)


_CASES = {}


@pytest.fixture(scope="module")
def case(oracle):
    """case(d) -> the 20 000-row / 32-list data set of row length d (100: dim 128, the spare pad holds the slot; 128: dim 192), its
    automatic bound and the IP oracle; built once per d."""
    def get(d):
        if d not in _CASES:
            n, k = 20_000, 32
            x, centres = raw_rows(n, d, k, seed=31 + d)
            if d == 100:   # centroids of d + 1 columns, as a caller who trains on augmented rows passes them
                centres = np.ascontiguousarray(np.concatenate([centres, np.full((k, 1), 0.25, F32)], axis=1))
            dim = im.ip_dim(d)
            P = synth.random_orthogonal(dim, seed=32)
            q, _ = raw_rows(4096, d, k, seed=33)
            S = im.auto_bound(oracle, x)
            _CASES[d] = dict(x=x, centres=centres, P=P, q=q, qq=im.pad_cols(q, dim), S=S, d=d, k=k, dim=dim,
                             oidx=im.ip_oracle(oracle, x, centres, P, S))
        return _CASES[d]
    yield get
    for c in _CASES.values():
        c["oidx"].close()
    _CASES.clear()


def same_arrays(g, o, what=""):
    assert (g.n, g.k, g.dim) == (o.n, o.k, o.dim), what
    for name in ARRAYS + ("map_ids",):
        assert np.array_equal(bits(getattr(g, name)), bits(getattr(o, name))), (what, name)


def oracle_answers(oracle, oidx, padded_queries, probe, topk, heur, ids=None):
    out, tr, tp = [], 0, 0
    for q in padded_queries:
        oracle.metrics_reset()
        try:
            od, oi = oidx.query(q, probe, topk, heur)
        except Exception:
            od, oi = np.zeros(0, F32), np.zeros(0, np.uint32)
        m = oracle.metrics()
        tr, tp = tr + m["rough"], tp + m["precise"]
        out.append((od, oi if ids is None else ids[oi]))
    return out, tr, tp


def same_answers(a, b, what=""):
    """Two (dist, ids, counts) answers: equal counts, and ids and distance bits equal up to each query's count."""
    assert np.array_equal(a[2], b[2]), what
    for r in range(len(a[2])):
        n = int(a[2][r])
        assert np.array_equal(a[1][r, :n], b[1][r, :n]) and np.array_equal(bits(a[0][r, :n]), bits(b[0][r, :n])), (what, r)


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


# ---- 1. augment and sqnorm on their own --------------------------------------------------------------------------------
def finite_families(oracle, d, rng):
    """The row families of test_cosine_gpu.families whose s stays finite, plus the metric's own edge rows."""
    from tests.test_cosine_gpu import families
    x = families(d, rng)
    with np.errstate(all="ignore"):
        x = x[np.isfinite(im.sqnorms(oracle, x))]
    edge = np.zeros((3, d), F32)
    edge[1, d - 1] = 2.0
    edge[2, :] = -0.0
    return np.ascontiguousarray(np.concatenate([x, edge]))


@pytest.mark.parametrize("d", [63, 64, 100, 128, 767, 768, 4095])
def test_augment_and_sqnorm_match_the_model(rq, oracle, d):
    import torch
    L = rq._lib.lib()
    x = finite_families(oracle, d, np.random.default_rng(d))
    n, dim = x.shape[0], im.ip_dim(d)
    s = im.sqnorms(oracle, x)
    S = im.auto_bound(oracle, x)
    assert n >= 80 and S == s.max() and S > 1e30               # the families reach up to the top of the f32 range
    assert bits(rq.row_sqnorm_max(x)).tobytes() == bits(S).tobytes()
    want = im.augment_rows(oracle, x, S)
    top = int(s.argmax())
    assert want[top, d] == 0 and not np.signbit(want[top, d])   # s == S: the slot is +0
    got = rq.augment(x)                                         # automatic bound
    assert got.shape == (n, dim)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (d, bad[:10])
    # a given bound: a modest one over the small rows, and the refusals
    small = np.ascontiguousarray(x[s <= 1e6])
    assert small.shape[0] >= 40
    for bound in (1e6, float(np.float32(3.0e38))):
        assert np.array_equal(bits(rq.augment(small, bound)), bits(im.augment_rows(oracle, small, bound))), (d, bound)
    first_bad = int(np.nonzero(im.invalid_rows(oracle, x, 1e6))[0][0])
    out = np.full((n, dim), 7.0, F32)
    for bound, row in ((1e6, first_bad), (float(np.nextafter(S, F32(0))), top)):     # s one ulp above S is refused
        assert L.rq_augment(x.ctypes.data, n, d, C.c_float(bound), out.ctypes.data) == -1
        assert f"row {row}:" in L.rq_last_error().decode(), (L.rq_last_error(), row)
    for bound in (-1.0, float("inf"), -0.5):
        assert L.rq_augment(x.ctypes.data, n, d, C.c_float(bound), out.ctypes.data) == -1
    poisoned = x.copy()
    poisoned[5, d // 2], poisoned[11, 0] = np.inf, np.nan
    mx = C.c_float(-1.0)
    assert L.rq_row_sqnorm_max(poisoned.ctypes.data, n, d, C.byref(mx)) == -1 and "row 5:" in L.rq_last_error().decode()
    assert L.rq_augment(poisoned.ctypes.data, n, d, C.c_float(float("nan")), out.ctypes.data) == -1 and "row 5:" in L.rq_last_error().decode()
    assert L.rq_augment(poisoned[6:].ctypes.data, n - 6, d, C.c_float(3e38), out.ctypes.data) == -1 and "row 5:" in L.rq_last_error().decode()
    # S = 0 with an all-zero base
    z = np.zeros((9, d), F32)
    assert rq.row_sqnorm_max(z) == 0 and not rq.augment(z).any() and not rq.augment(z, 0.0).any()
    assert rq.augment(np.zeros((0, d), F32)).shape == (0, dim) and rq.row_sqnorm_max(np.zeros((0, d), F32)) == 0
    # device pointers: aligned, and rows starting 4 bytes off a 16-byte boundary (the scalar load / store path)
    dev = torch.device("cuda", 0)
    for off in (0, 1):
        src = torch.zeros(x.size + 4, device=dev)
        src[off:off + x.size] = torch.from_numpy(x.reshape(-1)).to(dev)
        dst = torch.full((want.size + 4,), 7.0, device=dev)
        torch.cuda.synchronize()
        assert bits(rq.ops.row_sqnorm_max_device(src[off:].data_ptr(), n, d)).tobytes() == bits(S).tobytes()
        rq.ops.augment_device(src[off:].data_ptr(), n, d, None, dst[off:].data_ptr())
        o = dst.cpu().numpy()
        assert np.array_equal(o[off:off + want.size].view(np.uint32), want.reshape(-1).view(np.uint32)), (d, off)
        assert (o[:off] == 7.0).all() and (o[off + want.size:] == 7.0).all()      # nothing written outside n x dim


# ---- 2. builds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 128])
def test_build_paths_store_the_augmented_rows(rq, oracle, case, d):
    """rq_build_ip, rq_build_device_ip, the streamed builder on shuffled uneven chunks, split rows and a tiered index: every array
    is the oracle's; a chunk with a row over the bound is refused."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    c = case(d)
    x, centres, P, oidx, k, S = c["x"], c["centres"], c["P"], c["oidx"], c["k"], c["S"]
    n, cc = x.shape[0], centres.shape[1]
    ax = im.augment_rows(oracle, x, S)
    g = rq.RaBitQ.build(x, centres, P, metric="ip")                  # automatic bound
    assert g.metric == "ip" and g.dim == c["dim"] and g.ip_params[0] == d and bits(g.ip_params[1]).tobytes() == bits(S).tobytes()
    same_arrays(g, oidx, "rq_build_ip")
    assert np.array_equal(bits(g.base), bits(ax[oidx.map_ids]))      # RQ_ARR_BASE returns the augmented rows
    l2 = rq.RaBitQ.build(ax, im.pad_cols(centres, c["dim"]), P)      # the L2 twin: same arrays, same rq_info but the metric
    same_arrays(l2, oidx, "twin")
    assert (g.n, g.k, g.dim, g.max_list_len, g.n_hbm, g.split_rows) == (l2.n, l2.k, l2.dim, l2.max_list_len, l2.n_hbm, l2.split_rows)
    g.close(), l2.close()
    g = rq.RaBitQ.build(x, centres, P, metric="ip", max_sq_norm=float(S))
    same_arrays(g, oidx, "rq_build_ip, given bound")
    g.close()
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(centres).to(dev)
    torch.cuda.synchronize()
    g = rq.RaBitQ.build_device(xd.data_ptr(), n, d, cd.data_ptr(), k, P, metric="ip", centroid_cols=cc)
    same_arrays(g, oidx, "rq_build_device_ip")
    g.close()
    # the streamed builder: shuffled chunks of uneven size, the bound from rq_row_sqnorm_max_device over the chunks
    rng = np.random.default_rng(d)
    cuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n), size=6, replace=False)), [n]])
    chunks = [(int(a), int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])]
    bound = max(rq.ops.row_sqnorm_max_device(xd[i0:i0 + m].data_ptr(), m, d) for i0, m in chunks)
    assert bits(bound).tobytes() == bits(S).tobytes()
    b = rq.RaBitQ.builder(n, d, cd.data_ptr(), k, P, metric="ip", max_sq_norm=bound, centroid_cols=cc)
    for j in rng.permutation(len(chunks)):
        b.assign_chunk(xd[chunks[j][0]:].data_ptr(), *chunks[j])
    b.order()
    for j in rng.permutation(len(chunks)):
        b.place_chunk(xd[chunks[j][0]:].data_ptr(), *chunks[j])
    g = b.finish()
    assert g.metric == "ip"
    same_arrays(g, oidx, "streamed builder")
    g.close()
    with pytest.raises(rq.RabitqError) as e:                          # no automatic mode
        rq.RaBitQ.builder(n, d, cd.data_ptr(), k, P, metric="ip", centroid_cols=cc)
    assert e.value.status == -1
    top = int(im.sqnorms(oracle, x).argmax())
    b = rq.RaBitQ.builder(n, d, cd.data_ptr(), k, P, metric="ip", max_sq_norm=float(np.nextafter(S, F32(0))), centroid_cols=cc)
    i0, m = next(ch for ch in chunks if ch[0] <= top < ch[0] + ch[1])
    with pytest.raises(rq.RabitqError) as e:
        b.assign_chunk(xd[i0:].data_ptr(), i0, m)
    assert e.value.status == -1 and f"row {top}:" in str(e.value)
    for call in (lambda: b.assign_chunk(xd.data_ptr(), 0, chunks[0][1]), b.order):   # a refused builder can only be freed
        with pytest.raises(rq.RabitqError) as e:
            call()
        assert e.value.status == -1
    del b
    want = oracle_answers(oracle, oidx, c["qq"][:300], 6, 10, False)
    try:
        ix.set_option("base_device_mb", max(1, (n * c["dim"] * 4 * 4 // 5) >> 20))
        g = rq.RaBitQ.build(x, centres, P, metric="ip")
        assert g.n_hbm < g.n, (g.n_hbm, g.n)
        same_arrays(g, oidx, "tiered")
        check_topk(rq, g, c["q"][:300], want, 6, 10, False, "tiered")
        g.close()
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 2)
        g = rq.RaBitQ.build(x, centres, P, metric="ip")
        assert g.split_rows and g.n_hbm == g.n
        same_arrays(g, oidx, "split_rows 2")
        check_topk(rq, g, c["q"][:300], want, 6, 10, False, "split rows")
        g.close()
    finally:
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)


def test_d768_generic_width(rq, oracle):
    """3 000 x 768: dim 832, the generic-width scan."""
    x, centres = raw_rows(3000, 768, 8, seed=41)
    P = synth.random_orthogonal(832, seed=42)
    q, _ = raw_rows(70, 768, 8, seed=43)
    S = im.auto_bound(oracle, x)
    oidx = im.ip_oracle(oracle, x, centres, P, S)
    g = rq.RaBitQ.build(x, centres, P, metric="ip")
    assert g.dim == 832
    same_arrays(g, oidx, "d768")
    qq = im.pad_cols(q, 832)
    for m in (1, 70):
        for heur in (False, True):
            check_topk(rq, g, q[:m], oracle_answers(oracle, oidx, qq[:m], 4, 10, heur), 4, 10, heur, ("d768", m, heur))
    g.close(), oidx.close()


# ---- 3. queries --------------------------------------------------------------------------------------------------------
_GBIG = {}


@pytest.fixture(scope="module")
def gbig(rq, case):
    def get(d):
        if d not in _GBIG:
            c = case(d)
            _GBIG[d] = rq.RaBitQ.build(c["x"], c["centres"], c["P"], metric="ip")
        return _GBIG[d]
    yield get
    for g in _GBIG.values():
        g.close()
    _GBIG.clear()


@pytest.mark.parametrize("d,heur", [(128, False), (128, True), (100, False), (100, True)])
def test_query_batches_against_the_ip_oracle(rq, oracle, case, gbig, d, heur):
    from rabitq_amd import index as ix
    c, g = case(d), gbig(d)
    probe, topk = 6, 10
    sizes = (1, 64, 300, 4096) if d == 128 else (1, 64, 300)
    want_all = oracle_answers(oracle, c["oidx"], c["qq"][:sizes[-1]], probe, topk, heur)

    def cut(m):   # (the oracle's counters are per call: recount for a prefix)
        return want_all if m == len(want_all[0]) else oracle_answers(oracle, c["oidx"], c["qq"][:m], probe, topk, heur)

    for m in sizes[:3]:
        check_topk(rq, g, c["q"][:m], cut(m), probe, topk, heur, (d, m))
    if d == 128:
        try:
            for impl in (1, 2):
                ix.set_option("scan_impl", impl)
                check_topk(rq, g, c["q"], want_all, probe, topk, heur, (d, 4096, impl))
        finally:
            ix.set_option("scan_impl", 0)
    for bad in (d - 1, d + 1, c["dim"]):                              # exactly d floats, nothing else
        with pytest.raises(rq.RabitqError) as e:
            g.query_batch(np.zeros((3, bad), F32), probe, topk, heur)
        assert e.value.status == -2, bad


# ---- 4. features -------------------------------------------------------------------------------------------------------
def test_filter_ticket_and_range(rq, oracle, case, gbig):
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    c, g = case(128), gbig(128)
    probe, topk, m, d = 6, 10, 300, 128
    q, qq, oidx, S = c["q"][:m], c["qq"][:m], c["oidx"], c["S"]
    allowed = np.random.default_rng(7).random(g.n) < 0.1
    ov = oracle.OracleIndex.view(oidx.dim, *sub_arrays(oidx, allowed))
    with g.make_filter(mask=allowed) as filt:
        for heur in (False, True):
            check_topk(rq, g, q, oracle_answers(oracle, ov, qq, probe, topk, heur), probe, topk, heur, ("filtered", heur), filter=filt)
            want40 = oracle_answers(oracle, ov, qq[:40], probe, topk, heur)
            try:
                for v in (0, 2):                                     # the staged path, and the few-launch path wherever the shape allows
                    ix.set_option("small_batch_filtered", v)
                    check_topk(rq, g, q[:40], want40, probe, topk, heur, ("filtered small", heur, v), filter=filt)
            finally:
                ix.set_option("small_batch_filtered", 1)
        # (dim 192 has no small-batch path: the d = 100 index, dim 128, takes the filtered few-launch path)
        c1, g1 = case(100), gbig(100)
        al1 = np.random.default_rng(8).random(g1.n) < 0.1
        ov1 = oracle.OracleIndex.view(c1["oidx"].dim, *sub_arrays(c1["oidx"], al1))
        with g1.make_filter(mask=al1) as f1:
            try:
                for v in (0, 2):
                    ix.set_option("small_batch_filtered", v)
                    pr = check_topk(rq, g1, c1["q"][:40], oracle_answers(oracle, ov1, c1["qq"][:40], probe, topk, False), probe, topk, False,
                                    ("filtered small, dim 128", v), filter=f1)
                    assert (pr["small_batch_passes"] > 0) == (v == 2), (v, pr)
            finally:
                ix.set_option("small_batch_filtered", 1)
        ov1.close()
        # range: "inner product above min_ip", radii from rq_ip_radius_device
        d10, i10, n10 = g.query_batch(q, probe, topk)
        assert (n10 == topk).all()
        ip10 = im.ip_from_dist(oracle, S, q, d10)
        min_ip = (ip10.min(axis=1) * np.array([1.1, 1.0, 0.8, 0.5], F32)[np.arange(m) % 4]).astype(F32)
        want_r = im.ip_radius(oracle, S, q, min_ip)
        qd, md, rd = torch.from_numpy(q).to(dev), torch.from_numpy(min_ip).to(dev), torch.zeros(m, device=dev)
        torch.cuda.synchronize()
        rq._lib.check(rq._lib.lib().rq_ip_radius_device(g._h, qd.data_ptr(), m, d, md.data_ptr(), rd.data_ptr()))
        radii = rd.cpu().numpy()
        assert np.array_equal(bits(radii), bits(want_r)) and np.array_equal(bits(g.ip_radius(q, min_ip)), bits(want_r))
        ref = Ref(oracle, oidx)
        for mm in (1, 40, m):
            want = ref.answer(qq[:mm], probe, radii[:mm])
            got, met, _ = run_range(rq, g, q[:mm], probe, radii[:mm])
            same_range(got, want[:3], ("range", mm))
            assert (met["rough"], met["precise"], met["query"]) == (want[3]["rough"], want[3]["precise"], mm)
        assert want[0][-1] > 300
        got = g.range_search(q, probe, min_ip=min_ip)                # the Python keyword
        same_range(got, want[:3], "range, min_ip=")
        wantf = Ref(oracle, ov).answer(qq, probe, radii)
        got, met, _ = run_range(rq, g, q, probe, radii, filter=filt)
        same_range(got, wantf[:3], "range filtered")
        # tickets: two plain batches in flight, then a filtered one
        want = oracle_answers(oracle, oidx, qq, probe, topk, False)
        wantf = oracle_answers(oracle, ov, qq, probe, topk, False)
        qds = [qd, torch.from_numpy(np.ascontiguousarray(q[::-1])).to(dev), qd]
        outs = [(torch.empty((m, topk), device=dev), torch.zeros((m, topk), device=dev, dtype=torch.int32), torch.zeros(m, device=dev, dtype=torch.int32))
                for _ in qds]
        torch.cuda.synchronize()
        rq.metrics_reset()
        tickets = [g.query_batch_device_begin(t.data_ptr(), m, d, probe, topk, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                              filter=(filt if j == 2 else None)) for j, (t, o) in enumerate(zip(qds, outs))]
        for t in tickets:
            g.query_batch_device_end(t)
        met = rq.metrics()
        assert (met["rough"], met["precise"], met["query"]) == (2 * want[1] + wantf[1], 2 * want[2] + wantf[2], 3 * m)
        for o, order, w in zip(outs, (np.arange(m), np.arange(m)[::-1], np.arange(m)), (want, want, wantf)):
            gd, gi, gn = o[0].cpu().numpy(), o[1].cpu().numpy().view(np.uint32), o[2].cpu().numpy()
            for b, src in enumerate(order):
                od, oi = w[0][src]
                assert gn[b] == oi.size and np.array_equal(gi[b, :oi.size], oi) and np.array_equal(bits(gd[b, :oi.size]), bits(od)), b
    ov.close()


def test_add_remove_equal_a_fresh_ip_build(rq, oracle):
    n, d, k, probe, topk = 6000, 128, 12, 4, 10
    pool, centres = raw_rows(n + 3000, d, k, seed=51)
    P = synth.random_orthogonal(im.ip_dim(d), seed=52)
    q, _ = raw_rows(120, d, k, seed=53)
    qq = im.pad_cols(q, im.ip_dim(d))
    S = im.auto_bound(oracle, pool)                                  # the bound of everything that will ever be added
    g = rq.RaBitQ.build(pool[:n], centres, P, metric="ip", max_sq_norm=float(S))
    live = Live(np.arange(n), pool[:n])
    rng = np.random.default_rng(54)

    def check(what):
        ids, rows = live.sorted()
        o = im.ip_oracle(oracle, rows, centres, P, S)
        try:
            assert g.metric == "ip" and (g.n, g.k) == (o.n, o.k) and bits(g.ip_params[1]).tobytes() == bits(S).tobytes(), what
            for name in ARRAYS:
                assert np.array_equal(bits(getattr(g, name)), bits(getattr(o, name))), (what, name)
            assert np.array_equal(g.map_ids, ids[o.map_ids]), what
            for heur in (False, True):
                check_topk(rq, g, q, oracle_answers(oracle, o, qq, probe, topk, heur, ids=ids), probe, topk, heur, (what, heur))
        finally:
            o.close()

    got = g.add(pool[n:n + 1500])
    live.add(got, pool[n:n + 1500])
    check("add 1500")
    drop = rng.choice(n + 1500, size=2000, replace=False)
    assert g.remove(ids=drop) == 2000
    live.remove(drop)
    check("remove 2000")
    # one row over the bound: RQ_ERR_INVALID, every array unchanged
    before = {name: getattr(g, name).copy() for name in ARRAYS + ("map_ids",)}
    over = pool[n + 1500:n + 1600].copy()
    over[37] = pool[int(im.sqnorms(oracle, pool).argmax())] * F32(1.001)
    for rows in (over, np.where(np.arange(100)[:, None] == 3, np.nan, over[:, :]).astype(F32)):
        with pytest.raises(rq.RabitqError) as e:
            g.add(np.ascontiguousarray(rows))
        assert e.value.status == -1
    assert "row 3 " in str(e.value)
    for name, a in before.items():
        assert np.array_equal(bits(getattr(g, name)), bits(a)), name
    with pytest.raises(rq.RabitqError) as e:                          # rows of the index's own d, not of its dim
        g.add(np.zeros((2, g.dim), F32))
    assert e.value.status == -2
    import torch
    rows = torch.from_numpy(pool[n + 1500:n + 3000]).to(torch.device("cuda", 0))   # device rows, explicit ids (some re-used)
    new_ids = np.concatenate([drop[:700], np.arange(20_000, 20_800)]).astype(np.uint32)
    rng.shuffle(new_ids)
    idd = torch.from_numpy(new_ids.view(np.int32)).to(rows.device)
    torch.cuda.synchronize()
    g.add_device(rows.data_ptr(), 1500, d, idd.data_ptr())
    live.add(new_ids, pool[n + 1500:n + 3000])
    check("add_device 1500 with ids")
    g.close()


def test_round_trips_from_arrays_and_shards(rq, oracle, tmp_path):
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    d, dim, k, probe, topk = 100, 128, 6, 3, 10
    x, centres = raw_rows(3000, d, k, seed=61)
    P = synth.random_orthogonal(dim, seed=62)
    q, _ = raw_rows(80, d, k, seed=63)
    g = rq.RaBitQ.build(x, centres, P, metric="ip")
    S = im.auto_bound(oracle, x)
    twin = rq.RaBitQ.build(im.augment_rows(oracle, x, S), im.pad_cols(centres, dim), P)
    want = g.query_batch(q, probe, topk)
    tw = twin.query_batch(im.pad_cols(q, dim), probe, topk)
    same_answers(want, tw, "twin")

    def same_index(h, what):
        assert h.metric == "ip" and h.ip_params[0] == d and bits(h.ip_params[1]).tobytes() == bits(S).tobytes(), what
        for name in ARRAYS + ("map_ids",):
            assert np.array_equal(bits(getattr(h, name)), bits(getattr(g, name))), (what, name)
        got = h.query_batch(q, probe, topk)
        same_answers(got, want, what)

    g.dump_to_dir(str(tmp_path / "ip"))
    twin.dump_to_dir(str(tmp_path / "l2"))
    assert sorted(os.listdir(tmp_path / "ip")) == sorted(FILES + ["metric"]) and sorted(os.listdir(tmp_path / "l2")) == FILES
    assert open(tmp_path / "ip" / "metric", "rb").read() == b"ip %d %08x\n" % (d, int(np.float32(S).view(np.uint32)))
    for f in FILES:                                                  # the dump of the L2 index of the augmented rows, byte for byte
        assert open(tmp_path / "ip" / f, "rb").read() == open(tmp_path / "l2" / f, "rb").read(), f
    g.dump_to_json(str(tmp_path / "ip.json"))
    text = open(tmp_path / "ip.json").read()
    assert '"metric":"ip","ip_d":100,"ip_sq_bound_bits":%d' % int(np.float32(S).view(np.uint32)) in text
    for load, path in ((rq.RaBitQ.load_from_dir, tmp_path / "ip"), (rq.RaBitQ.load_from_json, tmp_path / "ip.json")):
        h = load(str(path))
        same_index(h, path)
        h.close()
    for text in ("ip\n", "ip 100\n", "ip 100 4\n", "ip 100 zzzzzzzz\n", "ip 63 %08x\n" % int(np.float32(S).view(np.uint32)), "ip 100 7f800000\n", "dot\n"):
        open(tmp_path / "ip" / "metric", "w").write(text)            # malformed content: RQ_ERR_IO
        with pytest.raises(rq.RabitqError) as e:
            rq.RaBitQ.load_from_dir(str(tmp_path / "ip"))
        assert e.value.status == -3, text
    # rq_from_arrays_ip takes the arrays as they are; without max_sq_norm the *_metric entry still refuses id 2
    h = rq.RaBitQ.from_arrays(g.base, g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors, metric="ip", max_sq_norm=S, d=d)
    same_index(h, "from_arrays")
    h.close()
    with pytest.raises(rq.RabitqError) as e:
        rq.RaBitQ.from_arrays(g.base, g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors, metric="ip")
    assert e.value.status == -1 and "_ip" in str(e.value)
    with pytest.raises(rq.RabitqError) as e:
        rq.RaBitQ.from_arrays(g.base, g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors, metric="ip", max_sq_norm=S, d=63)
    assert e.value.status == -2
    with pytest.raises(rq.RabitqError) as e:
        twin.ip_params
    assert e.value.status == -1
    # shards of a 2-way partition: each is an IP index with d and S, equal to the twin's shard; merged on the host they give the
    # whole index's ids, by the rule of tests/test_sharded_gpu.py (a shard's own thresholds are looser than the single sequential
    # one, so a shard may return a true neighbour that the single index's gate skipped: at most 2 % of the ids may differ)
    owner, _ = g.partition_lists(2)
    parts = []
    for r in (0, 1):
        sh, ts = g.shard(owner, r), twin.shard(owner, r)
        assert sh.metric == "ip" and sh.ip_params[0] == d and bits(sh.ip_params[1]).tobytes() == bits(S).tobytes() and ts.metric == "l2"
        a, b = sh.query_batch(q, probe, topk), ts.query_batch(im.pad_cols(q, dim), probe, topk)
        same_answers(a, b, ("shard", r))                             # (a query whose probed lists all live on the other shard: count 0)
        parts.append(a)
        sh.close(), ts.close()
    diff = 0
    for b in range(q.shape[0]):
        dd = np.concatenate([p[0][b, :p[2][b]] for p in parts])
        ii = np.concatenate([p[1][b, :p[2][b]] for p in parts])
        order = np.lexsort((ii, dd))[:topk]
        n = int(want[2][b])
        assert order.size == n, b
        diff += len(set(ii[order].tolist()) - set(want[1][b, :n].tolist()))
    assert diff / (q.shape[0] * topk) <= 0.02, diff
    # the world-1 sharded step with the shared-threshold path forced == the twin's
    m = q.shape[0]
    res = []
    try:
        ix.set_option("shared_thresholds", 2)
        for idx, queries, length in ((g, q, d), (twin, im.pad_cols(q, dim), dim)):
            qd = torch.from_numpy(np.ascontiguousarray(queries)).to(dev)
            od, oi, on = torch.full((m, topk), -1.0, device=dev), torch.zeros((m, topk), device=dev, dtype=torch.int32), torch.zeros(m, device=dev, dtype=torch.int32)
            torch.cuda.synchronize()
            rq.metrics_reset()
            idx.query_batch_sharded_device(0, 1, 1000, qd.data_ptr(), m, length, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
            met = rq.metrics()
            res.append((od.cpu().numpy(), oi.cpu().numpy(), on.cpu().numpy(), (met["rough"], met["precise"], met["query"])))
    finally:
        ix.set_option("shared_thresholds", 1)
    a, b = res
    assert np.array_equal(a[2], b[2]) and a[3] == b[3]
    for r in range(m):
        n = int(a[2][r])
        assert np.array_equal(a[1][r, :n], b[1][r, :n]) and np.array_equal(bits(a[0][r, :n]), bits(b[0][r, :n])), r
        order = np.lexsort((want[1][r, :n], want[0][r, :n]))
        assert n == want[2][r] and np.array_equal(a[1][r, :n].view(np.uint32), want[1][r, :n][order] + 1000), r
    g.close(), twin.close()


# ---- 5. conversion -----------------------------------------------------------------------------------------------------
def test_ip_from_dist_bits(rq, oracle, case, gbig):
    import torch
    dev = torch.device("cuda", 0)
    c, g = case(100), gbig(100)
    m, topk = 300, 10
    q = c["q"][:m]
    with g.make_filter(mask=np.random.default_rng(3).random(g.n) < 0.002) as filt:       # some queries return fewer than topk
        dist, ids, cnt = g.query_batch(q, 6, topk, filter=filt)
    assert cnt.min() < topk
    want = im.ip_from_dist(oracle, c["S"], q, dist)
    want[np.arange(topk)[None, :] >= cnt[:, None]] = -np.inf
    assert np.array_equal(bits(g.inner_product(dist, q, cnt)), bits(want))
    full = g.inner_product(dist, q)
    live = np.arange(topk)[None, :] < cnt[:, None]
    assert np.array_equal(bits(full[live]), bits(want[live]))
    qd, dd, nd = torch.from_numpy(q).to(dev), torch.from_numpy(dist).to(dev), torch.from_numpy(cnt.astype(np.int32)).to(dev)
    out = torch.zeros((m, topk), device=dev)
    torch.cuda.synchronize()
    rq._lib.check(rq._lib.lib().rq_ip_from_dist_device(g._h, qd.data_ptr(), m, 100, dd.data_ptr(), topk, nd.data_ptr(), out.data_ptr()))
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    L = rq._lib.lib()
    assert L.rq_ip_from_dist_device(g._h, qd.data_ptr(), m, 101, dd.data_ptr(), topk, nd.data_ptr(), out.data_ptr()) == -2


# ---- 6. meaning --------------------------------------------------------------------------------------------------------
def test_meaning_against_float64(rq, oracle, case, gbig):
    """Each returned inner product against float64 <x, q> computed from the ORIGINAL rows.
    ip = 0.5 * ((S + s_q) - D).  Against the exact value <x, q> = 0.5 * (|A|^2 + |q|^2 - D_exact) on the stored f32 rows:
      * D: the f32 rerank is within rtol 1e-5 of D_exact (the relative tolerance of the f64 checks in tests/test_gpu_parity.py);
      * S stands for |A|^2: off by at most aug_sq_error_bound(dim) * S (tests/ip_model.py, from the chain length dim/8 + 3);
      * s_q stands for |q|^2: off by at most sq_error_bound(dim) * s_q (the same chain);
      * the conversion's own three f32 roundings (S + s_q, the subtraction, the halving is exact): each at most 2^-24 of an
        operand no larger than max(S + s_q, D) <= S + s_q + D.
    So |ip - <x, q>| <= 0.5 * (1e-5 * D + aug * S + sq * s_q + 2 * 2^-24 * (S + s_q + D))."""
    c, g = case(128), gbig(128)
    dim, S = g.dim, float(c["S"])
    q = c["q"][:1000]
    x64, q64 = c["x"].astype(np.float64), q.astype(np.float64)
    d, ids, cnt = g.query_batch(q, 6, 10)
    assert (cnt == 10).all()
    ip = g.inner_product(d, q, cnt).astype(np.float64)
    want = np.einsum("bkd,bd->bk", x64[ids.astype(np.int64)], q64)
    sq = (q64 ** 2).sum(axis=1)[:, None]
    D = d.astype(np.float64)
    tol = 0.5 * (1e-5 * D + im.aug_sq_error_bound(dim) * S + im.sq_error_bound(dim) * sq + 2 * 2.0 ** -24 * (S + sq + D))
    err = np.abs(ip - want)
    print("meaning: max abs err", err.max(), "max err / tol", (err / tol).max(), "S", S)
    assert (err <= tol).all()


# ---- 7. planted rows ---------------------------------------------------------------------------------------------------
def test_direction_planted_rows_through_the_engine(rq, oracle):
    x, centres, P, q, planted = planted_case()
    g = rq.RaBitQ.build(x, centres, P, metric="ip")
    for heur in (False, True):
        d, ids, cnt = g.query_batch(q, 8, 10, heur)
        first = np.array([ids[b, :cnt[b]][np.lexsort((ids[b, :cnt[b]], d[b, :cnt[b]]))[0]] for b in range(q.shape[0])])
        assert np.array_equal(first, planted), heur
        if heur:
            assert np.array_equal(ids[:, 0], planted)
    g.close()
