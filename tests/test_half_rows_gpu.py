"""Half-precision rows (RQ_ROWS_F16 / RQ_ROWS_BF16): indexes that store the caller's 2-byte elements as given.

The contract (include/rabitq_hip.h): a half-row L2 index of (h, centroids, P) equals, bit for bit, the L2 index of (W(h), centroids,
P) -- every array, rq_info, every query entry's ids, order, distance bits, counts, status and counters; a cosine index stores
R_t(N(W(h))) and equals the L2 index of W(R_t(N(W(h)))).  W and R_t are modelled in tests/half_model.py.  Every check is bit-exact.

Run on the GPU box:  python -m pytest tests/test_half_rows_gpu.py -m gpu -q
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import cosine_model as cm
from tests import half_model as hm
from tests import synth
from tests.models import ARRAYS, Ref, bits, run_range, same_range

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, IO, UNSUPPORTED = -1, -3, -6
PROBE = 8
FILES = ["base.fvecs", "centroids.fvecs", "factors.fvecs", "offsets_ids.ivecs", "orthogonal.fvecs", "x_binary_vec.u64vecs"]
F16_SHAPES = [(64, 3000, 8), (100, 5000, 16), (128, 20000, 32), (192, 5000, 16), (320, 3000, 8), (768, 3000, 8)]
BF16_SHAPES = [(100, 5000, 16), (128, 20000, 32)]
CASES = [("f16",) + s for s in F16_SHAPES] + [("bf16",) + s for s in BF16_SHAPES]
CASE_IDS = ["%s-d%d-n%d-k%d" % c for c in CASES]


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def _addr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def half_data(rows, n, d, k, seed):
    """synth.mixture rounded to the type, with injected rows: f16 subnormals, +-0, +-65504 (f16) / magnitudes up to 2^60 (bf16),
    magnitudes spread over the type's range, all with finite squared norms."""
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=seed, centre_scale=0.6)
    rng = np.random.default_rng(seed + 500)
    at = rng.choice(n, size=12, replace=False)
    x[at[0]] = 0.0
    x[at[1]] = -0.0
    x[at[2], ::2] = -0.0
    big = 65504.0 if rows == "f16" else 2.0 ** 60          # (d * big^2 stays finite in f32 for both)
    x[at[3]] = big
    x[at[4]] = -big
    x[at[5], : d // 2] = big
    spread = np.exp2(rng.integers(-14 if rows == "f16" else -100, 15 if rows == "f16" else 50, size=(3, d))).astype(F32)
    x[at[6:9]] = spread * rng.choice([-1.0, 1.0], size=(3, d)).astype(F32)
    h = hm.narrow(x, rows)
    if rows == "f16":   # subnormal elements: patterns 0x0001 .. 0x03FF with either sign
        h[at[9:12]] = (rng.integers(1, 0x400, size=(3, d)) | (rng.integers(0, 2, size=(3, d)) << 15)).astype(np.uint16)
    else:               # values far below the f16 range, and f32-subnormal ones (bf16 holds them)
        h[at[9:12]] = (rng.integers(1, 0x0100, size=(3, d)) | (rng.integers(0, 2, size=(3, d)) << 15)).astype(np.uint16)
    return np.ascontiguousarray(h), np.ascontiguousarray(centres)


def typed(h, rows):
    """bit patterns -> what RaBitQ.build takes for the type."""
    return h.view(np.float16) if rows == "f16" else h


_WORLD = {}


@pytest.fixture(scope="module")
def world(rq, oracle):
    """case -> the half index, the oracle of W(h), the data; built on first use, shared by the tests of the module."""
    def get(case):
        if case not in _WORLD:
            rows, d, n, k = case
            h, centres = half_data(rows, n, d, k, seed=71 + d)
            dim = (d + 63) // 64 * 64
            P = synth.random_orthogonal(dim, seed=72)
            wx = hm.widen(h, rows)
            q, _, _ = synth.mixture(1024 if d == 128 else 300, d, k, sigma=0.7, seed=73 + d, centre_scale=0.6)
            gidx = rq.RaBitQ.build(typed(h, rows), centres, P, rows=rows)
            oidx = oracle.OracleIndex.build(wx, centres, P)
            _WORLD[case] = dict(rows=rows, d=d, n=n, k=k, dim=dim, h=h, wx=wx, centres=centres, P=P, q=np.ascontiguousarray(q), gidx=gidx, oidx=oidx)
        return _WORLD[case]
    yield get
    for c in _WORLD.values():
        c["gidx"].close()
        c["oidx"].close()
        if "twin" in c:
            c["twin"].close()
    _WORLD.clear()


def twin_of(rq, c):
    """The f32 GPU index of W(h) with the same centroids and P."""
    if "twin" not in c:
        c["twin"] = rq.RaBitQ.build(c["wx"], c["centres"], c["P"])
    return c["twin"]


def same_arrays(g, o, what=""):
    assert (g.n, g.k, g.dim) == (o.n, o.k, o.dim), what
    for name in ARRAYS + ("map_ids",):
        assert np.array_equal(bits(getattr(g, name)), bits(getattr(o, name))), (what, name)


def info_tuple(g):
    return (g.dim, g.k, g.n, g.max_list_len, g.n_hbm, g.split_rows, g.metric)


# ---- 1. rq_widen_device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", hm.TYPES)
def test_widen_device_all_patterns(rq, rows):
    import torch
    from rabitq_amd import _lib
    L = _lib.lib()
    h = np.arange(65536, dtype=np.uint16)
    want, nan = hm.widen(h, rows), hm.nan_patterns(rows)
    dh = torch.from_numpy(h.view(np.int16)).cuda()
    out = torch.zeros(65536, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.rq_widen_device(C.c_void_p(dh.data_ptr()), _lib.row_type_id(rows), 65536, C.c_void_p(out.data_ptr())))
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.isnan(got[nan]).all()
    if rows == "bf16":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # an odd count from a pointer that is only 2-byte aligned; nothing is written past the count
    h2 = np.concatenate([h, h[:5]])
    d2 = torch.from_numpy(h2.view(np.int16)).cuda()
    out2 = torch.full((65539 + 8,), -7.0, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.rq_widen_device(C.c_void_p(d2.data_ptr() + 2), _lib.row_type_id(rows), 65539, C.c_void_p(out2.data_ptr())))
    got2 = out2.cpu().numpy()
    w2, n2 = hm.widen(h2[1:65540], rows), np.isnan(hm.widen(h2[1:65540], rows))
    assert np.array_equal(got2[:65539].view(np.uint32)[~n2], w2.view(np.uint32)[~n2]) and np.isnan(got2[:65539][n2]).all()
    assert (got2[65539:] == -7.0).all()
    # the host form, through the package
    assert np.array_equal(rq.widen(typed(h, rows), rows=rows).view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert L.rq_widen_device(C.c_void_p(dh.data_ptr()), 0, 4, C.c_void_p(out.data_ptr())) == INVALID


# ---- 2. build parity against the oracle of W(h) -----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_build_equals_the_oracle_of_widened_rows(rq, world, case):
    c = world(case)
    g, o = c["gidx"], c["oidx"]
    same_arrays(g, o, case)                                   # (base: RQ_ARR_BASE == W(h) in cluster order, zero-padded)
    assert g.row_type == c["rows"]
    assert (g.n_hbm, g.split_rows, g.metric) == (c["n"], False, "l2")
    stored = g.base_rows
    assert stored.dtype == hm.NP_DTYPE[c["rows"]] and stored.shape == (c["n"], c["dim"])
    want = hm.pad_bits(c["h"], c["dim"])[g.map_ids]           # the raw bits, cluster order, padding 0x0000
    assert np.array_equal(hm.as_bits(stored), want)
    assert np.array_equal(bits(g.base), bits(hm.widen(want, c["rows"])))
    t = twin_of(rq, c)
    assert info_tuple(g) == info_tuple(t) and t.row_type == "f32"


# ---- 3. query parity against the oracle, both rerank routes ------------------------------------------------------------
def oracle_answers(oracle, oidx, queries, probe, topk, heur):
    out = []
    for q in queries:
        oracle.metrics_reset()
        try:
            od, oi = oidx.query(q, probe, topk, heur)
        except Exception:
            od, oi = np.zeros(0, F32), np.zeros(0, np.uint32)
        m = oracle.metrics()
        out.append((od, oi, m["rough"], m["precise"]))
    return out


def check_topk(rq, gidx, queries, ans, probe, topk, heur, what):
    from rabitq_amd import index as ix
    rq.metrics_reset()
    d, gids, cnt = gidx.query_batch(queries, probe, topk, heur)
    m = rq.metrics()
    for b, (od, oi, _, _) in enumerate(ans):
        n = int(cnt[b])
        assert n == oi.size, (what, b, n, oi.size)
        assert np.array_equal(gids[b, :n], oi), (what, b)
        assert np.array_equal(bits(d[b, :n]), bits(od)), (what, b)
    assert (m["rough"], m["precise"], m["query"]) == (sum(a[2] for a in ans), sum(a[3] for a in ans), len(ans)), (what, m)
    return ix.last_profile()


@pytest.mark.parametrize("heur", [False, True], ids=["heap", "heuristic"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_queries_equal_the_oracle(rq, oracle, world, case, heur):
    c = world(case)
    sizes = (1, 64, 300, 1024) if c["d"] == 128 else (300,)
    for topk in (1, 10, 100):
        ans = oracle_answers(oracle, c["oidx"], c["q"][:max(sizes)], PROBE, topk, heur)
        for nq in sizes:
            prof = check_topk(rq, c["gidx"], c["q"][:nq], ans[:nq], PROBE, topk, heur, (case, heur, topk, nq))
            # nq <= 64: the small-batch path (sb_query_kernel / the finish kernels); nq >= 300: the staged launches (accurate_kernel<ROW_KIND_HALF>)
            assert (prof["small_batch_passes"] > 0) == (nq <= 64), (case, heur, topk, nq, prof["small_batch_passes"])
            assert prof["rerank_shadow_rejects"] == 0


# ---- 4. twins: the half index against the f32 GPU index of W(h) --------------------------------------------------------
def _same_answers(a, b, what):
    assert np.array_equal(a[2], b[2]), what
    for r in range(len(a[2])):
        n = int(a[2][r])
        assert np.array_equal(a[1][r, :n], b[1][r, :n]) and np.array_equal(bits(a[0][r, :n]), bits(b[0][r, :n])), (what, r)


def _counted(rq, f):
    rq.metrics_reset()
    out = f()
    m = rq.metrics()
    return out, (m["rough"], m["precise"], m["query"])


TWIN_CASES = [("f16", 128, 20000, 32), ("bf16", 128, 20000, 32), ("f16", 192, 5000, 16)]
TWIN_IDS = ["%s-d%d" % (c[0], c[1]) for c in TWIN_CASES]


@pytest.mark.parametrize("case", TWIN_CASES, ids=TWIN_IDS)
def test_twin_filtered_and_range(rq, world, case):
    c = world(case)
    g, t, q = c["gidx"], twin_of(rq, c), c["q"][:300]
    mask = np.random.default_rng(5).random(c["n"]) < 0.10
    with g.make_filter(mask=mask) as fg, t.make_filter(mask=mask) as ft:
        assert fg.rows == ft.rows
        for nq in (40, 300):
            a, ma = _counted(rq, lambda: g.query_batch(q[:nq], PROBE, 10, filter=fg))
            b, mb = _counted(rq, lambda: t.query_batch(q[:nq], PROBE, 10, filter=ft))
            _same_answers(a, b, (case, "filtered", nq))
            assert ma == mb
        d10 = t.query_batch(q, PROBE, 10)[0][:, :10]
        radius = F32(np.median(np.nanmax(d10, axis=1)))       # the median 10th-neighbour distance
        for f_g, f_t in ((None, None), (fg, ft)):
            got, mg, _ = run_range(rq, g, q[:100], PROBE, radius, filter=f_g)
            want, mt, _ = run_range(rq, t, q[:100], PROBE, radius, filter=f_t)
            same_range(got, want, (case, "range", f_g is not None))
            assert (mg["rough"], mg["precise"], mg["query"]) == (mt["rough"], mt["precise"], mt["query"])
            assert got[0][-1] > 0


def _device_batch(idx, q, topk, begin_only=False, **kw):
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nq = q.shape[0]
    out = (torch.full((nq, topk), float("nan"), device="cuda"), torch.zeros((nq, topk), device="cuda", dtype=torch.int32),
           torch.zeros(nq, device="cuda", dtype=torch.int32))
    torch.cuda.synchronize()
    return qd, out


def _host(out):
    return out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32), out[2].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", TWIN_CASES[:2], ids=TWIN_IDS[:2])
def test_twin_tickets_probed_seeded_rerank(rq, world, case):
    import torch
    c = world(case)
    g, t, q = c["gidx"], twin_of(rq, c), c["q"]
    nq, topk = 300, 10
    want = t.query_batch(q[:2 * nq], PROBE, topk)
    # two tickets in flight
    qa, oa = _device_batch(g, q[:nq], topk)
    qb, ob = _device_batch(g, q[nq:2 * nq], topk)
    ta = g.query_batch_device_begin(qa.data_ptr(), nq, c["d"], PROBE, topk, oa[0].data_ptr(), oa[1].data_ptr(), oa[2].data_ptr())
    tb = g.query_batch_device_begin(qb.data_ptr(), nq, c["d"], PROBE, topk, ob[0].data_ptr(), ob[1].data_ptr(), ob[2].data_ptr())
    g.query_batch_device_end(tb)
    g.query_batch_device_end(ta)
    _same_answers(_host(oa), tuple(w[:nq] for w in want), (case, "ticket a"))
    _same_answers(_host(ob), tuple(w[nq:2 * nq] for w in want), (case, "ticket b"))
    # probed and seeded: the probe lists of the coarse ranking, reversed so that the visiting order is the caller's
    _, cl, cd = rq.ops.coarse_rank(t, q[:nq], PROBE)
    cl, cd = np.ascontiguousarray(cl[:, ::-1]), np.ascontiguousarray(cd[:, ::-1])
    dcl, dcd = torch.from_numpy(cl.view(np.int32)).cuda(), torch.from_numpy(cd).cuda()
    thr = torch.from_numpy(np.ascontiguousarray(want[0][:nq, :topk].max(axis=1) * F32(1.5))).cuda()
    res = {}
    for name, idx in (("half", g), ("f32", t)):
        qd, o1 = _device_batch(idx, q[:nq], topk)
        _, o2 = _device_batch(idx, q[:nq], topk)
        rq.metrics_reset()
        idx.query_batch_device_probed(qd.data_ptr(), nq, c["d"], dcl.data_ptr(), dcd.data_ptr(), PROBE, topk, o1[0].data_ptr(), o1[1].data_ptr(), o1[2].data_ptr())
        idx.query_batch_device_seeded(qd.data_ptr(), nq, c["d"], dcl.data_ptr(), dcd.data_ptr(), PROBE, topk, thr.data_ptr(), o2[0].data_ptr(), o2[1].data_ptr(),
                                      o2[2].data_ptr(), heuristic_rank=True)
        m = rq.metrics()
        res[name] = (_host(o1), _host(o2), (m["rough"], m["precise"], m["query"]))
    _same_answers(res["half"][0], res["f32"][0], (case, "probed"))
    _same_answers(res["half"][1], res["f32"][1], (case, "seeded"))
    assert res["half"][2] == res["f32"][2]
    # rq_rerank: the exact distance of arbitrary positions (the padding of the last-but-one row included)
    pos = np.random.default_rng(9).integers(0, c["n"], 777).astype(np.uint32)
    qp = cm.pad64(q[:1])[0]
    assert np.array_equal(bits(rq.ops.rerank(g, qp, pos)), bits(rq.ops.rerank(t, qp, pos)))


@pytest.mark.parametrize("case", [("f16", 100, 5000, 16), ("bf16", 100, 5000, 16)], ids=["f16-d100", "bf16-d100"])
def test_twin_shards(rq, world, case):
    c = world(case)
    g, t, q = c["gidx"], twin_of(rq, c), c["q"][:300]
    owner, load = g.partition_lists(2)
    owner_t, load_t = t.partition_lists(2)
    assert np.array_equal(owner, owner_t) and np.array_equal(load, load_t)
    for rank in (0, 1):
        sg, st = g.shard(owner, rank), t.shard(owner, rank)
        try:
            assert sg.row_type == c["rows"] and st.row_type == "f32" and info_tuple(sg) == info_tuple(st)
            same_arrays(sg, st, (case, rank))
            assert np.array_equal(hm.as_bits(sg.base_rows), hm.pad_bits(c["h"], c["dim"])[sg.map_ids])
            for nq in (30, 300):
                a, ma = _counted(rq, lambda: sg.query_batch(q[:nq], PROBE, 10))
                b, mb = _counted(rq, lambda: st.query_batch(q[:nq], PROBE, 10))
                _same_answers(a, b, (case, rank, nq))
                assert ma == mb
        finally:
            sg.close()
            st.close()


# ---- 5. the streamed builder ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,metric", [("f16", "l2"), ("bf16", "l2"), ("f16", "cosine")])
def test_streamed_builder_equals_the_one_shot_build(rq, rows, metric):
    import torch
    from rabitq_amd import _lib
    L = _lib.lib()
    n, d, k = 5000, 100, 16
    h, centres = half_data(rows, n, d, k, seed=91)
    P = synth.random_orthogonal(128, seed=92)
    dh, dc = torch.from_numpy(h.view(np.int16)).cuda(), torch.from_numpy(centres).cuda()
    torch.cuda.synchronize()
    one = rq.RaBitQ.build_device(dh.data_ptr(), n, d, dc.data_ptr(), k, P, metric=metric, rows=rows)
    cuts = [0, 1, 700, 701, 2048, 3333, n]
    chunks = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)]
    b = rq.RaBitQ.builder(n, d, dc.data_ptr(), k, P, metric=metric, rows=rows)
    plain = rq.RaBitQ.builder(n, d, dc.data_ptr(), k, P, metric=metric)
    try:
        # a plain chunk call on a typed builder and a typed chunk call on a plain builder are refused (and leave them usable)
        assert L.rq_builder_assign_chunk(b._b, C.c_void_p(dh.data_ptr()), 0, 1) == INVALID
        assert L.rq_builder_assign_chunk_rows(plain._b, C.c_void_p(dh.data_ptr()), 0, 1) == INVALID
        for j in (3, 0, 5, 1, 4, 2):
            i0, m = chunks[j]
            b.assign_chunk(dh.data_ptr() + i0 * d * 2, i0, m)
        b.order()
        assert L.rq_builder_place_chunk(b._b, C.c_void_p(dh.data_ptr()), 0, 1) == INVALID
        for j in (2, 5, 0, 4, 3, 1):
            i0, m = chunks[j]
            b.place_chunk(dh.data_ptr() + i0 * d * 2, i0, m)
        st = b.stats()
        assert (st["rows_in_hbm"], st["rows_in_host_memory"]) == (n, 0)
        g = b.finish()
        try:
            assert g.row_type == rows and g.metric == metric
            same_arrays(g, one, (rows, metric))
            assert np.array_equal(hm.as_bits(g.base_rows), hm.as_bits(one.base_rows))
        finally:
            g.close()
    finally:
        one.close()
        del plain


# ---- 6. cosine -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 128])
@pytest.mark.parametrize("rows", hm.TYPES)
def test_cosine_equals_the_oracle_of_the_rounded_rows(rq, oracle, rows, d):
    n, k = 5000, 16
    h, centres = half_data(rows, n, d, k, seed=111 + d)
    centres = cm.normalize_rows(oracle, centres)[:, :d].copy()
    P = synth.random_orthogonal(128, seed=112)
    q, _, _ = synth.mixture(300, d, k, sigma=0.7, seed=113, centre_scale=0.6)
    g = rq.RaBitQ.build(typed(h, rows), centres, P, metric="cosine", rows=rows)
    o = oracle.OracleIndex.build(hm.cosine_l2_rows(oracle, h, rows), cm.pad64(centres), P)
    try:
        assert g.metric == "cosine" and g.row_type == rows
        same_arrays(g, o, (rows, d))
        stored = hm.cosine_stored_bits(oracle, h, rows)
        assert np.array_equal(hm.as_bits(g.base_rows), stored[g.map_ids])
        nq = cm.normalize_rows(oracle, q)
        for heur, topk, m in ((False, 10, 300), (True, 10, 300), (False, 10, 40)):
            ans = oracle_answers(oracle, o, nq[:m], PROBE, topk, heur)
            check_topk(rq, g, q[:m], ans, PROBE, topk, heur, (rows, d, heur, m))
    finally:
        g.close()
        o.close()


# ---- 7. persistence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,metric", [("f16", "l2"), ("bf16", "cosine")])
def test_dump_and_load(rq, tmp_path, rows, metric):
    from rabitq_amd import vecs
    n, d, k = 600, 100, 4
    h, centres = half_data(rows, n, d, k, seed=131)
    P = synth.random_orthogonal(128, seed=132)
    q, _, _ = synth.mixture(70, d, k, sigma=0.7, seed=133, centre_scale=0.6)
    g = rq.RaBitQ.build(typed(h, rows), centres, P, metric=metric, rows=rows)
    t = rq.RaBitQ.build(hm.widen(h, rows), centres, P)
    try:
        dg, dt = str(tmp_path / "half"), str(tmp_path / "f32")
        g.dump_to_dir(dg)
        t.dump_to_dir(dt)
        assert sorted(os.listdir(dg)) == sorted(FILES + ["rows"] + (["metric"] if metric == "cosine" else []))
        assert sorted(os.listdir(dt)) == sorted(FILES)                      # an f32 dump is unchanged: no `rows` file
        assert open(os.path.join(dg, "rows"), "rb").read() == (rows + "\n").encode()
        base = np.asarray(vecs.read_vecs(os.path.join(dg, "base.fvecs"), np.float32))
        assert np.array_equal(bits(base), bits(hm.widen(hm.as_bits(g.base_rows), rows)))
        if metric == "l2":
            for f in FILES:   # the reference loads the directory and answers as for the f32 index of W(h): the same files
                assert open(os.path.join(dg, f), "rb").read() == open(os.path.join(dt, f), "rb").read(), f
        g2 = rq.RaBitQ.load_from_dir(dg)
        try:
            assert g2.row_type == rows and g2.metric == metric
            same_arrays(g2, g, "load_dir")
            assert np.array_equal(hm.as_bits(g2.base_rows), hm.as_bits(g.base_rows))
            _same_answers(g2.query_batch(q, 3, 10), g.query_batch(q, 3, 10), "load_dir")
        finally:
            g2.close()
        jp = str(tmp_path / "half.json")
        g.dump_to_json(jp)
        assert json.load(open(jp))["rows"] == rows
        g3 = rq.RaBitQ.load_from_json(jp)
        try:
            assert g3.row_type == rows and g3.metric == metric
            same_arrays(g3, g, "load_json")
            assert np.array_equal(hm.as_bits(g3.base_rows), hm.as_bits(g.base_rows))
        finally:
            g3.close()
        jt = str(tmp_path / "f32.json")
        t.dump_to_json(jt)
        assert "rows" not in json.load(open(jt))
        # a directory whose `rows` says f16 but whose base.fvecs holds 0.1f, and one with an unknown text: RQ_ERR_IO
        from rabitq_amd import _lib
        L = _lib.lib()
        bad = t.base.copy()
        bad[n // 2, 3] = F32(0.1)
        vecs.write_vecs(os.path.join(dt, "base.fvecs"), bad)
        hnd = C.c_void_p()
        for text, want in (("f16\n", IO), ("fp8\n", IO), ("f16", IO)):
            open(os.path.join(dt, "rows"), "w").write(text)
            assert L.rq_load_dir(os.fsencode(dt), C.byref(hnd)) == want, text
            assert not hnd.value
    finally:
        g.close()
        t.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(rq, world):
    import torch
    from rabitq_amd import _lib
    from rabitq_amd import index as ix
    L = _lib.lib()
    c = world(("f16", 100, 5000, 16))
    g, h, centres, P, n, d, k = c["gidx"], c["h"], c["centres"], c["P"], c["n"], c["d"], c["k"]
    hnd = C.c_void_p()
    dh, dc = torch.from_numpy(h.view(np.int16)).cuda(), torch.from_numpy(centres).cuda()
    torch.cuda.synchronize()

    def build(metric, row_type):
        return L.rq_build_rows(_addr(h), n, d, _addr(centres), k, _addr(P), 0, metric, row_type, C.byref(hnd))
    # the inner-product metric with half rows; an unknown row type
    assert build(2, 1) == UNSUPPORTED and not hnd.value
    assert L.rq_build_device_rows(C.c_void_p(dh.data_ptr()), n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, 2, 2, C.byref(hnd)) == UNSUPPORTED
    assert L.rq_builder_create_rows(n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, 0, 2, 1, C.byref(hnd)) == UNSUPPORTED
    assert build(0, 3) == INVALID and not hnd.value
    assert L.rq_build_device_rows(C.c_void_p(dh.data_ptr()), n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, 0, 7, C.byref(hnd)) == INVALID
    assert L.rq_builder_create_rows(n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, 0, 0, 3, C.byref(hnd)) == INVALID
    arrays = [np.ascontiguousarray(a) for a in (hm.as_bits(g.base_rows), g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors)]
    assert L.rq_from_arrays_rows(g.dim, g.n, g.k, *[_addr(a) for a in arrays], 0, 3, C.byref(hnd)) == INVALID
    assert L.rq_from_arrays_rows(g.dim, g.n, g.k, *[_addr(a) for a in arrays], 2, 1, C.byref(hnd)) == UNSUPPORTED
    assert L.rq_from_arrays_rows(g.dim, g.n, g.k, *[_addr(a) for a in arrays], 0, 1, C.byref(hnd)) == 0
    g4 = rq.RaBitQ(hnd)
    try:
        same_arrays(g4, g, "from_arrays_rows")
        assert g4.row_type == "f16"
    finally:
        g4.close()
    # mutation: refused, index untouched
    before = g.query_batch(c["q"][:70], PROBE, 10)
    first, removed = C.c_uint32(), C.c_uint64()
    rowsf = np.ones((2, d), F32)
    assert L.rq_add(g._h, _addr(rowsf), 2, d, None, 0, C.cast(C.byref(first), C.c_void_p)) == UNSUPPORTED
    words, nbits = ix.pack_filter_bits(ids=[1, 2, 3])
    assert L.rq_remove(g._h, _addr(words), nbits, 0, C.cast(C.byref(removed), C.c_void_p)) == UNSUPPORTED
    g._refresh()
    assert g.n == n
    _same_answers(g.query_batch(c["q"][:70], PROBE, 10), before, "after refused mutations")
    same_arrays(g, c["oidx"], "after refused mutations")
    # the HBM budget: no tiers for half rows
    try:
        ix.set_option("base_device_mb", 1)                                # n * dim * 2 = 1.28 MB
        assert build(0, 1) == UNSUPPORTED and not hnd.value
    finally:
        ix.set_option("base_device_mb", -1)
    assert L.rq_builder_create_rows(n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, 1 << 20, 0, 1, C.byref(hnd)) == 0
    b = hnd.value
    try:
        assert L.rq_builder_assign_chunk_rows(C.c_void_p(b), C.c_void_p(dh.data_ptr()), 0, n) == 0
        assert L.rq_builder_order(C.c_void_p(b)) == UNSUPPORTED
    finally:
        L.rq_builder_free(C.c_void_p(b))
    # device pointers: the f32 array does not exist; the stored rows are n * dim * 2 bytes
    p, nbytes = C.c_void_p(), C.c_uint64()
    assert L.rq_get_device_ptr(g._h, ix.ARR_BASE, C.byref(p), C.byref(nbytes)) == UNSUPPORTED
    assert L.rq_get_device_ptr(g._h, ix.ARR_BASE_ROWS, C.byref(p), C.byref(nbytes)) == 0
    assert nbytes.value == n * c["dim"] * 2 and p.value
    t = twin_of(rq, c)
    assert L.rq_get_device_ptr(t._h, ix.ARR_BASE_ROWS, C.byref(p), C.byref(nbytes)) == INVALID
    buf = np.zeros(4, np.uint16)
    assert L.rq_get_array(t._h, ix.ARR_BASE_ROWS, _addr(buf), buf.nbytes) == INVALID
