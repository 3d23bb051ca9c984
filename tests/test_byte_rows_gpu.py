"""Byte rows (RQ_ROWS_U8 / RQ_ROWS_I8): indexes that store the caller's one-byte elements as given.

The contract (include/rabitq_hip.h): a byte-row L2 index of (b, centroids, P) equals, bit for bit, the f32 L2 index of (W(b),
centroids, P) -- every array, rq_info, every query entry's ids, order, distance bits, counts, status and counters.  W is modelled
in tests/byte_model.py, which also makes the data: integer rows with dense exact-distance ties.  Every check is bit-exact.

Run on the GPU box:  python -m pytest tests/test_byte_rows_gpu.py -m gpu -q
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import byte_model as bm
from tests import cosine_model as cm
from tests import synth
from tests.models import ARRAYS, bits, run_range, same_range

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, IO, UNSUPPORTED = -1, -3, -6
PROBE = 8
FILES = ["base.fvecs", "centroids.fvecs", "factors.fvecs", "offsets_ids.ivecs", "orthogonal.fvecs", "x_binary_vec.u64vecs"]
# every round structure of the byte rerank loop (dim = 64 x: 1 = tail 64; 2 = tail 128; 3 = 128 + 64; 4 = one round; 5 = round + 64;
# 7 = round + 128 + 64; 12 = three rounds)
U8_SHAPES = [(64, 3000, 8), (100, 5000, 16), (128, 20000, 32), (192, 5000, 16), (256, 3000, 8), (320, 3000, 8), (448, 3000, 8), (768, 3000, 8)]
I8_SHAPES = [(100, 5000, 16), (128, 20000, 32), (448, 3000, 8)]
CASES = [("u8",) + s for s in U8_SHAPES] + [("i8",) + s for s in I8_SHAPES]
CASE_IDS = ["%s-d%d-n%d-k%d" % c for c in CASES]
SB_WIDTHS = (1, 2, 4, 8, 12, 16)   # dim / 64 of the sb_query_kernel instantiations (kernel_shapes.h; tests/test_kernel_shapes.py compares): other widths have no small-batch path


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def _addr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


_WORLD = {}


@pytest.fixture(scope="module")
def world(rq, oracle):
    """case -> the byte index, the oracle of W(b), the data; built on first use, shared by the tests of the module."""
    def get(case):
        if case not in _WORLD:
            rows, d, n, k = case
            b, centres, marks = bm.byte_data(rows, n, d, k, seed=71 + d)
            dim = (d + 63) // 64 * 64
            P = synth.random_orthogonal(dim, seed=72)
            wx = bm.widen(b, rows)
            q = bm.byte_queries(rows, b, marks, 1024 if d == 128 else 300, d, k, seed=73 + d)
            gidx = rq.RaBitQ.build(b, centres, P, rows=rows)
            oidx = oracle.OracleIndex.build(wx, centres, P)
            _WORLD[case] = dict(rows=rows, d=d, n=n, k=k, dim=dim, b=b, wx=wx, centres=centres, P=P, q=q, marks=marks, gidx=gidx, oidx=oidx)
        return _WORLD[case]
    yield get
    for c in _WORLD.values():
        c["gidx"].close()
        c["oidx"].close()
        if "twin" in c:
            c["twin"].close()
    _WORLD.clear()


def twin_of(rq, c):
    """The f32 GPU index of W(b) with the same centroids and P."""
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
@pytest.mark.parametrize("rows", bm.TYPES)
def test_widen_device_all_patterns(rq, rows):
    import torch
    from rabitq_amd import _lib
    L = _lib.lib()
    rt = _lib.row_type_id(rows)
    pat = np.arange(256, dtype=np.uint8)
    want = bm.widen(pat, rows)
    dp = torch.from_numpy(pat).cuda()
    out = torch.zeros(256, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.rq_widen_device(C.c_void_p(dp.data_ptr()), rt, 256, C.c_void_p(out.data_ptr())))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # an odd count from a pointer offset by one byte; nothing is written past the count
    p2 = np.concatenate([pat, pat[:8]])
    d2 = torch.from_numpy(p2).cuda()
    out2 = torch.full((259 + 8,), -7.0, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.rq_widen_device(C.c_void_p(d2.data_ptr() + 1), rt, 259, C.c_void_p(out2.data_ptr())))
    got2 = out2.cpu().numpy()
    assert np.array_equal(got2[:259].view(np.uint32), bm.widen(p2[1:260], rows).view(np.uint32))
    assert (got2[259:] == -7.0).all()
    # the host form, through the package
    assert np.array_equal(rq.widen(bm.typed(pat, rows), rows=rows).view(np.uint32), want.view(np.uint32))
    for bad in (0, 3, 7):
        assert L.rq_widen_device(C.c_void_p(dp.data_ptr()), bad, 4, C.c_void_p(out.data_ptr())) == INVALID, bad
    # the array type must be the row type's
    with pytest.raises(TypeError):
        rq.widen(pat.astype(np.int16), rows=rows)


# ---- 2. build parity against the oracle of W(b) -----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_build_equals_the_oracle_of_widened_rows(rq, world, case):
    c = world(case)
    g, o = c["gidx"], c["oidx"]
    same_arrays(g, o, case)                                   # (base: RQ_ARR_BASE == W(b) in cluster order, zero-padded)
    assert g.row_type == c["rows"]
    assert (g.n_hbm, g.split_rows, g.metric) == (c["n"], False, "l2")
    stored = g.base_rows
    assert stored.dtype == bm.NP_DTYPE[c["rows"]] and stored.shape == (c["n"], c["dim"])
    want = bm.pad_bits(c["b"], c["dim"])[g.map_ids]           # the raw bytes, cluster order, padding 0x00
    assert np.array_equal(bm.as_bytes(stored), want)
    assert np.array_equal(bits(g.base), bits(bm.widen(want, c["rows"])))
    t = twin_of(rq, c)
    assert info_tuple(g) == info_tuple(t) and t.row_type == "f32"
    if case == CASES[0]:   # rows=None keeps its meaning: a uint8 array without rows= is converted to f32
        f = rq.RaBitQ.build(bm.as_bytes(c["b"]), c["centres"], c["P"])
        try:
            assert f.row_type == "f32"
            same_arrays(f, t, "uint8 without rows=")
        finally:
            f.close()


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
    large = 1024 if c["d"] == 128 else 300
    sizes = (1, 16, 64, large)
    for topk in (1, 10, 100):
        ans = oracle_answers(oracle, c["oidx"], c["q"][:large], PROBE, topk, heur)
        for nq in sizes:
            prof = check_topk(rq, c["gidx"], c["q"][:nq], ans[:nq], PROBE, topk, heur, (case, heur, topk, nq))
            # nq <= 64 at a width the small-batch kernels are instantiated for: the small-batch path; nq <= 64 at another width: one
            # fused launch per stage (stage_finish_kernel<*, ROW_KIND_BYTE> reranks); nq >= 300: the staged launches (accurate_kernel<ROW_KIND_BYTE>)
            assert (prof["small_batch_passes"] > 0) == (nq <= 64 and c["dim"] // 64 in SB_WIDTHS), (case, heur, topk, nq, prof["small_batch_passes"])
            assert prof["rerank_shadow_rejects"] == 0


# ---- 4. twins: the byte index against the f32 GPU index of W(b) --------------------------------------------------------
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


TWIN_CASES = [("u8", 128, 20000, 32), ("i8", 128, 20000, 32), ("u8", 192, 5000, 16), ("i8", 448, 3000, 8)]
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


def _device_batch(q, topk):
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
    qa, oa = _device_batch(q[:nq], topk)
    qb, ob = _device_batch(q[nq:2 * nq], topk)
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
    for name, idx in (("byte", g), ("f32", t)):
        qd, o1 = _device_batch(q[:nq], topk)
        _, o2 = _device_batch(q[:nq], topk)
        rq.metrics_reset()
        idx.query_batch_device_probed(qd.data_ptr(), nq, c["d"], dcl.data_ptr(), dcd.data_ptr(), PROBE, topk, o1[0].data_ptr(), o1[1].data_ptr(), o1[2].data_ptr())
        idx.query_batch_device_seeded(qd.data_ptr(), nq, c["d"], dcl.data_ptr(), dcd.data_ptr(), PROBE, topk, thr.data_ptr(), o2[0].data_ptr(), o2[1].data_ptr(),
                                      o2[2].data_ptr(), heuristic_rank=True)
        m = rq.metrics()
        res[name] = (_host(o1), _host(o2), (m["rough"], m["precise"], m["query"]))
    _same_answers(res["byte"][0], res["f32"][0], (case, "probed"))
    _same_answers(res["byte"][1], res["f32"][1], (case, "seeded"))
    assert res["byte"][2] == res["f32"][2]
    # rq_rerank: the exact distance of arbitrary positions, the last-but-one row and the last one included
    pos = np.random.default_rng(9).integers(0, c["n"], 777).astype(np.uint32)
    pos[:3] = (c["n"] - 2, c["n"] - 1, 0)
    qp = cm.pad64(q[:1])[0]
    assert np.array_equal(bits(rq.ops.rerank(g, qp, pos)), bits(rq.ops.rerank(t, qp, pos)))


@pytest.mark.parametrize("case", [("u8", 100, 5000, 16), ("i8", 100, 5000, 16)], ids=["u8-d100", "i8-d100"])
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
            assert np.array_equal(bm.as_bytes(sg.base_rows), bm.pad_bits(c["b"], c["dim"])[sg.map_ids])
            for nq in (30, 300):
                a, ma = _counted(rq, lambda: sg.query_batch(q[:nq], PROBE, 10))
                b, mb = _counted(rq, lambda: st.query_batch(q[:nq], PROBE, 10))
                _same_answers(a, b, (case, rank, nq))
                assert ma == mb
        finally:
            sg.close()
            st.close()


@pytest.mark.parametrize("rows", bm.TYPES)
def test_twin_sharded_step(rq, world, rows):
    """The sharded step behind the C ABI, one rank (no communicator), plain and with the shared-threshold path forced: the byte
    index against its f32 twin."""
    from rabitq_amd import index as ix
    c = world((rows, 100, 5000, 16))
    g, t, q = c["gidx"], twin_of(rq, c), c["q"][:120]
    nq, topk = q.shape[0], 10
    try:
        for shared in (1, 2):
            ix.set_option("shared_thresholds", shared)
            res = {}
            for name, idx in (("byte", g), ("f32", t)):
                qd, o = _device_batch(q, topk)
                rq.metrics_reset()
                idx.query_batch_sharded_device(0, 1, 1000, qd.data_ptr(), nq, c["d"], PROBE, topk, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
                m = rq.metrics()
                res[name] = (_host(o), (m["rough"], m["precise"], m["query"]))
            _same_answers(res["byte"][0], res["f32"][0], (rows, "sharded", shared))
            assert res["byte"][1] == res["f32"][1]
            assert (res["byte"][0][2] > 0).all()
    finally:
        ix.set_option("shared_thresholds", 1)


# ---- 5. the streamed builder ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", bm.TYPES)
def test_streamed_builder_equals_the_one_shot_build(rq, rows):
    import torch
    from rabitq_amd import _lib
    L = _lib.lib()
    n, d, k = 5000, 100, 16
    b, centres, _ = bm.byte_data(rows, n, d, k, seed=91)
    P = synth.random_orthogonal(128, seed=92)
    db, dc = torch.from_numpy(bm.as_bytes(b)).cuda(), torch.from_numpy(centres).cuda()
    torch.cuda.synchronize()
    one = rq.RaBitQ.build_device(db.data_ptr(), n, d, dc.data_ptr(), k, P, rows=rows)
    cuts = [0, 1, 700, 701, 2048, 3333, n]                     # (d = 100: chunks start at odd byte offsets too)
    chunks = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)]
    bld = rq.RaBitQ.builder(n, d, dc.data_ptr(), k, P, rows=rows)
    plain = rq.RaBitQ.builder(n, d, dc.data_ptr(), k, P)
    try:
        # a plain chunk call on a typed builder and a typed chunk call on a plain builder are refused (and leave them usable)
        assert L.rq_builder_assign_chunk(bld._b, C.c_void_p(db.data_ptr()), 0, 1) == INVALID
        assert L.rq_builder_assign_chunk_rows(plain._b, C.c_void_p(db.data_ptr()), 0, 1) == INVALID
        for j in (3, 0, 5, 1, 4, 2):
            i0, m = chunks[j]
            bld.assign_chunk(db.data_ptr() + i0 * d, i0, m)
        bld.order()
        assert L.rq_builder_place_chunk(bld._b, C.c_void_p(db.data_ptr()), 0, 1) == INVALID
        for j in (2, 5, 0, 4, 3, 1):
            i0, m = chunks[j]
            bld.place_chunk(db.data_ptr() + i0 * d, i0, m)
        st = bld.stats()
        assert (st["rows_in_hbm"], st["rows_in_host_memory"]) == (n, 0)
        g = bld.finish()
        try:
            assert g.row_type == rows and g.metric == "l2"
            same_arrays(g, one, rows)
            assert np.array_equal(bm.as_bytes(g.base_rows), bm.as_bytes(one.base_rows))
            assert np.array_equal(bm.as_bytes(g.base_rows), bm.pad_bits(b, 128)[g.map_ids])
        finally:
            g.close()
    finally:
        one.close()
        del plain


# ---- 6. persistence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", bm.TYPES)
def test_dump_and_load(rq, tmp_path, rows):
    from rabitq_amd import _lib, vecs
    L = _lib.lib()
    n, d, k = 600, 100, 4
    b, centres, marks = bm.byte_data(rows, n, d, k, seed=131)
    P = synth.random_orthogonal(128, seed=132)
    q = bm.byte_queries(rows, b, marks, 70, d, k, seed=133)
    g = rq.RaBitQ.build(b, centres, P, rows=rows)
    t = rq.RaBitQ.build(bm.widen(b, rows), centres, P)
    try:
        dg, dt = str(tmp_path / "byte"), str(tmp_path / "f32")
        g.dump_to_dir(dg)
        t.dump_to_dir(dt)
        assert sorted(os.listdir(dg)) == sorted(FILES + ["rows"])
        assert sorted(os.listdir(dt)) == sorted(FILES)                      # an f32 dump is unchanged: no `rows` file
        assert open(os.path.join(dg, "rows"), "rb").read() == (rows + "\n").encode()
        base = np.asarray(vecs.read_vecs(os.path.join(dg, "base.fvecs"), np.float32))
        assert np.array_equal(bits(base), bits(bm.widen(bm.as_bytes(g.base_rows), rows)))
        for f in FILES:   # the reference loads the directory and answers as for the f32 index of W(b): the same files
            assert open(os.path.join(dg, f), "rb").read() == open(os.path.join(dt, f), "rb").read(), f
        g2 = rq.RaBitQ.load_from_dir(dg)
        try:
            assert g2.row_type == rows and g2.metric == "l2"
            same_arrays(g2, g, "load_dir")
            assert np.array_equal(bm.as_bytes(g2.base_rows), bm.as_bytes(g.base_rows))
            _same_answers(g2.query_batch(q, 3, 10), g.query_batch(q, 3, 10), "load_dir")
        finally:
            g2.close()
        jp = str(tmp_path / "byte.json")
        g.dump_to_json(jp)
        assert json.load(open(jp))["rows"] == rows
        g3 = rq.RaBitQ.load_from_json(jp)
        try:
            assert g3.row_type == rows and g3.metric == "l2"
            same_arrays(g3, g, "load_json")
            assert np.array_equal(bm.as_bytes(g3.base_rows), bm.as_bytes(g.base_rows))
        finally:
            g3.close()
        jt = str(tmp_path / "f32.json")
        t.dump_to_json(jt)
        assert "rows" not in json.load(open(jt))
        # a base.fvecs value the named type cannot represent, and an unknown text: RQ_ERR_IO, nothing allocated
        hnd = C.c_void_p()
        good = t.base.copy()
        open(os.path.join(dt, "rows"), "w").write(rows + "\n")
        assert L.rq_load_dir(os.fsencode(dt), C.byref(hnd)) == 0 and hnd.value   # (the f32 dump of W(b) with the tag loads as byte rows)
        g4 = rq.RaBitQ(hnd)
        try:
            assert g4.row_type == rows
            same_arrays(g4, g, "tagged f32 dump")
        finally:
            g4.close()
        hnd = C.c_void_p()
        for value in (0.5, 256.0, -1.0):
            bad = good.copy()
            bad[n // 2, 3] = F32(value)
            vecs.write_vecs(os.path.join(dt, "base.fvecs"), bad)
            open(os.path.join(dt, "rows"), "w").write("u8\n")
            assert L.rq_load_dir(os.fsencode(dt), C.byref(hnd)) == IO, value
            assert not hnd.value
        for value in (0.5, 128.0, -129.0):
            bad = good.copy()
            bad[n // 2, 3] = F32(value)
            vecs.write_vecs(os.path.join(dt, "base.fvecs"), bad)
            open(os.path.join(dt, "rows"), "w").write("i8\n")
            assert L.rq_load_dir(os.fsencode(dt), C.byref(hnd)) == IO, value
            assert not hnd.value
        vecs.write_vecs(os.path.join(dt, "base.fvecs"), good)
        for text in ("u16\n", "u8", "U8\n", "\n"):
            open(os.path.join(dt, "rows"), "w").write(text)
            assert L.rq_load_dir(os.fsencode(dt), C.byref(hnd)) == IO, text
            assert not hnd.value
        # the JSON image likewise: an unknown "rows" member
        img = open(jp).read()
        assert ('"rows":"%s"' % rows) in img
        jbad = str(tmp_path / "bad.json")
        open(jbad, "w").write(img.replace('"rows":"%s"' % rows, '"rows":"u16"'))
        assert L.rq_load_json(os.fsencode(jbad), C.byref(hnd)) == IO and not hnd.value
    finally:
        g.close()
        t.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", bm.TYPES)
def test_refusals(rq, world, rows):
    import torch
    from rabitq_amd import _lib
    from rabitq_amd import index as ix
    L = _lib.lib()
    rt = _lib.row_type_id(rows)
    c = world((rows, 100, 5000, 16))
    g, b, centres, P, n, d, k = c["gidx"], c["b"], c["centres"], c["P"], c["n"], c["d"], c["k"]
    hnd = C.c_void_p()
    db, dc = torch.from_numpy(bm.as_bytes(b)).cuda(), torch.from_numpy(centres).cuda()
    torch.cuda.synchronize()

    def build(metric, row_type):
        return L.rq_build_rows(_addr(b), n, d, _addr(centres), k, _addr(P), 0, metric, row_type, C.byref(hnd))
    # the cosine and the inner-product metric with byte rows, on every _rows entry
    arrays = [np.ascontiguousarray(a) for a in (bm.as_bytes(g.base_rows), g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors)]
    for metric in (1, 2):
        assert build(metric, rt) == UNSUPPORTED and not hnd.value
        assert L.rq_build_device_rows(C.c_void_p(db.data_ptr()), n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, metric, rt, C.byref(hnd)) == UNSUPPORTED
        assert not hnd.value
        assert L.rq_builder_create_rows(n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, 0, metric, rt, C.byref(hnd)) == UNSUPPORTED and not hnd.value
        assert L.rq_from_arrays_rows(g.dim, g.n, g.k, *[_addr(a) for a in arrays], metric, rt, C.byref(hnd)) == UNSUPPORTED and not hnd.value
    with pytest.raises(_lib.RabitqError):
        rq.RaBitQ.build(b, centres, P, metric="cosine", rows=rows)
    # the values between and beyond the row types stay invalid
    for bad in (3, 6, 7):
        assert build(0, bad) == INVALID and not hnd.value
    # the array type must be the row type's
    with pytest.raises(TypeError):
        rq.RaBitQ.build(bm.typed(b, "i8" if rows == "u8" else "u8"), centres, P, rows=rows)
    assert L.rq_from_arrays_rows(g.dim, g.n, g.k, *[_addr(a) for a in arrays], 0, rt, C.byref(hnd)) == 0
    g4 = rq.RaBitQ(hnd)
    hnd = C.c_void_p()
    try:
        same_arrays(g4, g, "from_arrays_rows")
        assert g4.row_type == rows
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
    assert np.array_equal(bm.as_bytes(g.base_rows), bm.pad_bits(b, c["dim"])[g.map_ids])
    # the HBM budget: no tiers for byte rows
    try:
        ix.set_option("base_device_mb", 0)                                # n * dim = 0.64 MB: not a single megabyte is allowed
        assert build(0, rt) == UNSUPPORTED and not hnd.value
    finally:
        ix.set_option("base_device_mb", -1)
    assert L.rq_builder_create_rows(n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, 1 << 19, 0, rt, C.byref(hnd)) == 0
    bptr = hnd.value
    try:
        assert L.rq_builder_assign_chunk_rows(C.c_void_p(bptr), C.c_void_p(db.data_ptr()), 0, n) == 0
        assert L.rq_builder_order(C.c_void_p(bptr)) == UNSUPPORTED
    finally:
        L.rq_builder_free(C.c_void_p(bptr))
    # device pointers: the f32 array does not exist; the stored rows are n * dim bytes
    p, nbytes = C.c_void_p(), C.c_uint64()
    assert L.rq_get_device_ptr(g._h, ix.ARR_BASE, C.byref(p), C.byref(nbytes)) == UNSUPPORTED
    assert L.rq_get_device_ptr(g._h, ix.ARR_BASE_ROWS, C.byref(p), C.byref(nbytes)) == 0
    assert nbytes.value == n * c["dim"] and p.value


# ---- 8. the new kernels ran ----------------------------------------------------------------------------------------------
def test_the_byte_kernels_ran(rq, world):
    """The profile fields tests/test_option_paths_gpu.py reads, on a byte index.  A batch with small_batch_passes > 0 ran the
    small-batch path: its rerank is sb_query_kernel's run-time byte branch (and, heap ranker with nq <= 32, accurate_kernel<ROW_KIND_BYTE>),
    its finish sb_finish_kernel<*, ROW_KIND_BYTE> (heap ranker) or stage_finish_kernel<*, ROW_KIND_BYTE> (heuristic ranker).  A batch with
    small_batch_passes == 0 ran the staged launches: the flat rerank accurate_kernel<ROW_KIND_BYTE> and stage_finish_kernel<*, ROW_KIND_BYTE>.  The host
    has no other kernels to launch for a byte index; rerank_candidates > 0 shows survivors were reranked, rerank_shadow_rejects == 0
    that no shadow row stood in for a byte row.  The profile has no field that tells sb_query_kernel's own rerank from
    sb_finish_kernel<*, ROW_KIND_BYTE>'s: both belong to a small-batch pass."""
    from rabitq_amd import index as ix
    c = world(("u8", 128, 20000, 32))
    g, q = c["gidx"], c["q"]
    seen = {}
    for name, nq, heur in (("small heap, whole-chip rerank", 1, False), ("small heap", 64, False), ("small heuristic", 16, True),
                           ("large heap", 1024, False), ("large heuristic", 300, True)):
        rq.metrics_reset()
        g.query_batch(q[:nq], PROBE, 10, heur)
        seen[name] = (ix.last_profile(), rq.metrics())
    # dim 192 has no small-batch path: a batch of 16 is one fused launch per stage, reranked by stage_finish_kernel<*, ROW_KIND_BYTE> itself
    c3 = world(("u8", 192, 5000, 16))
    rq.metrics_reset()
    c3["gidx"].query_batch(c3["q"][:16], PROBE, 10, False)
    seen["large-form stages of a few queries"] = (ix.last_profile(), rq.metrics())
    for name, (prof, m) in seen.items():
        assert (prof["small_batch_passes"] > 0) == name.startswith("small"), (name, prof["small_batch_passes"])
        assert prof["rerank_candidates"] > 0 and m["precise"] > 0, (name, prof["rerank_candidates"], m)
        assert prof["rerank_shadow_rejects"] == 0, name
