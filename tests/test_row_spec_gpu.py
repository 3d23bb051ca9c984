"""What the row-type description (RowSpec, rabitq_amd/csrc/rows.h) centralises, on an MI355X:

1. metric x row type: every entry that takes a row type, and both loaders, answer each of the 3 metrics x 5 row types (and the
   values 3 and 6, which are no row type) with the status code written in the tables below.
2. every instantiation of the rerank kernels on the row kind is launched -- accurate_kernel<K>, sb_finish_kernel<*, K> with
   topk < 64 and topk >= 64, stage_finish_kernel<*, K> with both rankers -- for each of f32, f16, bf16, u8 and i8, and answers as
   the CPU oracle of the widened rows does.  The five indexes of one shape hold the same values (integers 0 .. 127, which every row
   type represents exactly), so one oracle index and one set of oracle answers per shape serve all five.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import byte_model as bm
from tests import synth
from tests.models import bits

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, IO, UNSUPPORTED = -1, -3, -6
PROBE = 8
ROW_TYPES = {"f32": 0, "f16": 1, "bf16": 2, "u8": 4, "i8": 5}   # RQ_ROWS_* (include/rabitq_hip.h)
L2, COSINE, IP = 0, 1, 2                                        # RQ_METRIC_*

# The status code per row_type value, for metric = L2, cosine, inner product.
# Entries (rq_build_rows, rq_build_device_rows, rq_builder_create_rows, rq_from_arrays_rows): a value that is no row type is invalid
# whatever the metric; the inner product has no typed rows and the cosine metric no byte rows (unsupported); the inner product with
# f32 rows is not a metric these entries take (it needs a row length and a bound: the _ip entries), which is invalid.
ENTRY_CODES = {
    0: (0, 0, INVALID),
    1: (0, 0, UNSUPPORTED),
    2: (0, 0, UNSUPPORTED),
    3: (INVALID, INVALID, INVALID),
    4: (0, UNSUPPORTED, UNSUPPORTED),
    5: (0, UNSUPPORTED, UNSUPPORTED),
    6: (INVALID, INVALID, INVALID),
}
# Loaders (rq_load_dir with its `rows` / `metric` files, rq_load_json with its "rows" / "metric" members): a pair the entries refuse,
# and a tag that names no row type, is an I/O error; an inner-product index of f32 rows loads.
LOAD_CODES = {
    0: (0, 0, 0),
    1: (0, 0, IO),
    2: (0, 0, IO),
    3: (IO, IO, IO),
    4: (0, IO, IO),
    5: (0, IO, IO),
    6: (IO, IO, IO),
}
TAGS = {0: None, 1: "f16", 2: "bf16", 3: "3", 4: "u8", 5: "i8", 6: "6"}   # what a dump announces (3, 6: nothing a dump writes)
ROW_VALUES = sorted(ENTRY_CODES)
IP_D, IP_S = 63, F32(1.0e6)                                              # an inner-product spec a dim-64 index can have


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def _addr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def typed(wx, rows):
    """f32 integers 0 .. 127 -> the same values as an array of the row type (f16: float16; bf16: uint16 bit patterns)."""
    wx = np.ascontiguousarray(wx, dtype=F32)
    assert np.array_equal(wx, np.rint(wx)) and wx.min() >= 0 and wx.max() <= 127
    if rows == "f32":
        return wx
    if rows == "f16":
        return np.ascontiguousarray(wx.astype(np.float16))
    if rows == "bf16":
        assert not (wx.view(np.uint32) & 0xFFFF).any()
        return np.ascontiguousarray((wx.view(np.uint32) >> 16).astype(np.uint16))
    return np.ascontiguousarray(wx.astype(bm.NP_DTYPE[rows]))


def small_values(n, d, k, seed):
    """-> (wx: n x d f32 integers 0 .. 127, centres, queries(nq)): tests/byte_model.py's u8 data set, halved."""
    b, centres, marks = bm.byte_data("u8", n, d, k, seed=seed)
    wx = np.ascontiguousarray((b >> 1).astype(F32))

    def queries(nq):
        return np.ascontiguousarray(bm.byte_queries("u8", b, marks, nq, d, k, seed=seed + 2) * F32(0.5))
    return wx, np.ascontiguousarray(centres * F32(0.5)), queries


# ---- 1. metric x row type ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(rq):
    """n = 256, d = 64, k = 4: the values, an f32 L2 index of them, its arrays."""
    n, d, k = 256, 64, 4
    wx, centres, _ = small_values(n, d, k, seed=5)
    P = synth.random_orthogonal(d, seed=6)
    g = rq.RaBitQ.build(wx, centres, P)
    stored = np.ascontiguousarray(g.base)            # cluster order, n x dim
    rest = [np.ascontiguousarray(a) for a in (g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors)]
    yield dict(n=n, d=d, k=k, wx=wx, centres=centres, P=P, g=g, stored=stored, rest=rest)
    g.close()


def rows_arg(values, rt):
    """The array an entry gets as its rows for row_type rt (a value that is no row type: bytes, which the entry must not read)."""
    name = {v: k for k, v in ROW_TYPES.items()}.get(rt)
    return typed(values, name) if name else typed(values, "u8")


@pytest.mark.parametrize("entry", ["rq_build_rows", "rq_build_device_rows", "rq_builder_create_rows", "rq_from_arrays_rows"])
def test_entries_metric_x_row_type(rq, tiny, entry):
    import torch
    from rabitq_amd import _lib
    L = _lib.lib()
    n, d, k, centres, P = tiny["n"], tiny["d"], tiny["k"], tiny["centres"], tiny["P"]
    dc = torch.from_numpy(centres).cuda()
    torch.cuda.synchronize()
    for rt in ROW_VALUES:
        for metric in (L2, COSINE, IP):
            hnd = C.c_void_p()
            if entry == "rq_build_rows":
                a = rows_arg(tiny["wx"], rt)
                got = L.rq_build_rows(_addr(a), n, d, _addr(centres), k, _addr(P), 0, metric, rt, C.byref(hnd))
            elif entry == "rq_build_device_rows":
                da = torch.from_numpy(rows_arg(tiny["wx"], rt)).cuda()
                torch.cuda.synchronize()
                got = L.rq_build_device_rows(C.c_void_p(da.data_ptr()), n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, metric, rt, C.byref(hnd))
            elif entry == "rq_builder_create_rows":
                got = L.rq_builder_create_rows(n, d, C.c_void_p(dc.data_ptr()), k, _addr(P), 0, 0, metric, rt, C.byref(hnd))
            else:
                a = rows_arg(tiny["stored"], rt)
                got = L.rq_from_arrays_rows(d, n, k, _addr(a), *[_addr(x) for x in tiny["rest"]], metric, rt, C.byref(hnd))
            want = ENTRY_CODES[rt][metric]
            print(entry, "row_type", rt, "metric", metric, "->", got, "want", want)
            assert got == want, (entry, rt, metric, got, want)
            assert bool(hnd.value) == (want == 0), (entry, rt, metric)
            if hnd.value and entry == "rq_builder_create_rows":
                L.rq_builder_free(hnd)
            elif hnd.value:
                out = C.c_uint32(99)
                assert L.rq_row_type(hnd, C.byref(out)) == 0 and out.value == rt
                L.rq_free(hnd)


def _metric_file(metric):
    if metric == COSINE:
        return "cosine\n"
    return "ip %u %08x\n" % (IP_D, int(np.array([IP_S]).view(np.uint32)[0])) if metric == IP else None


def _metric_members(metric):
    if metric == COSINE:
        return ',"metric":"cosine"'
    return ',"metric":"ip","ip_d":%u,"ip_sq_bound_bits":%u' % (IP_D, int(np.array([IP_S]).view(np.uint32)[0])) if metric == IP else ""


@pytest.mark.parametrize("loader", ["rq_load_dir", "rq_load_json"])
def test_loaders_metric_x_row_type(rq, tiny, tmp_path, loader):
    from rabitq_amd import _lib
    L = _lib.lib()
    g = tiny["g"]
    if loader == "rq_load_dir":
        path = str(tmp_path / "dir")
        g.dump_to_dir(path)
        assert not os.path.exists(os.path.join(path, "rows")) and not os.path.exists(os.path.join(path, "metric"))
    else:
        path = str(tmp_path / "index.json")
        g.dump_to_json(path)
        text = open(path).read()
        assert text.endswith("}") and '"rows"' not in text and '"metric"' not in text
    for rt in ROW_VALUES:
        for metric in (L2, COSINE, IP):
            if loader == "rq_load_dir":
                for name, content in (("rows", TAGS[rt] + "\n" if TAGS[rt] else None), ("metric", _metric_file(metric))):
                    f = os.path.join(path, name)
                    if os.path.exists(f):
                        os.remove(f)
                    if content is not None:
                        with open(f, "w") as fh:
                            fh.write(content)
                src = path
            else:
                src = str(tmp_path / ("pair_%d_%d.json" % (rt, metric)))
                with open(src, "w") as fh:
                    fh.write(text[:-1] + _metric_members(metric) + (',"rows":"%s"' % TAGS[rt] if TAGS[rt] else "") + "}")
            hnd = C.c_void_p()
            got = getattr(L, loader)(os.fsencode(src), C.byref(hnd))
            want = LOAD_CODES[rt][metric]
            print(loader, "rows", TAGS[rt], "metric", metric, "->", got, "want", want)
            assert got == want, (loader, rt, metric, got, want)
            assert bool(hnd.value) == (want == 0), (loader, rt, metric)
            if hnd.value:
                out = C.c_uint32(99)
                assert L.rq_row_type(hnd, C.byref(out)) == 0 and out.value == rt
                L.rq_free(hnd)


# ---- 2. each instantiation is launched -----------------------------------------------------------------------------------------
SHAPES = {128: (20000, 32), 192: (5000, 16)}   # dim -> (n, k): dim 128 has a small-batch path, dim 192 has none
TOPKS = (10, 64)                               # sb_finish_kernel<true, K> below 64, <false, K> from 64 on
# name, dim, queries, heuristic ranker: the batch shapes of tests/test_byte_rows_gpu.py::test_the_byte_kernels_ran
BATCHES = (("small heap, whole-chip rerank", 128, 1, False), ("small heap", 128, 64, False), ("small heuristic", 128, 16, True),
           ("large heap", 128, 1024, False), ("large heuristic", 128, 300, True), ("large-form stages of a few queries", 192, 16, False))


@pytest.fixture(scope="module")
def shapes(oracle):
    """dim -> the values, the oracle index of them, and the oracle's answers per (topk, ranker): computed once, read by all five
    row types."""
    out = {}
    for dim, (n, k) in SHAPES.items():
        wx, centres, queries = small_values(n, dim, k, seed=71 + dim)
        P = synth.random_orthogonal(dim, seed=72)
        q = queries(max(nq for _, d, nq, _ in BATCHES if d == dim))
        oidx = oracle.OracleIndex.build(wx, centres, P)
        ans = {}
        for topk in TOPKS:
            for heur in sorted({h for _, d, _, h in BATCHES if d == dim}):
                nq = max(nq for _, d, nq, h in BATCHES if d == dim and h == heur)
                rows = []
                for qi in range(nq):
                    oracle.metrics_reset()
                    try:
                        od, oi = oidx.query(q[qi], PROBE, topk, heur)
                    except Exception:
                        od, oi = np.zeros(0, F32), np.zeros(0, np.uint32)
                    m = oracle.metrics()
                    rows.append((od, oi, m["rough"], m["precise"]))
                ans[(topk, heur)] = rows
        oidx.close()
        out[dim] = dict(wx=wx, centres=centres, P=P, q=q, ans=ans)
    return out


@pytest.mark.parametrize("rows", list(ROW_TYPES))
def test_every_row_kind_instantiation_is_launched(rq, shapes, rows):
    from rabitq_amd import index as ix
    built = {}
    try:
        for dim, s in shapes.items():
            built[dim] = rq.RaBitQ.build(typed(s["wx"], rows), s["centres"], s["P"], rows=rows)
            assert built[dim].row_type == rows
        for name, dim, nq, heur in BATCHES:
            s, g = shapes[dim], built[dim]
            for topk in TOPKS:
                ans = s["ans"][(topk, heur)][:nq]
                rq.metrics_reset()
                d, gids, cnt = g.query_batch(s["q"][:nq], PROBE, topk, heur)
                m, prof = rq.metrics(), ix.last_profile()
                what = (rows, name, topk)
                for b, (od, oi, _, _) in enumerate(ans):
                    c = int(cnt[b])
                    assert c == oi.size, (what, b, c, oi.size)
                    assert np.array_equal(gids[b, :c], oi), (what, b)
                    assert np.array_equal(bits(d[b, :c]), bits(od)), (what, b)
                assert (m["rough"], m["precise"], m["query"]) == (sum(a[2] for a in ans), sum(a[3] for a in ans), nq), (what, m)
                assert (prof["small_batch_passes"] > 0) == name.startswith("small"), (what, prof["small_batch_passes"])
                assert prof["rerank_candidates"] > 0 and m["precise"] > 0, (what, prof["rerank_candidates"], m)
                if rows != "f32":   # (an f32 index of this size has shadow rows; a typed one never does)
                    assert prof["rerank_shadow_rejects"] == 0, what
    finally:
        for g in built.values():
            g.close()
