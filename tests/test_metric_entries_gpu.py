"""What an index's metric decides at the C boundary, entry by entry: the refusals of the build / load / query / add entries of the
three metrics (one status per call), and the four places a raw query is turned into what gets rotated (rq_coarse_rank,
rq_coarse_topk_device, the small-batch front and the large-batch front of rq_query_batch), which must agree with the L2 twin of
the index bit for bit.  The twins are built from the CPU models tests/ip_model.py and tests/cosine_model.py.

Run on the GPU box:  python -m pytest tests/test_metric_entries_gpu.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import cosine_model as cm
from tests import ip_model as im
from tests import synth
from tests.models import bits

pytestmark = pytest.mark.gpu
F32 = np.float32
N, K = 300, 5
INVALID, DIM_MISMATCH, UNSUPPORTED = -1, -2, -6
PROBE, TOPK = 3, 10


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def _addr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_rows(n, d, seed):
    x, centres, _ = synth.mixture(n, d, K, sigma=0.7, seed=seed, centre_scale=0.6)
    scale = np.exp2(np.random.default_rng(seed + 1000).uniform(-2.0, 2.0, size=(n, 1))).astype(F32)
    return np.ascontiguousarray(x * scale), np.ascontiguousarray(centres)


@pytest.fixture(scope="module")
def world(rq, oracle, tmp_path_factory):
    """Per (metric, d): the raw data, the index, its L2 twin and the twin's queries; the files the from-path entries read."""
    w = {}
    tmp = tmp_path_factory.mktemp("metric_entries")
    for metric, d in (("ip", 100), ("ip", 127), ("cosine", 100), ("l2", 100), ("l2", 128)):
        x, centres = raw_rows(N, d, seed=51 + d)
        q, _ = raw_rows(70, d, seed=52 + d)
        dim = im.ip_dim(d) if metric == "ip" else (d + 63) // 64 * 64
        P = synth.random_orthogonal(dim, seed=53)
        c = dict(metric=metric, d=d, dim=dim, x=x, centres=centres, P=P, q=q, twin=None)
        if metric == "ip":
            c["S"] = im.auto_bound(oracle, x)
            c["idx"] = rq.RaBitQ.build(x, centres, P, metric="ip", max_sq_norm=c["S"])
            c["twin"] = rq.RaBitQ.build(im.augment_rows(oracle, x, c["S"]), im.pad_cols(centres, dim), P)
            c["tq"] = im.pad_cols(q, dim)
        elif metric == "cosine":
            c["idx"] = rq.RaBitQ.build(x, centres, P, metric="cosine")
            c["twin"] = rq.RaBitQ.build(cm.normalize_rows(oracle, x), cm.pad64(centres), P)
            c["tq"] = cm.normalize_rows(oracle, q)
        else:
            c["idx"] = rq.RaBitQ.build(x, centres, P)
        w[(metric, d)] = c
    from rabitq_amd import vecs
    x, centres = w[("ip", 100)]["x"], w[("ip", 100)]["centres"]
    w["base_path"] = str(tmp / "base.fvecs")
    vecs.write_vecs(w["base_path"], x)
    for cols in (99, 100, 101, 129):
        w["cent_path_%d" % cols] = str(tmp / ("centroids_%d.fvecs" % cols))
        vecs.write_vecs(w["cent_path_%d" % cols], im.pad_cols(centres, 129)[:, :cols])
    yield w
    for c in w.values():
        if isinstance(c, dict):
            c["idx"].close()
            if c["twin"] is not None:
                c["twin"].close()


# ---- 1. refusals: one call, one status ---------------------------------------------------------------------------------
def _status(L, st):
    return int(st), L.rq_last_error().decode(errors="replace")


def _metric_entry(name, metric):
    """The *_metric entry `name` called with the metric id `metric` on otherwise good arguments (the ip d = 100 data, as L2 rows)."""
    def call(L, w):
        import torch
        c = w[("ip", 100)]
        x, cent, P = c["x"], c["centres"], synth.random_orthogonal(128, seed=53)
        h = C.c_void_p()
        if name == "rq_build_metric":
            return L.rq_build_metric(_addr(x), N, 100, _addr(cent), K, _addr(P), 0, metric, C.byref(h))
        if name == "rq_build_device_metric":
            dx, dc = torch.from_numpy(x).cuda(), torch.from_numpy(cent).cuda()
            return L.rq_build_device_metric(C.c_void_p(dx.data_ptr()), N, 100, C.c_void_p(dc.data_ptr()), K, _addr(P), 0, metric, C.byref(h))
        if name == "rq_build_from_path_metric":
            return L.rq_build_from_path_metric(os.fsencode(w["base_path"]), os.fsencode(w["cent_path_100"]), _addr(P), 0, metric, C.byref(h))
        if name == "rq_builder_create_metric":
            dc = torch.from_numpy(cent).cuda()
            return L.rq_builder_create_metric(N, 100, C.c_void_p(dc.data_ptr()), K, _addr(P), 0, 0, metric, C.byref(h))
        g = c["twin"]
        arrays = [np.ascontiguousarray(a) for a in (g.base, g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors)]
        return L.rq_from_arrays_metric(g.dim, g.n, g.k, *[_addr(a) for a in arrays], metric, C.byref(h))
    return call


def _build_ip(d=100, cols=None, S=None, n=N):
    def call(L, w):
        c = w[("ip", 100)]
        dd = max(d, 1)
        x = c["x"] if d == 100 else np.ones((n, dd), F32)
        cent = np.zeros((K, max(cols if cols is not None else d, 1) + 1), F32)
        h = C.c_void_p()
        return L.rq_build_ip(_addr(x), n, d, _addr(cent), K, None, 0, d if cols is None else cols, float(F32(c["S"] if S is None else S)), C.byref(h))
    return call


def _builder_ip(d, S):
    def call(L, w):
        import torch
        dc = torch.zeros((K, d), device="cuda")
        h = C.c_void_p()
        return L.rq_builder_create_ip(N, d, C.c_void_p(dc.data_ptr()), K, None, 0, 0, d, float(F32(S)), C.byref(h))
    return call


def _from_path(entry, cols):
    def call(L, w):
        h = C.c_void_p()
        b, c = os.fsencode(w["base_path"]), os.fsencode(w["cent_path_%d" % cols])
        if entry == "metric":
            return L.rq_build_from_path_metric(b, c, None, 0, 0, C.byref(h))
        return L.rq_build_from_path_ip(b, c, None, 0, float("nan"), C.byref(h))
    return call


def _from_arrays_ip(d, S):
    def call(L, w):
        g = w[("ip", 100)]["idx"]
        arrays = [np.ascontiguousarray(a) for a in (g.base, g.orthogonal, g.centroids, g.offsets, g.map_ids, g.codes, g.factors)]
        h = C.c_void_p()
        return L.rq_from_arrays_ip(g.dim, g.n, g.k, *[_addr(a) for a in arrays], d, float(F32(S)), C.byref(h))
    return call


def _query(entry, key, length):
    """One of the four raw-query entries on the index `key` with queries of `length` floats."""
    def call(L, w):
        import torch
        g = w[key]["idx"]
        nq = 4
        q = np.ones((nq, max(length, 1)), F32)
        if entry == "rq_query_batch":
            d, i, n = np.zeros((nq, TOPK), F32), np.zeros((nq, TOPK), np.uint32), np.zeros(nq, np.uint32)
            return L.rq_query_batch(g._h, _addr(q), nq, length, PROBE, TOPK, 0, _addr(d), _addr(i), _addr(n))
        if entry == "rq_range_search":
            r, h = np.ones(nq, F32), C.c_void_p()
            st = L.rq_range_search(g._h, None, _addr(q), nq, length, PROBE, _addr(r), C.byref(h))
            assert not h.value
            return st
        if entry == "rq_coarse_rank":
            y, cl, cd = np.zeros((nq, g.dim), F32), np.zeros((nq, PROBE), np.uint32), np.zeros((nq, PROBE), F32)
            return L.rq_coarse_rank(g._h, _addr(q), nq, length, PROBE, _addr(y), _addr(cl), _addr(cd))
        qd = torch.from_numpy(q).cuda()
        cl, cd = torch.zeros((nq, PROBE), device="cuda", dtype=torch.int32), torch.zeros((nq, PROBE), device="cuda")
        return L.rq_coarse_topk_device(g._h, C.c_void_p(qd.data_ptr()), nq, length, 0, g.k, PROBE, C.c_void_p(cl.data_ptr()), C.c_void_p(cd.data_ptr()))
    return call


def _add_dim_rows(L, w):
    g = w[("ip", 100)]["idx"]
    rows, first = np.zeros((2, g.dim), F32), C.c_uint32()
    return L.rq_add(g._h, _addr(rows), 2, g.dim, None, 0, C.cast(C.byref(first), C.c_void_p))


def _ip_entry(entry, key, length=None, topk=TOPK):
    def call(L, w):
        g = w[key]["idx"]
        nq = 4
        length_ = w[key]["d"] if length is None else length
        q, dist, out = np.ones((nq, max(length_, 1)), F32), np.ones((nq, max(topk, 1)), F32), np.zeros((nq, max(topk, 1)), F32)
        if entry == "rq_ip_params":
            d, s = C.c_uint32(), C.c_float()
            return L.rq_ip_params(g._h, C.byref(d), C.byref(s))
        if entry == "rq_ip_from_dist":
            return L.rq_ip_from_dist(g._h, _addr(q), nq, length_, _addr(dist), topk, None, _addr(out))
        return L.rq_ip_radius(g._h, _addr(q), nq, length_, _addr(dist), _addr(out))
    return call


METRIC_ENTRIES = ["rq_build_metric", "rq_build_device_metric", "rq_build_from_path_metric", "rq_builder_create_metric", "rq_from_arrays_metric"]
QUERY_ENTRIES = ["rq_query_batch", "rq_range_search", "rq_coarse_rank", "rq_coarse_topk_device"]
REFUSALS = (
    [("%s-metric2" % e, _metric_entry(e, 2), INVALID, "_ip") for e in METRIC_ENTRIES] +
    [("%s-metric7" % e, _metric_entry(e, 7), INVALID, "") for e in METRIC_ENTRIES] +
    [("build_ip-cols-d-1", _build_ip(cols=99), INVALID, ""),
     ("build_ip-cols-dim+1", _build_ip(cols=129), INVALID, ""),
     ("build_ip-d0", _build_ip(d=0, cols=0, n=2), INVALID, ""),
     ("build_ip-d4096", _build_ip(d=4096, n=2), UNSUPPORTED, ""),
     ("build_ip-S-1", _build_ip(S=-1.0), INVALID, ""),
     ("build_ip-Sinf", _build_ip(S=np.inf), INVALID, ""),
     ("builder_ip-Snan", _builder_ip(100, np.nan), INVALID, ""),
     ("builder_ip-d4096", _builder_ip(4096, 1.0), UNSUPPORTED, ""),
     ("from_path_metric-cols-d+1", _from_path("metric", 101), DIM_MISMATCH, ""),
     ("from_path_ip-cols-d-1", _from_path("ip", 99), DIM_MISMATCH, ""),
     ("from_path_ip-cols-dim+1", _from_path("ip", 129), DIM_MISMATCH, ""),
     ("from_arrays_ip-d-not-of-dim", _from_arrays_ip(63, 1.0), DIM_MISMATCH, ""),
     ("from_arrays_ip-S-1", _from_arrays_ip(100, -1.0), INVALID, "")] +
    [("%s-ip-len-dim" % e, _query(e, ("ip", 100), 128), DIM_MISMATCH, "") for e in QUERY_ENTRIES] +
    [("%s-ip-len-d-1" % e, _query(e, ("ip", 100), 99), DIM_MISMATCH, "") for e in QUERY_ENTRIES] +
    [("add-ip-rows-of-dim", _add_dim_rows, DIM_MISMATCH, "")] +
    [("%s-l2-len64" % e, _query(e, ("l2", 100), 64), DIM_MISMATCH, "") for e in QUERY_ENTRIES] +
    [("%s-l2-len0" % e, _query(e, ("l2", 100), 0), DIM_MISMATCH, "") for e in QUERY_ENTRIES] +
    [("%s-on-%s" % (e, m), _ip_entry(e, (m, 100)), INVALID, "") for m in ("l2", "cosine") for e in ("rq_ip_params", "rq_ip_from_dist", "rq_ip_radius")] +
    [("ip_from_dist-len-not-d", _ip_entry("rq_ip_from_dist", ("ip", 100), length=101), DIM_MISMATCH, ""),
     ("ip_from_dist-topk0", _ip_entry("rq_ip_from_dist", ("ip", 100), topk=0), INVALID, "")])


@pytest.mark.parametrize("call,want,fragment", [pytest.param(c, s, f, id=i) for i, c, s, f in REFUSALS])
def test_refusal(rq, world, call, want, fragment):
    from rabitq_amd import _lib
    L = _lib.lib()
    st, text = _status(L, call(L, world))
    assert st == want, (st, text)
    assert fragment in text, text


def test_build_ip_names_the_first_row_above_the_bound(rq, world, oracle):
    """sq_bound one ulp below the largest squared row norm: RQ_ERR_INVALID, and the text names the first row whose s exceeds it."""
    from rabitq_amd import _lib
    L = _lib.lib()
    c = world[("ip", 100)]
    below = np.nextafter(F32(c["S"]), F32(0.0))
    first = int(np.flatnonzero(im.sqnorms(oracle, c["x"]) > below)[0])
    st, text = _status(L, _build_ip(S=below)(L, world))
    assert st == INVALID, (st, text)
    assert ("row %d:" % first) in text, (first, text)


# ---- 2. the four places a raw query is transformed agree with the L2 twin ----------------------------------------------
def _coarse_topk(idx, q):
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    cl = torch.zeros((q.shape[0], PROBE), device="cuda", dtype=torch.int32)
    cd = torch.zeros((q.shape[0], PROBE), device="cuda")
    torch.cuda.synchronize()
    idx.coarse_topk_device(qd.data_ptr(), q.shape[0], q.shape[1], 0, idx.k, PROBE, cl.data_ptr(), cd.data_ptr())
    return cl.cpu().numpy().view(np.uint32), cd.cpu().numpy()


def _same_answers(a, b, what):
    assert np.array_equal(a[2], b[2]), what
    for r in range(len(a[2])):
        n = int(a[2][r])
        assert np.array_equal(a[1][r, :n], b[1][r, :n]) and np.array_equal(bits(a[0][r, :n]), bits(b[0][r, :n])), (what, r)


@pytest.mark.parametrize("key", [("ip", 100), ("ip", 127), ("cosine", 100)], ids=["ip-d100", "ip-d127", "cosine-d100"])
def test_query_transform_sites_equal_the_l2_twin(rq, world, key):
    from rabitq_amd import index as ix
    c = world[key]
    g, twin, q, tq = c["idx"], c["twin"], c["q"], c["tq"]
    assert g.metric == key[0] and twin.metric == "l2" and g.dim == twin.dim == c["dim"]
    y0, cl0, cd0 = rq.ops.coarse_rank(g, q, PROBE)
    y1, cl1, cd1 = rq.ops.coarse_rank(twin, tq, PROBE)
    assert np.array_equal(bits(y0), bits(y1)) and np.array_equal(cl0, cl1) and np.array_equal(bits(cd0), bits(cd1))
    k0, k1 = _coarse_topk(g, q), _coarse_topk(twin, tq)
    assert np.array_equal(k0[0], k1[0]) and np.array_equal(bits(k0[1]), bits(k1[1]))
    try:
        for small in (0, 1):
            ix.set_option("small_batch", small)
            for nq in (3, 64):
                got = g.query_batch(q[:nq], PROBE, TOPK)
                took_small = ix.last_profile()["small_batch_passes"] > 0   # option 0: the few-launch front (small_front), 1: the staged one
                assert took_small == (small == 0), (key, small, nq)
                _same_answers(got, twin.query_batch(tq[:nq], PROBE, TOPK), (key, small, nq))
    finally:
        ix.set_option("small_batch", 0)
    _same_answers(g.query_batch(q, PROBE, TOPK), twin.query_batch(tq, PROBE, TOPK), (key, 70))


def test_l2_unpadded_coarse_rank_equals_coarse_topk(rq, world):
    """An L2 index whose raw length is its dim (d = 128): nothing is padded, and rq_coarse_rank ranks as rq_coarse_topk_device
    does over all lists."""
    c = world[("l2", 128)]
    assert c["idx"].dim == 128
    _, cl, cd = rq.ops.coarse_rank(c["idx"], c["q"], PROBE)
    k = _coarse_topk(c["idx"], c["q"])
    assert np.array_equal(cl, k[0]) and np.array_equal(bits(cd), bits(k[1]))
