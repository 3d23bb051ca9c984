"""Centroid training (rq_train_centroids*): the GPU trainer against its CPU model, tests/train_model.py, bit for bit -- centroid
bits, iters_run, splits, sample_rows and the f64 bits of every objective.  No tolerance anywhere except the one quality check at
the end, which uses the recall the old trainer's test asks for.  Fixtures: tests/train_cases.py.

Run on the GPU box:  python -m pytest tests/test_train_gpu.py -m gpu -q
"""
import ctypes as C

import numpy as np
import pytest

from tests import byte_model, half_model, synth
from tests import train_cases as tc
from tests import train_model as tm
from tests.models import ARRAYS, bits

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def rq():
    import os
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


_MODELS, _BASES = {}, {}


def base_of(name):
    if name not in _BASES:
        _BASES[name] = tc.base_of(name)
    return _BASES[name]


def model_of(oracle, name):
    """The model's run of a fixture: computed once, shared, never modified."""
    if name not in _MODELS:
        _MODELS[name] = tc.run_model(oracle, name, base=base_of(name))
    return _MODELS[name]


def gpu_run(rq, name, **kw):
    _, _, k, ppc, iters = tc.SHAPES[name]
    return rq.train_centroids(base_of(name), k, iters=iters, points_per_centroid=ppc, return_stats=True, **kw)


def same_as_model(got, m, what=""):
    c, st = got
    assert (st.iters_run, st.sample_rows, st.splits) == (m.iters_run, m.sample_rows, m.splits), what
    assert st.objective.dtype == np.float64 and np.array_equal(st.objective.view(np.uint64), m.objective.view(np.uint64)), (what, st.objective, m.objective)
    assert c.shape == m.centroids.shape and c.dtype == np.float32, what
    assert np.array_equal(c.view(np.uint32), m.centroids.view(np.uint32)), (what, int((c.view(np.uint32) != m.centroids.view(np.uint32)).sum()))


def same_run(a, b, what=""):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what
    assert (a[1].iters_run, a[1].sample_rows, a[1].splits) == (b[1].iters_run, b[1].sample_rows, b[1].splits), what
    assert np.array_equal(a[1].objective.view(np.uint64), b[1].objective.view(np.uint64)), what


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_fixture_equals_the_model(rq, oracle, name):
    n, d, k, ppc, iters = tc.SHAPES[name]
    m = model_of(oracle, name)
    # what the fixture is for, on the model's own output
    assert m.sample_rows == min(n, ppc * k) and np.isfinite(m.objective).all() and m.objective.size == m.iters_run
    if name == "A":
        assert m.sample_rows == n and 1 < m.iters_run < iters                       # ns = n, early stop
    if name == "B":
        assert m.sample_rows == 2048 < n and m.splits > 0 and m.iters_run < iters    # strata sampling, natural empties
    if name == "C":
        assert m.splits > 0 and any(1 in c for c in m.counts)                       # a cluster of one member
    if name == "D":
        assert m.counts[0].count(0) == 3 and m.splits >= 3                          # three empties at iteration 0 by construction
    if name == "E":
        assert m.splits > 0
    if name == "F":
        assert m.iters_run == iters == 40 and max(max(c) for c in m.counts) > 2000  # the cap, a cluster of thousands
    if name == "G":
        assert d // 64 == 12
    same_as_model(gpu_run(rq, name), m, name)


def test_assign_impl_values_agree(rq, oracle):
    try:
        rq.index.set_option("assign_impl", 1)
        valu = gpu_run(rq, "B")
    finally:
        rq.index.set_option("assign_impl", 0)
    same_as_model(valu, model_of(oracle, "B"), "assign_impl=1")
    same_run(valu, gpu_run(rq, "B"), "assign_impl 1 vs 0")


def test_runs_repeat_and_seeds_differ(rq, oracle):
    a, b = gpu_run(rq, "B"), gpu_run(rq, "B")
    same_run(a, b, "two runs of seed 0")
    other = gpu_run(rq, "B", seed=1)
    n, _, k, ppc, iters = tc.SHAPES["B"]
    m1 = tm.train(oracle, base_of("B"), k, iters=iters, points_per_centroid=ppc, seed=1)
    assert not np.array_equal(m1.positions, model_of(oracle, "B").positions)       # another sample
    same_as_model(other, m1, "seed 1")
    assert not np.array_equal(other[0], a[0])


@pytest.mark.parametrize("name", ["B", "C"])
def test_host_entry_equals_device_entry(rq, oracle, name):
    import torch
    n, d, k, ppc, iters = tc.SHAPES[name]
    x = torch.from_numpy(base_of(name)).cuda()
    out = torch.zeros((k, d), dtype=torch.float32, device="cuda")
    st = rq.train_centroids_device(x.data_ptr(), n, d, k, out.data_ptr(), iters=iters, points_per_centroid=ppc)
    dev = (out.cpu().numpy(), st)
    same_as_model(dev, model_of(oracle, name), name + " device entry")
    same_run(dev, gpu_run(rq, name), name + " host vs device")


def typed_base(rows, n=3000, d=64, k=16):
    x, _, _ = synth.mixture(n, d, k, sigma=tc.SIGMA, seed=77)
    if rows == "f16":
        return x.astype(np.float16)
    if rows == "bf16":
        return half_model.narrow(x, "bf16")
    lo, hi = byte_model.RANGE[rows]
    return np.clip(np.rint(byte_model.scale_into(x, rows)), lo, hi).astype(byte_model.NP_DTYPE[rows])


@pytest.mark.parametrize("rows", ["f16", "bf16", "u8", "i8"])
def test_typed_rows_equal_the_f32_run_on_the_widened_rows(rq, oracle, rows):
    h = typed_base(rows)
    wide = tm.widen(h, rows)
    assert wide.dtype == np.float32 and np.array_equal(rq.widen(h, rows), wide)
    typed = rq.train_centroids(h, 16, rows=rows, return_stats=True)
    same_run(typed, rq.train_centroids(wide, 16, return_stats=True), rows)
    same_as_model(typed, tm.train(oracle, h, 16, rows=rows), rows)
    # and on the device, where the typed rows are gathered as stored
    import torch
    dh = torch.from_numpy(np.ascontiguousarray(h).view(np.uint8)).cuda()
    out = torch.zeros((16, 64), dtype=torch.float32, device="cuda")
    st = rq.train_centroids_device(dh.data_ptr(), h.shape[0], 64, 16, out.data_ptr(), points_per_centroid=100, rows=rows)   # ns = 1600 < n
    same_run((out.cpu().numpy(), st), rq.train_centroids(wide, 16, points_per_centroid=100, return_stats=True), rows + " device, sampled")


def test_cosine_equals_l2_on_normalised_rows(rq, oracle):
    x, _, _ = synth.mixture(4000, 100, 16, sigma=tc.SIGMA, seed=78)
    x *= np.exp2(np.random.default_rng(1).integers(-4, 5, size=(4000, 1))).astype(np.float32)
    cos = rq.train_centroids(x, 16, points_per_centroid=128, metric="cosine", return_stats=True)
    l2 = rq.train_centroids(rq.normalize(x), 16, points_per_centroid=128, return_stats=True)
    assert cos[0].shape == (16, 100) and l2[0].shape == (16, 128) and not l2[0][:, 100:].any()
    same_run((l2[0][:, :100].copy(), l2[1]), cos, "cosine")
    same_as_model(cos, tm.train(oracle, x, 16, points_per_centroid=128, metric="cosine"), "cosine model")
    # half-precision rows: N(W(h)), as the contract states it
    h = x.astype(np.float16)
    same_run(rq.train_centroids(h, 16, metric="cosine", return_stats=True),
             rq.train_centroids(h.astype(np.float32), 16, metric="cosine", return_stats=True), "cosine f16")


@pytest.mark.parametrize("explicit", [False, True])
def test_ip_equals_l2_on_augmented_rows(rq, oracle, explicit):
    x, _, _ = synth.mixture(4000, 100, 16, sigma=tc.SIGMA, seed=79)
    S = float(rq.row_sqnorm_max(x)) * 1.5 if explicit else None
    ip = rq.train_centroids(x, 16, points_per_centroid=128, metric="ip", max_sq_norm=S, return_stats=True)
    l2 = rq.train_centroids(rq.augment(x, S), 16, points_per_centroid=128, return_stats=True)
    assert ip[0].shape == (16, 101) and l2[0].shape == (16, 128) and not l2[0][:, 101:].any()
    assert ip[0][:, 100].min() > 0                                                   # the extra coordinate is trained too
    same_run((l2[0][:, :101].copy(), l2[1]), ip, "ip")
    same_as_model(ip, tm.train(oracle, x, 16, points_per_centroid=128, metric="ip", max_sq_norm=S), "ip model")
    # on the device, the automatic bound is the largest squared norm of all n rows there too
    import torch
    dx = torch.from_numpy(x).cuda()
    out = torch.zeros((16, 101), dtype=torch.float32, device="cuda")
    st = rq.train_centroids_device(dx.data_ptr(), 4000, 100, 16, out.data_ptr(), points_per_centroid=128, metric="ip", max_sq_norm=S)
    same_run((out.cpu().numpy(), st), ip, "ip device")


def refused(rq, status, fn):
    with pytest.raises(rq.RabitqError) as e:
        fn()
    assert e.value.status == status, e.value
    return str(e.value)


def test_refusals(rq, oracle):
    import torch
    x = base_of("B")
    n, d, k, ppc, iters = tc.SHAPES["B"]
    refused(rq, INVALID, lambda: rq.train_centroids(x[:10], 16))                                       # n < k
    refused(rq, UNSUPPORTED, lambda: rq.train_centroids(x[:100].astype(np.float16), 4, metric="ip"))   # ip with typed rows
    refused(rq, UNSUPPORTED, lambda: rq.train_centroids(np.zeros((100, 64), np.uint8), 4, metric="cosine", rows="u8"))   # cosine with bytes
    refused(rq, INVALID, lambda: rq.train_centroids(x, 4, metric="ip", max_sq_norm=-1.0))
    refused(rq, INVALID, lambda: rq.train_centroids(x, 4, metric="ip", max_sq_norm=1e-3))              # a sample row A refuses
    # a NaN inside the sample, on a sampled position: refused before any kernel computes with it, outputs untouched; the same NaN on
    # a row the sample does not hold changes nothing
    pos = model_of(oracle, "B").positions
    hit, miss = int(pos[1000]), int(pos[1000]) + 1
    assert miss not in set(pos.tolist())
    for entry in ("host", "device"):
        bad = x.copy()
        bad[hit, 77] = np.nan
        if entry == "host":
            msg = refused(rq, INVALID, lambda: rq.train_centroids(bad, k, iters=iters, points_per_centroid=ppc))
        else:
            db = torch.from_numpy(bad).cuda()
            out = torch.full((k, d), 7.0, dtype=torch.float32, device="cuda")
            msg = refused(rq, INVALID, lambda: rq.train_centroids_device(db.data_ptr(), n, d, k, out.data_ptr(), iters=iters, points_per_centroid=ppc))
            assert bool((out == 7.0).all())
            assert f"row {hit} " in msg
        assert "non-finite" in msg
    ok = x.copy()
    ok[miss, 77] = np.nan
    same_as_model(rq.train_centroids(ok, k, iters=iters, points_per_centroid=ppc, return_stats=True), model_of(oracle, "B"), "NaN outside the sample")
    # an oversize sample: ns * dim = 2^20 * 4096 > 2^31, refused on the numbers alone (nothing is read)
    small = torch.zeros(4096, dtype=torch.float32, device="cuda")
    refused(rq, UNSUPPORTED, lambda: rq.train_centroids_device(small.data_ptr(), 1 << 22, 4096, 1 << 10, small.data_ptr(), points_per_centroid=1 << 10))
    # struct_size is checked
    from rabitq_amd import _lib
    p = _lib.TrainParamsT(iters=1, points_per_centroid=1)
    p.struct_size = 8
    out = np.zeros((4, d), np.float32)
    assert _lib.lib().rq_train_centroids(C.c_void_p(x.ctypes.data), n, d, 4, C.byref(p), C.c_void_p(out.ctypes.data), None, None) == INVALID


def same_index(a, b, what=""):
    assert (a.n, a.k, a.dim, a.metric, a.row_type) == (b.n, b.k, b.dim, b.metric, b.row_type), what
    for name in ARRAYS + ("map_ids",):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), (what, name)


@pytest.mark.parametrize("metric", ["l2", "cosine", "ip"])
def test_build_with_a_list_count_trains_first(rq, metric):
    import torch
    x, _, _ = synth.mixture(6000, 96, 16, sigma=tc.SIGMA, seed=80)
    P = synth.random_orthogonal(128, seed=81)
    cent = rq.train_centroids(x, 16, seed=5, metric=metric)
    assert cent.shape == (16, 97 if metric == "ip" else 96)
    want = rq.RaBitQ.build(x, cent, P, seed=5, metric=metric)
    got = rq.RaBitQ.build(x, 16, P, seed=5, metric=metric)
    same_index(got, want, metric)
    dx = torch.from_numpy(x).cuda()
    dev = rq.RaBitQ.build_device(dx.data_ptr(), 6000, 96, centroids_ptr=None, k=16, orthogonal=P, seed=5, metric=metric)
    same_index(dev, want, metric + " device")
    for i in (want, got, dev):
        i.close()
    if metric == "l2":                                        # typed rows go the same way
        h = x.astype(np.float16)
        a = rq.RaBitQ.build(h, 16, P)
        b = rq.RaBitQ.build(h, rq.train_centroids(h, 16), P)
        same_index(a, b, "f16")
        a.close(), b.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_cli_trains_a_missing_centroid_file(rq, tmp_path, metric, capsys):
    from rabitq_amd import cli, vecs
    x, _, _ = synth.mixture(3000, 64, 8, sigma=tc.SIGMA, seed=82)
    b, c, q, t = (str(tmp_path / f) for f in ("base.fvecs", "cent.fvecs", "query.fvecs", "truth.ivecs"))
    vecs.write_vecs(b, x)
    vecs.write_vecs(q, x[:20] + np.float32(0.01))
    args = ["-b", b, "-c", c, "-q", q, "-t", t, "-k", "5", "-p", "8", "--metric", metric, "--seed", "4", "--make-truth"]
    assert cli.main(args + ["-s", str(tmp_path / "saved"), "--train", "8", "--train-iters", "6"]) == 0
    want = rq.train_centroids(x, 8, iters=6, seed=4, metric=metric)
    got = vecs.read_matrix(c)
    assert got.shape == (8, 65 if metric == "ip" else 64) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert "8 centroids trained" in capsys.readouterr().out
    # an existing file is used as it is
    vecs.write_vecs(c, want[::-1].copy())
    assert cli.main(args + ["-s", str(tmp_path / "saved2"), "--train", "8"]) == 0
    assert np.array_equal(vecs.read_matrix(c), want[::-1])
    assert "centroids trained" not in capsys.readouterr().out


def test_quality_on_the_old_trainers_shape(rq):
    """The shape and the recall of test_kmeans_centroids_give_recall (300 000 x 96, k = 64, nprobe 8, recall >= 0.95), with the
    index built on the new trainer's centroids."""
    import torch
    dev = torch.device("cuda", 0)
    n, d, k = 300_000, 96, 64
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    centres = torch.randn(k, d, generator=g, device=dev)
    u = torch.randint(0, k, (n,), generator=g, device=dev)
    x = (centres[u] + 0.5 * torch.randn(n, d, generator=g, device=dev)).contiguous()
    idx = rq.RaBitQ.build_device(x.data_ptr(), n, d, centroids_ptr=None, k=k, orthogonal=synth.random_orthogonal(128, 2), seed=3)
    assert np.isfinite(idx.centroids).all()
    q = x[:200] + 0.05
    _, ids, cnt = idx.query_batch(q.cpu().numpy(), 8, 10)
    d2 = torch.cdist(q.double(), x.double()) ** 2
    gt = torch.topk(d2, 10, dim=1, largest=False).indices.cpu().numpy()
    recall = np.mean([len(set(ids[j, :10].tolist()) & set(gt[j].tolist())) / 10 for j in range(200)])
    print("recall", recall)
    assert recall >= 0.95, recall
    idx.close()
