"""Inner-product metric (RQ_METRIC_IP), the part that needs no GPU: the ABI additions, the Python / CLI surface and the CPU model
(tests/ip_model.py).  Run:  python -m pytest tests/test_ip_abi.py -m "not gpu" -q
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ip_model as im
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rq_build_ip", "rq_build_device_ip", "rq_build_from_path_ip", "rq_builder_create_ip", "rq_from_arrays_ip", "rq_ip_params",
       "rq_augment", "rq_augment_device", "rq_row_sqnorm_max", "rq_row_sqnorm_max_device", "rq_ip_from_dist", "rq_ip_from_dist_device",
       "rq_ip_radius", "rq_ip_radius_device"]
F32 = np.float32


def header():
    return open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    return C.CDLL(_lib.SO_PATH)


def test_exports_declared_and_present(L):
    from rabitq_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    sig = lambda n: re.sub(r"\s+", " ", re.search(r"rq_status %s\((.*?)\);" % n, code, flags=re.S).group(1)).replace(" ", "")
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # the builds are their L2 twins' signatures plus `uint32_t centroid_cols, float sq_bound` before `out`
    for name in ("rq_build_ip", "rq_build_device_ip", "rq_builder_create_ip"):
        assert sig(name).replace("uint32_tcentroid_cols,floatsq_bound,", "") == sig(name[:-len("_ip")]), name
    assert sig("rq_build_from_path_ip").replace("floatsq_bound,", "") == sig("rq_build_from_path")   # (centroid_cols: the records' length)
    assert sig("rq_from_arrays_ip").replace("uint32_td,floatsq_bound,", "") == sig("rq_from_arrays")


def test_header_revision_enum_and_info_size(L, tmp_path):
    hdr = header()
    assert "0.9.0: inner-product metric, additions only" in hdr and "#define RQ_ABI_VERSION 4" in hdr
    assert L.rq_abi_version() == 4
    src = tmp_path / "m.c"
    src.write_text('#include <stdio.h>\n#include "rabitq_hip.h"\nint main(void) {\n'
                   '    printf("%d %d %d %zu\\n", RQ_METRIC_L2, RQ_METRIC_COSINE, RQ_METRIC_IP, sizeof(rq_info_t));\n    return 0;\n}\n')
    exe = tmp_path / "m"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [0, 1, 2, 40]


def test_python_surface():
    import inspect
    import rabitq_amd
    from rabitq_amd import _lib, cli
    assert _lib.METRIC_IP == 2 and _lib.metric_id("ip") == 2 and _lib.metric_id("IP") == 2 and C.sizeof(_lib.Info) == 40
    with pytest.raises(ValueError):
        _lib.metric_id("dot")
    R = rabitq_amd.RaBitQ
    for fn in (R.from_path, R.build, R.build_device, R.builder, R.from_arrays):
        p = inspect.signature(fn).parameters
        assert p["metric"].default == "l2" and p["max_sq_norm"].default is None, fn
    assert isinstance(R.ip_params, property) and callable(R.inner_product)
    assert inspect.signature(R.range_search).parameters["min_ip"].default is None
    assert rabitq_amd.augment is rabitq_amd.ops.augment and rabitq_amd.row_sqnorm_max is rabitq_amd.ops.row_sqnorm_max
    base = ["-b", "b", "-c", "c", "-q", "q", "-t", "t", "-s", "s"]
    a = cli.build_parser().parse_args(base + ["--metric", "ip", "-h"])
    assert a.metric == "ip" and a.heuristic_rank
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--metric", "dot"])


def test_no_cpu_fallback(L):
    import torch
    if torch.cuda.is_available():
        return   # (the GPU suite runs them for real)
    import rabitq_amd
    for call in (lambda: rabitq_amd.augment(np.ones((2, 64), np.float32)), lambda: rabitq_amd.row_sqnorm_max(np.ones((2, 64), np.float32)),
                 lambda: rabitq_amd.RaBitQ.build(np.ones((4, 64), np.float32), np.ones((1, 64), np.float32), metric="ip")):
        with pytest.raises(rabitq_amd.RabitqError) as e:
            call()
        assert e.value.status == -5


# ---- the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [63, 64, 100, 128, 768, 4095])
def test_model_identities_in_float64(oracle, d):
    """|A(x)|^2 = S and D = S + |q|^2 - 2<x, q>, both in float64 on the model's f32 rows.
    Tolerances: |A|^2 is off S by at most aug_sq_error_bound(dim) * S (derived there from the chain length dim/8 + 3, as
    cosine_model.unit_error_bound is).  D is then exact algebra on the f32 rows A(x) and Q(q): |A - Q|^2 = |A|^2 + |q|^2 - 2<x, q>
    holds in exact arithmetic, so in float64 only |A|^2 - S and float64's own rounding (dim terms, < dim * 2^-52 of the
    magnitudes) remain."""
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((40, d)) * np.exp2(rng.uniform(-3, 3, (40, 1)))).astype(F32)
    q = rng.standard_normal((5, d)).astype(F32)
    S = im.auto_bound(oracle, x)
    dim = im.ip_dim(d)
    ax = im.augment_rows(oracle, x, S)
    assert ax.shape == (40, dim) and ax.dtype == F32 and dim == (d // 64 + 1) * 64
    assert np.array_equal(ax[:, :d].view(np.uint32), x.view(np.uint32)) and not ax[:, d + 1:].any()
    assert not im.invalid_rows(oracle, x, S).any() and (ax[:, d] >= 0).all() and (ax[:, d] == 0).sum() >= 1   # the longest row sits on the sphere
    a64, S64 = ax.astype(np.float64), float(S)
    bound = im.aug_sq_error_bound(dim)
    err = np.abs((a64 ** 2).sum(axis=1) - S64).max() / S64
    assert err <= bound, (err, bound)
    qq = im.pad_cols(q, dim).astype(np.float64)
    D = ((a64[None, :, :] - qq[:, None, :]) ** 2).sum(axis=2)
    want = S64 + (qq ** 2).sum(axis=1)[:, None] - 2.0 * (qq[:, :d] @ x.astype(np.float64).T)
    assert np.abs(D - want).max() <= bound * S64 + dim * 2.0 ** -52 * np.abs(want).max()


def test_model_edge_rows(oracle):
    f = F32
    for d in (63, 64, 100):
        dim = im.ip_dim(d)
        assert dim == (64 if d == 63 else 128)       # d = 63: the slot is the last column; d = 64: it opens a new word
        rows = np.zeros((3, d), f)
        rows[0, :2] = [3.0, 4.0]                     # s = 25 = S: slot +0
        rows[2, 1] = -2.0
        a = im.augment_rows(oracle, rows, 25.0)
        assert a.shape == (3, dim)
        assert a[0, d] == 0 and not np.signbit(a[0, d])
        assert a[1, d] == f(5.0) and not a[1, :d].any()          # a zero row: sqrtf(S)
        assert a[2, d] == np.sqrt(f(21.0), dtype=f)
        assert not a[:, d + 1:].any()
    z = np.zeros((4, 100), f)                         # S = 0 with an all-zero base
    assert im.auto_bound(oracle, z) == 0 and not im.invalid_rows(oracle, z, 0.0).any() and not im.augment_rows(oracle, z, 0.0).any()
    x = np.random.default_rng(1).standard_normal((6, 100)).astype(f)
    s = im.sqnorms(oracle, x)
    below = np.nextafter(s[2], f(0))                  # s one ulp above S is refused, s == S is not
    assert im.invalid_rows(oracle, x, below)[2] and not im.invalid_rows(oracle, x, s[2])[2]
    bad = x.copy()
    bad[1, 5], bad[4, 99] = np.inf, np.nan
    assert np.array_equal(im.invalid_rows(oracle, bad, 1e30), [False, True, False, False, True, False])
    # the conversions, in f32 steps
    q = x[:2]
    D = np.array([[1.5, 2.5], [0.25, 8.0]], f)
    sq = im.sqnorms(oracle, q)
    assert np.array_equal(im.ip_from_dist(oracle, 9.0, q, D), (f(0.5) * ((f(9.0) + sq)[:, None] - D)).astype(f))
    assert np.array_equal(im.ip_radius(oracle, 9.0, q, [1.0, -2.0]), ((f(9.0) + sq) - f(2.0) * np.array([1.0, -2.0], f)).astype(f))


def planted_case(seed=17):
    """2 000 x 100 mixture rows, 8 lists, 32 queries; row 50 * b + 7 is replaced by 4 * query b."""
    n, d, k, nq = 2000, 100, 8, 32
    x, centres, _ = synth.mixture(n, d, k, sigma=0.6, seed=seed, centre_scale=0.5)
    q, _, _ = synth.mixture(nq, d, k, sigma=0.6, seed=seed + 1, centre_scale=0.5)
    planted = 50 * np.arange(nq) + 7
    x = np.ascontiguousarray(x)
    x[planted] = F32(4.0) * q
    return x, centres, synth.random_orthogonal(im.ip_dim(d), seed=seed + 2), np.ascontiguousarray(q), planted.astype(np.uint32)


def test_direction_planted_rows_on_the_oracle(oracle):
    """Ascending L2 order on the augmented rows is descending inner-product order: the planted row 4q has the largest inner product
    with q by far (4|q|^2 against |x||q| cos), so the oracle must return it first -- under the heap ranker's ascending view and as
    the heuristic ranker's first result -- with every list probed."""
    x, centres, P, q, planted = planted_case()
    ip = q.astype(np.float64) @ x.astype(np.float64).T
    assert np.array_equal(ip.argmax(axis=1), planted)                         # (the premise, in float64)
    S = im.auto_bound(oracle, x)
    oidx = im.ip_oracle(oracle, x, centres, P, S)
    qq = im.pad_cols(q, oidx.dim)
    try:
        for b in range(q.shape[0]):
            od, oi = oidx.query(qq[b], 8, 10, False)
            assert oi[np.lexsort((oi, od))[0]] == planted[b], b
            od, oi = oidx.query(qq[b], 8, 10, True)
            assert oi[0] == planted[b], b
    finally:
        oidx.close()
