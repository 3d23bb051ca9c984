"""Cosine metric, the part that needs no GPU: the new exports are declared and exported, the enum values, rq_info_t.metric at the
old reserved0 offset, the Python surface, and the CPU model of the normalisation (tests/cosine_model.py) against plain float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cosine_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rq_build_metric", "rq_build_device_metric", "rq_build_from_path_metric", "rq_builder_create_metric", "rq_from_arrays_metric",
       "rq_normalize", "rq_normalize_device"]


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def header():
    return open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()


def test_new_exports_are_declared_and_exported(L):
    from rabitq_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # every *_metric entry is its L2 twin's signature with `uint32_t metric` before `out`
    for name in NEW[:5]:
        twin = name[:-len("_metric")]
        sig = lambda n: re.sub(r"\s+", " ", re.search(r"rq_status %s\((.*?)\);" % n, code, flags=re.S).group(1))
        assert sig(name).replace("uint32_t metric, ", "").replace(" ", "") == sig(twin).replace(" ", ""), name


def test_header_revision_and_enum(L, tmp_path):
    hdr = header()
    assert "0.8.0: cosine metric" in hdr and "#define RQ_ABI_VERSION 4" in hdr
    assert L.rq_abi_version() == 4
    src = tmp_path / "m.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rabitq_hip.h"\nint main(void) {\n'
                   '    printf("%d %d %zu %zu %zu\\n", RQ_METRIC_L2, RQ_METRIC_COSINE, sizeof(rq_info_t), offsetof(rq_info_t, metric), '
                   'offsetof(rq_info_t, split_rows));\n    return 0;\n}\n')
    exe = tmp_path / "m"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals == [0, 1, 40, 36, 32]


def test_info_mirror_has_metric_at_the_reserved_offset():
    from rabitq_amd import _lib
    assert C.sizeof(_lib.Info) == 40
    assert _lib.Info.metric.offset == 36 and _lib.Info.metric.size == 4 and _lib.Info.split_rows.offset == 32
    assert not hasattr(_lib.Info, "reserved0")
    assert (_lib.METRIC_L2, _lib.METRIC_COSINE) == (0, 1)
    assert _lib.metric_id("l2") == 0 and _lib.metric_id("cosine") == 1 and _lib.metric_id("Cosine") == 1
    with pytest.raises(ValueError):
        _lib.metric_id("dot")


def test_python_surface():
    import inspect
    import rabitq_amd
    from rabitq_amd import cli
    for fn in (rabitq_amd.RaBitQ.from_path, rabitq_amd.RaBitQ.build, rabitq_amd.RaBitQ.build_device, rabitq_amd.RaBitQ.builder,
               rabitq_amd.RaBitQ.from_arrays):
        assert inspect.signature(fn).parameters["metric"].default == "l2", fn
    assert rabitq_amd.normalize is rabitq_amd.ops.normalize
    d = np.array([0.0, 0.5, 2.0, 4.0], dtype=np.float32)
    assert np.array_equal(rabitq_amd.cosine_similarity(d), np.array([1.0, 0.75, 0.0, -1.0]))
    base = ["-b", "b", "-c", "c", "-q", "q", "-t", "t", "-s", "s"]
    assert cli.build_parser().parse_args(base).metric == "l2"
    a = cli.build_parser().parse_args(base + ["--metric", "cosine", "-h"])
    assert a.metric == "cosine" and a.heuristic_rank          # the reference's flags keep their letters
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--metric", "dot"])


def test_no_cpu_fallback_for_normalize(L):
    import torch
    if torch.cuda.is_available():
        return   # (the GPU suite runs it for real)
    import rabitq_amd
    with pytest.raises(rabitq_amd.RabitqError) as e:
        rabitq_amd.normalize(np.ones((2, 64), np.float32))
    assert e.value.status == -5


@pytest.mark.parametrize("d", [64, 100, 128, 768, 4096])
def test_model_unit_norm(oracle, d):
    """The model's rows have norm 1 in float64 within the normalisation's own error bound, and are the f64 quotient within it."""
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((50, d)) * rng.uniform(1e-3, 1e3, (50, 1))).astype(np.float32)
    nx = cm.normalize_rows(oracle, x)
    dim = (d + 63) // 64 * 64
    assert nx.shape == (50, dim) and nx.dtype == np.float32
    assert not nx[:, d:].any()                                    # the padding stays zero
    n64 = np.sqrt((nx.astype(np.float64) ** 2).sum(axis=1))
    bound = cm.unit_error_bound(dim)
    assert np.abs(n64 - 1.0).max() <= bound, (np.abs(n64 - 1.0).max(), bound)
    exact = x.astype(np.float64) / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))[:, None]
    assert np.abs(nx[:, :d] - exact).max() <= bound


def test_model_identity_cases(oracle):
    f = np.float32
    rows = np.zeros((7, 128), dtype=np.float32)
    rows[1, :4] = [f(1e-30), f(-1e-30), f(1e-25), f(0.0)]         # s underflows: norm subnormal (or zero) -> identity
    rows[2, :3] = [f(3e38), f(3e38), f(-1e38)]                    # s overflows to inf -> identity
    rows[3, :3] = [f(np.inf), f(1.0), f(-2.0)]
    rows[4, :3] = [f(np.nan), f(1.0), f(-2.0)]
    rows[5, :] = f(-0.0)                                         # negative zeros: a zero row, bit for bit
    rows[6, :4] = [f(3.0), f(-0.0), f(4.0), f(0.0)]                # a normal row: signs of zero survive the division
    nx = cm.normalize_rows(oracle, rows)
    for i in range(6):
        assert np.array_equal(nx[i].view(np.uint32), rows[i].view(np.uint32)), i
    assert np.array_equal(nx[6, :4].view(np.uint32), np.array([0.6, -0.0, 0.8, 0.0], dtype=np.float32).view(np.uint32))
    # the smallest normal norm is divided by; just below it is not
    tiny = np.zeros((2, 64), dtype=np.float32)
    tiny[0, 0] = f(2.0 ** -63)          # s = 2^-126 = FLT_MIN, nrm = 2^-63: normal
    tiny[1, 0] = f(2.0 ** -75)          # s = 2^-150 -> 0 (or subnormal): identity
    nt = cm.normalize_rows(oracle, tiny)
    assert nt[0, 0] == 1.0 and nt[1, 0] == tiny[1, 0]


def test_model_padding_d100(oracle):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20, 100)).astype(np.float32)
    a = cm.normalize_rows(oracle, x)
    b = cm.normalize_rows(oracle, cm.pad64(x))                    # padding first or inside: the same rows
    assert a.shape == (20, 128) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(cm.normalize_rows(oracle, x[3]), a[3:4])
