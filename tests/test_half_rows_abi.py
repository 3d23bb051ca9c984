"""Half-precision rows without a GPU: the new entry points are exported, declared in the header and mirrored in _lib.py, and the
CPU model of the two roundings (tests/half_model.py) is the conversion torch's CPU tensors perform.

Run:  python -m pytest tests/test_half_rows_abi.py -m "not gpu" -q
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import half_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rq_build_rows", "rq_build_device_rows", "rq_builder_create_rows", "rq_builder_assign_chunk_rows", "rq_builder_place_chunk_rows",
       "rq_from_arrays_rows", "rq_row_type", "rq_widen", "rq_widen_device"]


def test_new_symbols_are_exported_declared_and_mirrored():
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rq_[a-z_0-9]+)\s*\(", hdr))
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    L = C.CDLL(_lib.SO_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(L, name) is not None, name
    assert re.search(r"RQ_ROWS_F32\s*=\s*0\s*,\s*RQ_ROWS_F16\s*=\s*1\s*,\s*RQ_ROWS_BF16\s*=\s*2", hdr)
    assert (_lib.ROWS_F32, _lib.ROWS_F16, _lib.ROWS_BF16) == (0, 1, 2)
    assert re.search(r"RQ_ARR_FACTORS\s*,\s*RQ_ARR_BASE_ROWS", hdr)   # = 7, the one after RQ_ARR_FACTORS = 6
    from rabitq_amd import index as ix
    assert ix.ARR_BASE_ROWS == 7 and ix.ARR_FACTORS == 6
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+4\b", hdr) and _lib.ABI_VERSION == 4


def test_the_ctypes_prototypes_have_the_headers_arity():
    """argtypes of every new entry against the parameter count of its declaration."""
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        assert len(getattr(L, name).argtypes) == len([p for p in m.group(1).split(",") if p.strip()]), name


def edge_values():
    f = np.float32
    allh = np.arange(65536, dtype=np.uint16)
    vals = [hm.widen(allh, "f16").view(np.uint32), hm.widen(allh, "bf16").view(np.uint32)]
    h16 = vals[0][~hm.nan_patterns("f16")]
    hbf = vals[1][~hm.nan_patterns("bf16")]
    # ties and their neighbours: half an ulp of the target above every representable value, and one f32 ulp to either side
    vals += [h16 + np.uint32(0x1000), h16 + np.uint32(0x0FFF), h16 + np.uint32(0x1001)]
    vals += [hbf + np.uint32(0x8000), hbf + np.uint32(0x7FFF), hbf + np.uint32(0x8001)]
    sub = np.linspace(0.0, 2.0 ** -13, 50001, dtype=f).view(np.uint32)   # the f16 subnormal range and its ties
    vals += [sub, sub | np.uint32(0x80000000)]
    vals.append(np.array([0x00000000, 0x80000000, 0x33000000, 0x33000001, 0x32FFFFFF, 0x477FE000, 0x477FEFFF, 0x477FF000, 0x477FF001,
                          0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00000001, 0x007FFFFF, 0x00800000], dtype=np.uint32))
    v = np.concatenate(vals).view(f)
    return v[~np.isnan(v)]


@pytest.mark.parametrize("rows", hm.TYPES)
def test_model_rounding_is_torchs_cpu_conversion(rows):
    import torch
    rng = np.random.default_rng(11)
    v = rng.integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    v = np.concatenate([v[~np.isnan(v)], edge_values()])
    t = torch.from_numpy(v).to(torch.float16 if rows == "f16" else torch.bfloat16)
    want = t.view(torch.int16).numpy().view(np.uint16)
    got = hm.narrow(v, rows)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    back = t.to(torch.float32).numpy()
    assert np.array_equal(hm.widen(got, rows).view(np.uint32), back.view(np.uint32))


@pytest.mark.parametrize("rows", hm.TYPES)
def test_widening_then_rounding_is_the_identity(rows):
    """W(R_t(W(h))) == W(h) for every non-NaN pattern (and R_t(W(h)) == h); a NaN stays a NaN."""
    h = np.arange(65536, dtype=np.uint16)
    nan = hm.nan_patterns(rows)
    w = hm.widen(h, rows)
    assert np.array_equal(np.isnan(w), nan)
    r = hm.narrow(w, rows)
    assert np.array_equal(r[~nan], h[~nan])
    assert np.array_equal(hm.widen(r, rows).view(np.uint32)[~nan], w.view(np.uint32)[~nan])
    assert np.isnan(hm.widen(r, rows)[nan]).all()
