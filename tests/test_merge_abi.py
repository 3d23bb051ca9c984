"""CPU-side checks of rq_merge_from / rq_extract: the header declares both entries and the three RQ_MERGE_IDS_* values, the built
library exports them, null handles are RQ_ERR_INVALID with or without a device (the check comes before the device is looked for),
and the Python methods refuse bad arguments before they reach the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def test_header_declares_and_library_exports(L):
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"rq_status\s+rq_merge_from\s*\(\s*rq_index\s*\*\s*dst\s*,\s*rq_index\s*\*\s*src\s*,\s*uint32_t id_mode\s*,"
                     r"\s*uint32_t id_shift\s*,\s*uint32_t\s*\*\s*out_shift\s*\)", code)
    assert re.search(r"rq_status\s+rq_extract\s*\(\s*rq_index\s*\*\s*src\s*,\s*const uint32_t\s*\*\s*id_bits\s*,\s*uint64_t nbits\s*,"
                     r"\s*int bits_on_device\s*,\s*rq_index\s*\*\*\s*out\s*\)", code)
    for name, value in (("KEEP", 0), ("SHIFT", 1), ("APPEND", 2)):
        assert re.search(rf"#define\s+RQ_MERGE_IDS_{name}\s+{value}u\b", code), name
        assert getattr(_lib, f"MERGE_IDS_{name}") == value
    assert re.search(r"#define\s+RQ_EXTRACT_ALL_IDS\s+0xFFFFFFFFFFFFFFFFull\b", code) and _lib.EXTRACT_ALL_IDS == (1 << 64) - 1
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+4\b", code)                 # additions only
    note = hdr.split("#define RQ_ABI_VERSION")[0]
    assert "0.12.0" in note and "rq_merge_from" in note and "rq_extract" in note
    for name in ("rq_merge_from", "rq_extract"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    assert L.rq_abi_version() == 4


def test_null_handles_are_invalid(L):
    shift = C.c_uint32(7)
    out = C.c_void_p(123)
    words = np.ones(1, dtype=np.uint32)
    assert L.rq_merge_from(None, None, 0, 0, C.byref(shift)) == INVALID
    assert L.rq_last_error()
    assert L.rq_extract(None, words.ctypes.data, 32, 0, C.byref(out)) == INVALID
    assert out.value is None                                                  # *out is cleared on every refusal
    assert L.rq_extract(None, words.ctypes.data, 32, 0, None) == INVALID
    from rabitq_amd import _lib
    st = _lib.MutateStatsT()
    assert L.rq_last_mutate_stats(C.byref(st)) == 0 and st.rows_after == 0 and st.ms_assign == 0


def _fake(dim=128):
    """A RaBitQ whose handle is never used: every refusal must come before the library is called."""
    from rabitq_amd.index import RaBitQ
    r = RaBitQ.__new__(RaBitQ)
    r._h = None
    r.dim, r.k, r.n = dim, 4, 10
    return r


@pytest.fixture
def no_library(monkeypatch):
    from rabitq_amd import index as ix

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(ix, "lib", boom)


@pytest.mark.parametrize("ids,exc", [
    ("prepend", ValueError),
    (-1, ValueError),
    (1 << 32, ValueError),
    (1.5, TypeError),
    (None, TypeError),
    (True, TypeError),
    (np.array([1, 2]), TypeError),
])
def test_merge_from_rejects_bad_ids_before_the_library(ids, exc, no_library):
    with pytest.raises(exc):
        _fake().merge_from(_fake(), ids=ids)


def test_merge_from_rejects_bad_others_before_the_library(no_library):
    r = _fake()
    with pytest.raises(TypeError):
        r.merge_from(np.zeros((2, 128), np.float32))
    with pytest.raises(TypeError):
        r.merge_from(None)
    with pytest.raises(ValueError):
        r.merge_from(r)


@pytest.mark.parametrize("kw,exc", [
    ({}, ValueError),                                        # neither ids nor mask
    ({"ids": [1], "mask": [True]}, ValueError),              # both
    ({"ids": np.array([1.5])}, TypeError),
    ({"ids": np.array([-3])}, ValueError),
    ({"ids": np.array([1 << 33], dtype=np.uint64)}, ValueError),   # past 2^32 bits
])
def test_extract_rejects_bad_ids_before_the_library(kw, exc, no_library):
    with pytest.raises(exc):
        _fake().extract(**kw)


def test_the_methods_exist_on_the_public_class():
    import rabitq_amd
    for name in ("merge_from", "extract", "copy"):
        assert callable(getattr(rabitq_amd.RaBitQ, name))
