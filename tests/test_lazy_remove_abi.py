"""CPU-side checks of lazy removal (rq_remove_lazy / rq_compact / rq_pending_removals): the header declares the three
entries, the built library exports them, the ctypes signatures exist, a null handle is RQ_ERR_INVALID with or without a device (the
check comes before the device is looked for), and the Python wrappers refuse bad ids before they reach the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
ENTRIES = ("rq_remove_lazy", "rq_compact", "rq_pending_removals")


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def test_header_declares_the_three_entries():
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"rq_status\s+rq_remove_lazy\s*\(\s*rq_index\s*\*\s*idx\s*,\s*const uint32_t\s*\*\s*id_bits\s*,\s*uint64_t nbits\s*,"
                     r"\s*int bits_on_device\s*,\s*uint64_t\s*\*\s*out_marked\s*\)", code)
    assert re.search(r"rq_status\s+rq_compact\s*\(\s*rq_index\s*\*\s*idx\s*,\s*uint64_t\s*\*\s*out_removed\s*\)", code)
    assert re.search(r"rq_status\s+rq_pending_removals\s*\(\s*const rq_index\s*\*\s*idx\s*,\s*uint64_t\s*\*\s*out_dead\s*\)", code)
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+4\b", code)                 # additions only
    note = hdr.split("#define RQ_ABI_VERSION")[0]
    for name in ENTRIES:
        assert name in note, name                                             # the history line of the version note


def test_library_exports_and_ctypes_signatures(L):
    from rabitq_amd import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 or fn.restype is C.c_int, name
        assert fn.argtypes, name
    assert len(L.rq_remove_lazy.argtypes) == 5 and len(L.rq_compact.argtypes) == 2 and len(L.rq_pending_removals.argtypes) == 2
    assert L.rq_abi_version() == 4


def test_null_handles_are_invalid(L):
    words = np.ones(1, dtype=np.uint32)
    out = C.c_uint64(77)
    assert L.rq_remove_lazy(None, words.ctypes.data, 32, 0, C.byref(out)) == INVALID
    assert L.rq_last_error()
    assert L.rq_compact(None, C.byref(out)) == INVALID
    assert L.rq_pending_removals(None, C.byref(out)) == INVALID
    assert out.value == 77                                                    # nothing is written on a refusal


def _fake(dim=128):
    """A RaBitQ whose handle is never used: every refusal must come before the library is called."""
    from rabitq_amd.index import RaBitQ
    r = RaBitQ.__new__(RaBitQ)
    r._h = None
    r.dim, r.k, r.n, r.pending_removals, r._ip_d = dim, 4, 10, 3, 0
    return r


@pytest.fixture
def no_library(monkeypatch):
    from rabitq_amd import index as ix

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(ix, "lib", boom)


@pytest.mark.parametrize("kw,exc", [
    ({}, ValueError),                                        # neither ids nor mask
    ({"ids": [1], "mask": [True]}, ValueError),              # both
    ({"ids": np.array([1.5])}, TypeError),
    ({"ids": ["a"]}, TypeError),
    ({"ids": np.array([-3])}, ValueError),
    ({"ids": np.array([1 << 33], dtype=np.uint64)}, ValueError),   # past 2^32 bits
])
def test_lazy_remove_rejects_bad_ids_before_the_library(kw, exc, no_library):
    with pytest.raises(exc):
        _fake().remove(lazy=True, **kw)


def test_lazy_update_rejects_bad_ids_before_the_library(no_library):
    with pytest.raises(TypeError):
        _fake().update(np.array([1.5, 2.5]), np.zeros((2, 128), np.float32), lazy=True)
    with pytest.raises(ValueError):
        _fake().update(np.array([4, 4]), np.zeros((2, 128), np.float32), lazy=True)


def test_the_methods_exist_on_the_public_class():
    import inspect
    import rabitq_amd
    for name in ("remove", "compact", "update"):
        assert callable(getattr(rabitq_amd.RaBitQ, name))
    assert inspect.signature(rabitq_amd.RaBitQ.remove).parameters["lazy"].default is False
    assert inspect.signature(rabitq_amd.RaBitQ.update).parameters["lazy"].default is False
    assert isinstance(rabitq_amd.RaBitQ.live_n, property)
    assert _fake().live_n == 7
