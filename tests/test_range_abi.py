"""CPU-side checks of the range-search boundary: the new names are in include/rabitq_hip.h, in the library's exports and in the
ctypes mirror with matching argument counts, and the header says what freeing NULL does."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["rq_range_search", "rq_range_search_device", "rq_range_result_info", "rq_range_result_device_ptrs", "rq_range_result_copy",
         "rq_range_result_free"]


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()


def _declarations():
    """name -> number of parameters, from the header's prototypes (comments removed)."""
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(rq_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", hdr):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_names_in_header_exports_and_mirror(L):
    from rabitq_amd import _lib
    decl = _declarations()
    for name in NAMES:
        assert name in decl, name
        assert name in _lib.EXPORTS, name
        fn = getattr(L, name)            # AttributeError if the library does not export it
        assert len(fn.argtypes) == decl[name], (name, len(fn.argtypes), decl[name])
    assert decl["rq_range_search"] == decl["rq_range_search_device"] == 8
    assert L.rq_range_result_free.restype is None
    assert "typedef struct rq_range_result rq_range_result;" in _header()


def test_header_documents_the_contract():
    hdr = _header()
    assert re.search(r"rq_range_result_free\(NULL\)\s+is\s+a\s+no-op", hdr)
    assert "0.7.0" in hdr and "range search" in hdr and "#define RQ_ABI_VERSION 4" in hdr


def test_python_surface():
    import rabitq_amd
    assert hasattr(rabitq_amd.RaBitQ, "range_search") and hasattr(rabitq_amd.RaBitQ, "range_search_device")
    for attr in ("device_ptrs", "to_host", "close", "__enter__", "__exit__"):
        assert hasattr(rabitq_amd.RangeResult, attr), attr


def test_freeing_null_and_refusing_without_a_device(L):
    import ctypes as C
    import torch
    L.rq_range_result_free(None)     # a no-op, with or without a device
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h = C.c_void_p(0xDEAD)
    q = (C.c_float * 64)()
    r = (C.c_float * 1)(1.0)
    st = L.rq_range_search(C.c_void_p(1), None, C.cast(q, C.c_void_p), 1, 64, 1, C.cast(r, C.c_void_p), C.byref(h))
    assert st == -5 and h.value is None      # RQ_ERR_NO_DEVICE: no CPU answer, *out NULL
