"""The boundary of the exact search on split-row and tiered indexes: the header declares the four entries with the arguments of the
plain ones, the built library exports them, the ctypes mirror lists them with the header's arity, the refusals that need no device
are made before one is looked for, and the Python layer has its methods.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"rq_exact_search_tiered": "rq_exact_search", "rq_exact_search_tiered_device": "rq_exact_search_device",
         "rq_exact_range_search_tiered": "rq_exact_range_search", "rq_exact_range_search_tiered_device": "rq_exact_range_search_device"}
INVALID = -1


def declared_params(code, name):
    m = re.search(r"\brq_status\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_header_declares_library_exports_and_mirror_matches():
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "rq_exact_search_tiered" in hdr.split("#define RQ_ABI_VERSION")[0]     # the revision note names the addition
    _lib.build()
    L = _lib.lib()
    for name, plain in PAIRS.items():
        assert name in _lib.EXPORTS, name
        assert declared_params(code, name) == declared_params(code, plain)       # the same arguments as the plain entry
        assert getattr(L, name).argtypes == getattr(L, plain).argtypes


def test_null_arguments_are_refused_before_a_device_is_looked_for_and_an_empty_batch_is_ok():
    from rabitq_amd import _lib
    _lib.build()
    L = _lib.lib()
    buf = (C.c_uint8 * 64)()
    junk = C.c_void_p(C.addressof(buf))   # a non-null address that is never dereferenced
    h = C.c_void_p()
    for name in ("rq_exact_search_tiered", "rq_exact_search_tiered_device"):
        fn = getattr(L, name)
        assert fn(None, None, junk, 1, 64, 10, None, junk, junk, junk) == INVALID
        assert fn(junk, None, None, 1, 64, 10, None, junk, junk, junk) == INVALID
        assert fn(junk, None, junk, 1, 64, 10, None, junk, junk, None) == INVALID
        assert b"null" in L.rq_last_error()
        assert fn(junk, None, None, 0, 64, 10, None, junk, junk, junk) == 0
    for name in ("rq_exact_range_search_tiered", "rq_exact_range_search_tiered_device"):
        fn = getattr(L, name)
        assert fn(None, None, junk, 1, 64, junk, None, C.byref(h)) == INVALID and not h.value
        assert fn(junk, None, junk, 1, 64, None, None, C.byref(h)) == INVALID
        assert fn(junk, None, junk, 1, 64, junk, None, None) == INVALID


def test_python_surface():
    import rabitq_amd
    R = rabitq_amd.RaBitQ
    for name in ("exact_search", "exact_search_device", "exact_range_search", "exact_range_search_device"):
        tiered = getattr(R, name.replace("search", "search_tiered"))
        assert list(inspect.signature(tiered).parameters) == list(inspect.signature(getattr(R, name)).parameters)
    for name in ("recall", "tune_nprobe"):
        assert inspect.signature(getattr(R, name)).parameters["tiered"].default is False
