"""The boundary of the exact range search: the header declares the two entries, the built library exports them, the ctypes mirror
lists them with the header's arity, and the Python layer has its methods.  No GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rq_exact_range_search", "rq_exact_range_search_device")


def declared_params(code, name):
    """The parameter list of `rq_status name(...)` in the header's code (comments removed), split at the commas."""
    m = re.search(r"\brq_status\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_library_exports_and_mirror_matches():
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+4\b", code)                 # additions only
    assert "rq_exact_range_search" in hdr.split("#define RQ_ABI_VERSION")[0]  # the revision note names the addition
    _lib.build()
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.EXPORTS, name
        params = declared_params(code, name)
        assert len(params) == 8 and params[-1].replace(" ", "") == "rq_range_result**out", params
        assert "rq_exact_params_t" in params[6] and "radius" in params[5]
        fn = getattr(L, name)                                                # AttributeError if the library lacks the symbol
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), len(params))
    # the same parameters, host and device entry
    strip = lambda ps: [re.sub(r"\b(d_)?(\w+)$", r"\2", p) for p in ps]
    assert strip(declared_params(code, ENTRIES[0])) == strip(declared_params(code, ENTRIES[1]))


def test_python_surface():
    import inspect
    import rabitq_amd
    R = rabitq_amd.RaBitQ
    assert list(inspect.signature(R.exact_range_search).parameters) == ["self", "queries", "radius", "filter", "min_ip", "params"]
    assert list(inspect.signature(R.exact_range_search_device).parameters) == ["self", "q_ptr", "nq", "length", "radius_ptr", "filter", "params"]
    assert list(inspect.signature(R.range_recall).parameters) == ["self", "queries", "probe", "radius", "filter", "min_ip"]
