"""The boundary of the complete exact grouped search: the header declares the new entries and the built library exports them, the
ctypes mirror lists them with the header's arity and the stats struct with gcc's layout, the history block names the addition, every
refusal that needs no device returns its status without one, and the Python layer has its methods.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rq_exact_search_grouped_full": 14, "rq_exact_search_grouped_full_device": 14, "rq_last_group_full_stats": 1}
INVALID, UNSUPPORTED = -1, -6


def test_header_declares_library_exports_and_mirror_matches():
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+4\b", code)                 # additions only
    note = hdr.split("#define RQ_ABI_VERSION")[0]
    assert "0.22.0: the complete exact grouped search, additions only" in note and "rq_group_full_stats_t" in note
    _lib.build()
    L = _lib.lib()
    params = {}
    for name, arity in ENTRIES.items():
        m = re.search(r"\brq_status\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        params[name] = [re.sub(r"\b(d_)?(\w+)$", r"\2", p.strip()) for p in m.group(1).split(",")]
        assert name in _lib.EXPORTS and name.replace("_device", "") in note and len(params[name]) == arity == len(getattr(L, name).argtypes), name
    assert params["rq_exact_search_grouped_full"] == params["rq_exact_search_grouped_full_device"]


def test_stats_layout_matches_the_header(tmp_path):
    from rabitq_amd import _lib
    S = _lib.GroupFullStatsT
    body = '    printf("%zu", sizeof(rq_group_full_stats_t));\n' + "".join(
        '    printf(" %%zu", offsetof(rq_group_full_stats_t, %s));\n' % f for f, _ in S._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rabitq_hip.h"\nint main(void) {\n' + body + '    return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "layout")]).decode().split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_] and C.sizeof(S) == 80 == S().struct_size


@pytest.mark.parametrize("dev", ["", "_device"])
def test_refusals_come_before_a_device_is_looked_for(dev):
    """RQ_ERR_INVALID / RQ_ERR_UNSUPPORTED (not RQ_ERR_NO_DEVICE) on a machine without a GPU too.  `fake` is a non-null address
    that is never dereferenced: the checks that need nothing of the index or the postings come first."""
    from rabitq_amd import _lib
    _lib.build()
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint64)
    fake, null = C.c_void_p(buf.ctypes.data), C.c_void_p(0)

    def prm(topk=2, g=2, fetch=0, flags=0, size=None):
        p = _lib.GroupParamsT(topk=topk, group_size=g, fetch=fetch, flags=flags)
        if size is not None:
            p.struct_size = size
        return C.byref(p)

    def call(idx=fake, post=fake, q=fake, p=None, outs=(fake,) * 6):
        return getattr(L, "rq_exact_search_grouped_full" + dev)(idx, post, null, q, 4, 64, None, prm() if p is None else p, *outs)

    for kw in (dict(idx=null), dict(post=null), dict(q=null), dict(p=C.cast(null, C.POINTER(_lib.GroupParamsT)))):
        assert call(**kw) == INVALID and b"null argument" in L.rq_last_error(), kw
    for k in range(5):                                                         # every output but out_fetched
        assert call(outs=tuple(null if j == k else fake for j in range(6))) == INVALID and b"null argument" in L.rq_last_error(), k
    for size in (0, 16, 24):
        assert call(p=prm(size=size)) == INVALID and b"struct_size" in L.rq_last_error()
    assert call(p=prm(flags=1)) == INVALID and b"flags" in L.rq_last_error()
    assert call(p=prm(fetch=64)) == INVALID and b"fetch must be 0" in L.rq_last_error()
    for bad in (dict(topk=0), dict(g=0), dict(topk=2049), dict(topk=683, g=3), dict(topk=1 << 31, g=2)):
        assert call(p=prm(**bad)) == UNSUPPORTED and b"topk * group_size <= 2048" in L.rq_last_error(), bad
    assert L.rq_last_group_full_stats(None) == INVALID
    st = _lib.GroupFullStatsT()
    st.struct_size = 0
    assert L.rq_last_group_full_stats(C.byref(st)) == INVALID                 # an unset struct_size, as every sized struct


def test_python_surface():
    import rabitq_amd as rq
    from rabitq_amd.index import CompleteGroupedResult as Complete
    assert callable(rq.RaBitQ.exact_search_grouped_full_device) and callable(rq.RaBitQ.last_group_full_stats) and callable(rq.last_group_full_stats)
    assert issubclass(Complete, rq.GroupedResult) and Complete.complete and not rq.GroupedResult.complete
