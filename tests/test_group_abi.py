"""The boundary of grouped search: the header declares every new entry and the built library exports it, the ctypes mirror lists
it with the header's arity and the structs with gcc's layout, the history block names the addition, every refusal that needs no
device returns its status without one, and the Python layer has its methods.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rq_query_batch_grouped": 15, "rq_query_batch_grouped_device": 15, "rq_exact_search_grouped": 14,
           "rq_exact_search_grouped_device": 14, "rq_group_results": 12, "rq_group_results_device": 12, "rq_last_group_stats": 1}
INVALID, UNSUPPORTED = -1, -6


def declared_params(code, name):
    m = re.search(r"\brq_status\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_library_exports_and_mirror_matches():
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+4\b", code)                 # additions only
    note = hdr.split("#define RQ_ABI_VERSION")[0]
    assert "0.16.0: grouped search, additions only" in note                   # the history block names the addition
    for name in ("rq_group_params_t", "rq_group_stats_t", "rq_query_batch_grouped", "rq_exact_search_grouped", "rq_group_results",
                 "rq_last_group_stats"):
        assert name in note, name
    _lib.build()
    L = _lib.lib()
    assert L.rq_abi_version() == 4
    strip = lambda ps: [re.sub(r"\b(d_)?(\w+)$", r"\2", p) for p in ps]
    for name, arity in ENTRIES.items():
        assert name in _lib.EXPORTS, name
        params = declared_params(code, name)
        assert len(params) == arity, (name, params)
        fn = getattr(L, name)                                                 # AttributeError if the library lacks the symbol
        assert len(fn.argtypes) == arity, (name, len(fn.argtypes))
    for name in ("rq_query_batch_grouped", "rq_exact_search_grouped", "rq_group_results"):   # the same parameters, host and device
        assert strip(declared_params(code, name)) == strip(declared_params(code, name + "_device")), name


def test_struct_layouts_match_the_header(tmp_path):
    from rabitq_amd import _lib
    structs = {"rq_group_params_t": _lib.GroupParamsT, "rq_group_stats_t": _lib.GroupStatsT}
    body = ""
    for cname, S in structs.items():
        body += '    printf("%%zu", sizeof(%s));\n' % cname
        body += "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in S._fields_)
        body += '    printf("\\n");\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rabitq_hip.h"\nint main(void) {\n' + body + '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    for line, (cname, S) in zip(lines, structs.items()):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_], cname
    assert C.sizeof(_lib.GroupParamsT) == 20 and C.sizeof(_lib.GroupStatsT) == 56
    assert _lib.GroupParamsT().struct_size == 20 and _lib.GroupStatsT().struct_size == 56
    assert [n for n, _ in _lib.GroupParamsT._fields_] == ["struct_size", "topk", "group_size", "fetch", "flags"]
    assert [n for n, _ in _lib.GroupStatsT._fields_][1:9] == ["fetch", "ms_source", "ms_group", "candidates", "absent", "kept", "groups",
                                                               "directory_built"]


def test_refusals_come_before_a_device_is_looked_for():
    """RQ_ERR_INVALID / RQ_ERR_UNSUPPORTED (not RQ_ERR_NO_DEVICE) on a machine without a GPU too.  `fake` is a non-null "index"
    that is never dereferenced: the checks that need nothing of the index come first."""
    from rabitq_amd import _lib
    _lib.build()
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint64)
    fake, null = C.c_void_p(buf.ctypes.data), C.c_void_p(0)
    o = fake                                                                   # any non-null address: nothing is written

    def prm(topk=2, g=2, fetch=8, flags=0, size=None):
        p = _lib.GroupParamsT(topk=topk, group_size=g, fetch=fetch, flags=flags)
        if size is not None:
            p.struct_size = size
        return C.byref(p)

    def query(idx=fake, q=fake, col=b"doc", p=None, outs=(o, o, o, o, o, o), dev=""):
        return getattr(L, "rq_query_batch_grouped" + dev)(idx, null, q, 4, 64, 8, 0, col, prm() if p is None else p, *outs)

    def exact(idx=fake, q=fake, col=b"doc", p=None, outs=(o, o, o, o, o, o), dev=""):
        return getattr(L, "rq_exact_search_grouped" + dev)(idx, null, q, 4, 64, None, col, prm() if p is None else p, *outs)

    def results(idx=fake, src=(fake, fake, fake), col=b"doc", p=None, outs=(o, o, o, o, o), dev=""):
        return getattr(L, "rq_group_results" + dev)(idx, *src, 4, col, prm() if p is None else p, *outs)

    for dev in ("", "_device"):
        for call in (query, exact, results):
            assert call(idx=null, dev=dev) == INVALID and b"null index" in L.rq_last_error()
            assert call(col=None, dev=dev) == INVALID and b"null argument" in L.rq_last_error()
            assert call(p=C.cast(null, C.POINTER(_lib.GroupParamsT)), dev=dev) == INVALID and b"null argument" in L.rq_last_error()
            n_out = 5 if call is results else 6
            for k in range(5):                                                 # every output but out_fetched
                outs = tuple(null if j == k else o for j in range(n_out))
                assert call(outs=outs, dev=dev) == INVALID and b"null argument" in L.rq_last_error(), (call.__name__, k)
            # a wrong struct_size, a set flag
            for size in (0, 16, 24):
                assert call(p=prm(size=size), dev=dev) == INVALID and b"struct_size" in L.rq_last_error()
            assert call(p=prm(flags=1), dev=dev) == INVALID and b"flags" in L.rq_last_error()
            # the limits, worded like the plain call's topk refusal
            for bad in (dict(topk=0), dict(g=0), dict(topk=3, g=3, fetch=8), dict(topk=1, g=1, fetch=2049), dict(topk=1, g=1, fetch=0),
                        dict(topk=1 << 31, g=2, fetch=8)):
                assert call(p=prm(**bad), dev=dev) == UNSUPPORTED and b"topk * group_size <= fetch <= 2048" in L.rq_last_error(), bad
            # a malformed column name
            for name in (b"", b"a" * 32, b"a-b", b"a b"):
                assert call(col=name, dev=dev) == INVALID and b"[A-Za-z0-9_]" in L.rq_last_error(), name
        assert query(q=null, dev=dev) == INVALID and exact(q=null, dev=dev) == INVALID
        for k in range(3):
            src = tuple(null if j == k else fake for j in range(3))
            assert results(src=src, dev=dev) == INVALID and b"null argument" in L.rq_last_error()
    assert L.rq_last_group_stats(None) == INVALID
    st = _lib.GroupStatsT()
    st.struct_size = 0
    assert L.rq_last_group_stats(C.byref(st)) == INVALID                      # an unset struct_size, as every sized struct


def test_python_surface():
    import rabitq_amd
    from rabitq_amd import _lib
    R = rabitq_amd.RaBitQ
    sig = lambda f: list(inspect.signature(f).parameters)
    dflt = lambda f, n: inspect.signature(f).parameters[n].default
    assert sig(R.query_batch_grouped) == ["self", "queries", "probe", "topk", "group_by", "group_size", "fetch", "heuristic_rank", "filter"]
    assert sig(R.exact_search_grouped) == ["self", "queries", "topk", "group_by", "group_size", "fetch", "filter", "params"]
    assert sig(R.group_results) == ["self", "dist", "ids", "counts", "topk", "group_by", "group_size"]
    for f in (R.query_batch_grouped, R.exact_search_grouped):
        assert dflt(f, "group_size") == 1 and dflt(f, "fetch") is None and dflt(f, "filter") is None
    assert dflt(R.query_batch_grouped, "heuristic_rank") is False and dflt(R.group_results, "group_size") == 1
    for m in ("query_batch_grouped_device", "exact_search_grouped_device", "group_results_device", "last_group_stats"):
        assert callable(getattr(R, m)), m
    assert callable(rabitq_amd.last_group_stats)
    assert rabitq_amd.GroupedResult.__slots__ == ("dist", "ids", "keys", "group_counts", "counts", "fetched")
    # fetch=None: min(2048, max(64, 4 * topk * group_size))
    assert [_lib.default_group_fetch(*a) for a in ((1, 1), (10, 1), (10, 3), (100, 2), (100, 10), (2048, 1))] == [64, 64, 120, 800, 2048, 2048]
