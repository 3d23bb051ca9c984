"""The boundary of diverse search: the header declares every new entry and the built library exports it, the ctypes mirror lists
it with the header's arity and the structs with gcc's layout, the history block names the addition, every refusal that needs no
device returns its status without one, and the Python layer has its methods.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rq_query_batch_diverse": 13, "rq_query_batch_diverse_device": 13, "rq_exact_search_diverse": 12,
           "rq_exact_search_diverse_device": 12, "rq_diversify_results": 10, "rq_diversify_results_device": 10, "rq_last_diverse_stats": 1}
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
    assert "0.17.0: diverse search, additions only -- " in note               # the history block names the addition
    for name in ("rq_diverse_params_t", "rq_diverse_stats_t", "rq_query_batch_diverse", "rq_exact_search_diverse", "rq_diversify_results",
                 "rq_last_diverse_stats"):
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
    for name in ("rq_query_batch_diverse", "rq_exact_search_diverse", "rq_diversify_results"):   # the same parameters, host and device
        assert strip(declared_params(code, name)) == strip(declared_params(code, name + "_device")), name


def test_struct_layouts_match_the_header(tmp_path):
    from rabitq_amd import _lib
    structs = {"rq_diverse_params_t": _lib.DiverseParamsT, "rq_diverse_stats_t": _lib.DiverseStatsT}
    body = ""
    for cname, S in structs.items():
        body += '    printf("%%zu", sizeof(%s));\n' % cname
        body += "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (cname, f.rstrip("_")) for f, _ in S._fields_)   # (lambda_: a Python keyword)
        body += '    printf("\\n");\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rabitq_hip.h"\nint main(void) {\n' + body + '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    for line, (cname, S) in zip(lines, structs.items()):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_], cname
    assert C.sizeof(_lib.DiverseParamsT) == 20 and C.sizeof(_lib.DiverseStatsT) == 64
    assert _lib.DiverseParamsT().struct_size == 20 and _lib.DiverseStatsT().struct_size == 64
    assert [n for n, _ in _lib.DiverseParamsT._fields_] == ["struct_size", "topk", "fetch", "lambda_", "flags"]
    assert [n for n, _ in _lib.DiverseStatsT._fields_][1:10] == ["fetch", "ms_source", "ms_select", "candidates", "absent", "skipped", "taken",
                                                                 "pair_distances", "directory_built"]


def test_refusals_come_before_a_device_is_looked_for():
    """RQ_ERR_INVALID / RQ_ERR_UNSUPPORTED (not RQ_ERR_NO_DEVICE) on a machine without a GPU too.  `fake` is a non-null "index"
    that is never dereferenced: the checks that need nothing of the index come first."""
    from rabitq_amd import _lib
    _lib.build()
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint64)
    fake, null = C.c_void_p(buf.ctypes.data), C.c_void_p(0)
    o = fake                                                                   # any non-null address: nothing is written

    def prm(topk=2, fetch=8, lam=0.5, flags=0, size=None):
        p = _lib.DiverseParamsT(topk=topk, fetch=fetch, lambda_=lam, flags=flags)
        if size is not None:
            p.struct_size = size
        return C.byref(p)

    def query(idx=fake, q=fake, p=None, outs=(o, o, o, o, o), dev=""):
        return getattr(L, "rq_query_batch_diverse" + dev)(idx, null, q, 4, 64, 8, 0, prm() if p is None else p, *outs)

    def exact(idx=fake, q=fake, p=None, outs=(o, o, o, o, o), dev=""):
        return getattr(L, "rq_exact_search_diverse" + dev)(idx, null, q, 4, 64, None, prm() if p is None else p, *outs)

    def results(idx=fake, src=(fake, fake, fake), p=None, outs=(o, o, o, o), dev=""):
        return getattr(L, "rq_diversify_results" + dev)(idx, *src, 4, prm() if p is None else p, *outs)

    for dev in ("", "_device"):
        for call in (query, exact, results):
            assert call(idx=null, dev=dev) == INVALID and b"null index" in L.rq_last_error()
            assert call(p=C.cast(null, C.POINTER(_lib.DiverseParamsT)), dev=dev) == INVALID and b"null argument" in L.rq_last_error()
            n_out = 4 if call is results else 5
            for k in range(4):                                                 # every output but out_fetched
                outs = tuple(null if j == k else o for j in range(n_out))
                assert call(outs=outs, dev=dev) == INVALID and b"null argument" in L.rq_last_error(), (call.__name__, k)
            for size in (0, 16, 24):                                           # a wrong struct_size, a set flag
                assert call(p=prm(size=size), dev=dev) == INVALID and b"struct_size" in L.rq_last_error()
            assert call(p=prm(flags=1), dev=dev) == INVALID and b"flags" in L.rq_last_error()
            for lam in (float("nan"), -0.25, 1.5, float("inf"), -float("inf")):
                assert call(p=prm(lam=lam), dev=dev) == INVALID and b"lambda must be in [0, 1]" in L.rq_last_error(), lam
            for bad in (dict(topk=0), dict(topk=9, fetch=8), dict(topk=1, fetch=2049), dict(topk=1, fetch=0), dict(topk=1 << 31, fetch=8)):
                assert call(p=prm(**bad), dev=dev) == UNSUPPORTED and b"topk <= fetch <= 2048" in L.rq_last_error(), bad
            # lambda is judged before the limits, the struct before lambda
            assert call(p=prm(topk=0, lam=2.0), dev=dev) == INVALID and call(p=prm(lam=2.0, size=16), dev=dev) == INVALID
            assert b"struct_size" in L.rq_last_error()
        assert query(q=null, dev=dev) == INVALID and exact(q=null, dev=dev) == INVALID
        for k in range(3):
            src = tuple(null if j == k else fake for j in range(3))
            assert results(src=src, dev=dev) == INVALID and b"null argument" in L.rq_last_error()
    assert L.rq_last_diverse_stats(None) == INVALID
    st = _lib.DiverseStatsT()
    st.struct_size = 0
    assert L.rq_last_diverse_stats(C.byref(st)) == INVALID                    # an unset struct_size, as every sized struct


def test_python_surface():
    import rabitq_amd
    from rabitq_amd import _lib
    R = rabitq_amd.RaBitQ
    sig = lambda f: list(inspect.signature(f).parameters)
    dflt = lambda f, n: inspect.signature(f).parameters[n].default
    assert sig(R.query_batch_diverse) == ["self", "queries", "probe", "topk", "lam", "fetch", "heuristic_rank", "filter"]
    assert sig(R.exact_search_diverse) == ["self", "queries", "topk", "lam", "fetch", "filter", "params"]
    assert sig(R.diversify_results) == ["self", "dist", "ids", "counts", "topk", "lam"]
    for f in (R.query_batch_diverse, R.exact_search_diverse):
        assert dflt(f, "lam") == 0.5 and dflt(f, "fetch") is None and dflt(f, "filter") is None
    assert dflt(R.query_batch_diverse, "heuristic_rank") is False
    for m in ("query_batch_diverse_device", "exact_search_diverse_device", "diversify_results_device", "last_diverse_stats"):
        assert callable(getattr(R, m)), m
    assert callable(rabitq_amd.last_diverse_stats)
    assert rabitq_amd.DiverseResult.__slots__ == ("dist", "ids", "div", "counts", "fetched")
    # fetch=None: min(2048, max(64, 4 * topk))
    assert [_lib.default_diverse_fetch(t) for t in (1, 10, 16, 17, 100, 512, 2048)] == [64, 64, 64, 68, 400, 2048, 2048]
