"""The boundary of the attribute columns: the header declares every new entry and the built library exports it, the ctypes mirror
lists it with the header's arity and the structs with gcc's layout, null arguments and malformed programs are refused before a
device is looked for, the history block names the addition, and the Python layer has its methods.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rq_attr_create": 4, "rq_attr_drop": 2, "rq_attr_count": 2, "rq_attr_info": 3, "rq_attr_index": 3, "rq_attr_set": 6,
           "rq_attr_set_device": 6, "rq_attr_get": 6, "rq_attr_get_device": 6, "rq_attr_get_array": 4, "rq_filter_create_where": 6,
           "rq_last_where_stats": 1, "rq_filter_combine": 5, "rq_filter_id_bits": 4, "rq_filter_ids_device": 4}
INVALID = -1
AND, OR, NOT = 0x80, 0x81, 0x82


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
    assert "0.15.0: attribute columns, additions only" in note                # the history block names the addition
    for name in ("rq_filter_create_where", "rq_filter_combine", "rq_filter_id_bits", "rq_filter_ids_device", "rq_last_where_stats"):
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
    for name in ("rq_attr_set", "rq_attr_get"):                               # the same parameters in the same order, host and device
        assert strip(declared_params(code, name)) == strip(declared_params(code, name + "_device")), name


def test_struct_and_union_layouts_match_the_header(tmp_path):
    """rq_attr_value_t, rq_attr_info_t, rq_where_term_t and rq_where_stats_t as gcc lays them out == the ctypes mirrors; the
    enums and limits have the documented values."""
    from rabitq_amd import _lib
    from rabitq_amd import where as W
    structs = {"rq_attr_info_t": _lib.AttrInfoT, "rq_where_term_t": _lib.WhereTermT, "rq_where_stats_t": _lib.WhereStatsT,
               "rq_attr_value_t": _lib.AttrValue}
    body = ""
    for cname, S in structs.items():
        body += '    printf("%%zu", sizeof(%s));\n' % cname
        body += "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in S._fields_)
        body += '    printf("\\n");\n'
    consts = ["RQ_ATTR_U32", "RQ_ATTR_I32", "RQ_ATTR_F32", "RQ_ATTR_U64", "RQ_ATTR_I64", "RQ_WHERE_EQ", "RQ_WHERE_NE", "RQ_WHERE_LT",
              "RQ_WHERE_LE", "RQ_WHERE_GT", "RQ_WHERE_GE", "RQ_WHERE_BETWEEN", "RQ_WHERE_IN", "RQ_WHERE_ANY_BITS", "RQ_WHERE_ALL_BITS",
              "RQ_WHERE_AND", "RQ_WHERE_OR", "RQ_WHERE_NOT", "RQ_WHERE_MAX_TERMS", "RQ_WHERE_MAX_TOKENS", "RQ_WHERE_MAX_COLUMNS",
              "RQ_WHERE_MAX_SET", "RQ_ATTR_MAX_COLUMNS", "RQ_FILTER_AND", "RQ_FILTER_OR", "RQ_FILTER_ANDNOT", "RQ_FILTER_NOT"]
    body += "".join('    printf("%%d ", (int)%s);\n' % c for c in consts)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rabitq_hip.h"\nint main(void) {\n' + body + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    for line, (cname, S) in zip(lines, structs.items()):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_], cname
    assert C.sizeof(_lib.AttrValue) == 8 and C.sizeof(_lib.AttrInfoT) == 56 and C.sizeof(_lib.WhereTermT) == 40
    assert C.sizeof(_lib.WhereStatsT) == 40 and _lib.WhereStatsT().struct_size == 40 and _lib.AttrInfoT().struct_size == 56
    got = [int(v) for v in lines[len(structs)].split()]
    assert got == [0, 1, 2, 3, 4] + list(range(10)) + [AND, OR, NOT, 32, 64, 8, 4096, 16, 0, 1, 2, 3]
    assert [t.id for t in _lib.ATTR_TABLE] == [0, 1, 2, 3, 4] and [t.elem_bytes for t in _lib.ATTR_TABLE] == [4, 4, 4, 8, 8]
    assert (W.OP_EQ, W.OP_BETWEEN, W.OP_IN, W.OP_ANY_BITS, W.OP_ALL_BITS) == (0, 6, 7, 8, 9)
    assert (W.TOK_AND, W.TOK_OR, W.TOK_NOT) == (AND, OR, NOT)
    assert (W.MAX_TERMS, W.MAX_TOKENS, W.MAX_DEPTH, W.MAX_COLUMNS, W.MAX_SET) == (32, 64, 32, 8, 4096)
    assert (_lib.FILTER_AND, _lib.FILTER_OR, _lib.FILTER_ANDNOT, _lib.FILTER_NOT) == (0, 1, 2, 3) and _lib.ATTR_MAX_COLUMNS == 16


def test_refusals_come_before_a_device_is_looked_for():
    """RQ_ERR_INVALID (not RQ_ERR_NO_DEVICE) on a machine without a GPU too.  `fake` is a non-null "index" that is never
    dereferenced: the checks that need nothing of the index come first."""
    from rabitq_amd import _lib
    _lib.build()
    L = _lib.lib()
    ids = np.arange(4, dtype=np.uint32)
    vals = np.zeros(4, dtype=np.uint64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    fake, null = C.c_void_p(ids.ctypes.data), C.c_void_p(0)
    h = C.c_void_p()
    cnt, absent = C.c_uint32(), C.c_uint64()
    info = _lib.AttrInfoT()
    # null index / name / arguments
    assert L.rq_attr_create(null, b"ts", 0, 0) == INVALID and b"null index" in L.rq_last_error()
    assert L.rq_attr_create(fake, None, 0, 0) == INVALID and b"null argument" in L.rq_last_error()
    assert L.rq_attr_drop(null, b"ts") == INVALID and L.rq_attr_drop(fake, None) == INVALID
    assert L.rq_attr_count(null, C.byref(cnt)) == INVALID and L.rq_attr_count(fake, None) == INVALID
    assert L.rq_attr_info(null, 0, C.byref(info)) == INVALID and L.rq_attr_info(fake, 0, None) == INVALID
    assert L.rq_attr_index(null, b"ts", C.byref(cnt)) == INVALID and L.rq_attr_index(fake, b"ts", None) == INVALID
    assert L.rq_attr_get_array(null, b"ts", p(vals), 32) == INVALID
    for dev in ("", "_device"):
        st, gt = getattr(L, "rq_attr_set" + dev), getattr(L, "rq_attr_get" + dev)
        assert st(null, b"ts", p(ids), p(vals), 4, C.byref(absent)) == INVALID
        assert st(fake, None, p(ids), p(vals), 4, C.byref(absent)) == INVALID
        assert st(fake, b"ts", null, p(vals), 4, C.byref(absent)) == INVALID and b"null argument" in L.rq_last_error()
        assert st(fake, b"ts", p(ids), null, 4, C.byref(absent)) == INVALID
        assert gt(null, b"ts", p(ids), 4, p(vals), p(ids)) == INVALID
        assert gt(fake, b"ts", null, 4, p(vals), p(ids)) == INVALID
        assert gt(fake, b"ts", p(ids), 4, null, p(ids)) == INVALID
    # malformed names and an unknown type
    for bad in (b"", b"a" * 32, b"a-b", b"caf\xc3\xa9", b"a b"):
        assert L.rq_attr_create(fake, bad, 0, 0) == INVALID and b"[A-Za-z0-9_]" in L.rq_last_error(), bad
        assert L.rq_attr_drop(fake, bad) == INVALID
    assert L.rq_attr_create(fake, b"ts", 5, 0) == INVALID and b"unknown column type" in L.rq_last_error()
    # predicates: null arguments, limits, malformed programs
    T = _lib.WhereTermT
    terms = (T * 33)()
    def where(idx, t, nt, toks, out=C.byref(h)):   # toks None: no program; else a non-null buffer, also for no token
        buf = np.asarray(list(toks or []) + [0], dtype=np.uint8)
        return L.rq_filter_create_where(idx, t, nt, p(buf) if toks is not None else null, len(toks) if toks is not None else 0, out)
    assert where(fake, terms, 1, [0], None) == INVALID
    assert where(null, terms, 1, [0]) == INVALID and b"null index" in L.rq_last_error()
    assert L.rq_filter_create_where(fake, None, 1, null, 0, C.byref(h)) == INVALID
    assert where(fake, terms, 33, None) == INVALID and b"32 terms" in L.rq_last_error()
    assert where(fake, terms, 1, [0, AND]) == INVALID and b"underflows" in L.rq_last_error()
    assert where(fake, terms, 1, [NOT]) == INVALID and b"underflows" in L.rq_last_error()
    assert where(fake, terms, 2, [0, 1]) == INVALID and b"depth 2, not 1" in L.rq_last_error()
    assert where(fake, terms, 1, []) == INVALID and b"depth 0, not 1" in L.rq_last_error()
    assert where(fake, terms, 1, [1]) == INVALID and b"pushes term 1 of 1" in L.rq_last_error()
    assert where(fake, terms, 1, [0, 0x83]) == INVALID and b"unknown token" in L.rq_last_error()
    assert where(fake, terms, 1, [0] * 33 + [AND] * 32) == INVALID and b"64 tokens" in L.rq_last_error()
    assert where(fake, terms, 1, [0] * 33 + [AND] * 31) == INVALID and b"depth 32" in L.rq_last_error()
    terms[0].op = 10
    assert where(fake, terms, 1, [0]) == INVALID and b"unknown op" in L.rq_last_error()
    terms[0].op, terms[0].set_count = 7, 4097
    assert where(fake, terms, 1, [0]) == INVALID and b"4096" in L.rq_last_error()
    terms[0].set_count = 3
    assert where(fake, terms, 1, [0]) == INVALID and b"null set" in L.rq_last_error()
    assert h.value is None
    # the entries on filters
    assert L.rq_filter_combine(null, fake, fake, 0, C.byref(h)) == INVALID
    assert L.rq_filter_combine(fake, fake, fake, 0, None) == INVALID
    assert L.rq_filter_combine(fake, fake, fake, 4, C.byref(h)) == INVALID and b"unknown op" in L.rq_last_error()
    assert L.rq_filter_combine(fake, null, fake, 0, C.byref(h)) == INVALID and b"null filter" in L.rq_last_error()
    assert L.rq_filter_combine(fake, fake, null, 2, C.byref(h)) == INVALID
    assert L.rq_filter_id_bits(null, p(ids), 64, 0) == INVALID
    assert L.rq_filter_id_bits(fake, null, 64, 0) == INVALID
    assert L.rq_filter_id_bits(fake, p(ids), (1 << 32) + 1, 0) == INVALID
    assert L.rq_filter_ids_device(null, p(ids), 4, C.byref(absent)) == INVALID
    assert L.rq_filter_ids_device(fake, p(ids), 4, None) == INVALID
    assert L.rq_last_where_stats(None) == INVALID
    st = _lib.WhereStatsT()
    st.struct_size = 0
    assert L.rq_last_where_stats(C.byref(st)) == INVALID                      # an unset struct_size, as every sized struct


def test_python_surface():
    import rabitq_amd
    R, F = rabitq_amd.RaBitQ, rabitq_amd.Filter
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(R.create_attr) == ["self", "name", "dtype", "fill"] and inspect.signature(R.create_attr).parameters["fill"].default == 0
    assert sig(R.drop_attr) == ["self", "name"] and sig(R.attrs) == ["self"]
    assert sig(R.set_attr) == ["self", "name", "ids", "values"] and sig(R.get_attr) == ["self", "name", "ids"]
    assert sig(R.attr_array) == ["self", "name"] and sig(R.where) == ["self", "expr"]
    for m in ("__and__", "__or__", "__sub__", "__invert__", "ids", "id_bits"):
        assert callable(getattr(F, m)), m
    assert sig(F.id_bits) == ["self", "nbits"] and inspect.signature(F.id_bits).parameters["nbits"].default is None
    assert callable(R.last_where_stats) and callable(rabitq_amd.last_where_stats)
    c = rabitq_amd.col("ts")
    for m in ("between", "isin", "any_bits", "all_bits"):
        assert callable(getattr(c, m)), m
    from rabitq_amd import where as W
    assert isinstance(c >= 5, W.Expr) and isinstance((c >= 5) & ~(c == 1) | (c < 0), W.Expr)
