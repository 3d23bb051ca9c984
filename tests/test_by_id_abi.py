"""The boundary of the rows-by-id entries: the header declares them and rq_by_id_stats_t, the built library exports them, the
ctypes mirror lists them with the header's arity and the struct with gcc's layout, null arguments are refused before a device is
looked for, and the Python layer has its methods.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rq_locate": 4, "rq_fetch_rows": 5, "rq_fetch_stored": 5, "rq_pair_distances": 7, "rq_neighbours_of": 10,
           "rq_neighbours_of_exact": 9}
INVALID = -1


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
    note = hdr.split("#define RQ_ABI_VERSION")[0]
    assert "rows by id" in note and "rq_neighbours_of" in note and "rq_last_by_id_stats" in note   # the history block names the addition
    assert re.search(r"#define\s+RQ_POS_ABSENT\s+0xFFFFFFFFu", code) and _lib.POS_ABSENT == 0xFFFFFFFF
    _lib.build()
    L = _lib.lib()
    assert L.rq_abi_version() == 4
    strip = lambda ps: [re.sub(r"\b(d_)?(\w+)$", r"\2", p) for p in ps]
    for name, arity in ENTRIES.items():
        for entry in (name, name + "_device"):
            assert entry in _lib.EXPORTS, entry
            params = declared_params(code, entry)
            assert len(params) == arity, (entry, params)
            fn = getattr(L, entry)                                            # AttributeError if the library lacks the symbol
            assert len(fn.argtypes) == len(params), (entry, len(fn.argtypes), len(params))
        # the same parameters in the same order, host and device entry
        assert strip(declared_params(code, name)) == strip(declared_params(code, name + "_device")), name
    assert "rq_last_by_id_stats" in _lib.EXPORTS and len(L.rq_last_by_id_stats.argtypes) == 1
    assert len(declared_params(code, "rq_last_by_id_stats")) == 1


def test_stats_layout_matches_the_header(tmp_path):
    """rq_by_id_stats_t as gcc lays it out from include/rabitq_hip.h == the ctypes mirror."""
    from rabitq_amd import _lib
    fields = [n for n, _ in _lib.ByIdStatsT._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rabitq_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(rq_by_id_stats_t));\n'
                   + "".join('    printf(" %%zu", offsetof(rq_by_id_stats_t, %s));\n' % f for f in fields)
                   + '    printf(" %d %d %d\\n", RQ_DIRECTORY_NONE, RQ_DIRECTORY_DENSE, RQ_DIRECTORY_HASH);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.ByIdStatsT
    assert got[:-3] == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got[0] == 64 and got[1] == 0
    assert got[-3:] == [0, 1, 2] and _lib.DIRECTORY_FORMS == {0: "none", 1: "dense", 2: "hash"}
    assert S().struct_size == 64                                             # the mirror fills struct_size itself


def test_null_arguments_are_refused_before_a_device_is_looked_for():
    """RQ_ERR_INVALID (not RQ_ERR_NO_DEVICE) on a machine without a GPU too: the checks come first."""
    from rabitq_amd import _lib
    _lib.build()
    L = _lib.lib()
    ids = np.arange(4, dtype=np.uint32)
    out = np.zeros(4 * 64, dtype=np.float32)
    u = np.zeros(4, dtype=np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    fake = C.c_void_p(ids.ctypes.data)      # a non-null "index" that is never dereferenced: a null ARGUMENT is refused first
    null = C.c_void_p(0)
    for dev in ("", "_device"):
        f = lambda name: getattr(L, name + dev)
        # a null index
        assert f("rq_locate")(null, p(ids), 4, p(u)) == INVALID
        assert b"null index" in L.rq_last_error()
        assert f("rq_fetch_rows")(null, p(ids), 4, p(out), p(u)) == INVALID
        assert f("rq_fetch_stored")(null, p(ids), 4, p(out), p(u)) == INVALID
        assert f("rq_pair_distances")(null, p(out), 2, 64, p(ids), 2, p(out)) == INVALID
        assert f("rq_neighbours_of")(null, p(ids), 4, 4, 5, 0, null, p(out), p(u), p(u)) == INVALID
        assert f("rq_neighbours_of_exact")(null, p(ids), 4, 5, null, None, p(out), p(u), p(u)) == INVALID
        # null ids / outputs with m > 0
        assert f("rq_locate")(fake, null, 4, p(u)) == INVALID
        assert b"null argument" in L.rq_last_error()
        assert f("rq_locate")(fake, p(ids), 4, null) == INVALID
        assert f("rq_fetch_rows")(fake, null, 4, p(out), p(u)) == INVALID
        assert f("rq_fetch_rows")(fake, p(ids), 4, null, p(u)) == INVALID
        assert f("rq_fetch_stored")(fake, p(ids), 4, null, p(u)) == INVALID
        assert f("rq_pair_distances")(fake, null, 2, 64, p(ids), 2, p(out)) == INVALID
        assert f("rq_pair_distances")(fake, p(out), 2, 64, null, 2, p(out)) == INVALID
        assert f("rq_pair_distances")(fake, p(out), 2, 64, p(ids), 2, null) == INVALID
        for hole in range(3):
            args = [p(out), p(u), p(u)]
            args[hole] = null
            assert f("rq_neighbours_of")(fake, p(ids), 4, 4, 5, 0, null, *args) == INVALID, hole
            assert f("rq_neighbours_of_exact")(fake, p(ids), 4, 5, null, None, *args) == INVALID, hole
        assert f("rq_neighbours_of")(fake, null, 4, 4, 5, 0, null, p(out), p(u), p(u)) == INVALID
    assert L.rq_last_by_id_stats(None) == INVALID
    st = _lib.ByIdStatsT()
    st.struct_size = 0
    assert L.rq_last_by_id_stats(C.byref(st)) == INVALID                      # an unset struct_size, as every sized struct


def test_python_surface():
    import rabitq_amd
    R = rabitq_amd.RaBitQ
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(R.locate) == ["self", "ids"] and sig(R.contains) == ["self", "ids"]
    assert sig(R.fetch) == ["self", "ids", "stored", "raw"]
    d = inspect.signature(R.fetch).parameters
    assert d["stored"].default is False and d["raw"].default is True
    assert sig(R.distances_to) == ["self", "queries", "ids"]
    assert sig(R.neighbours_of) == ["self", "ids", "probe", "topk", "filter", "heuristic_rank", "exact"]
    d = inspect.signature(R.neighbours_of).parameters
    assert d["filter"].default is None and d["heuristic_rank"].default is False and d["exact"].default is False
    assert sig(R.knn_graph) == ["self", "probe", "topk", "exact", "chunk"]
    d = inspect.signature(R.knn_graph).parameters
    assert d["exact"].default is False and d["chunk"].default == 65536
    assert sig(R.locate_device)[:4] == ["self", "ids_ptr", "m", "out_pos_ptr"]
    assert sig(R.fetch_device)[:4] == ["self", "ids_ptr", "m", "out_rows_ptr"]
    assert sig(R.neighbours_of_device)[:8] == ["self", "ids_ptr", "m", "probe", "topk", "out_dist_ptr", "out_id_ptr", "out_found_ptr"]
    assert callable(R.last_by_id_stats) and callable(rabitq_amd.last_by_id_stats)
