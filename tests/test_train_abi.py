"""The boundary of centroid training: the header declares rq_train_params_t, rq_train_stats_t and the two entries, the built library
exports them, the ctypes mirror lists them with the header's arity and the structs with gcc's layout, and the Python layer has its
functions.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rq_train_centroids_device": 8, "rq_train_centroids": 8}


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
    assert "centroid training" in note and "rq_train_centroids_device" in note   # the revision note names the addition
    _lib.build()
    L = _lib.lib()
    assert b"abi 4" in L.rq_version() and L.rq_abi_version() == 4
    assert L.rq_version() == b"rabitq_hip 0.7.0 (gfx950, abi 4)"                # the text other ABI tests pin
    for name, arity in ENTRIES.items():
        assert name in _lib.EXPORTS, name
        params = declared_params(code, name)
        assert len(params) == arity, (name, params)
        assert any("rq_train_params_t" in p and "params" in p for p in params), params
        assert params[-1].replace(" ", "").endswith("rq_train_stats_t*stats_out"), params
        assert params[-2].replace(" ", "").endswith("double*objective_out"), params
        fn = getattr(L, name)                                                # AttributeError if the library lacks the symbol
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), len(params))
    # the same parameters in the same order, host and device entry
    strip = lambda ps: [re.sub(r"\b(d_)?(\w+)$", r"\2", p) for p in ps]
    assert strip(declared_params(code, "rq_train_centroids")) == strip(declared_params(code, "rq_train_centroids_device"))
    # the old trainer is still declared, exported and mirrored as it was
    assert len(declared_params(code, "rq_kmeans_device")) == 8 and len(L.rq_kmeans_device.argtypes) == 8
    # rq_profile_t is not changed by this addition
    assert C.sizeof(_lib.ProfileT) == 144


def test_struct_layouts_match_the_header(tmp_path):
    """rq_train_params_t and rq_train_stats_t as gcc lays them out from include/rabitq_hip.h == the ctypes mirrors."""
    from rabitq_amd import _lib
    pf = ["struct_size", "iters", "points_per_centroid", "seed", "metric", "row_type", "sq_bound"]
    sf = ["struct_size", "iters_run", "sample_rows", "splits"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rabitq_hip.h"\nint main(void) {\n'
                   + '    printf("%zu", sizeof(rq_train_params_t));\n'
                   + "".join('    printf(" %%zu", offsetof(rq_train_params_t, %s));\n' % f for f in pf)
                   + '    printf("\\n%zu", sizeof(rq_train_stats_t));\n'
                   + "".join('    printf(" %%zu", offsetof(rq_train_stats_t, %s));\n' % f for f in sf)
                   + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got_p, got_s = ([int(v) for v in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines())
    P, S = _lib.TrainParamsT, _lib.TrainStatsT
    assert [n for n, _ in P._fields_] == pf and [n for n, _ in S._fields_] == sf
    assert got_p == [C.sizeof(P)] + [getattr(P, f).offset for f in pf]
    assert got_s == [C.sizeof(S)] + [getattr(S, f).offset for f in sf]
    assert got_p == [40, 0, 4, 8, 16, 24, 28, 32] and got_s == [16, 0, 4, 8, 12]
    assert P().struct_size == 40 and S().struct_size == 16                   # the mirrors fill struct_size themselves


def test_python_surface():
    import rabitq_amd
    sig = lambda f: list(inspect.signature(f).parameters)
    dflt = lambda f: {n: p.default for n, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert sig(rabitq_amd.train_centroids) == ["base", "k", "iters", "points_per_centroid", "seed", "metric", "max_sq_norm", "rows", "return_stats"]
    assert dflt(rabitq_amd.train_centroids) == dict(iters=20, points_per_centroid=256, seed=0, metric="l2", max_sq_norm=None, rows=None,
                                                    return_stats=False)
    assert sig(rabitq_amd.train_centroids_device) == ["base_ptr", "n", "d", "k", "out_ptr", "iters", "points_per_centroid", "seed", "metric",
                                                      "max_sq_norm", "rows"]
    assert dflt(rabitq_amd.train_centroids_device) == dict(iters=20, points_per_centroid=256, seed=0, metric="l2", max_sq_norm=None, rows="f32")
    st = rabitq_amd.TrainStats(3, 100, 1, [2.0, 1.0, 0.5])
    assert (st.iters_run, st.sample_rows, st.splits, st.objective) == (3, 100, 1, [2.0, 1.0, 0.5])
    # the constructors take a list count where they took centroids; from_path is as it was
    R = rabitq_amd.RaBitQ
    assert sig(R.build) == ["base", "centroids", "orthogonal", "seed", "metric", "max_sq_norm", "rows"]
    assert sig(R.build_device)[:5] == ["base_ptr", "n", "d", "centroids_ptr", "k"] and "centroids=<int>" in R.build.__doc__
    assert "centroids_ptr=None" in R.build_device.__doc__
    assert sig(R.from_path) == ["base_path", "centroid_path", "orthogonal", "seed", "metric", "max_sq_norm"]
    # the old trainer's Python entry is as it was
    assert sig(rabitq_amd.ops.kmeans_device) == ["base_ptr", "n", "d", "k", "out_ptr", "iters", "points_per_centroid", "seed"]
    from rabitq_amd import cli
    a = cli.build_parser().parse_args("-b b -c c -q q -t t -s s --train 64 --train-iters 5".split())
    assert (a.train, a.train_iters) == (64, 5)
    a = cli.build_parser().parse_args("-b b -c c -q q -t t -s s".split())
    assert (a.train, a.train_iters) == (0, 20)
