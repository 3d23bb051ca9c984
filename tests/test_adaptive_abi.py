"""The boundary of adaptive probing: the header declares rq_probe_rule_t and the three entries, the built library exports them, the
ctypes mirror lists them with the header's arity and the struct with gcc's layout, and the Python layer has its methods.  No GPU
needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rq_query_batch_device_adaptive": 13, "rq_query_batch_adaptive": 13, "rq_probe_counts_device": 7}


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
    assert "adaptive probing" in note and "rq_probe_counts_device" in note    # the revision note names the addition
    _lib.build()
    L = _lib.lib()
    assert b"abi 4" in L.rq_version() and L.rq_abi_version() == 4
    for name, arity in ENTRIES.items():
        assert name in _lib.EXPORTS, name
        params = declared_params(code, name)
        assert len(params) == arity, (name, params)
        assert any("rq_probe_rule_t" in p and "rule" in p for p in params), params
        assert params[-1].replace(" ", "").endswith("out_nprobe"), params
        fn = getattr(L, name)                                                # AttributeError if the library lacks the symbol
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), len(params))
    # the same parameters in the same order, host and device entry
    strip = lambda ps: [re.sub(r"\b(d_)?(\w+)$", r"\2", p) for p in ps]
    assert strip(declared_params(code, "rq_query_batch_adaptive")) == strip(declared_params(code, "rq_query_batch_device_adaptive"))
    # rq_profile_t is not changed by this addition
    assert C.sizeof(_lib.ProfileT) == 144


def test_probe_rule_layout_matches_the_header(tmp_path):
    """rq_probe_rule_t as gcc lays it out from include/rabitq_hip.h == the ctypes mirror."""
    from rabitq_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "rabitq_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rq_probe_rule_t), offsetof(rq_probe_rule_t, struct_size), offsetof(rq_probe_rule_t, min_probe),
           offsetof(rq_probe_rule_t, ratio), offsetof(rq_probe_rule_t, reserved), offsetof(rq_probe_rule_t, max_probe));
    return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R = _lib.ProbeRuleT
    assert got == [C.sizeof(R), R.struct_size.offset, R.min_probe.offset, R.ratio.offset, R.reserved.offset, R.max_probe.offset]
    assert got == [24, 0, 4, 8, 12, 16]
    assert R().struct_size == 24                                             # the mirror fills struct_size itself


def test_python_surface():
    import rabitq_amd
    R = rabitq_amd.RaBitQ
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(R.query_batch_adaptive) == ["self", "queries", "probe", "topk", "ratio", "min_probe", "max_probe", "heuristic_rank", "filter"]
    d = inspect.signature(R.query_batch_adaptive).parameters
    assert d["ratio"].default == float("inf") and d["min_probe"].default == 1 and d["max_probe"].default is None
    assert d["heuristic_rank"].default is False and d["filter"].default is None
    assert sig(R.query_batch_adaptive_device)[:9] == ["self", "q_ptr", "nq", "length", "probe", "topk", "out_dist_ptr", "out_id_ptr", "out_n_ptr"]
    assert sig(R.probe_counts) == ["self", "queries", "probe", "ratio", "min_probe", "max_probe"]
    assert sig(R.tune_probe_ratio) == ["self", "queries", "probe", "topk", "target_recall", "min_probe", "filter"]
    assert "nearly monotone" in R.tune_probe_ratio.__doc__
