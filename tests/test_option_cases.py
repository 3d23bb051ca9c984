"""The table of tests/option_cases.py checked without a GPU: every option rq_set_option knows has a row (a future option cannot ship
without an engaged case), every value of the golden sweep has one, every `covered_by` names a test that exists, and the CPU oracle
alone answers every case -- no reference panic, full topk counts -- so the GPU test has an answer to compare with."""
import ast
import os
import re

import numpy as np
import pytest

from tests import option_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def option_rows():
    """-> [(name, default)]: the rows of the option table rq_set_option looks its argument up in (host_options.h: the X(...) rows
    of RQ_OPTIONS and the two written-out rows of g_options)."""
    src = open(os.path.join(ROOT, "rabitq_amd", "csrc", "host_options.h")).read()
    src = src[src.index("#define RQ_OPTIONS(X)"):]
    rows = re.findall(r'^\s*(?:X\(|\{)"([a-z0-9_]+)", *&?\w+, *(-?\d+),', src, flags=re.M)
    return [(name, int(default)) for name, default in rows]


def option_names():
    """The names rq_set_option knows."""
    return [name for name, _ in option_rows()]


def test_every_option_has_a_row():
    names = option_names()
    assert len(names) == len(set(names)) >= 25 and "scan_impl" in names and "scan_debug" in names, names
    in_table = {r.option for r in oc.TABLE}
    assert set(names) <= in_table, sorted(set(names) - in_table)
    assert in_table <= set(names), sorted(in_table - set(names))
    # ... an ENGAGED row, unless the option's paths all need a shape too big for this module
    engaged = {r.option for r in oc.ENGAGED}
    assert set(names) - engaged == {"pass_overlap", "shared_thresholds"}, sorted(set(names) - engaged)
    assert set(oc.DEFAULTS) == set(names)
    assert dict(option_rows()) == oc.DEFAULTS     # the table's default column, option by option


def test_every_value_of_the_golden_sweep_has_a_row():
    from tests.test_gpu_parity import OPTION_DEFAULTS, OPTION_VALUES
    have = {(r.option, r.value) for r in oc.TABLE}
    missing = [(name, v) for name, values in OPTION_VALUES.items() for v in values if (name, v) not in have]
    assert not missing, missing
    for name in ("prep_placement", "small_batch_filtered", "base_device_mb"):   # options the golden sweep does not know
        assert name not in OPTION_VALUES and len({v for o, v in have if o == name}) >= 2, name
    assert all(oc.DEFAULTS[name] == v for name, v in OPTION_DEFAULTS.items())
    assert {(r.option, r.value) for r in oc.TABLE if r.covered_by} >= {("pass_overlap", 0), ("pass_overlap", 1), ("shared_thresholds", 2),
                                                                       ("survivor_segments", 3)}


def test_rows_are_well_formed():
    ids = [oc.row_id(r) for r in oc.ENGAGED]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    for r in oc.ENGAGED:
        assert r.case in oc.CASES and callable(r.engaged) and set(r.also) <= set(oc.DEFAULTS) and r.option not in r.also, r
    for c in oc.CASES.values():
        assert c.index in oc.INDEXES and c.filter in (None, "half", "sparse")
    assert set(oc.GRID) <= set(oc.DEFAULTS) and np.prod([len(v) for v in oc.GRID.values()]) == 81


def test_covered_by_names_tests_that_exist():
    for r in oc.TABLE:
        if r.covered_by is None:
            continue
        path, name = r.covered_by.split("::")
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        assert name in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, r.covered_by
        assert r.option in open(os.path.join(ROOT, path)).read() or r.option in ("stage_growth", "scan_tile_table", "group_rank"), r


def test_trace_parser():
    err = ("[rabitq_hip] plan: coarse=exact kernel=sreg nq=5 k=7\n"
           "[rabitq_hip] plan: pass nq=5 nprobe=3 large=0 small=1 will_list=0 placed=0 fin_additive=0 qn_slots=3 nstages=1 seg_final=0 sb_nstages=1 sb_whole=0\n"
           "[rabitq_hip] plan: sb_stage=0 lo=0 hi=160\n"
           "[rabitq_hip] stage 0: [160, 4294967295) span 9 est_pairs 9 VALU, pair-major\n"
           "[rabitq_hip] plan: stage=0 lo=160 hi=4294967295 matrix=0 cluster_major=0 ranked=0 additive=0 arena=0 placed=0 table=0 dense_cells=0 slot_hi=3\n")
    ev = oc.Evidence(err)
    assert ev.coarse == ["exact"] and ev.coarse_kernels == ["sreg"] and len(ev.passes) == 1 and ev.passes[0]["qn_slots"] == 3
    assert ev.final() == ev.stages and ev.stages[0]["lo"] == 160 and ev.sb_stages == [{"sb_stage": 0, "lo": 0, "hi": 160}]
    with pytest.raises(AssertionError):
        oc.Evidence(err.replace("nstages=1 ", "nstages=2 "))


@pytest.fixture(scope="module")
def answers(oracle):
    a = oc.Answers(oracle)
    yield a
    a.close()


@pytest.mark.parametrize("case", sorted(oc.CASES))
def test_oracle_answers_every_case(answers, case):
    c = oc.CASES[case]
    assert case in {r.case for r in oc.ENGAGED}, "a case no row uses"
    for heur in (False, True):
        w = answers.want(case, heur)     # (raises where the reference panics)
        assert w["cnt"].shape == (c.nq,) and (w["cnt"] == c.topk).all(), (case, heur, np.bincount(w["cnt"]))
        assert w["rough"] >= w["precise"] >= c.nq * c.topk
    if c.filter:
        mask = answers.mask(c.index, c.filter)
        assert mask[answers.want(case, False)["ids"]].all()
    lens = np.diff(answers.index(c.index)[1].offsets.astype(np.int64))
    assert lens.min() > 0, "the slot bounds of the planner (qn_slots, slot_hi) need lists without an empty one"
