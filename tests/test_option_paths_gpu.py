"""Every value of every option, on an index and a batch where the value's code path really runs (tests/option_cases.py): the index
is built under the option, the case's batch goes through query_batch with both rankers, the answer is compared with the CPU oracle's
bit for bit (counts, ids in order, distance bits, the rough / precise / query counters: no tolerance), and the row's `engaged`
predicate must hold on the plan trace (scan_debug bit 16384), the profile and rq_info -- a value whose path did not run fails.
tests/test_gpu_parity.py::test_every_option_value_keeps_golden_results runs the same values on a 1000-vector golden, where most of
these paths never start.

The planner grid runs the 81 combinations of the four planner knobs on case A against the same answers and checks what
host_plan.h promises about the 4-bit operand: no VALU stage reaches a probe slot beyond qn_slots.

Run on the GPU box:  python -m pytest tests/test_option_paths_gpu.py -m gpu -x -q
"""
import itertools

import numpy as np
import pytest

from tests import option_cases as oc
from tests.models import ARRAYS
from tests.test_gpu_parity import assert_bits_equal, rq  # noqa: F401  (rq: module-scoped fixture)

pytestmark = pytest.mark.gpu
TRACE = 16384


@pytest.fixture(scope="module")
def answers(oracle):
    """The oracle's answers, once per case for the whole module (every option value compares with the same arrays)."""
    a = oc.Answers(oracle)
    a.base = {}   # (case, ranker) -> the evidence of the run under the default options
    yield a
    a.close()


def _set(opts):
    from rabitq_amd import index as ix
    for name, v in opts.items():
        ix.set_option(name, v)


def _info(gidx):
    lens = np.diff(gidx.offsets.astype(np.int64))
    return dict(n=gidx.n, n_hbm=gidx.n_hbm, split_rows=gidx.split_rows, k=gidx.k, dim=gidx.dim, max_list_len=gidx.max_list_len,
                min_list_len=int(lens.min()), lens=lens)


def _call(rq, capfd, answers, gidx, case, heur, filt, info, what):
    """One query_batch of the case: compared with the oracle's answer; -> the call's evidence."""
    from rabitq_amd import index as ix
    c = oc.CASES[case]
    capfd.readouterr()
    rq.metrics_reset()
    got = gidx.query_batch(answers.queries(case), c.probe, c.topk, heur, filter=filt)
    counters, profile = rq.metrics(), ix.last_profile()
    err = capfd.readouterr().err
    oc.same_answer(got, answers.want(case, heur), counters, what)
    return oc.Evidence(err, profile, info, answers.base.get((case, heur)))


def _run_case(rq, capfd, answers, case, opts, engaged=None, what=""):
    """Per ranker: build the case's index under `opts` (+ the trace bit), check the built arrays, run the batch; -> the evidence of
    each.  (A fresh index per ranker: what an index learns from a batch -- on case A the automatic gate of the matrix-core scan
    falls back to the bf16 form after the first one, rq_index::additive_loose -- must not decide which path the second call takes.)"""
    c = oc.CASES[case]
    (x, centres, P, _), oidx = answers.index(c.index)
    opts = dict(opts, scan_debug=opts.get("scan_debug", 0) | TRACE)
    out = []
    for heur in (False, True):
        gidx = filt = None
        try:
            _set(opts)
            gidx = rq.RaBitQ.build(x, centres, P)   # (several options act at build time)
            assert (gidx.n, gidx.k) == (oidx.n, oidx.k)
            for name in ARRAYS + ("map_ids",):
                assert_bits_equal(getattr(gidx, name), getattr(oidx, name), f"{what}: built {name}")
            info = _info(gidx)
            if c.filter:
                filt = gidx.make_filter(mask=answers.mask(c.index, c.filter))
            ev = _call(rq, capfd, answers, gidx, case, heur, filt, info, f"{what} heur={heur}")
            with capfd.disabled():
                print(what, "heur", heur, "passes", [(p["large"], p["small"], p["qn_slots"], oc.stage_list(p), p["sb_stages"]) for p in ev.passes],
                      "coarse", ev.coarse, ev.coarse_kernels, {key: v for key, v in ev.profile.items() if not key.startswith("ms_")})
            if engaged is not None:
                assert engaged(ev), (what, heur, ev.passes, ev.coarse, ev.coarse_kernels, ev.profile, {k: v for k, v in info.items() if k != "lens"})
            out.append(ev)
        finally:
            _set(oc.DEFAULTS)
            if filt is not None:
                filt.close()
            if gidx is not None:
                gidx.close()
    return out


def _baseline(rq, capfd, answers, case):
    if (case, False) not in answers.base:
        evs = _run_case(rq, capfd, answers, case, {}, what=f"defaults@{case}")
        answers.base[case, False], answers.base[case, True] = evs


@pytest.mark.parametrize("row", oc.ENGAGED, ids=[oc.row_id(r) for r in oc.ENGAGED])
def test_option_value_runs_its_path_and_keeps_results(rq, answers, capfd, row):
    _baseline(rq, capfd, answers, row.case)
    _run_case(rq, capfd, answers, row.case, dict(row.also, **{row.option: row.value}), row.engaged, oc.row_id(row))


@pytest.mark.parametrize("heur", [False, True])
def test_planner_grid(rq, answers, capfd, heur):
    """large_batch_from x stage_settle_pct x stage_growth x cluster_major_div on case A, one index, the same cached answers: the
    knobs plan_pass turns into stage boundaries, VALU versus matrix cores, the work records' layout, dense directories and
    qn_slots, the probe slots that get the 4-bit operand at all.  A stage that reached a slot beyond qn_slots would scan an
    operand that was never written."""
    case = "A"
    c = oc.CASES[case]
    (x, centres, P, _), oidx = answers.index(c.index)
    names = list(oc.GRID)
    plans, slots = set(), set()
    gidx = None
    try:
        _set({"scan_debug": TRACE})
        gidx = rq.RaBitQ.build(x, centres, P)
        info = _info(gidx)
        for values in itertools.product(*(oc.GRID[n] for n in names)):
            _set(dict(zip(names, values)))
            ev = _call(rq, capfd, answers, gidx, case, heur, None, info, f"grid {dict(zip(names, values))} heur={heur}")
            assert len(ev.passes) == 1 and ev.passes[0]["nprobe"] == c.probe, ev.passes
            for p in ev.passes:
                plans.add(oc.stage_list(p))
                slots.add(p["qn_slots"])
                assert all(s["slot_hi"] <= p["qn_slots"] for s in p["stages"] if not s["matrix"]), (values, p)
                assert all(s["slot_hi"] <= p["nprobe"] for s in p["stages"]), (values, p)
        with capfd.disabled():
            print("distinct stage lists", len(plans), "qn_slots", sorted(slots))
        assert len(plans) >= 8, sorted(plans)
        assert len(slots) >= 3 and min(slots) < c.probe, sorted(slots)
    finally:
        _set(oc.DEFAULTS)
        if gidx is not None:
            gidx.close()
