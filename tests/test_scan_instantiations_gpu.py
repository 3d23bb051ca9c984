"""Every separately compiled instantiation of the two scan kernels against the CPU oracle, on data where the final stage has
survivors that decide answers (tests/scan_cases.py; its conditions are asserted in tests/test_scan_cases.py):

  scan_kernel<W, CPL, ARENA, FILT>            (inst_scan_valu.hip)   W in {1,2,3,4,6,8,12,16} x ARENA x FILT
  scan_mfma_kernel<W, NT, ARENA, ADD, FILT>   (inst_scan_mfma.hip)   the same, plus the additive gate at W = 1 and 2

ARENA: survivor_segments = 2 (the final stage appends to the shared arena and is scattered into per-query segments); FILT: a filtered
call.  After every call the profile must show that the intended kernel ran.  Bit for bit everywhere -- ids in order, distance
bits, counts, the rough / precise counters: no tolerance appears in this file.

Run on the GPU box:  python -m pytest tests/test_scan_instantiations_gpu.py -m gpu -q
"""
import numpy as np
import pytest

from tests import scan_cases as sc
from tests.models import Ref, compare_with_oracle, run_range, same_range

pytestmark = pytest.mark.gpu

ENGINES = {"valu": 1, "matrix": 2}                    # option scan_impl
BUFFERS = {"uniform": 0, "arena": 2}                  # option survivor_segments
CONFIGS = ((None, 10, False), (None, 100, False), (3, 10, True))   # probe (None: k), topk, heuristic ranker


@pytest.fixture(scope="module")
def rq():
    import os
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def build_both(rq, oracle, W):
    x, centres, P, queries = sc.make_case(W)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert gidx.dim == 64 * W
    assert np.array_equal(gidx.map_ids, oidx.map_ids) and np.array_equal(gidx.offsets, oidx.offsets)
    return x, queries, oidx, gidx


def check_profile(pr, engine, buffers, what):
    assert pr["small_batch_passes"] == 0, (what, pr)
    if engine == "matrix":
        assert pr["matrix_launches"] == pr["scan_launches"] > 0 and pr["matrix_exact_steps"] > 0, (what, pr)
    else:
        assert pr["matrix_launches"] == 0 and pr["scan_launches"] > 0, (what, pr)
    if buffers == "arena":
        assert pr["segmented_passes"] >= 1, (what, pr)
    else:
        assert pr["segmented_passes"] == 0, (what, pr)


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("W", sc.WIDTHS)
def test_every_instantiation_matches_oracle(rq, oracle, W, engine):
    from rabitq_amd import index as ix
    _, queries, oidx, gidx = build_both(rq, oracle, W)
    k = gidx.k
    masks = dict({"none": None}, **sc.make_filters(oidx.map_ids, oidx.offsets))
    filters = {name: None if m is None else gidx.make_filter(mask=m) for name, m in masks.items()}
    seen = []
    try:
        ix.set_option("scan_impl", ENGINES[engine])
        ix.set_option("scan_gate", 1)        # the bf16 threshold form at every width (left to itself, dim 64 / 128 may pick the additive gate)
        for buffers, seg in BUFFERS.items():
            ix.set_option("survivor_segments", seg)
            for name, f in filters.items():
                for probe, topk, heur in CONFIGS:
                    what = (W, engine, buffers, name, probe, topk, heur)
                    compare_with_oracle(rq, oracle, oidx, gidx, queries, probe or k, topk, heur,
                                        filter=None if f is None else (f, masks[name]))
                    pr = ix.last_profile()
                    check_profile(pr, engine, buffers, what)
                    assert pr["matrix_additive_launches"] == 0, (what, pr)
                    seen.append((buffers, name, topk, heur, pr["scan_launches"], pr["matrix_launches"], pr["matrix_exact_steps"],
                                 pr["segmented_passes"], pr["retries"]))
        if engine == "matrix" and W in (1, 2):
            # the additive gate (ADD instantiations: dim 64 / 128, uniform buffers, unfiltered); a filtered stage must fall back to the
            # bf16 threshold form, for which alone the filtered instantiations exist
            ix.set_option("survivor_segments", 0)
            ix.set_option("scan_gate", 2)
            for probe, topk, heur in CONFIGS:
                compare_with_oracle(rq, oracle, oidx, gidx, queries, probe or k, topk, heur)
                pr = ix.last_profile()
                check_profile(pr, engine, "uniform", (W, "additive", topk, heur))
                assert pr["matrix_additive_launches"] > 0, (W, topk, heur, pr)
                seen.append(("uniform+additive", "none", topk, heur, pr["scan_launches"], pr["matrix_launches"], pr["matrix_exact_steps"],
                             pr["segmented_passes"], pr["retries"], pr["matrix_additive_launches"]))
            for name in ("half", "lists"):
                compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 10, False, filter=(filters[name], masks[name]))
                pr = ix.last_profile()
                check_profile(pr, engine, "uniform", (W, "additive, filtered", name))
                assert pr["matrix_additive_launches"] == 0, (W, name, pr)
    finally:
        ix.set_option("scan_impl", 0)
        ix.set_option("scan_gate", 0)
        ix.set_option("survivor_segments", 1)
        for f in filters.values():
            if f is not None:
                f.close()
        gidx.close()
        oidx.close()
        print(f"W={W} {engine}: (buffers, filter, topk, heuristic, scan_launches, matrix_launches, matrix_exact_steps, segmented_passes, "
              f"retries[, matrix_additive_launches])")
        for s in seen:
            print("   ", s)


@pytest.mark.parametrize("W", sc.WIDTHS)
def test_range_search_every_width(rq, oracle, W):
    """One stage under a fixed radius per query, on both engines.  The radii come from the oracle: most queries their own
    20th-neighbour distance over all lists, one radius 0 (an empty answer), one that admits hundreds of rows from several lists."""
    from rabitq_amd import index as ix
    x, queries, oidx, gidx = build_both(rq, oracle, W)
    k = gidx.k
    try:
        radii = np.array([oidx.query(q, k, 20)[0].max() for q in queries], dtype=np.float32)
        radii[9] = 0.0
        wide = 12
        radii[wide] = np.partition(((x.astype(np.float64) - queries[wide]) ** 2).sum(axis=1), 400)[400]
        ref = Ref(oracle, oidx)
        want = ref.answer(queries, k, radii)
        lims = want[0].astype(np.int64)
        counts = np.diff(lims)
        assert counts[9] == 0 and counts[wide] >= 200 and (counts > 0).sum() >= sc.NQ - 2, (counts[9], counts[wide], (counts > 0).sum())
        # from the oracle's answer alone: most non-empty answers hold a row outside the query's nearest list, and a row from the second
        # half of the stream (one stage: there is no final stage to speak of)
        nonempty = np.nonzero(counts)[0]
        outside, _ = sc.spread(oidx, queries[nonempty], [want[2][lims[b]:lims[b + 1]] for b in nonempty])
        assert 2 * outside.sum() >= nonempty.size, (outside.sum(), nonempty.size)
        wide_lists = np.unique(np.searchsorted(oidx.offsets.astype(np.int64), np.argsort(oidx.map_ids)[want[2][lims[wide]:lims[wide + 1]]],
                                               side="right") - 1)
        assert wide_lists.size >= 3, wide_lists
        for engine, impl in ENGINES.items():
            ix.set_option("scan_impl", impl)
            got, m, pr = run_range(rq, gidx, queries, k, radii)
            same_range(got, want[:3], (W, engine))
            assert (m["rough"], m["precise"], m["query"]) == (want[3]["rough"], want[3]["precise"], sc.NQ), (W, engine, m, want[3])
            assert pr["small_batch_passes"] == 0 and pr["scan_launches"] > 0, (W, engine, pr)
            if engine == "matrix":
                assert pr["matrix_launches"] > 0, (W, pr)
            else:
                assert pr["matrix_launches"] == 0, (W, pr)
    finally:
        ix.set_option("scan_impl", 0)
        gidx.close()
        oidx.close()
