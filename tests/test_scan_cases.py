"""The conditions tests/test_scan_instantiations_gpu.py relies on, asserted on the CPU oracle alone (no GPU): the inputs of
tests/scan_cases.py give four long lists, one shorter than a candidate sub-tile and an empty one; the final stage of a pass is long
enough to be an arena stage under survivor_segments = 2; and it decides part of most answers -- unfiltered and under each filter.
The thresholds are conditions on the inputs, not measurements: the unfiltered mixture alone gives 290 of 290."""
import numpy as np
import pytest

from tests import scan_cases as sc
from tests.models import sub_arrays


@pytest.mark.parametrize("W", [3, 16])
def test_case_conditions(oracle, W):
    x, centres, P, queries = sc.make_case(W)
    assert x.shape == (sc.N, 64 * W) and centres.shape == (6, 64 * W) and queries.shape == (sc.NQ, 64 * W)
    assert sc.NQ > 9 * 32 and sc.NQ % 32                                 # ten query tiles per list, the last one ragged
    assert np.array_equal(queries[sc.QUERY_IS_ROW], x[11]) and np.array_equal(queries[sc.QUERY_IS_CENTROID], centres[1])
    oidx = oracle.OracleIndex.build(x, centres, P)
    try:
        k = oidx.k
        lens = np.sort(np.diff(oidx.offsets.astype(np.int64)))
        # (a) four long lists, one shorter than a 32-row sub-tile, one empty
        assert lens[0] == 0 and 1 <= lens[1] <= 31 and (lens[2:] >= 2000).all(), lens
        mll = int(lens[-1])
        # (b) the final stage's span exceeds the uniform capacity: an arena stage -- at probe = k and at the probe-3 configuration
        assert sc.final_span(mll, k) > sc.DEFAULT_CAP and sc.final_span(mll, 3) > sc.DEFAULT_CAP, mll
        # the short list's centroid is a query whose nearest list is the short one
        first, _ = oidx.coarse_rank(oidx.rotate_query(queries[sc.QUERY_IS_SHORT_CENTROID]), 1)
        off = oidx.offsets.astype(np.int64)
        assert off[int(first[0]) + 1] - off[int(first[0])] == lens[1]
        # (c) probe = k, topk 10: at least half of the queries return a neighbour outside their nearest list -- and, stricter, a
        # neighbour from the stream positions the final stage scans
        answers = [oidx.query(q, k, 10)[1] for q in queries]
        outside, final = sc.spread(oidx, queries, answers)
        print(f"W={W} unfiltered: outside the nearest list {outside.sum()} / {sc.NQ}, from the final stage {final.sum()} / {sc.NQ}")
        assert 2 * outside.sum() >= sc.NQ and 2 * final.sum() >= sc.NQ
        # (d) the same under each filter, on the sub-index the filter leaves
        filters = sc.make_filters(oidx.map_ids, oidx.offsets)
        longest = int(np.argmax(np.diff(off)))
        assert not filters["lists"][oidx.map_ids[off[longest]:off[longest + 1]]].any() and 0.4 < filters["half"].mean() < 0.6
        for name, allowed in filters.items():
            ov = oracle.OracleIndex.view(oidx.dim, *sub_arrays(oidx, allowed))
            try:
                answers = [ov.query(q, k, 10)[1] for q in queries]
                assert all(allowed[a].all() for a in answers)
                outside, final = sc.spread(ov, queries, answers, full=oidx)
                print(f"W={W} filter {name}: outside the nearest list {outside.sum()} / {sc.NQ}, from the final stage {final.sum()} / {sc.NQ}")
                assert 2 * outside.sum() >= sc.NQ and 2 * final.sum() >= sc.NQ, name
                # the heuristic ranker's configuration answers every query (the reference panics on a query without a candidate)
                for q in queries:
                    ov.query(q, 3, 10, True)
            finally:
                ov.close()
    finally:
        oidx.close()
