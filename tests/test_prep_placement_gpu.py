"""Option prep_placement: the pass's final matrix-core stage is grouped BEFORE the query quantisation, which then writes every
pair's fp6 operand row (and the threshold-free part of its tail) straight into the stage's tile images; a list-major kernel
completes the tails once the early stages have set the thresholds (with the lists' v' ranges on the way).  0 = the older kernels
everywhere (pair-major operand, stage_fill_kernel, group_vrange_kernel).

Both settings must return the same bits on the same index and queries: distances, ids in the same order, counts, and the always-on
counters -- equal matrix_exact_steps is the check that V0 / DV and C_q are the same bits (a different bound flags different steps).

matrix_exact_steps counts the 32-query x 32-candidate sub-tile steps in which any cell passed the gate, so it depends on WHICH
queries share a 32-row tile of a list's group -- and the places inside a group are handed out by atomics (group_rank_kernel's LDS
histogram, or one global atomic per pair) in whatever order the waves arrive.  Measured on the first case below (9001 queries x 64
probes, 852 960 sub-tile steps), eight calls in a row: prep_placement 0 alone gave 708 418, 707 991, 707 782, 707 846 flagged
steps, prep_placement 1 gave 708 969, 708 622, 707 973, 707 946; with group_rank 0 (the older kernels under either setting) 707 739
to 709 597.  The counter is therefore compared where it is a function of the inputs alone: the cases whose queries are chosen so
that no list is probed by more than 32 of them -- every group is ONE tile, whatever the order inside it -- assert it equal, for
both gates; the cases with many tiles per list compare every other counter (and matrix_subtile_steps, which does not depend on
the order).
Indexes on which the matrix-core final stage really engages; whether a pass took the new path is read from the stage-list hook
(scan_debug 16384 prints "placed ahead of the quantisation" for such a stage).

Run on the GPU box:  python -m pytest tests/test_prep_placement_gpu.py -m gpu -x -q
"""
import numpy as np
import pytest

from tests import synth
from tests.test_gpu_parity import _compare_with_oracle, assert_bits_equal, rq  # noqa: F401  (rq: module-scoped fixture)

pytestmark = pytest.mark.gpu

COUNTERS = ("rerank_candidates", "rerank_shadow_rejects", "matrix_subtile_steps", "matrix_exact_steps", "retries",
            "matrix_launches", "matrix_additive_launches", "scan_launches", "segmented_passes")
MARK = "placed ahead of the quantisation"


def _run(rq, capfd, gidx, queries, probe, topk, heur, placement, **kw):
    """One batch under prep_placement = placement: results, metrics + profile counters, and whether a stage was placed ahead."""
    from rabitq_amd import index as ix
    ix.set_option("prep_placement", placement)
    ix.set_option("scan_debug", 16384)
    try:
        capfd.readouterr()
        rq.metrics_reset()
        d, ids, cnt = gidx.query_batch(queries, probe, topk, heur, **kw)
        m = rq.metrics()
        pr = ix.last_profile()
        err = capfd.readouterr().err
    finally:
        ix.set_option("scan_debug", 0)
        ix.set_option("prep_placement", 1)
    counters = {"rough": m["rough"], "precise": m["precise"], **{c: pr[c] for c in COUNTERS}}
    return (d, ids, cnt), counters, err


def _same(rq, capfd, gidx, queries, probe, topk, heur, expect_placed, exact_steps=False, **kw):
    """prep_placement 1 against 0, twice each after a first call that learns capacities and hints; bit for bit."""
    from rabitq_amd import index as ix
    got = {}
    # a pass that learns of survivor overflows turns later ones into arena passes, which keep the older kernels: the cases that
    # expect the new path stay on the uniform survivor buffers (capacities learnt in the first calls, for both settings alike)
    if expect_placed:
        ix.set_option("survivor_segments", 0)
    try:
        for _ in range(2):
            _run(rq, capfd, gidx, queries, probe, topk, heur, 0, **kw)
        return _same_body(rq, capfd, gidx, queries, probe, topk, heur, expect_placed, exact_steps, got, **kw)
    finally:
        if expect_placed:
            ix.set_option("survivor_segments", 1)


def _same_body(rq, capfd, gidx, queries, probe, topk, heur, expect_placed, exact_steps, got, **kw):
    for rep in range(2):
        for placement in (0, 1):
            got[placement] = _run(rq, capfd, gidx, queries, probe, topk, heur, placement, **kw)
        (a, ca, ea), (b, cb, eb) = got[1], got[0]
        for u, v, what in zip(a, b, ("distances", "ids", "counts")):
            assert_bits_equal(u, v, f"prep_placement 1 vs 0, call {rep}: {what}")
        print("counters, call", rep, ca, cb)
        if not exact_steps:   # (several tiles per list: the flagged steps depend on the order inside the groups, module docstring)
            ca, cb = ({k: v for k, v in c.items() if k != "matrix_exact_steps"} for c in (ca, cb))
        assert ca == cb, (rep, ca, cb)
        assert MARK not in eb, "prep_placement = 0 must run the older kernels everywhere"
        assert (MARK in ea) == expect_placed, (expect_placed, ea)
        assert ca["matrix_launches"] > 0, "the matrix-core final stage must engage in this case"
    return got[1]


def _index(rq, n, d, k, seed, empty=0, sigma=0.8):
    x, centres, _ = synth.mixture(n, d, k - empty, sigma=sigma, seed=seed, centre_scale=0.6)
    if empty:   # lists that stay empty: nobody's pairs land in them, their groups have no rows
        centres = np.concatenate([centres, 50.0 + np.arange(empty * d, dtype=np.float32).reshape(empty, d)])
    P = synth.random_orthogonal(d, seed=seed + 1)
    return x, centres, P, rq.RaBitQ.build(x, centres, P)


@pytest.mark.parametrize("heur", [False, True])
def test_dim128_additive_big_stage_reached_automatically(rq, capfd, heur):
    """9001 queries (not a multiple of 32) x 64 probes: a final stage of more than 16 blocks of pairs, placed by rank the
    automatic way; six lists are empty: groups without a row, lists whose pairs are never inside the stage."""
    from rabitq_amd import index as ix
    n, d, k = 30_000, 128, 96
    x, centres, P, gidx = _index(rq, n, d, k, 91, empty=6)
    queries, _, _ = synth.mixture(9001, d, k - 6, sigma=0.8, seed=93, centre_scale=0.6)
    ix.set_option("scan_gate", 2)
    try:
        _, c, _ = _same(rq, capfd, gidx, queries, 64, 10, heur, True)
        assert c["matrix_additive_launches"] > 0
    finally:
        ix.set_option("scan_gate", 0)
        gidx.close()


@pytest.mark.parametrize("heur", [False, True])
def test_dim64_additive_forced_rank(rq, capfd, heur):
    from rabitq_amd import index as ix
    n, d, k = 40_000, 64, 64
    x, centres, P, gidx = _index(rq, n, d, k, 191)
    queries, _, _ = synth.mixture(3007, d, k, sigma=0.8, seed=193, centre_scale=0.6)
    ix.set_option("scan_gate", 2)
    ix.set_option("group_rank", 2)
    try:
        _, c, _ = _same(rq, capfd, gidx, queries, 32, 10, heur, True)
        assert c["matrix_additive_launches"] > 0
    finally:
        ix.set_option("scan_gate", 0)
        ix.set_option("group_rank", 1)
        gidx.close()


@pytest.mark.parametrize("n,d,k,nq,probe", [(20_000, 256, 32, 1003, 16), (12_000, 768, 12, 515, 12), (20_000, 128, 32, 1003, 16)])
@pytest.mark.parametrize("heur", [False, True])
def test_bf16_gate_wide_dims(rq, capfd, n, d, k, nq, probe, heur):
    """The bf16 threshold form of the tile images (rows of 12 W + 2 dwords, 20-dword tails): the only form at dim > 128, pinned at 128."""
    from rabitq_amd import index as ix
    x, centres, P, gidx = _index(rq, n, d, k, 291 + d)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=293 + d, centre_scale=0.6)
    ix.set_option("scan_gate", 1)
    ix.set_option("group_rank", 2)
    try:
        _, c, _ = _same(rq, capfd, gidx, queries, probe, 10, heur, True)
        assert c["matrix_additive_launches"] == 0
    finally:
        ix.set_option("scan_gate", 0)
        ix.set_option("group_rank", 1)
        gidx.close()


def _balanced_queries(centres, pool, probe, cap, want):
    """Queries of the pool, taken in order while none of their probe lists is probed by `cap` queries already."""
    d2 = (pool * pool).sum(1)[:, None] - 2 * pool @ centres.T + (centres * centres).sum(1)[None, :]
    cl = np.argsort(d2, 1)[:, :probe]
    cnt = np.zeros(len(centres), np.int64)
    keep = []
    for i in range(len(pool)):
        if (cnt[cl[i]] < cap).all():
            cnt[cl[i]] += 1
            keep.append(i)
            if len(keep) == want:
                break
    return pool[np.array(keep)]


@pytest.mark.parametrize("n,d,gate,want", [(60_000, 128, 2, 333), (60_000, 64, 2, 333), (40_000, 256, 1, 290), (60_000, 128, 1, 333)])
@pytest.mark.parametrize("heur", [False, True])
def test_one_tile_per_list_flags_the_same_steps(rq, capfd, n, d, gate, want, heur):
    """No list is probed by more than 32 queries: every group of the final stage is one tile, so the flagged
    sub-tile steps depend on V0 / DV, C_q and the thresholds alone, and must be the same number under both settings."""
    from rabitq_amd import index as ix
    k, probe = 512, 20
    x, centres, P, gidx = _index(rq, n, d, k, 491 + d)
    pool, _, _ = synth.mixture(4000, d, k, sigma=0.8, seed=493 + d, centre_scale=0.6)
    queries = np.ascontiguousarray(_balanced_queries(centres, pool, probe, 28, want))
    assert len(queries) == want and want % 32 != 0
    _, cl, _ = rq.ops.coarse_rank(gidx, queries, probe)
    per_list = np.bincount(np.asarray(cl).reshape(-1), minlength=k)
    assert per_list.max() <= 32, per_list.max()
    ix.set_option("scan_gate", gate)
    ix.set_option("group_rank", 2)
    try:
        _, c, _ = _same(rq, capfd, gidx, queries, probe, 10, heur, True, exact_steps=True)
        assert (c["matrix_additive_launches"] > 0) == (gate == 2)
        assert c["matrix_subtile_steps"] > 0
    finally:
        ix.set_option("scan_gate", 0)
        ix.set_option("group_rank", 1)
        gidx.close()


@pytest.mark.parametrize("d,gate", [(128, 2), (64, 2), (256, 0)])
def test_placed_pass_matches_oracle(rq, oracle, capfd, d, gate):
    from rabitq_amd import index as ix
    n, k = 20_000, 32
    x, centres, P, gidx = _index(rq, n, d, k, 391 + d, empty=2)
    oidx = oracle.OracleIndex.build(x, centres, P)
    queries, _, _ = synth.mixture(333, d, k - 2, sigma=0.8, seed=393 + d, centre_scale=0.6)
    queries[1] = x[17]
    ix.set_option("scan_gate", gate)
    ix.set_option("group_rank", 2)
    ix.set_option("scan_debug", 16384)
    try:
        for probe, topk, heur in ((20, 10, False), (32, 5, True)):
            capfd.readouterr()
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, heur)
            assert MARK in capfd.readouterr().err
    finally:
        ix.set_option("scan_debug", 0)
        ix.set_option("scan_gate", 0)
        ix.set_option("group_rank", 1)
        gidx.close()
        oidx.close()


def test_filtered_pass_keeps_the_older_kernels(rq, capfd):
    n, d, k = 30_000, 128, 96
    x, centres, P, gidx = _index(rq, n, d, k, 91, empty=6)
    queries, _, _ = synth.mixture(9001, d, k - 6, sigma=0.8, seed=93, centre_scale=0.6)
    allowed = np.random.default_rng(7).random(n) < 0.5
    try:
        with gidx.make_filter(mask=allowed) as f:
            _same(rq, capfd, gidx, queries, 64, 10, False, False, filter=f)
    finally:
        gidx.close()


def test_shard_like_pass_keeps_the_older_kernels(rq, capfd):
    """A quarter shard: most probed lists are empty here, the pass lists its non-empty pairs (pair_split_kernel)."""
    n, d, k = 60_000, 128, 64
    x, centres, P, gidx = _index(rq, n, d, k, 61)
    owner, _ = gidx.partition_lists(4)
    shard = gidx.shard(owner, 1)
    assert int((np.diff(shard.offsets.astype(np.int64)) > 0).sum()) * 2 < k
    queries, _, _ = synth.mixture(9001, d, k, sigma=0.8, seed=63, centre_scale=0.6)
    from rabitq_amd import index as ix
    ix.set_option("scan_gate", 2)
    try:
        _same(rq, capfd, shard, queries, 64, 10, False, False)
    finally:
        ix.set_option("scan_gate", 0)
        shard.close()
        gidx.close()


def test_arena_pass_keeps_the_older_kernels(rq, capfd):
    """survivor_segments = 2: every batch of >= 256 queries runs its final stage through the survivor arena (seg_final)."""
    from rabitq_amd import index as ix
    n, d, k = 30_000, 128, 96
    x, centres, P, gidx = _index(rq, n, d, k, 91, empty=6)
    queries, _, _ = synth.mixture(9001, d, k - 6, sigma=0.8, seed=93, centre_scale=0.6)
    ix.set_option("survivor_segments", 2)
    try:
        _, c, _ = _same(rq, capfd, gidx, queries, 64, 10, False, False)
        assert c["segmented_passes"] == 1
    finally:
        ix.set_option("survivor_segments", 1)
        gidx.close()


def test_option_range(rq):
    from rabitq_amd import index as ix
    for bad in (-1, 2):
        with pytest.raises(rq.RabitqError):
            ix.set_option("prep_placement", bad)
    ix.set_option("prep_placement", 0)
    ix.set_option("prep_placement", 1)
