"""Range search where its tail changes shape: per-query result lengths set EXACTLY on the boundaries of the sort's length
classes (kernels_range.h: one wave up to RQ_RANGE_WAVE_MAX = 64 keys, a 256-thread block up to RQ_RANGE_SMALL_MAX = 2048, a
1024-thread block up to RQ_RANGE_TILE = 16 384, beyond that tiles + merge passes), on whole numbers of tiles, on 2^m tiles and
one more key -- and results that are runs of thousands of equal distances, which only the id orders, across tile and merge
boundaries (range_merge_kernel places every key by rank on the promise that keys are unique).

How a length is set: centroids far apart (30 sigma), lists of chosen sizes, probe = 1 and radius f32::MAX: the answer is the
query's own list, whole.  Every test first asserts on the CPU oracle that its build has exactly these list sizes and that the
model's answer (tests/models.py: Ref) has exactly these counts, then compares the engine with it: lims, ids in order, distance
bits, counters.  No tolerance.

Run on the GPU box:  python -m pytest tests/test_range_edges_gpu.py -m gpu -q
"""
import os

import numpy as np
import pytest

from tests import synth
from tests.models import FMAX, Live, Ref, check_oracle, run_range, same_range, sub_arrays

pytestmark = pytest.mark.gpu

D = 64
# list c holds SIZES[c] rows: both sides of every class boundary, 2 and 3 whole tiles, 2 and 4 tiles and one key, one empty list
SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 16_383, 16_384, 16_385, 32_768, 32_769, 49_152, 65_537, 0]
DEFAULT_CAP = 4096        # candidates per query a first range pass holds; RQ_MAX_CAP_HINT = 32 768 is the most an index learns
MAX_CAP_HINT = 32_768


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def make(sizes, copies=False, seed=1):
    """-> rows (list c = ids [sum(sizes[:c]), sum(sizes[:c + 1]))), centroids, rotation, one query per list.
    copies: every row of a list is an exact copy of one of three vectors of that list."""
    rng = np.random.default_rng(seed)
    k = len(sizes)
    centres = np.zeros((k, D), dtype=np.float32)
    centres[np.arange(k), np.arange(k)] = 30.0
    lists = np.repeat(np.arange(k), sizes)
    if copies:
        three = rng.standard_normal((k, 3, D)).astype(np.float32)
        x = centres[lists] + three[lists, rng.integers(0, 3, lists.size)]
    else:
        x = centres[lists] + rng.standard_normal((lists.size, D)).astype(np.float32)
    queries = centres + 0.5 * rng.standard_normal((k, D)).astype(np.float32)
    return np.ascontiguousarray(x, np.float32), centres, synth.random_orthogonal(D, seed=seed + 1), np.ascontiguousarray(queries, np.float32)


def batch(oidx, queries, probe):
    """Every query twice, interleaved: radius f32::MAX (its probed lists, whole) and 1.3 x the oracle's own 10th distance (a
    handful) -- so the wave, small-block, block and tiled segments alternate in the call."""
    q2 = np.repeat(queries, 2, axis=0)
    radii = np.full(len(q2), FMAX, dtype=np.float32)
    for b, q in enumerate(queries):
        od = oidx.query(q, probe, 10)[0]
        radii[2 * b + 1] = od.max() * np.float32(1.3) if od.size else 0.0
    return q2, radii


def classes(counts):
    return {int(np.searchsorted([64, 2048, 16_384], c)) for c in counts if c > 0}      # 0 wave, 1 small block, 2 block, 3 tiles


def compare(rq, g, ref, q2, probe, radii, want, what, fresh=True, filt=None):
    """One engine call against `want`; -> profile.  fresh: the index has learnt no capacity yet, so every query with more than
    DEFAULT_CAP candidates must have been run again; otherwise at least those beyond MAX_CAP_HINT."""
    got, m, pr = run_range(rq, g, q2, probe, radii, filter=filt)
    same_range(got, want[:3], what)
    assert (m["rough"], m["precise"], m["query"]) == (want[3]["rough"], want[3]["precise"], len(q2)), (what, m, want[3])
    assert pr["retries"] >= int((ref.candidates > (DEFAULT_CAP if fresh else MAX_CAP_HINT)).sum()), (what, pr["retries"])
    return pr


@pytest.fixture(scope="module")
def plain(oracle):
    x, centres, P, queries = make(SIZES)
    oidx = oracle.OracleIndex.build(x, centres, P)
    assert np.diff(oidx.offsets.astype(np.int64)).tolist() == SIZES       # the oracle's build has exactly these lists
    yield x, centres, P, queries, oidx
    oidx.close()


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_lengths_on_class_boundaries(rq, oracle, plain, impl):
    """probe 1: the counts are SIZES themselves; probe 2 and 3: sums that cross a class.  Each call mixes queries that are run
    again (more candidates than the first pass holds) with queries that are not -- the answer is united from the pieces --; the
    second call on the index runs with the capacity the first one learnt and must give the same answer.  scan_impl 0 / 1 / 2."""
    from rabitq_amd import index as ix
    x, centres, P, queries, oidx = plain
    ref = Ref(oracle, oidx)
    ix.set_option("scan_impl", impl)
    try:
        g = rq.RaBitQ.build(x, centres, P)
        for probe in (1, 2, 3):
            q2, radii = batch(oidx, queries, probe)
            want = ref.answer(q2, probe, radii)
            counts = np.diff(want[0].astype(np.int64))
            if probe == 1:
                assert counts[0::2].tolist() == SIZES                      # the model's answer has exactly these lengths
                assert (counts[1::2] <= counts[0::2]).all() and counts[1::2].max() < 2048
            assert classes(counts) == {0, 1, 2, 3}, counts
            assert ((ref.candidates > DEFAULT_CAP).sum() >= 5) and ((ref.candidates <= DEFAULT_CAP).sum() >= 5)
            cands = ref.candidates.copy()
            pr1 = compare(rq, g, ref, q2, probe, radii, want, (impl, probe, "first"), fresh=(probe == 1))
            ref.candidates = cands
            pr2 = compare(rq, g, ref, q2, probe, radii, want, (impl, probe, "second"), fresh=False)
            print(f"scan_impl {impl} probe {probe}: counts {sorted(counts.tolist())[-6:]} retries {pr1['retries']} then {pr2['retries']}")
            assert pr2["retries"] <= pr1["retries"]
        g.close()
    finally:
        ix.set_option("scan_impl", 0)


def test_runs_of_equal_distances_across_tiles(rq, oracle):
    """The same lists with every row an exact copy of one of three vectors: a result is at most three runs of equal distance
    bits, thousands of entries long, ordered by id alone -- across the tiles of the LDS sorts and the runs of the merge passes."""
    x, centres, P, queries = make(SIZES, copies=True, seed=3)
    oidx = oracle.OracleIndex.build(x, centres, P)
    try:
        assert np.diff(oidx.offsets.astype(np.int64)).tolist() == SIZES
        ref = Ref(oracle, oidx)
        g = rq.RaBitQ.build(x, centres, P)
        for probe in (1, 3):
            q2, radii = batch(oidx, queries, probe)
            want = ref.answer(q2, probe, radii)
            counts = np.diff(want[0].astype(np.int64))
            if probe == 1:
                assert counts[0::2].tolist() == SIZES
                for b in range(0, len(q2), 2):           # at most three distinct distances per list, ids ascending inside a run
                    lo, hi = int(want[0][b]), int(want[0][b + 1])
                    dist, ids = want[1][lo:hi], want[2][lo:hi]
                    assert np.unique(dist.view(np.uint32)).size <= 3
                    run_start = np.r_[True, dist.view(np.uint32)[1:] != dist.view(np.uint32)[:-1]]
                    assert (np.diff(ids.astype(np.int64))[~run_start[1:]] > 0).all()
                longest = max(np.diff(np.nonzero(np.r_[True, want[1].view(np.uint32)[1:] != want[1].view(np.uint32)[:-1], True])[0]))
                assert longest > 16_384, longest             # a single run of equal keys longer than a tile
            cands = ref.candidates.copy()
            compare(rq, g, ref, q2, probe, radii, want, ("copies", probe, "first"), fresh=(probe == 1))
            ref.candidates = cands
            compare(rq, g, ref, q2, probe, radii, want, ("copies", probe, "second"), fresh=False)
        g.close()
    finally:
        oidx.close()


def test_ids_out_of_storage_order(rq, oracle):
    """The copies again, but 60 % of the rows built and the others added under explicit ids, permuted and descending, that
    interleave with nothing the build gave out: the order inside a run of equal distances is the id's, not the order the rows
    were stored or added in.  Expected: the oracle's build of the live rows in id order, ids translated."""
    sizes = SIZES[:12] + [0, 0, 0, 0]                        # (up to two tiles and one key: the live rows are rebuilt on the host)
    x, centres, P, queries = make(sizes, copies=True, seed=5)
    n = x.shape[0]
    rng = np.random.default_rng(6)
    order = rng.permutation(n)
    first, rest = np.sort(order[:n * 6 // 10]), order[n * 6 // 10:]
    g = rq.RaBitQ.build(x[first], centres, P)
    live = Live(np.arange(first.size), x[first])
    half = rest.size // 2
    new_ids = np.concatenate([(1 << 24) + rng.permutation(half), (1 << 22) - np.arange(rest.size - half)]).astype(np.uint32)
    assert np.array_equal(g.add(x[rest], ids=new_ids), new_ids)
    live.add(new_ids, x[rest])
    oidx, ids = check_oracle(oracle, g, live, centres, P, "explicit ids", keep=True)
    try:
        assert np.diff(oidx.offsets.astype(np.int64)).tolist() == sizes
        assert not np.array_equal(np.sort(ids[oidx.map_ids[:sizes[0] + sizes[1] + sizes[2]]]), ids[oidx.map_ids[:sizes[0] + sizes[1] + sizes[2]]])
        ref = Ref(oracle, oidx, ids)
        for probe in (1, 2):
            q2, radii = batch(oidx, queries, probe)
            want = ref.answer(q2, probe, radii)
            if probe == 1:
                assert np.diff(want[0].astype(np.int64))[0::2].tolist() == sizes
            compare(rq, g, ref, q2, probe, radii, want, ("explicit ids", probe), fresh=(probe == 1))
    finally:
        oidx.close()
        g.close()


def test_filtered_lengths_on_class_boundaries(rq, oracle):
    """Lists of twice the sizes under a filter that admits every other id: the FILTERED counts are SIZES.  Expected: the model on
    the oracle's view of the sub-index."""
    x, centres, P, queries = make([2 * s for s in SIZES], copies=False, seed=7)
    n = x.shape[0]
    allowed = np.arange(n) % 2 == 0                          # (every list starts on an even id: exactly half of each is admitted)
    oidx = oracle.OracleIndex.build(x, centres, P)
    ov = oracle.OracleIndex.view(oidx.dim, *sub_arrays(oidx, allowed))
    try:
        assert np.diff(ov.offsets.astype(np.int64)).tolist() == SIZES
        ref = Ref(oracle, ov)
        g = rq.RaBitQ.build(x, centres, P)
        with g.make_filter(mask=allowed) as f:
            for probe in (1, 3):
                q2, radii = batch(ov, queries, probe)
                want = ref.answer(q2, probe, radii)
                counts = np.diff(want[0].astype(np.int64))
                if probe == 1:
                    assert counts[0::2].tolist() == SIZES
                assert classes(counts) == {0, 1, 2, 3}, counts
                cands = ref.candidates.copy()
                compare(rq, g, ref, q2, probe, radii, want, ("filtered", probe, "first"), fresh=(probe == 1), filt=f)
                ref.candidates = cands
                compare(rq, g, ref, q2, probe, radii, want, ("filtered", probe, "second"), fresh=False, filt=f)
        g.close()
    finally:
        ov.close()
        oidx.close()
