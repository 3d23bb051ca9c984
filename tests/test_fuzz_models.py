"""The models the GPU tests take their expected answers from (tests/models.py), checked on the CPU: the range answer assembled
from the oracle's stage functions against plain float64, its consistency with the oracle's own top-k, the sub-index a filter
stands for, the batched exact-distance entry of the oracle against the single-pair one -- and the CPU half of the feature fuzz:
the seeded slice of tests/test_fuzz_features_gpu.py replayed with the engine left out must meet the slice's coverage conditions
from the oracle's answers alone."""
import numpy as np
import pytest

from tests import fuzz_parity as fz
from tests import models as mo
from tests.test_fuzz_features_gpu import SLICE_NMAX, SLICE_ROUNDS, SLICE_SEED

DIMS = [64, 100, 128, 192, 256, 384, 512, 768, 960]


def test_batched_distance_equals_the_single_pair_entry(oracle):
    """rqo_l2_squared_distance_rows == rqo_l2_squared_distance bit for bit on every supported dim (and on lengths with a scalar
    tail, which the padded rows of an index never have), positions repeated and out of order; the empty call is empty."""
    rng = np.random.default_rng(1)
    for dim in DIMS + [1024, 3, 8, 13]:
        base = np.ascontiguousarray(rng.standard_normal((40, dim)) * rng.choice([1e-3, 1.0, 3e4]), dtype=np.float32)
        base[3] = base[7]
        q = base[7].copy() if dim % 2 else rng.standard_normal(dim).astype(np.float32)
        pos = rng.integers(0, 40, 100)
        got = oracle.l2_squared_distance_rows(q, base, pos)
        want = np.array([oracle.l2_squared_distance(q, base[p]) for p in pos], dtype=np.float32)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), dim
        assert oracle.l2_squared_distance_rows(q, base, np.zeros(0, np.int64)).size == 0
    # a known answer: (1 - 0)^2 * 64 lanes
    assert oracle.l2_squared_distance_rows(np.ones(64, np.float32), np.zeros((2, 64), np.float32), [1, 0]).tolist() == [64.0, 64.0]


def _cases(per_kind=2, nmax=1500):
    """a few fuzz cases per data family -> (x, centres, P, queries, desc), deterministic."""
    rng = np.random.default_rng(77)
    seen, it = {}, 0
    while any(seen.get(kd, 0) < per_kind for kd in set(fz.KINDS)) and it < 400:
        x, centres, P, queries, desc = fz.make_case(rng, it, nmax)
        it += 1
        if seen.get(desc["kind"], 0) < per_kind and desc["n"] <= 2500:
            seen[desc["kind"]] = seen.get(desc["kind"], 0) + 1
            yield x, centres, P, queries[:24], desc
    assert all(seen.get(kd, 0) >= per_kind for kd in set(fz.KINDS)), seen


def _f64_dist(base64, q, dim):
    qp = np.zeros(dim)
    qp[:q.size] = q
    return ((base64 - qp) ** 2).sum(axis=1)


def test_range_answer_against_float64(oracle):
    """Every distance of Ref.answer against the float64 squared distance of the same row: relative error at most
    gamma = (d + 2) u / (1 - (d + 2) u), u = 2^-24 -- a term (a - b)^2 carries the rounding of the difference twice (the product
    itself is exact inside the fused multiply-add), and then at most d roundings of the sum of non-negative terms however the
    lanes are ordered and reduced (d / 8 additions in its lane, three in the reduction): (1 + u)^(d + 2) at the most, and
    (1 - u)^(d + 2) >= 1 - (d + 2) u = 1 / (1 + gamma) at the least.  Membership: every probed row with rough < r and float64
    distance < r (1 - gamma) is in the answer, none with float64 distance > r (1 + gamma) is; the order is (distance bits, id)."""
    u = 2.0 ** -24
    checked = 0
    for x, centres, P, queries, desc in _cases():
        oidx = oracle.OracleIndex.build(x, centres, P)
        try:
            ref = mo.Ref(oracle, oidx)
            dim, k = oidx.dim, desc["k"]
            gamma = (dim + 2) * u / (1 - (dim + 2) * u)
            base64 = oidx.base.astype(np.float64)
            pos_of = np.empty(oidx.n, dtype=np.int64)
            pos_of[oidx.map_ids] = np.arange(oidx.n)
            probe = max(1, k // 2)
            radii = np.empty(len(queries), dtype=np.float32)
            for b, q in enumerate(queries):
                od = oidx.query(q, probe, 10)[0]
                radii[b] = (od.max() if od.size else 1.0) * np.float32([1.0, 1.15, 1.6, 3.0][b % 4])
            lims, dist, ids, _ = ref.answer(queries, probe, radii)
            for b, q in enumerate(queries):
                lo, hi = int(lims[b]), int(lims[b + 1])
                d_b, i_b = dist[lo:hi], ids[lo:hi]
                assert np.array_equal(np.lexsort((i_b, d_b.view(np.int32))), np.arange(hi - lo)), (desc, b)
                exact = _f64_dist(base64, q, dim)
                e_hit = exact[pos_of[i_b]]
                assert (np.abs(d_b.astype(np.float64) - e_hit) <= gamma * e_hit).all(), (desc, b)
                pos, rough = ref.rows(q, probe)
                r = float(radii[b])
                inside = set(i_b.tolist())
                must = pos[(rough < radii[b]) & (exact[pos] < r * (1 - gamma))]
                never = pos[exact[pos] > r * (1 + gamma)]
                assert all(int(i) in inside for i in oidx.map_ids[must]), (desc, b)
                assert not any(int(i) in inside for i in oidx.map_ids[never]), (desc, b)
                checked += hi - lo
        finally:
            oidx.close()
    assert checked > 1000, checked


def test_range_answer_against_the_oracles_top_k(oracle):
    """Radius +inf returns every row of the probed lists; with the oracle's k-th top-k distance nudged up as the radius, every
    oracle top-k entry whose estimate is below the radius is in the range answer with the same distance bits."""
    matched = 0
    for x, centres, P, queries, desc in _cases(per_kind=1):
        oidx = oracle.OracleIndex.build(x, centres, P)
        try:
            ref = mo.Ref(oracle, oidx)
            probe = max(1, desc["k"] // 2)
            lims, dist, ids, cnt = ref.answer(queries, probe, np.full(len(queries), np.inf, np.float32))
            for b, q in enumerate(queries):
                pos, _ = ref.rows(q, probe)
                assert int(lims[b + 1] - lims[b]) == pos.size, (desc, b)
                assert np.array_equal(np.sort(ids[int(lims[b]):int(lims[b + 1])]), np.sort(oidx.map_ids[pos])), (desc, b)
            assert cnt["rough"] == cnt["precise"] == int(lims[-1])
            tops = [oidx.query(q, probe, 10) for q in queries]
            radii = np.array([np.nextafter(od.max(), np.float32(np.inf)) if od.size else 0 for od, _ in tops], dtype=np.float32)
            lims, dist, ids, _ = ref.answer(queries, probe, radii)
            pos_of = np.empty(oidx.n, dtype=np.int64)
            pos_of[oidx.map_ids] = np.arange(oidx.n)
            for b, (q, (od, oi)) in enumerate(zip(queries, tops)):
                pos, rough = ref.rows(q, probe)
                rough_of = dict(zip(pos.tolist(), rough.tolist()))
                got = {int(i): dd.tobytes() for dd, i in zip(dist[int(lims[b]):int(lims[b + 1])], ids[int(lims[b]):int(lims[b + 1])])}
                for dd, i in zip(od, oi):
                    if np.float32(rough_of[int(pos_of[i])]) < radii[b]:
                        assert got.get(int(i)) == dd.tobytes(), (desc, b, int(i))
                        matched += 1
        finally:
            oidx.close()
    assert matched > 500, matched


def test_sub_arrays(oracle):
    """The oracle on sub_arrays(all admitted) equals the oracle on the index; sub_arrays of a random mask keeps the stored order,
    its offsets sum per list, ids beyond the mask are not admitted, and an id translation is applied to map_ids alone."""
    rng = np.random.default_rng(5)
    for x, centres, P, queries, desc in _cases(per_kind=1):
        oidx = oracle.OracleIndex.build(x, centres, P)
        try:
            n, k = oidx.n, oidx.k
            ov = oracle.OracleIndex.view(oidx.dim, *mo.sub_arrays(oidx, np.ones(n, dtype=bool)))
            try:
                for q in queries[:8]:
                    for heur in (False, True):
                        try:
                            a = oidx.query(q, k, 10, heur)
                        except RuntimeError:
                            with pytest.raises(RuntimeError):
                                ov.query(q, k, 10, heur)
                            continue
                        b = ov.query(q, k, 10, heur)
                        assert np.array_equal(a[1], b[1]) and np.array_equal(mo.bits(a[0]), mo.bits(b[0])), desc
            finally:
                ov.close()
            allowed = rng.random(n - n // 10) < 0.4                 # the last ids lie beyond the mask
            base, _, _, off, mids, codes, factors = mo.sub_arrays(oidx, allowed)
            full_mids, full_off = oidx.map_ids, oidx.offsets.astype(np.int64)
            keep = np.array([i < allowed.size and allowed[i] for i in full_mids])
            assert np.array_equal(mids, full_mids[keep]) and off[-1] == keep.sum() == mids.size
            assert np.array_equal(mo.bits(base), mo.bits(oidx.base[keep])) and np.array_equal(codes, oidx.codes[keep])
            assert np.array_equal(mo.bits(factors), mo.bits(oidx.factors[keep]))
            for c in range(k):
                assert off[c + 1] - off[c] == keep[full_off[c]:full_off[c + 1]].sum(), (desc, c)
            ids = (np.arange(n, dtype=np.uint32) * 3 + 7)
            t = mo.sub_arrays(oidx, np.ones(3 * n + 8, dtype=bool), ids)
            assert np.array_equal(t[4], ids[full_mids]) and np.array_equal(t[3], oidx.offsets)
        finally:
            oidx.close()


def test_tied_entries():
    lims = np.array([0, 3, 3, 5], dtype=np.uint64)
    dist = np.array([1, 1, 2, 2, 2], dtype=np.float32)     # the 2 that opens the last segment is no tie with the one before it
    assert mo.tied_entries(lims, dist) == 2
    assert mo.tied_entries(np.array([0, 1], np.uint64), np.array([1], np.float32)) == 0


def test_knobs_and_cases_keep_their_streams():
    """make_case and the first fourteen knobs consume the round's generator draw for draw as they did before the feature knobs
    were added (a committed regression test restores a saved generator state into make_case); the new knobs come from a child
    generator of the round number and are restored by KNOB_DEFAULTS."""
    a, b = np.random.default_rng(3), np.random.default_rng(3)
    fz.make_case(a, 0, 800), fz.make_case(b, 0, 800)
    knobs = fz.draw_knobs(a, 0)
    for choices in ([-1, -1, 0, 1], [0, 0, 3, 40], [0, 1, 2], [0, 1, 2], [0, 1, 2, 2], [0, 1, 2, 3, 4], [0, 1, 1], [0, 0, 1],
                    [100, 2560, 2560, 65536], [0, 0, 2, 16], [0, 1, 2], [1, 1, 2], [0, 1, 2], [0, 1, 1, 2, 2]):
        b.choice(choices)
    assert a.bit_generator.state == b.bit_generator.state
    assert set(knobs) == set(fz.KNOB_DEFAULTS) and list(knobs)[-3:] == ["prep_placement", "pair_split", "assign_impl"]
    assert fz.draw_knobs(np.random.default_rng(9), 5)["pair_split"] == fz.draw_knobs(np.random.default_rng(10), 5)["pair_split"]
    rng = np.random.default_rng(0)
    rng.bit_generator.state = {"bit_generator": "PCG64", "state": {"state": 39638530704376725464236549544941942162,
                                                                     "inc": 90750984832771704908184579979025356679},
                               "has_uint32": 0, "uinteger": 2370564739}
    desc = fz.make_case(rng, 327, 40000)[4]
    assert (desc["n"], desc["d"], desc["k"], desc["nq"], desc["kind"]) == (33664, 128, 120, 700, "sparse"), desc


def test_feature_fuzz_slice_models(oracle):
    """The GPU slice's generator with the engine left out: the oracle's answers alone meet the slice's coverage conditions."""
    from tests import fuzz_features as ff
    cov = ff.run_rounds(None, oracle, SLICE_SEED, SLICE_ROUNDS, SLICE_NMAX)
    print("feature fuzz slice, models only:", cov.summary())
    cov.check(engine=False)
