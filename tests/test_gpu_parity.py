"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle and the
committed golden fixtures.  Bit-exact everywhere (integer work AND f32 work: the kernels reproduce
the reference's operation order), so no tolerances appear below except where stated.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import glob
import os

import numpy as np
import pytest

from tests import coarse_cases, synth
from tests.models import bits, compare_with_oracle as _compare_with_oracle

pytestmark = pytest.mark.gpu
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
IDS = [os.path.basename(p)[:-4] for p in GOLDEN]


# scan implementation x gate of the matrix-core scan: VALU (v_dot8), matrix cores with the bf16 rank-5 threshold MFMA, matrix cores
# with the additive bound (dim 64 / 128; elsewhere the option leaves the bf16 form in place)
SCAN_VARIANTS = [(1, 0), (2, 1), (2, 2)]


def assert_bits_equal(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(bits(a), bits(b)):
        bad = np.nonzero(a.reshape(-1).view(np.uint8 if a.dtype.itemsize == 1 else f"u{a.dtype.itemsize}") !=
                         b.reshape(-1).view(np.uint8 if b.dtype.itemsize == 1 else f"u{b.dtype.itemsize}"))[0]
        raise AssertionError(f"{what}: {bad.size} of {a.size} elements differ; first at {bad[:5]}: "
                             f"{a.reshape(-1)[bad[:5]]} vs {b.reshape(-1)[bad[:5]]}")


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


# ---- a5: rotation -------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(64, 70), (128, 333), (256, 65), (768, 130)])
def test_rotate_bit_exact_both_kernels(rq, oracle, dim, n):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    P = synth.random_orthogonal(dim, seed=dim + 1)
    want = oracle.project_rows(x, P)
    assert_bits_equal(rq.ops.rotate(x, P, use_mfma=False), want, "valu rotate")
    assert_bits_equal(rq.ops.rotate(x, P, use_mfma=True), want, "mfma rotate")


def test_rotate_asymmetric_matrix_catches_transposes(rq, oracle):
    dim = 128
    P = (np.arange(dim * dim, dtype=np.float32).reshape(dim, dim) % 17 - 8) / 4   # not symmetric
    x = np.eye(dim, dtype=np.float32)[:40] * 3
    want = oracle.project_rows(x, P)
    assert_bits_equal(rq.ops.rotate(x, P, use_mfma=True), want, "mfma rotate, x = rows of 3I")
    assert np.array_equal(want[5], 3 * P[5])


# ---- a6-a8: assign + sign-pack + factors --------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_quantize_pack_matches_oracle(rq, oracle, path):
    g = np.load(path)
    label, dist, codes, factors = rq.ops.quantize_pack(g["rotated"], g["centroids"])
    ids, off = g["map_ids"], g["offsets"]
    want_label = np.empty(ids.size, np.uint32)
    for c in range(off.size - 1):
        want_label[ids[off[c]:off[c + 1]]] = c
    assert np.array_equal(label, want_label)
    for i in (0, 1, ids.size - 1):
        lab, d = oracle.kmeans_nearest_cluster(g["centroids"], g["rotated"][i])
        assert lab == label[i] and np.float32(d).tobytes() == dist[i].tobytes()
    assert_bits_equal(codes[ids], g["codes"], "codes")
    assert_bits_equal(factors[ids], g["factors"], "factors")


# ---- a3-a9: whole build -------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_build_matches_golden(rq, path):
    g = np.load(path)
    idx = rq.RaBitQ.build(g["base_in"], g["centroids_in"], g["orthogonal"])
    assert idx.dim == g["orthogonal"].shape[0] and idx.n == g["base_in"].shape[0]
    assert_bits_equal(idx.centroids, g["centroids"], "centroids")
    assert np.array_equal(idx.offsets, g["offsets"])
    assert np.array_equal(idx.map_ids, g["map_ids"])
    assert_bits_equal(idx.codes, g["codes"], "codes")
    assert_bits_equal(idx.factors, g["factors"], "factors")
    pad = np.pad(g["base_in"], ((0, 0), (0, idx.dim - g["base_in"].shape[1])))
    assert_bits_equal(idx.base, pad[g["map_ids"]], "base")
    assert_bits_equal(idx.orthogonal, g["orthogonal"], "orthogonal")
    assert idx.max_list_len == int(np.diff(g["offsets"].astype(np.int64)).max())
    idx.close()


# ---- a10-a16: query stages ----------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_query_stages_match_golden(rq, path):
    g = np.load(path)
    pad = np.pad(g["base_in"], ((0, 0), (0, g["orthogonal"].shape[0] - g["base_in"].shape[1])))
    idx = rq.RaBitQ.from_arrays(pad[g["map_ids"]], g["orthogonal"], g["centroids"], g["offsets"], g["map_ids"],
                                g["codes"], g["factors"])
    k = idx.k
    y, cl, cd = rq.ops.coarse_rank(idx, g["queries"], k)
    assert_bits_equal(y, g["y"], "rotated queries")
    assert np.array_equal(cl, g["coarse_cluster"])
    assert_bits_equal(cd, g["coarse_dist"], "coarse distances")
    y2, cl2, cd2 = rq.ops.coarse_rank(idx, g["queries"], 2)          # partial selection
    assert np.array_equal(cl2, g["coarse_cluster"][:, :2]) and np.array_equal(bits(cd2), bits(g["coarse_dist"][:, :2]))
    lo, delta, s, planes = rq.ops.query_prep(idx, g["y"], g["coarse_cluster"][:, 0])
    assert_bits_equal(lo, g["prep_lower"], "lower")
    assert_bits_equal(delta, g["prep_delta"], "delta")
    assert np.array_equal(s, g["prep_sum"])
    assert_bits_equal(planes, g["prep_planes"], "bit planes")
    at = 0
    off = g["offsets"]
    for qi in range(g["queries"].shape[0]):
        c = int(g["coarse_cluster"][qi, 0])
        n = int(g["rough_nearest_len"][qi])
        rough = rq.ops.scan(idx, c, g["coarse_dist"][qi, 0], g["prep_planes"][qi], g["prep_lower"][qi],
                            np.float32(g["prep_sum"][qi]), g["prep_delta"][qi], n)
        assert_bits_equal(rough, g["rough_nearest"][at:at + n], f"rough distances q{qi}")
        at += n
        assert n == off[c + 1] - off[c]
    idx.close()


def test_rerank_distances_exact(rq, oracle):
    g = np.load(GOLDEN[0])
    pad = np.pad(g["base_in"], ((0, 0), (0, g["orthogonal"].shape[0] - g["base_in"].shape[1])))
    base = pad[g["map_ids"]]
    idx = rq.RaBitQ.from_arrays(base, g["orthogonal"], g["centroids"], g["offsets"], g["map_ids"], g["codes"],
                                g["factors"])
    q = np.zeros(idx.dim, np.float32)
    q[:g["queries"].shape[1]] = g["queries"][1]
    pos = np.array([0, 5, 17, idx.n - 1, 3, 3, 100, 101, 102], dtype=np.uint32)
    got = rq.ops.rerank(idx, q, pos)
    want = np.array([oracle.l2_squared_distance(base[p], q) for p in pos], np.float32)
    assert_bits_equal(got, want, "accurate distances")
    idx.close()


# ---- whole query: ids, order, distances and the METRICS counters ---------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_query_matches_golden(rq, path):
    g = np.load(path)
    idx = rq.RaBitQ.build(g["base_in"], g["centroids_in"], g["orthogonal"])
    ci = 0
    while f"q{ci}_cfg" in g:
        probe, topk, heur = (int(v) for v in g[f"q{ci}_cfg"])
        want_n = g[f"q{ci}_n"]
        # one at a time, like the crate's CLI loop (crates/cli/src/main.rs:69-75)
        for qi, q in enumerate(g["queries"]):
            rq.metrics_reset()
            res = idx.query(q, probe, topk, bool(heur))
            n = int(want_n[qi])
            assert len(res) == n
            assert [i for _, i in res] == g[f"q{ci}_ids"][qi, :n].tolist(), (ci, qi)
            assert_bits_equal(np.array([d for d, _ in res], np.float32), g[f"q{ci}_dist"][qi, :n], "distances")
            m = rq.metrics()
            assert (m["rough"], m["precise"], m["query"]) == (int(g[f"q{ci}_counts"][qi, 0]),
                                                              int(g[f"q{ci}_counts"][qi, 1]), 1)
        # and as one batch
        rq.metrics_reset()
        d, ids, cnt = idx.query_batch(g["queries"], probe, topk, bool(heur))
        assert np.array_equal(cnt, want_n)
        for qi in range(len(cnt)):
            n = int(cnt[qi])
            assert np.array_equal(ids[qi, :n], g[f"q{ci}_ids"][qi, :n])
            assert_bits_equal(d[qi, :n], g[f"q{ci}_dist"][qi, :n], "batch distances")
        m = rq.metrics()
        assert m["rough"] == int(g[f"q{ci}_counts"][:, 0].sum()) and m["precise"] == int(g[f"q{ci}_counts"][:, 1].sum())
        assert m["query"] == len(cnt)
        ci += 1
    idx.close()


# ---- every value rq_set_option accepts in the SHIPPED library is result-neutral -------------------------------------
# (the timing ablations -- results wrong -- exist in the developer build only; what the product accepts must
# leave the golden results untouched, and may be changed while queries are in flight)
OPTION_VALUES = {
    "scan_impl": [0, 1, 2], "scan_gate": [0, 1, 2], "coarse_impl": [0, 1, 2, 3, 4], "coarse_tiled_from": [0, 4096, 1000000], "group_rank": [0, 1, 2], "scan_tile_table": [0, 1, 2],
    "dense_dir": [0, 1], "small_batch": [0, 1], "small_batch_span": [64, 2560, 100000], "stage_growth": [0, 2, 16],
    "survivor_segments": [0, 1, 2], "max_scan_blocks": [0, 1, 7], "shared_thresholds": [0, 1, 2], "assign_impl": [0, 1],
    "rerank_shadow": [0, 1, 2], "pair_split": [0, 1], "scan_debug": [0, 128, 512, 2048, 4096, 16384, 128 | 512 | 4096],
    "split_rows": [0, 1, 2], "pass_overlap": [0, 1], "large_batch_from": [2, 256, 100000], "cluster_major_div": [2, 32, 1024], "stage_settle_pct": [25, 100, 400],
}
OPTION_DEFAULTS = {"scan_impl": 0, "scan_gate": 0, "coarse_impl": 0, "coarse_tiled_from": 4096, "group_rank": 1, "scan_tile_table": 1, "dense_dir": 1,
                   "small_batch": 0, "small_batch_span": 2560, "stage_growth": 0, "survivor_segments": 1, "max_scan_blocks": 0,
                   "shared_thresholds": 1, "assign_impl": 0, "rerank_shadow": 2, "pair_split": 1, "scan_debug": 0,
                   "split_rows": 1, "pass_overlap": 1, "large_batch_from": 256, "cluster_major_div": 32, "stage_settle_pct": 100}


def test_every_option_value_keeps_golden_results(rq):
    from rabitq_amd import index as ix
    g = np.load(GOLDEN[0])
    probe, topk, heur = (int(v) for v in g["q0_cfg"])
    want_n = g["q0_n"]

    def check(idx, what):
        d, ids, cnt = idx.query_batch(g["queries"], probe, topk, bool(heur))
        assert np.array_equal(cnt, want_n), what
        for qi in range(len(cnt)):
            n = int(cnt[qi])
            assert np.array_equal(ids[qi, :n], g["q0_ids"][qi, :n]), (what, qi)
            assert_bits_equal(d[qi, :n], g["q0_dist"][qi, :n], f"{what}: distances")
        res = idx.query(g["queries"][0], probe, topk, bool(heur))
        assert [i for _, i in res] == g["q0_ids"][0, :int(want_n[0])].tolist(), what
    try:
        for name, values in OPTION_VALUES.items():
            for v in values:
                ix.set_option(name, v)
                idx = rq.RaBitQ.build(g["base_in"], g["centroids_in"], g["orthogonal"])   # (some options act at build time)
                check(idx, f"{name}={v}")
                idx.close()
            ix.set_option(name, OPTION_DEFAULTS[name])
        # the result-changing developer bits are refused by the shipped library
        for bad in (1, 2, 4, 64, 256, 1024, 8192, 128 | 64):
            with pytest.raises(rq.RabitqError):
                ix.set_option("scan_debug", bad)
        for name, bad in (("scan_gate", 3), ("scan_impl", 3), ("coarse_impl", 5), ("scan_dense", 1), ("split_rows", 3), ("stage_settle_pct", 0)):
            with pytest.raises(rq.RabitqError):
                ix.set_option(name, bad)
    finally:
        for name, v in OPTION_DEFAULTS.items():
            ix.set_option(name, v)


def test_options_flipped_under_concurrent_queries(rq, oracle):
    """Options are process-global; a pass reads the ones its plan depends on once, in plan_pass (the batch form, the stage
    boundaries and the records' layout among them), so flipping them while other threads query the same handle changes which
    kernels later passes run, never a result."""
    import threading
    from rabitq_amd import index as ix
    n, d, k = 16000, 128, 20
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=131, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=132)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(330, d, k, sigma=0.8, seed=133, centre_scale=0.6)
    want = [oidx.query(q, 8, 10)[1].tolist() for q in queries]
    stop = threading.Event()
    errs = []

    def flipper():
        rng = np.random.default_rng(5)
        # (the planner's knobs too: a pass reads each of them once, in plan_pass, and everything that executes it asks the plan)
        names = ["scan_impl", "scan_gate", "group_rank", "scan_tile_table", "dense_dir", "small_batch", "stage_growth", "coarse_impl",
                 "large_batch_from", "cluster_major_div", "stage_settle_pct"]
        while not stop.is_set():
            name = names[int(rng.integers(len(names)))]
            ix.set_option(name, int(rng.choice(OPTION_VALUES[name])))

    def worker(t):
        try:
            for rep in range(3):
                if t % 2:   # big batches (list-major / matrix-core stages) ...
                    _, ids, cnt = gidx.query_batch(queries, 8, 10)
                    got = [ids[i, :cnt[i]].tolist() for i in range(len(queries))]
                    assert got == want
                else:       # ... next to small ones (the small-batch path)
                    for j in range(t, 60, 4):
                        _, ids, cnt = gidx.query_batch(queries[j:j + 3], 8, 10)
                        assert [ids[i, :cnt[i]].tolist() for i in range(len(ids))] == want[j:j + 3]
        except BaseException as ex:  # noqa: BLE001
            errs.append(ex)
    fl = threading.Thread(target=flipper)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    fl.start()
    [t.start() for t in th]
    [t.join() for t in th]
    stop.set()
    fl.join()
    for name, v in OPTION_DEFAULTS.items():
        ix.set_option(name, v)
    assert not errs, errs
    gidx.close()
    oidx.close()


def test_additive_gate_falls_back_when_it_flags_too_much(rq, oracle):
    """The additive gate of the matrix-core scan (dim 64 / 128) is looser than the rank-5 threshold it replaces; an index whose
    batches send more than 3 % of the sub-tile steps down the exact path goes back to the bf16 threshold MFMA for good.  Queries
    of two very different scales make the per-list range of v' (and with it the candidates' side of the bound) useless: the
    first batch runs additive and flags nearly everything, later batches run the bf16 form -- with identical results throughout."""
    from rabitq_amd import index as ix
    n, d, k = 20000, 128, 8
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=211, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=212)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(400, d, k, sigma=0.8, seed=213, centre_scale=0.6)
    queries[::2] *= np.float32(40.0)          # every other query far outside the data: huge ycd, delta, v'
    ix.set_option("scan_impl", 2)              # matrix cores wherever the kernel exists (the batch is small)
    try:
        seen = []
        for rep in range(3):
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 10, False)
            pr = ix.last_profile()
            seen.append((pr["matrix_launches"], pr["matrix_additive_launches"], pr["matrix_subtile_steps"], pr["matrix_exact_steps"]))
        assert seen[0][1] > 0 and seen[0][3] * 32 > seen[0][2], seen        # first batch: additive, and it flagged > 3 %
        assert seen[1][0] > 0 and seen[1][1] == 0 and seen[2][1] == 0, seen  # afterwards: the bf16 threshold
        ix.set_option("scan_gate", 2)          # pinned additive: still the same answers
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 10, False)
        assert ix.last_profile()["matrix_additive_launches"] > 0
    finally:
        ix.set_option("scan_gate", 0)
        ix.set_option("scan_impl", 0)
    gidx.close()
    oidx.close()


@pytest.mark.parametrize("d,k,nq,probe,kind", coarse_cases.PREFILTER_CASES)
def test_prefiltered_coarse_ranking_equals_exact_order_kernels(rq, d, k, nq, probe, kind):
    """Coarse ranking through the bf16 matrix-core pre-filter + exact-order refinement (coarse_impl = 3; automatic for big batches)
    against the plain exact-order kernel + selection (rq_coarse_rank): list ids and distance bits of every probe list.
    ties: duplicate centroids (exact ties at the selection threshold); equidistant: centroids on a sphere around the queries (more
    candidates than the refinement holds: the in-kernel exact fall-back); scaled: coordinates x 3e3; nan: a NaN query.  The inputs
    come from tests/coarse_cases.py; test_coarse_cases.py shows that its last case drives the tiled selection through its second collect."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    centres, queries, x = coarse_cases.prefilter_case(d, k, nq, kind)
    idx = rq.RaBitQ.build(x.astype(np.float32), centres, synth.random_orthogonal(d, seed=9))
    _, want_cl, want_cd = rq.ops.coarse_rank(idx, queries, probe)          # the plain exact-order kernel + selection
    q = torch.from_numpy(queries).to(dev)
    try:
        for impl in (3, 4, 0):
            ix.set_option("coarse_impl", impl)
            pc = torch.zeros((nq, probe), device=dev, dtype=torch.int32)
            pdd = torch.zeros((nq, probe), device=dev, dtype=torch.float32)
            idx.coarse_topk_device(q.data_ptr(), nq, d, 0, k, probe, pc.data_ptr(), pdd.data_ptr())
            got_cl, got_cd = pc.cpu().numpy().view(np.uint32), pdd.cpu().numpy()
            # (the NaN row included: its margin is not finite, so the pre-filter hands the row to the exact-order kernels + the
            # block-per-query selection -- the very kernels `want` came from; the REFERENCE's behaviour on NaN input is not matched,
            # INTEGRATION.md, only the engine's own paths agree with each other)
            assert np.array_equal(got_cl, want_cl), (impl, np.argwhere(got_cl != want_cl)[:5])
            assert np.array_equal(got_cd.view(np.uint32), want_cd.view(np.uint32)), impl
    finally:
        ix.set_option("coarse_impl", 0)
    idx.close()


@pytest.mark.parametrize("n,d,k", [(3000, 64, 9), (200_000, 128, 64), (60_000, 128, 700), (9000, 256, 20), (40_000, 512, 16),
                                   (30_000, 768, 12), (6000, 1024, 5), (5000, 100, 8)])
def test_small_batch_path_matches_oracle(rq, oracle, n, d, k):
    """The few-launch path of batches of <= 64 queries (kernels_small.h: rotate + coarse in one launch, then one block per
    query for probe selection, query quantisation and the early stages in LDS, then the whole-chip scan of the rest and a
    finish that writes the results): every supported dim, one query per call (crates/cli/src/main.rs:69-80) up to 64,
    both rankers, heap sizes around a wave, probe counts from 1 to beyond k; indexes small enough to end inside the block
    and large enough for the separate final stage (pair-major records written by the block for one or two queries,
    cluster-major beyond).  Checked against the oracle AND against the staged path (option small_batch = 1), bit for bit,
    counters included."""
    from rabitq_amd import index as ix
    x, centres, _ = synth.mixture(n, d, k, sigma=0.9, seed=n + d, centre_scale=0.6)
    if k > 4:
        centres[3] = centres[1]                      # duplicate centroid: a tie in the probe selection
        centres[k - 1] += 50.0                       # an empty list
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=d + 7)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(64, d, k, sigma=0.9, seed=n + d + 1, centre_scale=0.6)
    queries[1] = x[11]
    cfgs = [(1, min(k, 64), 10, False), (2, min(k, 32), 10, False), (64, min(k, 64), 10, False), (33, 5, 63, False),
            (7, k + 3 if k < 60 else 64, 64, False), (16, min(k, 8), 256, False), (5, 1, 1, False), (20, min(k, 16), 10, True),
            (1, min(k, 6), 100, True)]
    try:
        for nq, probe, topk, heur in cfgs:
            q = queries[:nq]
            ix.set_option("small_batch", 0)
            try:
                _compare_with_oracle(rq, oracle, oidx, gidx, q, probe, topk, heur)
            except RuntimeError as e:       # the oracle reports a reference panic (heuristic ranker without a candidate)
                if "reference panics" not in str(e):
                    raise
                continue
            assert ix.last_profile()["small_batch_passes"] == 1, (nq, probe, topk, heur)
            a = gidx.query_batch(q, probe, topk, heur)
            ma = rq.metrics()
            ix.set_option("small_batch", 1)
            rq.metrics_reset()
            bres = gidx.query_batch(q, probe, topk, heur)
            assert ix.last_profile()["small_batch_passes"] == 0
            for u, v in zip(a, bres):
                assert_bits_equal(u, v, f"small-batch path vs staged path {(nq, probe, topk, heur)}")
            mb = rq.metrics()
            assert (ma["rough"], ma["precise"]) == (2 * mb["rough"], 2 * mb["precise"])   # ma: two calls since the reset
    finally:
        ix.set_option("small_batch", 0)
    gidx.close()
    oidx.close()


def test_probe_selection_splits_tied_pairs(rq, oracle):
    """Exact ties AT the selection threshold, in both wave selections (kernels_coarse.h): every centroid appears twice, at
    neighbouring list ids, so an odd probe count always cuts a pair and the smaller id must win (the oracle's order: ascending
    list id among equal distances).  40 queries take the small-batch path, where each of the 16 slices of 76 lists selects its own
    33 smallest (a cut pair in every slice) before the merge; 100 queries take select_probe_wave_kernel<64> over the whole row.
    probe = 1 cuts the nearest pair.  The twin with the larger id owns no vectors (assignment takes the first minimum), so a pair
    cut the wrong way changes the candidates scanned, which the comparison counts (rough / precise), and at probe = 1 the answer."""
    from rabitq_amd import index as ix
    d, k, n = 64, 1200, 6000
    rng = np.random.default_rng(d + k)
    centres = rng.standard_normal((k, d)).astype(np.float32)
    centres[1::2] = centres[0::2]
    x = (centres[rng.integers(0, k, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    queries = (centres[rng.integers(0, k, 100)] + 0.5 * rng.standard_normal((100, d))).astype(np.float32)
    P = synth.random_orthogonal(d, seed=d + 7)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert np.array_equal(gidx.offsets, oidx.offsets) and np.all(np.diff(oidx.offsets.astype(np.int64))[1::2] == 0)
    for nq, small in ((40, 1), (100, 0)):
        for probe in (33, 1):
            _compare_with_oracle(rq, oracle, oidx, gidx, queries[:nq], probe, 10, False)
            assert ix.last_profile()["small_batch_passes"] == small, (nq, probe)
    gidx.close()
    oidx.close()


@pytest.mark.parametrize("n,d,k,sigma,nq,cfgs", [
    (20000, 128, 32, 0.8, 96, [(8, 10, False), (32, 1, False), (64, 100, False), (5, 10, True)]),
    (6000, 64, 300, 1.0, 300, [(20, 10, False), (300, 5, False)]),       # cluster-major path, tiny lists
    (3000, 256, 8, 0.7, 40, [(8, 10, False), (3, 30, True)]),
    (2500, 960, 6, 0.7, 20, [(6, 10, False)]),                           # W = 15: generic scan kernel
])
def test_random_indexes_match_oracle(rq, oracle, n, d, k, sigma, nq, cfgs):
    x, centres, _ = synth.mixture(n, d, k, sigma=sigma, seed=n + d, centre_scale=0.6)
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=d)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert np.array_equal(gidx.map_ids, oidx.map_ids) and np.array_equal(gidx.offsets, oidx.offsets)
    assert_bits_equal(gidx.codes, oidx.codes, "codes")
    assert_bits_equal(gidx.factors, oidx.factors, "factors")
    queries, _, _ = synth.mixture(nq, d, k, sigma=sigma, seed=n + d + 1, centre_scale=0.6)
    queries[1] = x[17]
    for probe, topk, heur in cfgs:
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, heur)
    gidx.close()
    oidx.close()


def test_survivor_overflow_retry_is_exact(rq, oracle):
    # one huge list and a large topk: the second stage's survivors exceed the default per-query
    # buffer, which must trigger the exact-capacity re-run and still match the reference id for id
    n, d = 24000, 64
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    centres = np.zeros((1, d), np.float32)
    P = synth.random_orthogonal(d, seed=3)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries = rng.standard_normal((6, d)).astype(np.float32) * 0.2
    from rabitq_amd import index as ix
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 1, 2000, False)
    assert ix.last_profile()["retries"] > 0, "the test no longer exercises the overflow path"
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 1, 2000, False)
    assert ix.last_profile()["retries"] == 0, "the learnt capacity hint should prevent a second overflow"
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 1, 1000, True)   # window-12 threshold: no overflow
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 1, 400, False)
    gidx.close()


def test_edge_cases(rq, oracle):
    d, k = 64, 6
    x, centres, _ = synth.mixture(40, d, 3, sigma=0.5, seed=9)
    centres = np.concatenate([centres, centres[:1] + 100.0, centres[:1] - 100.0, centres[1:2] + 50.0])  # empty lists
    P = np.eye(d, dtype=np.float32)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert np.array_equal(gidx.offsets, oidx.offsets) and (np.diff(oidx.offsets.astype(np.int64)) == 0).any()
    qs = np.stack([x[0], centres[0], np.zeros(d, np.float32), x[5] * 1.5])  # query == centroid: delta = 0 edge
    for probe, topk in ((k, 10), (2, 64), (1, 3), (100, 1)):                # topk > n in list, probe > k
        _compare_with_oracle(rq, oracle, oidx, gidx, qs, probe, topk, False)
    # fewer candidates than topk
    d_, ids_, cnt_ = gidx.query_batch(qs, k, 64)
    assert cnt_.tolist() == [40, 40, 40, 40]
    # error behaviour mirrors the reference's panics
    with pytest.raises(rq.RabitqError) as e:
        gidx.query(np.zeros(65, np.float32), 2, 5)       # rabitq.rs:275
    assert e.value.status == -2
    with pytest.raises(rq.RabitqError):
        gidx.query(x[0], 0, 5)                           # rabitq.rs:295
    with pytest.raises(rq.RabitqError):
        rq.RaBitQ.build(x, centres[:, :32], P)           # rabitq.rs:165
    # short query is zero padded (rabitq.rs:277-280): d = 40 pads to 64
    x2 = x[:, :40].copy()
    o2 = oracle.OracleIndex.build(x2, centres[:, :40], P)
    g2 = rq.RaBitQ.build(x2, centres[:, :40], P)
    _compare_with_oracle(rq, oracle, o2, g2, x2[:5], 3, 5, False)
    gidx.close()
    g2.close()


# ---- persistence: byte-compatible with the crate's directory -------------------------------------
def test_dump_is_byte_identical_and_loads(rq, oracle, tmp_path):
    g = np.load(GOLDEN[1])   # d = 100 -> padded to 128
    oidx = oracle.OracleIndex.build(g["base_in"], g["centroids_in"], g["orthogonal"])
    gidx = rq.RaBitQ.build(g["base_in"], g["centroids_in"], g["orthogonal"])
    oidx.dump_to_dir(str(tmp_path / "o"))
    gidx.dump_to_dir(str(tmp_path / "g"))
    for name in ("base.fvecs", "orthogonal.fvecs", "centroids.fvecs", "offsets_ids.ivecs", "factors.fvecs",
                 "x_binary_vec.u64vecs"):
        assert (tmp_path / "o" / name).read_bytes() == (tmp_path / "g" / name).read_bytes(), name
    back = rq.RaBitQ.load_from_dir(str(tmp_path / "o"))
    for name in ("base", "orthogonal", "centroids", "offsets", "map_ids", "codes", "factors"):
        assert np.array_equal(bits(getattr(back, name)), bits(getattr(gidx, name))), name
    q = g["queries"][2]
    assert back.query(q, 3, 7) == gidx.query(q, 3, 7)
    with pytest.raises(rq.RabitqError) as e:
        rq.RaBitQ.load_from_dir(str(tmp_path / "missing"))
    assert e.value.status == -3
    # from_path on fvecs files
    from rabitq_amd import vecs
    vecs.write_vecs(tmp_path / "b.fvecs", g["base_in"])
    vecs.write_vecs(tmp_path / "c.fvecs", g["centroids_in"])
    fp = rq.RaBitQ.from_path(tmp_path / "b.fvecs", tmp_path / "c.fvecs", orthogonal=g["orthogonal"])
    assert np.array_equal(fp.map_ids, gidx.map_ids) and np.array_equal(bits(fp.factors), bits(gidx.factors))
    # generated rotation (orthogonal = None) is orthogonal and seeded
    gen = rq.RaBitQ.build(g["base_in"], g["centroids_in"], None, seed=7)
    Pg = gen.orthogonal.astype(np.float64)
    assert np.abs(Pg @ Pg.T - np.eye(gen.dim)).max() < 1e-5
    gen2 = rq.RaBitQ.build(g["base_in"], g["centroids_in"], None, seed=7)
    assert np.array_equal(gen.orthogonal, gen2.orthogonal)
    for i in (oidx, gidx, back, fp, gen, gen2):
        i.close()


# ---- f1: the CLI harness (crates/cli/src/main.rs) -------------------------------------------------
def test_cli_harness_build_then_load(rq, oracle, tmp_path, capsys):
    from rabitq_amd import cli, vecs
    n, d, k = 3000, 128, 12
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=77, centre_scale=0.6)
    queries, _, _ = synth.mixture(25, d, k, sigma=0.7, seed=78, centre_scale=0.6)
    gt = synth.brute_force_topk(x, queries, 10)
    vecs.write_vecs(tmp_path / "base.fvecs", x)
    vecs.write_vecs(tmp_path / "cent.fvecs", centres)
    vecs.write_vecs(tmp_path / "query.fvecs", queries)
    vecs.write_vecs(tmp_path / "truth.ivecs", gt)
    argv = ["-b", str(tmp_path / "base.fvecs"), "-c", str(tmp_path / "cent.fvecs"), "-q", str(tmp_path / "query.fvecs"),
            "-t", str(tmp_path / "truth.ivecs"), "-s", str(tmp_path / "saved"), "-p", "12", "-k", "10", "--batch", "8"]
    assert cli.main(argv) == 0                      # builds + dumps
    out1 = capsys.readouterr().out
    assert "training..." in out1 and os.path.isdir(tmp_path / "saved")
    assert cli.main(argv) == 0                      # second run loads the dumped index
    out2 = capsys.readouterr().out
    assert "loading from" in out2

    def parse(out):
        line = [l for l in out.splitlines() if l.startswith("QPS:")][0]
        met = [l for l in out.splitlines() if l.startswith("Metrics [")][0]
        return float(line.split("recall:")[1]), met
    r1, m1 = parse(out1)
    r2, m2 = parse(out2)
    assert r1 == r2 and m1 == m2 and r1 >= 0.95
    # the dumped directory is the crate's format: the oracle loads it and gives the same counters
    oidx = oracle.OracleIndex.load_from_dir(str(tmp_path / "saved"))
    oracle.metrics_reset()
    for q in queries:
        oidx.query(q, 12, 10)
    m = oracle.metrics()
    assert f"query: {m['query']}, rough: {m['rough']}, precise: {m['precise']}" in m1


# ---- properties at larger sizes (what the oracle cannot check in seconds) ---------------------------
# (100M x 128, 4096 lists, nprobe 64) is BASELINE.json configs[2] at its full size.
# (3M x 768 with a 4 GiB HBM budget) is configs[3]'s regime in small: raw vectors tiered per list between HBM and pinned
# host memory, built through the streamed builder path, wide-vector scan kernels.
@pytest.mark.parametrize("n,d,k,probe,hbm_mb", [(2_000_000, 128, 1024, 32, -1), (200_000, 768, 256, 32, -1),
                                                (100_000_000, 128, 4096, 64, -1), (3_000_000, 768, 1024, 32, 4096)])
def test_large_index_properties(rq, n, d, k, probe, hbm_mb):
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    centres = torch.randn(k, d, generator=g, device=dev)
    x = torch.empty((n, d), device=dev)
    counts = torch.zeros(k, dtype=torch.int64, device=dev)
    for ci, i0 in enumerate(range(0, n, 4_000_000)):       # chunked: no n x d temporaries beside the base itself
        m = min(4_000_000, n - i0)
        x[i0:i0 + m], u = synth.device_mixture_chunk(centres, i0, m, 0.5, ci, seed_base=500)
        counts += torch.bincount(u, minlength=k)
    del u
    nq = 256
    uq = torch.randint(0, k, (nq,), generator=g, device=dev)
    q = (centres[uq] + 0.5 * torch.randn(nq, d, generator=g, device=dev)).contiguous()
    P = synth.random_orthogonal(d, seed=1)
    ix.set_option("base_device_mb", hbm_mb)
    try:
        idx = rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=P)
    finally:
        ix.set_option("base_device_mb", -1)
    off, ids = idx.offsets.astype(np.int64), idx.map_ids
    if hbm_mb > 0:   # every list keeps floor(len * budget_rows / n) members in HBM, the rest is host-resident
        budget_rows = (hbm_mb << 20) // (4 * idx.dim)
        assert idx.n_hbm == int((np.diff(off) * budget_rows // n).sum()) and 0 < idx.n_hbm < n
    else:
        assert idx.n_hbm == n
    assert off[0] == 0 and off[-1] == n and np.all(np.diff(off) >= 0)
    assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))              # a permutation
    assert np.array_equal(np.diff(off), counts.cpu().numpy())  # well separated mixture
    fac, codes = idx.factors, idx.codes
    pop = np.zeros(2000, np.int64)
    for w in range(codes.shape[1]):
        pop += np.array([bin(int(v)).count("1") for v in codes[:2000, w]])
    np.testing.assert_array_equal(fac[:2000, 1], fac[:2000, 0] * (2 * pop - idx.dim).astype(np.float32))
    # rotation is orthogonal and codes are the signs of the rotated residual: check a sample
    cent = idx.centroids
    sample = np.arange(0, n, n // 500)[:500]
    pos_of = np.empty(n, np.int64)
    pos_of[ids] = np.arange(n)
    xs = rq.ops.rotate(x[torch.from_numpy(sample).to(dev)].cpu().numpy(), P)
    lab = np.searchsorted(off, pos_of[sample], side="right") - 1
    r = xs - cent[lab]
    bits_ = (r > 0)
    want = np.zeros((len(sample), d // 64), np.uint64)
    for j in range(d):
        want[:, j // 64] |= bits_[:, j].astype(np.uint64) << np.uint64(j % 64)
    assert np.array_equal(codes[pos_of[sample]], want)
    np.testing.assert_allclose(fac[pos_of[sample], 3], (r.astype(np.float64) ** 2).sum(1), rtol=1e-5)
    # queries: batch == one-at-a-time, recall against an exact f64 brute force
    dist, got, cnt = idx.query_batch(q.cpu().numpy(), probe, 10)
    for j in (0, 7, 100):
        single = idx.query(q[j].cpu().numpy(), probe, 10)
        assert [i for _, i in single] == got[j, :cnt[j]].tolist()
    qd = q.double()
    best = torch.full((nq, 10), float("inf"), device=dev, dtype=torch.float64)
    besti = torch.full((nq, 10), -1, device=dev, dtype=torch.int64)
    for i0 in range(0, n, 500_000):
        xb = x[i0:i0 + 500_000].double()
        d2 = (qd * qd).sum(1, keepdim=True) - 2 * qd @ xb.T + (xb * xb).sum(1)[None]
        cd, ci = torch.topk(d2, 10, dim=1, largest=False)
        alld, alli = torch.cat([best, cd], 1), torch.cat([besti, ci + i0], 1)
        sel = torch.topk(alld, 10, dim=1, largest=False).indices
        best, besti = torch.gather(alld, 1, sel), torch.gather(alli, 1, sel)
    gt = besti.cpu().numpy()
    recall = np.mean([len(set(got[j, :10].tolist()) & set(gt[j].tolist())) / 10 for j in range(nq)])
    assert recall >= 0.95, recall
    # returned distances are the exact squared L2 of the returned ids
    xr = x[torch.from_numpy(got[:8, :10].astype(np.int64)).to(dev)].double()
    exact = ((xr - qd[:8, None, :]) ** 2).sum(-1).cpu().numpy()
    np.testing.assert_allclose(dist[:8, :10], exact, rtol=1e-5)
    idx.close()


def test_config1_sift_like_1m_matches_oracle(rq, oracle):
    """BASELINE.json configs[1] at its own size: 1M x 128, 1024 lists, nprobe 32, top-10.  The SIFT files are not in this
    image, so the data is SIFT-LIKE (non-negative integer coordinates 0..255 around 1024 centres); the oracle builds the
    whole index itself (~10 s of one core), every array of the two builds is compared bit for bit, then 300 queries through
    both rankers and a batch of one: ids in order, distance bits, rough / precise counters."""
    n, d, k, probe = 1_000_000, 128, 1024, 32
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=1001, centre_scale=0.7)
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=1002, centre_scale=0.7)
    x, centres, queries = (np.rint(a * 40 + 128).clip(0, 255).astype(np.float32) for a in (x, centres, queries))
    queries[3] = x[12345]                                   # a query that IS a base vector (distance 0 to itself)
    P = synth.random_orthogonal(d, seed=1003)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert_bits_equal(gidx.centroids, oidx.centroids, "rotated centroids")
    assert np.array_equal(gidx.offsets, oidx.offsets)
    assert np.array_equal(gidx.map_ids, oidx.map_ids)
    assert_bits_equal(gidx.codes, oidx.codes, "codes")
    assert_bits_equal(gidx.factors, oidx.factors, "factors")
    assert_bits_equal(gidx.base, x[oidx.map_ids], "base in cluster order")
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, 10, False)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries[:64], probe, 10, True)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries[:1], probe, 10, False)     # the reference harness's one query per call
    _compare_with_oracle(rq, oracle, oidx, gidx, queries[:40], probe, 100, False)
    gidx.close()
    oidx.close()


@pytest.mark.parametrize("d", [64, 100, 192, 256, 384, 512, 768])
def test_prefiltered_assignment_equals_exact_order_kernels(rq, oracle, d):
    """Nearest-list assignment through the matrix cores (assign_approx_kernel: bf16 MFMA approximation, candidates within
    2 m of the minimum, exact-order refinement) against the exact-order VALU kernels (option assign_impl = 1) and the
    oracle: labels and distances bit for bit.  Data that stress the candidate logic: duplicate centroids (exact ties:
    the first one must win), a tight ring of near-equidistant centroids (more candidates than the list holds: the
    exact-order kernel takes those vectors), vectors ON centroids, huge and tiny scales in one index, a NaN and an inf
    coordinate (no candidate at all)."""
    from rabitq_amd import index as ix
    rng = np.random.default_rng(d)
    n, k = 6000, 70
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=d, centre_scale=0.7)
    centres[9] = centres[4]                                               # exact ties
    centres[20:50] = centres[20] + 1e-5 * rng.standard_normal((30, d))    # thirty lists within the error bound of each other (> the 16 candidate slots)
    x[:200] = centres[rng.integers(20, 50, 200)] + 1e-3 * rng.standard_normal((200, d))
    x[200:260] = centres[rng.integers(0, k, 60)]                          # on a centroid
    x[260:300] *= 1.0e4
    x[300:340] *= 1.0e-4
    x = x.astype(np.float32)
    x[400, 3] = np.nan
    x[401, 5] = np.inf
    dp = (d + 63) // 64 * 64
    P = synth.random_orthogonal(dp, seed=d + 1)
    xr = rq.ops.rotate(np.pad(x, ((0, 0), (0, dp - d))), P)
    cr = rq.ops.rotate(np.pad(centres, ((0, 0), (0, dp - d))), P)
    got = {}
    try:
        for impl in (0, 1):
            ix.set_option("assign_impl", impl)
            got[impl] = rq.ops.quantize_pack(xr, cr)
    finally:
        ix.set_option("assign_impl", 0)
    for a, b, name in zip(got[0], got[1], ("label", "dist", "codes", "factors")):
        assert_bits_equal(np.asarray(a), np.asarray(b), f"assign_impl 0 vs 1: {name}")
    ok = np.isfinite(x).all(axis=1)
    for i in np.nonzero(ok)[0][::7]:
        lab, dist = oracle.kmeans_nearest_cluster(cr, xr[i])
        assert int(got[0][0][i]) == lab, i
        assert np.float32(got[0][1][i]).view(np.uint32) == np.float32(dist).view(np.uint32), i


# ---- f2: centroid training on the GPU (scripts/cluster.py's role) -----------------------------------
def test_kmeans_centroids_give_recall(rq):
    import torch
    dev = torch.device("cuda", 0)
    n, d, k = 300_000, 96, 64      # d = 96 pads to 128
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    centres = torch.randn(k, d, generator=g, device=dev)
    u = torch.randint(0, k, (n,), generator=g, device=dev)
    x = (centres[u] + 0.5 * torch.randn(n, d, generator=g, device=dev)).contiguous()
    learnt = torch.zeros((k, d), device=dev)
    rq.ops.kmeans_device(x.data_ptr(), n, d, k, learnt.data_ptr(), iters=15, seed=3)
    assert torch.isfinite(learnt).all()

    def qerr(c):  # mean squared distance to the nearest centroid
        d2 = torch.cdist(x[:20000], c) ** 2
        return float(d2.min(1).values.mean())
    # Lloyd from a random start can merge/split a few of the well-separated generating clusters (faiss does
    # too); what matters is that the error is of the same order and that the index built on it recalls
    ratio = qerr(learnt) / qerr(centres)
    assert ratio < 3.0, ratio
    idx = rq.RaBitQ.build_device(x.data_ptr(), n, d, learnt.data_ptr(), k, orthogonal=synth.random_orthogonal(128, 2))
    q = x[:200] + 0.05
    _, ids, cnt = idx.query_batch(q.cpu().numpy(), 8, 10)
    d2 = torch.cdist(q.double(), x.double()) ** 2
    gt = torch.topk(d2, 10, dim=1, largest=False).indices.cpu().numpy()
    recall = np.mean([len(set(ids[j, :10].tolist()) & set(gt[j].tolist())) / 10 for j in range(200)])
    assert recall >= 0.95, recall
    idx.close()


# ---- ties, degenerate sizes, concurrency -------------------------------------------------------------
def test_duplicates_and_ties_match_oracle(rq, oracle):
    # exact duplicate vectors => equal rough AND equal accurate distances: which of the tied candidates
    # survives in the heap depends on Rust's BinaryHeap sift order and on strict `<` gates
    rng = np.random.default_rng(12)
    d, k = 64, 4
    uniq = rng.standard_normal((60, d)).astype(np.float32)
    x = np.concatenate([uniq, uniq[:40], uniq[:40], uniq[10:30]])            # many exact duplicates
    x = x[rng.permutation(len(x))]
    centres = np.concatenate([uniq[:2] * 0.5, uniq[:2] * 0.5])                # duplicate centroids: coarse ties
    P = synth.random_orthogonal(d, seed=8)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert np.array_equal(gidx.map_ids, oidx.map_ids) and np.array_equal(gidx.offsets, oidx.offsets)
    qs = np.concatenate([uniq[:6], uniq[:3] + 0.01]).astype(np.float32)
    for probe, topk in ((4, 5), (2, 10), (4, 64), (1, 1)):
        _compare_with_oracle(rq, oracle, oidx, gidx, qs, probe, topk, False)
    _compare_with_oracle(rq, oracle, oidx, gidx, qs, 4, 7, True)
    gidx.close()
    oidx.close()


def test_degenerate_sizes(rq, oracle):
    d = 64
    P = np.eye(d, dtype=np.float32)
    centres = np.zeros((3, d), np.float32)
    centres[1] += 1.0
    centres[2] -= 1.0
    # empty index: every list empty -> no results, no crash
    empty = rq.RaBitQ.build(np.zeros((0, d), np.float32), centres, P)
    assert empty.n == 0 and empty.max_list_len == 0 and empty.offsets.tolist() == [0, 0, 0, 0]
    dd, ii, cnt = empty.query_batch(np.ones((3, d), np.float32), 3, 5)
    assert cnt.tolist() == [0, 0, 0]
    empty.close()
    # one vector, one list, topk at the engine limit
    one = rq.RaBitQ.build(np.ones((1, d), np.float32), centres[:1], P)
    res = one.query(np.ones(d, np.float32), 1, 2048)
    assert res == [(0.0, 0)]
    with pytest.raises(rq.RabitqError) as e:
        one.query(np.ones(d, np.float32), 1, 2049)
    assert e.value.status == -6
    one.close()
    # zero queries is a no-op
    x, c2, _ = synth.mixture(200, d, 3, seed=4)
    g = rq.RaBitQ.build(x, c2, P)
    dd, ii, cnt = g.query_batch(np.zeros((0, d), np.float32), 2, 5)
    assert dd.shape[0] == 0
    g.close()


def test_concurrent_queries_one_handle(rq, oracle):
    # `RaBitQ::query(&self)` is called from many tokio workers in the service (crates/service/src/main.rs:36-44)
    import threading
    n, d, k = 8000, 128, 16
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=31, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=32)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(48, d, k, sigma=0.8, seed=33, centre_scale=0.6)
    want = [oidx.query(q, 6, 10)[1].tolist() for q in queries]
    got = [None] * len(queries)
    errs = []

    def worker(t):
        try:
            for j in range(t, len(queries), 6):
                if j % 2:
                    got[j] = [i for _, i in gidx.query(queries[j], 6, 10)]
                else:
                    _, ids, cnt = gidx.query_batch(queries[j:j + 1], 6, 10)
                    got[j] = ids[0, :cnt[0]].tolist()
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    assert got == want
    gidx.close()


# ---- the two scan implementations (VALU v_dot8 / fp6 matrix cores) must be indistinguishable ----------
@pytest.mark.parametrize("impl,gate", SCAN_VARIANTS)
@pytest.mark.parametrize("n,d,k,nq", [(12000, 128, 24, 160), (5000, 64, 10, 70), (4000, 256, 6, 50), (3000, 100, 8, 40),
                                      (6000, 128, 4, 420),    # 420 pairs per list: 14 query tiles through the 3-slot ring
                                      (3000, 192, 6, 70), (2500, 384, 5, 70), (2000, 512, 4, 66), (2500, 768, 4, 80),
                                      (1500, 1024, 3, 40)])   # the wide-vector instantiations (W = 3, 6, 8, 12, 16)
def test_scan_implementations_match_oracle(rq, oracle, impl, gate, n, d, k, nq):
    from rabitq_amd import index as ix
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=n + impl, centre_scale=0.6)
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=d + 3)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=n + 7, centre_scale=0.6)
    queries[2] = x[11]
    ix.set_option("scan_impl", impl)
    ix.set_option("scan_gate", gate)
    try:
        for probe, topk, heur in ((k, 10, False), (3, 1, False), (k, 50, False), (4, 10, True)):
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, heur)
        # ragged: a single query, and a batch that is not a multiple of the 32-query tile
        _compare_with_oracle(rq, oracle, oidx, gidx, queries[:1], k, 10, False)
        _compare_with_oracle(rq, oracle, oidx, gidx, queries[:33], k, 10, False)
    finally:
        ix.set_option("scan_impl", 0)
        ix.set_option("scan_gate", 0)
    gidx.close()
    oidx.close()


def test_eight_shards_on_one_gpu_merge_to_the_single_index(rq, oracle):
    """BASELINE.json configs[4] in small and in ONE process: an index cut into eight shards of whole lists
    (rq_partition_lists / rq_shard_index, the partitioning of the 8-GPU run), every shard queried with the same 2100-query
    batch -- its pass names the lists of all eight shards, 7 of 8 pairs are empty here -- and the eight top-k lists merged
    by (Ord32 distance, id).  Every shard answers exactly as the oracle does on that shard's arrays (bit for bit); the
    merged ids are the single index's except where a shard's own, looser threshold sequence re-ranks a candidate the
    single sequential stream skipped (the reference's own approximation: a lower-bound violation on a true neighbour)."""
    n, d, k, nq, probe, topk = 400_000, 128, 256, 2100, 32, 10
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=71, centre_scale=0.7)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.7, seed=72, centre_scale=0.7)
    full = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=73))
    fd, fi, fn = full.query_batch(queries, probe, topk, False)
    owner, load = full.partition_lists(8)
    assert int(load.sum()) == n and load.min() > 0
    md = np.full((nq, 8 * topk), np.inf, np.float32)
    mi = np.full((nq, 8 * topk), 0xFFFFFFFF, np.uint32)
    for r in range(8):
        shard = full.shard(owner, r)
        dist, ids, cnt = shard.query_batch(queries, probe, topk, False)
        if r in (0, 5):   # the shard is a RaBitQ index of its own: the oracle on its arrays agrees bit for bit
            ov = oracle.OracleIndex.view(shard.dim, base=shard.base, orthogonal=shard.orthogonal, centroids=shard.centroids,
                                         offsets=shard.offsets, map_ids=shard.map_ids, codes=shard.codes, factors=shard.factors)
            _compare_with_oracle(rq, oracle, ov, shard, queries[:120], probe, topk, False)
            ov.close()
        for qi in range(nq):
            c = int(cnt[qi])
            md[qi, r * topk:r * topk + c] = dist[qi, :c]
            mi[qi, r * topk:r * topk + c] = ids[qi, :c]
        shard.close()
    order = np.lexsort((mi, md), axis=1)[:, :topk]          # by distance, ties by id
    merged = np.take_along_axis(mi, order, axis=1)
    same = sum(len(set(merged[qi].tolist()) & set(fi[qi, :fn[qi]].tolist())) for qi in range(nq))
    total = int(fn.sum())
    assert total == nq * topk and same >= total - total // 200, (same, total)   # >= 99.5 % of the ids identical
    # and the merged lists are at least as good as the single index's where they differ (true distances, f64)
    worse = 0
    for qi in range(nq):
        a, b = merged[qi], fi[qi, :topk]
        if set(a.tolist()) != set(b.tolist()):
            da = np.sort(((x[a].astype(np.float64) - queries[qi]) ** 2).sum(1))
            db = np.sort(((x[b].astype(np.float64) - queries[qi]) ** 2).sum(1))
            worse += int(da[-1] > db[-1] * (1 + 1e-9))
    assert worse == 0, worse
    full.close()


def test_shard_pass_lists_its_nonempty_pairs(rq, oracle):
    """A shard of a multi-GPU deployment ranks over the lists of ALL shards, so most of a pass's (query, list) pairs name
    lists that are empty here.  Large passes settle those by one thread each and run the query quantisation over a
    compacted list of the others (pair_split_kernel, prep_small_listed_kernel); ranked stage placement skips them before
    their scalars are fetched.  A quarter shard (16 of 64 lists), 2100 queries x 32 probes = 67 200 pairs: both rankers,
    option pair_split 1 against 0 bit for bit, and against the oracle on the shard's own arrays."""
    from rabitq_amd import index as ix
    n, d, k = 60000, 128, 64
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=61, centre_scale=0.6)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=62))
    owner, load = gidx.partition_lists(4)
    from rabitq_amd import sharding
    for w in (2, 4, 8):   # the host restatement of the rule (what the two-rank gloo test partitions with) == rq_partition_lists
        o_c, l_c = gidx.partition_lists(w)
        o_n, l_n = sharding.partition_lists(gidx.offsets, w)
        assert np.array_equal(o_c, o_n) and np.array_equal(l_c, l_n), w
    shard = gidx.shard(owner, 1)
    assert int((np.diff(shard.offsets.astype(np.int64)) > 0).sum()) * 2 < k
    queries, _, _ = synth.mixture(2100, d, k, sigma=0.8, seed=63, centre_scale=0.6)
    ov = oracle.OracleIndex.view(shard.dim, base=shard.base, orthogonal=shard.orthogonal, centroids=shard.centroids, offsets=shard.offsets,
                                 map_ids=shard.map_ids, codes=shard.codes, factors=shard.factors)
    try:
        got = {}
        for split in (1, 0):
            ix.set_option("pair_split", split)
            got[split] = [shard.query_batch(queries, 32, 10, heur) for heur in (False, True)]
        for a, b in zip(got[1], got[0]):
            for u, v in zip(a, b):
                assert_bits_equal(u, v, "pair_split 1 vs 0")
        ix.set_option("pair_split", 1)
        _compare_with_oracle(rq, oracle, ov, shard, queries, 32, 10, False)
        _compare_with_oracle(rq, oracle, ov, shard, queries[:300], 40, 20, True)
    finally:
        ix.set_option("pair_split", 1)
    shard.close()
    gidx.close()
    ov.close()


# A stage whose grid exceeds the launch bound is issued as several launches over (group, tile) sub-ranges
# (launch_scan_chunks): lowered test-only bound, one artificially long list, both implementations, both work layouts.
@pytest.mark.parametrize("impl,gate", SCAN_VARIANTS)
@pytest.mark.parametrize("max_blocks,tile_table", [(1, 2), (5, 2), (5, 0), (0, 1)])
def test_scan_grid_chunking_matches_oracle(rq, oracle, impl, gate, max_blocks, tile_table):
    from rabitq_amd import index as ix
    n, d = 9000, 128
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, d)).astype(np.float32)
    centres = np.concatenate([np.zeros((1, d), np.float32), rng.standard_normal((5, d)).astype(np.float32) * 4])
    x[:300] += centres[1 + (np.arange(300) % 5)]           # one list of ~8700 (many tiles), five short ones
    P = synth.random_orthogonal(d, seed=78)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert gidx.max_list_len > 8000
    queries = (rng.standard_normal((70, d)) * 0.5).astype(np.float32)
    ix.set_option("scan_impl", impl)
    ix.set_option("scan_gate", gate)
    ix.set_option("max_scan_blocks", max_blocks)
    ix.set_option("scan_tile_table", tile_table)   # full-list stages: one block per existing (list, tile) (2), plain grid (0), auto (1)
    try:
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, 6, 10, False)      # cluster-major stages
        _compare_with_oracle(rq, oracle, oidx, gidx, queries[:3], 6, 10, False)  # pair-major stages
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, 2, 30, True)
    finally:
        ix.set_option("max_scan_blocks", 0)
        ix.set_option("scan_tile_table", 1)
        ix.set_option("scan_impl", 0)
        ix.set_option("scan_gate", 0)
    gidx.close()
    oidx.close()


@pytest.mark.parametrize("impl,gate", SCAN_VARIANTS)
def test_ranked_group_placement_matches_oracle(rq, oracle, impl, gate):
    """Cluster-major stages place their (query, list) pairs either with one atomic per pair or through per-block
    LDS histograms (group_rank_kernel, what big stages use).  Forced on a small batch (several shapes of stage, empty
    lists, padding rows of the matrix-core tiles), then reached the automatic way: 9000 queries x 64 probes is a stage
    of more than 16 blocks of pairs."""
    from rabitq_amd import index as ix
    n, d, k = 30_000, 128, 96
    x, centres, _ = synth.mixture(n, d, k - 6, sigma=0.8, seed=91, centre_scale=0.6)
    centres = np.concatenate([centres, 50.0 + np.arange(6 * d, dtype=np.float32).reshape(6, d)])   # six lists stay empty
    P = synth.random_orthogonal(d, seed=92)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(9000, d, k - 6, sigma=0.8, seed=93, centre_scale=0.6)
    ix.set_option("scan_impl", impl)
    ix.set_option("scan_gate", gate)
    try:
        ix.set_option("group_rank", 2)
        _compare_with_oracle(rq, oracle, oidx, gidx, queries[:300], 20, 10, False)
        _compare_with_oracle(rq, oracle, oidx, gidx, queries[:77], 96, 5, True)
        ix.set_option("group_rank", 1)
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, 64, 10, False)
        a = gidx.query_batch(queries, 64, 10, False)
        ix.set_option("group_rank", 0)
        b = gidx.query_batch(queries, 64, 10, False)
        for u, v in zip(a, b):
            assert_bits_equal(u, v, "ranked / per-pair placement")
    finally:
        ix.set_option("group_rank", 1)
        ix.set_option("scan_impl", 0)
        ix.set_option("scan_gate", 0)
    gidx.close()
    oidx.close()


def test_wide_vectors_dim_3072(rq, oracle):
    # dim in (2048, 4096]: assign_generic_kernel<8> needs > 64 KiB of dynamic LDS, so the attribute must be in
    # place before the FIRST build / quantize of a process (ensure_kernel_attributes); generic-W scan (W = 48)
    n, d, k = 600, 3072, 5
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=31, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=32)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert np.array_equal(gidx.map_ids, oidx.map_ids) and np.array_equal(gidx.offsets, oidx.offsets)
    assert_bits_equal(gidx.codes, oidx.codes, "codes")
    assert_bits_equal(gidx.factors, oidx.factors, "factors")
    queries, _, _ = synth.mixture(12, d, k, sigma=0.8, seed=33, centre_scale=0.6)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 10, False)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 2, 5, True)
    gidx.close()
    oidx.close()


@pytest.mark.parametrize("impl,gate", SCAN_VARIANTS)
def test_scan_degenerate_factors_both_implementations(rq, oracle, impl, gate):
    # vectors that coincide with their centroid (zero residual: norm not `is_normal` -> ip = 0.8, factor_ip = -0,
    # rabitq.rs:211-215) and queries that coincide with a centroid (delta = 0 -> 1/delta = inf): the integer
    # threshold form of the matrix-core scan is not applicable there and must fall back to the exact gate
    from rabitq_amd import index as ix
    d, k, n = 128, 6, 3000
    x, centres, _ = synth.mixture(n, d, k, sigma=0.6, seed=91, centre_scale=0.7)
    x[:40] = centres[np.arange(40) % k]                  # exact copies of centroids
    x[40:60] = x[60:80]                                  # duplicates
    P = np.eye(d, dtype=np.float32)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert np.array_equal(bits(gidx.factors), bits(oidx.factors))
    assert (oidx.factors[:, 0] == 0).sum() >= 40          # the -0.0 factor_ip rows are really there
    queries = np.concatenate([centres[:4], x[:4], x[100:140] + np.float32(0.01)]).astype(np.float32)
    ix.set_option("scan_impl", impl)
    ix.set_option("scan_gate", gate)
    try:
        for probe, topk, heur in ((k, 10, False), (2, 3, False), (k, 100, False), (k, 10, True)):
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, heur)
    finally:
        ix.set_option("scan_impl", 0)
        ix.set_option("scan_gate", 0)
    gidx.close()
    oidx.close()


# ---- sharded coarse ranking + externally supplied probe lists -----------------------------------------
def test_sharded_coarse_and_probed_query_equal_single(rq):
    import torch
    from rabitq_amd import sharding
    dev = torch.device("cuda", 0)
    n, d, k, nq, probe, topk = 6000, 128, 40, 50, 12, 10
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=61, centre_scale=0.6)
    centres[7] = centres[3]                                   # tied coarse distances across the two "shards"
    idx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=62))
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=63, centre_scale=0.6)
    _, want_cl, want_cd = rq.ops.coarse_rank(idx, queries, probe)
    q = torch.from_numpy(queries).to(dev)
    parts = []
    for lo, hi in ((0, 5), (5, 23), (23, 40)):                # first range holds fewer lists than `probe`: padding
        pc = torch.zeros((nq, probe), device=dev, dtype=torch.int32)
        pdd = torch.zeros((nq, probe), device=dev, dtype=torch.float32)
        idx.coarse_topk_device(q.data_ptr(), nq, d, lo, hi, probe, pc.data_ptr(), pdd.data_ptr())
        parts.append((pc, pdd))
    assert (parts[0][0][:, 5:] == -1).all() and torch.isinf(parts[0][1][:, 5:]).all()
    pc = torch.cat([p[0] for p in parts], 1)
    pdd = torch.cat([p[1] for p in parts], 1)
    mc, md = sharding.merge_probe_lists(pc, pdd, probe)      # world 1: the merge of the concatenated rows
    assert np.array_equal(mc.cpu().numpy().view(np.uint32), want_cl)
    assert np.array_equal(md.cpu().numpy().view(np.uint32), want_cd.view(np.uint32))
    od = torch.empty((nq, topk), device=dev)
    oi = torch.zeros((nq, topk), device=dev, dtype=torch.int32)
    on = torch.zeros(nq, device=dev, dtype=torch.int32)
    rq.metrics_reset()
    idx.query_batch_device_probed(q.data_ptr(), nq, d, mc.data_ptr(), md.data_ptr(), probe, topk, od.data_ptr(),
                                  oi.data_ptr(), on.data_ptr())
    m1 = rq.metrics()
    rq.metrics_reset()
    wd, wi, wn = idx.query_batch(queries, probe, topk)
    assert rq.metrics() == m1
    assert np.array_equal(on.cpu().numpy().view(np.uint32), wn)
    assert np.array_equal(oi.cpu().numpy().view(np.uint32), wi) and np.array_equal(od.cpu().numpy().view(np.uint32), wd.view(np.uint32))
    idx.close()


def test_one_sharded_pass_of_more_than_65536_queries(rq):
    """A shard's pass (caller-supplied probe lists) may hold 16 x the queries of a plain pass -- the multi-GPU step scales its batch
    with the number of ranks (524 288 queries at eight GPUs) -- so every launch sized by the query count (grid.y = nq of the exact-distance
    kernels, one block per query of the ordering / replay kernels, the ranked placement's per-block histograms) runs beyond 65 536.
    70 000 queries against one shard of four (most pairs name lists of other shards: the pair-split path) in ONE pass, both halves of the step (probed, then seeded with tight thresholds), compared
    bit for bit with the same queries in two calls of 35 000 (passes that stay below 65 536)."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    n, d, k, nq, probe, topk = 40_000, 64, 32, 70_000, 6, 5
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=91, centre_scale=0.6)
    full = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=92))
    owner, _ = full.partition_lists(4)
    shard = full.shard(owner, 0)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=93, centre_scale=0.6)
    q = torch.from_numpy(queries).to(dev)
    pc = torch.zeros((nq, probe), device=dev, dtype=torch.int32)
    pdd = torch.zeros((nq, probe), device=dev, dtype=torch.float32)
    full.coarse_topk_device(q.data_ptr(), nq, d, 0, k, probe, pc.data_ptr(), pdd.data_ptr())

    def run(lo, hi, thr=None):
        m = hi - lo
        od = torch.zeros((m, topk), device=dev)
        oi = torch.zeros((m, topk), device=dev, dtype=torch.int32)
        on = torch.zeros(m, device=dev, dtype=torch.int32)
        qq, cc, dd = q[lo:hi].contiguous(), pc[lo:hi].contiguous(), pdd[lo:hi].contiguous()
        torch.cuda.synchronize()
        if thr is None:
            shard.query_batch_device_probed(qq.data_ptr(), m, d, cc.data_ptr(), dd.data_ptr(), probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        else:
            t = thr[lo:hi].contiguous()
            shard.query_batch_device_seeded(qq.data_ptr(), m, d, cc.data_ptr(), dd.data_ptr(), probe, topk, t.data_ptr(), od.data_ptr(), oi.data_ptr(),
                                            on.data_ptr())
        torch.cuda.synchronize()
        pr = ix.last_profile()
        return od.cpu().numpy().view(np.uint32), oi.cpu().numpy().view(np.uint32), on.cpu().numpy().view(np.uint32), pr

    for seeded in (False, True):
        thr = None
        if seeded:   # thresholds as the step's all-reduce would hand them over: a little above each query's k-th distance on this shard
            kth = np.where(one[2] == topk, one[0].view(np.float32).max(axis=1), np.finfo(np.float32).max).astype(np.float32)
            thr = torch.from_numpy(kth * np.float32(1.001)).to(dev)
        one = run(0, nq, thr)
        halves = [run(0, nq // 2, thr), run(nq // 2, nq, thr)]
        for a in range(3):
            assert np.array_equal(one[a], np.concatenate([h[a] for h in halves])), ("seeded" if seeded else "probed", a)
        assert (one[2] > 0).any()
    shard.close()
    full.close()


@pytest.mark.parametrize("nq", [40, 300])
def test_seeded_probed_query(rq, nq):
    """rq_query_batch_device_seeded (the multi-GPU step's second call): the ranker starts from a per-query threshold and
    the whole stream runs as one stage.  (i) seeds of f32::MAX: nothing is pruned by them -- the single stage lets every
    candidate through, the survivor buffers overflow, the re-run stages as usual (thresholds through the row map) -- and the
    result is the plain probed query's, bit for bit; (ii) seeds just above each query's final k-th distance: the same
    top-k, far fewer exact distances; (iii) seeds below a query's best distance: nothing is returned for it."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    n, d, k, probe, topk = 30_000, 128, 24, 8, 10
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=81, centre_scale=0.6)
    idx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=82))
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=83, centre_scale=0.6)
    wd, wi, wn = idx.query_batch(queries, probe, topk)
    plain_rerank = ix.last_profile()["rerank_candidates"]
    assert (wn == topk).all()
    _, cl, cd = rq.ops.coarse_rank(idx, queries, probe)
    q = torch.from_numpy(queries).to(dev)
    pc = torch.from_numpy(cl.view(np.int32)).to(dev)
    pdd = torch.from_numpy(cd).to(dev)
    od = torch.empty((nq, topk), device=dev)
    oi = torch.zeros((nq, topk), device=dev, dtype=torch.int32)
    on = torch.zeros(nq, device=dev, dtype=torch.int32)

    def run(thr):
        t = torch.from_numpy(np.ascontiguousarray(thr, np.float32)).to(dev)
        torch.cuda.synchronize()
        idx.query_batch_device_seeded(q.data_ptr(), nq, d, pc.data_ptr(), pdd.data_ptr(), probe, topk, t.data_ptr(),
                                      od.data_ptr(), oi.data_ptr(), on.data_ptr())
        return od.cpu().numpy(), oi.cpu().numpy().view(np.uint32), on.cpu().numpy().view(np.uint32), ix.last_profile()

    fmax = np.finfo(np.float32).max
    gd, gi, gn, pr = run(np.full(nq, fmax))                                   # (i)
    assert pr["retries"] > 0, "f32::MAX seeds should overflow the single stage"
    assert np.array_equal(gn, wn) and np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
    kth = wd.max(axis=1)
    gd, gi, gn, pr = run(np.nextafter(kth, np.float32(np.inf)) * np.float32(1.0001))   # (ii)
    assert pr["retries"] == 0 and pr["rerank_candidates"] < plain_rerank
    # every returned entry is one of the plain top-k with the same distance; a plain neighbour can be missing only where its
    # ESTIMATE (rough) is not below the seed although its exact distance is (the plain run met it under a looser threshold)
    missing = 0
    for b in range(nq):
        plain = {int(i): wd[b, e].tobytes() for e, i in enumerate(wi[b, :topk])}
        for e in range(gn[b]):
            assert int(gi[b, e]) in plain and gd[b, e].tobytes() == plain[int(gi[b, e])], (b, e)
        missing += topk - int(gn[b])
    assert missing <= nq * topk // 50, missing
    seeds = kth.copy()
    seeds[::2] = wd.min(axis=1)[::2]                                          # (iii) every other query: nothing is below its best
    gd, gi, gn, pr = run(seeds)
    assert (gn[::2] == 0).all() and (gn[1::2] <= topk - 1).all() and (gn[1::2] >= topk - 3).all()   # strict "<": the k-th itself is cut too
    idx.close()


@pytest.mark.parametrize("tiered", [False, True])
def test_probed_query_with_padded_slots(rq, tiered):
    """Caller-supplied probe lists may be padded (id 0xFFFFFFFF, distance +inf: rq_coarse_topk_device pads when fewer lists exist
    than asked for): padded slots contribute nothing -- the answer is the one for the unpadded lists, bit for bit, through the
    re-rankers that stage per-probe records in LDS (8-bit shadow maps; tier records of split rows)."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    n, d, k, probe, topk, nq = 30_000, 128, 24, 8, 10, 300
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=61, centre_scale=0.6)
    ix.set_option("base_device_mb", (n * d * 4 * 4 // 5) >> 20 if tiered else -1)
    try:
        idx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=62))
    finally:
        ix.set_option("base_device_mb", -1)
    assert idx.split_rows == tiered
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=63, centre_scale=0.6)
    _, cl, cd = rq.ops.coarse_rank(idx, queries, probe)
    q = torch.from_numpy(queries).to(dev)

    def run(lists, dists):
        pc = torch.from_numpy(np.ascontiguousarray(lists).view(np.int32)).to(dev)
        pdd = torch.from_numpy(np.ascontiguousarray(dists, np.float32)).to(dev)
        od = torch.empty((nq, topk), device=dev)
        oi = torch.zeros((nq, topk), device=dev, dtype=torch.int32)
        on = torch.zeros(nq, device=dev, dtype=torch.int32)
        idx.query_batch_device_probed(q.data_ptr(), nq, d, pc.data_ptr(), pdd.data_ptr(), lists.shape[1], topk, od.data_ptr(),
                                      oi.data_ptr(), on.data_ptr())
        torch.cuda.synchronize()
        return od.cpu().numpy().view(np.uint32), oi.cpu().numpy(), on.cpu().numpy()

    want = run(cl[:, :6], cd[:, :6])
    padded_l, padded_d = cl.copy(), cd.copy()
    padded_l[:, 6:] = 0xFFFFFFFF
    padded_d[:, 6:] = np.inf
    got = run(padded_l, padded_d)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    idx.close()


def test_call_of_several_passes_overlaps_them_with_the_same_results(rq):
    """A call of more than 65 536 queries runs as several passes; two of them are kept in flight (option pass_overlap = 1, the
    default).  150 000 queries -- three passes -- give the bits of the same call with the passes one after the other, and of the
    queries sent in two separate calls; the counters add up."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    n, d, k, probe, topk, nq = 60_000, 128, 48, 6, 10, 150_000
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=171, centre_scale=0.6)
    idx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=172))
    g = torch.Generator(device=dev)
    g.manual_seed(173)
    q = (torch.from_numpy(centres).to(dev)[torch.randint(0, k, (nq,), generator=g, device=dev)] +
         0.8 * torch.randn(nq, d, generator=g, device=dev)).contiguous()

    def run(lo, hi):
        m = hi - lo
        od = torch.empty((m, topk), device=dev)
        oi = torch.zeros((m, topk), device=dev, dtype=torch.int32)
        on = torch.zeros(m, device=dev, dtype=torch.int32)
        rq.metrics_reset()
        idx.query_batch_device(q[lo:hi].data_ptr(), m, d, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        torch.cuda.synchronize()
        mt = rq.metrics()
        return od.cpu().numpy().view(np.uint32), oi.cpu().numpy(), on.cpu().numpy(), (mt["rough"], mt["precise"], mt["query"])

    try:
        a = run(0, nq)
        ix.set_option("pass_overlap", 0)
        b = run(0, nq)
        c1, c2 = run(0, 70_000), run(70_000, nq)
    finally:
        ix.set_option("pass_overlap", 1)
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(u, v)
    assert a[3] == b[3] and a[3] == tuple(s1 + s2 for s1, s2 in zip(c1[3], c2[3]))
    for i in range(3):
        assert np.array_equal(a[i], np.concatenate([c1[i], c2[i]]))
    idx.close()


def test_overflow_reruns_inside_the_second_pass_of_a_call(rq, oracle):
    """Overflow re-runs in a pass that does not start at query 0: the re-run's row map and the pass's offset into the call's arrays
    meet.  70 000 queries at 32 far, short lists (100 rows: nothing overflows, so the first pass of 65 536 teaches the index no
    capacity), except four planted ones in the second pass that sit in the one long list (12 000 rows): topk = 600 puts 600 x 8 or more
    positions into the first stage, whose threshold is f32::MAX -- more than the default capacity of 4096.  The whole call with two
    passes in flight, the whole call with the passes one after the other and the two passes as separate calls, each on a fresh
    index (a learnt capacity would change later calls), give the same bits; the planted rows are the CPU oracle's."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    d, n0, far, per, nq, cut, probe, topk = 64, 12_000, 32, 100, 70_000, 65_536, 1, 600
    planted = [65_536, 65_537, 68_000, 69_999]
    rng = np.random.default_rng(411)
    # far centres: norm 40 (rows of list 0 have norm ~8, at most ~13: nearer the origin; a point drawn at a far centre is ~8 from it,
    # ~41 from the origin and ~57 from the other far centres)
    fc = rng.standard_normal((far, d)).astype(np.float32)
    fc *= np.float32(40.0) / np.linalg.norm(fc, axis=1, keepdims=True).astype(np.float32)
    centres = np.concatenate([np.zeros((1, d), np.float32), fc])
    x = np.concatenate([rng.standard_normal((n0, d)).astype(np.float32),
                        np.repeat(fc, per, axis=0) + rng.standard_normal((far * per, d)).astype(np.float32)])
    P = synth.random_orthogonal(d, seed=412)
    queries = fc[rng.integers(0, far, nq)] + rng.standard_normal((nq, d)).astype(np.float32)
    queries[planted] = rng.standard_normal((len(planted), d)).astype(np.float32) * np.float32(0.2)
    q = torch.from_numpy(np.ascontiguousarray(queries)).to(dev)

    def run(idx, lo, hi):
        m = hi - lo
        od = torch.zeros((m, topk), device=dev)
        oi = torch.zeros((m, topk), device=dev, dtype=torch.int32)
        on = torch.zeros(m, device=dev, dtype=torch.int32)
        rq.metrics_reset()
        idx.query_batch_device(q[lo:hi].data_ptr(), m, d, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        torch.cuda.synchronize()
        mt = rq.metrics()
        return od.view(torch.int32), oi, on, (mt["rough"], mt["precise"], mt["query"]), ix.last_profile()["retries"]

    def fresh():
        return rq.RaBitQ.build(x, centres, P)

    try:
        idx = fresh()
        a = run(idx, 0, nq)
        idx.close()
        ix.set_option("pass_overlap", 0)
        idx = fresh()
        b = run(idx, 0, nq)
        idx.close()
        idx = fresh()
        c1, c2 = run(idx, 0, cut), run(idx, cut, nq)
        idx.close()
    finally:
        ix.set_option("pass_overlap", 1)
    for name, r in (("overlapped call", a), ("serial call", b), ("second slice", c2)):
        print(f"{name}: retries {r[4]}, metrics {r[3]}")
        assert r[4] >= 4, f"{name}: the test no longer exercises the overflow path"
    for i in range(3):
        assert torch.equal(a[i], b[i]), i
        assert torch.equal(a[i][:cut], c1[i]) and torch.equal(a[i][cut:], c2[i]), i
    assert a[3] == b[3] and a[3] == tuple(s1 + s2 for s1, s2 in zip(c1[3], c2[3]))
    oidx = oracle.OracleIndex.build(x, centres, P)
    cnt = a[2].cpu().numpy()
    for p in planted:
        assert cnt[p] == topk, (p, cnt[p])
        od, oi = oidx.query(queries[p], probe, topk, False)
        assert np.array_equal(a[1][p].cpu().numpy(), oi), p
        assert np.array_equal(a[0][p].cpu().numpy().view(np.uint32), od.view(np.uint32)), p
    oidx.close()


# ---- batches in flight: begin / end halves of the device batch call -----------------------------------
def test_begin_end_batches_overlap_and_match_sync(rq):
    import torch
    n, d, k, nq = 20000, 128, 16, 300
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=5, centre_scale=0.8)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=8))
    dev = torch.device("cuda", 0)
    qs = [torch.from_numpy(synth.mixture(nq, d, k, sigma=0.7, seed=100 + i, centre_scale=0.8)[0]).to(dev) for i in range(3)]
    want = []
    for q in qs:
        od = torch.zeros((nq, 10), device=dev)
        oi = torch.zeros((nq, 10), device=dev, dtype=torch.int32)
        on = torch.zeros((nq,), device=dev, dtype=torch.int32)
        gidx.query_batch_device(q.data_ptr(), nq, d, 6, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        want.append((od.cpu().numpy().copy(), oi.cpu().numpy().copy(), on.cpu().numpy().copy()))
    m0 = rq.metrics()
    outs, tickets = [], []
    for q in qs:   # three batches in flight at once
        od = torch.zeros((nq, 10), device=dev)
        oi = torch.zeros((nq, 10), device=dev, dtype=torch.int32)
        on = torch.zeros((nq,), device=dev, dtype=torch.int32)
        tickets.append(gidx.query_batch_device_begin(q.data_ptr(), nq, d, 6, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr()))
        outs.append((od, oi, on))
    for t in tickets:
        gidx.query_batch_device_end(t)
    m1 = rq.metrics()
    for (od, oi, on), (wd, wi, wn) in zip(outs, want):
        cnt = on.cpu().numpy()
        assert np.array_equal(cnt, wn)
        valid = np.arange(10)[None, :] < cnt[:, None]
        assert np.array_equal(oi.cpu().numpy()[valid], wi[valid])
        assert np.array_equal(od.cpu().numpy().view(np.uint32)[valid], wd.view(np.uint32)[valid])
    assert m1["query"] - m0["query"] == 3 * nq
    gidx.close()


def test_begin_end_overflow_retry_matches_sync(rq):
    # the survivor-buffer overflow re-run must also work from the _end half (fresh index: no learnt capacity yet)
    import torch
    from rabitq_amd import index as ix
    n, d = 24000, 64
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    centres = np.zeros((1, d), np.float32)
    P = synth.random_orthogonal(d, seed=3)
    queries = rng.standard_normal((6, d)).astype(np.float32) * 0.2
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(queries).to(dev)
    res = []
    for mode in ("split", "sync"):
        gidx = rq.RaBitQ.build(x, centres, P)
        od = torch.zeros((6, 2000), device=dev)
        oi = torch.zeros((6, 2000), device=dev, dtype=torch.int32)
        on = torch.zeros((6,), device=dev, dtype=torch.int32)
        if mode == "split":
            t = gidx.query_batch_device_begin(q.data_ptr(), 6, d, 1, 2000, od.data_ptr(), oi.data_ptr(), on.data_ptr())
            gidx.query_batch_device_end(t)
        else:
            gidx.query_batch_device(q.data_ptr(), 6, d, 1, 2000, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        assert ix.last_profile()["retries"] > 0, "the test no longer exercises the overflow path"
        res.append((od.cpu().numpy().view(np.uint32), oi.cpu().numpy(), on.cpu().numpy()))
        gidx.close()
    assert np.array_equal(res[0][2], res[1][2]) and (res[0][2] == 2000).all()
    assert np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][0], res[1][0])


@pytest.mark.parametrize("coarse_impl", [0, 2, 3, 4])
@pytest.mark.parametrize("k", [2000, 5000, 9000])
def test_many_lists_probe_selection_matches_oracle(rq, oracle, k, coarse_impl):
    # the register-resident probe selection is instantiated per list-count bracket (<= 1024, <= 4096, <= 8192):
    # exercise the two larger ones (and many tiny / empty lists) against the oracle; beyond 8192 lists the block-per-query
    # selection (coarse_impl 0 / 2) and the tile-minima pre-filtered selection (coarse_impl 3)
    n, d, nq = 30000, 64, 24
    x, _, _ = synth.mixture(n, d, 50, sigma=0.9, seed=k, centre_scale=0.8)
    rng = np.random.default_rng(k)
    centres = x[rng.choice(n, k, replace=False)] + rng.standard_normal((k, d)).astype(np.float32) * 0.05
    centres[7] = centres[3]                                   # duplicate centroids: ties in the coarse ranking
    P = synth.random_orthogonal(d, seed=11)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    assert np.array_equal(gidx.offsets, oidx.offsets)
    queries = (x[rng.choice(n, nq, replace=False)] + 0.05).astype(np.float32)
    from rabitq_amd import index as ix
    ix.set_option("coarse_impl", coarse_impl)
    try:
        for probe, topk in ((64, 10), (33, 5), (1, 3)):
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, False)
    finally:
        ix.set_option("coarse_impl", 0)
    gidx.close()
    oidx.close()


@pytest.mark.parametrize("d,k,nq", [(128, 300, 50), (64, 1000, 37), (192, 77, 19), (768, 40, 21), (256, 401, 45), (128, 4100, 33)])
def test_coarse_distance_kernels_agree_bitwise(rq, oracle, d, k, nq):
    """The coarse ranking (src/rabitq.rs:283-297) has two exact distance kernels -- query rows broadcast through LDS (small
    batches), query rows in scalar registers (large batches).  Forcing either
    must give the oracle's probe lists and distances bit for bit (ragged sizes: nq not a multiple of 16 / 32, k
    not a multiple of 32 / 256; duplicate centroids: ties at the selection threshold)."""
    from rabitq_amd import index as ix
    n = 6000
    x, centres, _ = synth.mixture(n, d, k, sigma=0.9, seed=d + k, centre_scale=0.8)
    centres[5] = centres[2]
    P = synth.random_orthogonal(d, seed=21)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.9, seed=d + k + 1, centre_scale=0.8)
    try:
        for impl in (1, 2, 3, 4):
            ix.set_option("coarse_impl", impl)
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, min(k, 40), 10, False)
            _compare_with_oracle(rq, oracle, oidx, gidx, queries[:3], 7, 5, False)
    finally:
        ix.set_option("coarse_impl", 0)
    gidx.close()
    oidx.close()


@pytest.mark.parametrize("topk", [63, 64, 65])
def test_large_batch_heap_sizes_around_a_wave(rq, oracle, topk):
    """Large batches keep the ranker's heap in registers (one element per lane) while it fits: a push before a pop holds
    topk + 1 elements, so 63 is the last register-resident size and 64 / 65 use the LDS heap (a fuzz run caught 64 being
    sent to the register path: the 65th element was dropped)."""
    n, d, k, nq = 18_000, 128, 2, 260
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=1003, centre_scale=1.5)
    P = synth.random_orthogonal(d, seed=3)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=5003, centre_scale=0.7)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 1, topk, False)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 2, topk, False)
    gidx.close()
    oidx.close()


def test_wide_probe_and_deep_topk_match_oracle(rq, oracle):
    # nprobe > 64 (block-wide probe selection, many pairs per query) together with a deep top-k, on a batch large
    # enough for the matrix-core final stage and the rerank-order grouping (nq >= 256)
    n, d, k, nq = 40000, 128, 160, 288
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=77, centre_scale=0.7)
    P = synth.random_orthogonal(d, seed=13)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.8, seed=78, centre_scale=0.7)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 128, 100, False)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries[:40], 160, 300, True)
    gidx.close()
    oidx.close()


def test_begin_end_heuristic_ranker_matches_sync(rq):
    import torch
    n, d, k, nq = 8000, 64, 8, 260
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=21, centre_scale=0.6)
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=4))
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(synth.mixture(nq, d, k, sigma=0.8, seed=22, centre_scale=0.6)[0]).to(dev)
    outs = []
    for split in (False, True):
        od = torch.zeros((nq, 7), device=dev)
        oi = torch.zeros((nq, 7), device=dev, dtype=torch.int32)
        on = torch.zeros((nq,), device=dev, dtype=torch.int32)
        if split:
            t = gidx.query_batch_device_begin(q.data_ptr(), nq, d, 5, 7, od.data_ptr(), oi.data_ptr(), on.data_ptr(), True)
            gidx.query_batch_device_end(t)
        else:
            gidx.query_batch_device(q.data_ptr(), nq, d, 5, 7, od.data_ptr(), oi.data_ptr(), on.data_ptr(), True)
        outs.append((od.cpu().numpy().view(np.uint32), oi.cpu().numpy(), on.cpu().numpy()))
    assert np.array_equal(outs[0][2], outs[1][2]) and (outs[0][2] > 0).all()
    valid = np.arange(7)[None, :] < outs[0][2][:, None]
    assert np.array_equal(outs[0][1][valid], outs[1][1][valid])
    assert np.array_equal(outs[0][0][valid], outs[1][0][valid])
    gidx.close()


def test_engine_shard_merge_matches_torch(rq):
    # the GPU merge kernel behind sharding.merge_probe_lists / merge_shard_topk against the torch formulation
    import torch
    from rabitq_amd import sharding
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    for world, nq, width, m_out in ((1, 50, 64, 64), (4, 300, 64, 64), (8, 77, 10, 10), (3, 5, 700, 100), (2, 9, 5, 8)):
        keys = torch.randint(0, 2**62, (world, nq, width), generator=g, device=dev, dtype=torch.int64)
        keys[:, :, : width // 3] = keys[:, :, :1]                       # duplicates
        if world > 1:
            keys[1, :, -1] = -1                                         # all-ones pattern: sorts last as u64
        got = sharding._engine_merge(keys.contiguous(), world, nq, width, m_out).cpu().numpy().view(np.uint64)
        flat = keys.permute(1, 0, 2).reshape(nq, -1).cpu().numpy().view(np.uint64)
        want = np.sort(flat, axis=1)[:, :m_out]
        if want.shape[1] < m_out:
            want = np.concatenate([want, np.full((nq, m_out - want.shape[1]), np.uint64(2**64 - 1))], axis=1)
        assert np.array_equal(got, want), (world, nq, width, m_out)
    # whole functions, world of one: engine path (GPU tensors) == torch path (CPU tensors)
    nq, nprobe, topk = 200, 64, 10
    cl = torch.randint(0, 4096, (nq, nprobe), generator=g, device=dev, dtype=torch.int32)
    dd = torch.sort(torch.rand((nq, nprobe), generator=g, device=dev), dim=1).values
    a_c, a_d = sharding.merge_probe_lists(cl, dd, nprobe)
    b_c, b_d = sharding.merge_probe_lists(cl.cpu(), dd.cpu(), nprobe)
    assert torch.equal(a_c.cpu(), b_c) and torch.equal(a_d.cpu(), b_d)
    d = torch.rand((nq, topk), generator=g, device=dev)
    i = torch.randint(0, 10**8, (nq, topk), generator=g, device=dev)
    n = torch.randint(0, topk + 1, (nq,), generator=g, device=dev)
    pay = sharding.pack_topk(d, i, n, 5)
    a = sharding.merge_shard_topk(pay, topk, id_bound=2 * 10**8)
    b = sharding.merge_shard_topk(pay.cpu(), topk)
    assert torch.equal(a[2].cpu(), b[2])
    valid = (torch.arange(topk)[None, :] < b[2][:, None])
    assert torch.equal(a[1].cpu()[valid], b[1][valid])
    assert torch.equal(a[0].cpu().view(torch.int32)[valid], b[0].view(torch.int32)[valid])


# ---- beyond-HBM indexes: raw vectors tiered between HBM and pinned host memory; streamed two-pass build ------------
@pytest.mark.parametrize("dev_mb", [0, 1])
def test_host_resident_rerank_matches_oracle(rq, oracle, tmp_path, dev_mb):
    """The rerank gathers rows from pinned host memory (all of them with a 0 MiB HBM budget; with 1 MiB every list
    keeps its first ~17 % in HBM and its tail on the host): ids, order, distances and counters still equal the oracle's, in both rerank kernels (the fused
    small-batch finish and the full-chip accurate_kernel), both rankers; base / dump / shard read through the tiers."""
    from rabitq_amd import index as ix
    n, d, k = 12000, 128, 24
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=91, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=92)
    oidx = oracle.OracleIndex.build(x, centres, P)
    ix.set_option("base_device_mb", dev_mb)
    try:
        gidx = rq.RaBitQ.build(x, centres, P)
        lidx = rq.RaBitQ.from_arrays(oidx.base, P, oidx.centroids, oidx.offsets, oidx.map_ids, oidx.codes, oidx.factors)
    finally:
        ix.set_option("base_device_mb", -1)
    # the split is per list: every list keeps floor(len * budget / n) of its members (its head) in HBM
    lens = np.diff(oidx.offsets.astype(np.int64))
    heads = lens * (0 if dev_mb == 0 else 2048) // n
    assert gidx.n_hbm == lidx.n_hbm == int(heads.sum()) and gidx.n_hbm <= 2048
    assert_bits_equal(gidx.base, oidx.base, "base through both tiers")
    queries, _, _ = synth.mixture(300, d, k, sigma=0.8, seed=93, centre_scale=0.6)
    for g in (gidx, lidx):
        _compare_with_oracle(rq, oracle, oidx, g, queries, 8, 10, False)        # nq >= 256: accurate_kernel
        _compare_with_oracle(rq, oracle, oidx, g, queries[:40], k, 20, False)   # nq < 256: stage_finish_kernel
        _compare_with_oracle(rq, oracle, oidx, g, queries[:40], 4, 10, True)
    for j in (0, 5):
        single = gidx.query(queries[j], 8, 10)
        od, oi = oidx.query(queries[j], 8, 10)
        assert [i for _, i in single] == oi.tolist()
    c3 = int(oidx.offsets[3])
    pos = np.array([0, max(int(heads[0]) - 1, 0), int(heads[0]), c3 + max(int(heads[3]) - 1, 0), c3 + int(heads[3]),
                    c3 + int(lens[3]) - 1, n - 1], np.uint32)   # heads and tails of lists, either side of the split
    qp = queries[3]
    assert_bits_equal(rq.ops.rerank(gidx, qp, pos), np.array([oracle.l2_squared_distance(oidx.base[p], qp) for p in pos], np.float32),
                      "rq_rerank on both sides of the per-list split")
    gidx.dump_to_dir(str(tmp_path / "g"))
    oidx.dump_to_dir(str(tmp_path / "o"))
    assert (tmp_path / "g" / "base.fvecs").read_bytes() == (tmp_path / "o" / "base.fvecs").read_bytes()
    owner, _ = gidx.partition_lists(2)
    ix.set_option("base_device_mb", dev_mb)
    try:
        sh = gidx.shard(owner, 1)
    finally:
        ix.set_option("base_device_mb", -1)
    keep = np.concatenate([np.arange(oidx.offsets[c], oidx.offsets[c + 1]) for c in range(k) if owner[c] == 1])
    assert_bits_equal(sh.base, oidx.base[keep], "shard of a tiered index")
    assert np.array_equal(sh.map_ids, oidx.map_ids[keep])
    for g in (gidx, lidx, sh):
        g.close()
    oidx.close()


@pytest.mark.parametrize("d,budget", [(128, 2**64 - 1), (100, 300 * 512), (768, 0)])
def test_streamed_builder_equals_one_shot_build(rq, oracle, d, budget):
    """rq_builder_* (input fed twice in ragged, out-of-order chunks) == rq_build == the oracle, array for array."""
    import torch
    dev = torch.device("cuda", 0)
    n, k = 5000, 12
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=d, centre_scale=0.6)
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=d + 1)
    oidx = oracle.OracleIndex.build(x, centres, P)
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(centres).to(dev)
    b = rq.RaBitQ.builder(n, d, cd.data_ptr(), k, orthogonal=P, max_device_base_bytes=budget)
    cuts = [0, 1, 700, 701, 3000, 4999, n]
    chunks = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)]
    for i0, m in reversed(chunks):
        buf = xd[i0:i0 + m].clone()                 # a chunk buffer of its own, as a streaming caller would have
        b.assign_chunk(buf.data_ptr(), i0, m)
    with pytest.raises(rq.RabitqError):
        b.place_chunk(xd.data_ptr(), 0, 1)          # before order()
    b.order()
    st = b.stats()
    assert st["rows_assigned"] == n and st["rows_in_hbm"] + st["rows_in_host_memory"] == n and st["ms_rotate"] > 0
    if budget == 300 * 512:
        assert 300 - k < st["rows_in_hbm"] <= 300      # per list floor(len * 300 / n) members stay in HBM
    for i0, m in chunks[::2] + chunks[1::2]:
        buf = xd[i0:i0 + m].clone()
        b.place_chunk(buf.data_ptr(), i0, m)
    gidx = b.finish()
    for name in ("base", "centroids", "offsets", "map_ids", "codes", "factors"):
        assert_bits_equal(getattr(gidx, name), getattr(oidx, name), name)
    queries, _, _ = synth.mixture(50, d, k, sigma=0.8, seed=d + 2, centre_scale=0.6)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 6, 10, False)
    # an unfinished builder can be abandoned; finishing early is refused
    b2 = rq.RaBitQ.builder(n, d, cd.data_ptr(), k, orthogonal=P)
    b2.assign_chunk(xd.data_ptr(), 0, 10)
    with pytest.raises(rq.RabitqError):
        b2.order()
    del b2
    # a duplicated chunk whose sizes still sum to n is refused (the uncovered rows would keep uninitialised labels and
    # codes), in both passes; touching and out-of-order chunks are fine
    h = n // 2
    b3 = rq.RaBitQ.builder(n, d, cd.data_ptr(), k, orthogonal=P)
    b3.assign_chunk(xd.data_ptr(), 0, h)
    for bad in ((0, h), (h - 1, 5), (10, 1)):
        with pytest.raises(rq.RabitqError) as e:
            b3.assign_chunk(xd[bad[0]:].data_ptr(), bad[0], bad[1])
        assert e.value.status == -1 and "overlap" in str(e.value)
    with pytest.raises(rq.RabitqError):
        b3.order()                                   # rows [h, n) are still missing
    b3.assign_chunk(xd[h + 100:].data_ptr(), h + 100, n - h - 100)
    b3.assign_chunk(xd[h:].data_ptr(), h, 100)       # fills the gap between two covered stretches
    b3.order()
    b3.place_chunk(xd[h:].data_ptr(), h, n - h)
    with pytest.raises(rq.RabitqError) as e:
        b3.place_chunk(xd[h:].data_ptr(), h, n - h)  # the same half again instead of the first one
    assert e.value.status == -1
    b3.place_chunk(xd.data_ptr(), 0, h)
    g3 = b3.finish()
    for name in ("base", "map_ids", "codes", "factors"):
        assert_bits_equal(getattr(g3, name), getattr(oidx, name), name + " (builder with refused duplicates)")
    g3.close()
    if st["rows_in_host_memory"]:
        with pytest.raises(rq.RabitqError) as e:     # tiered: no single device array of the raw vectors
            gidx.device_ptr(0)
        assert e.value.status == -6
    else:
        assert gidx.device_ptr(0)[1] == n * gidx.dim * 4
    gidx.close()
    oidx.close()


def test_fuzz_scale_slice(rq):
    """A bounded slice of tests/fuzz_scale.py (the engine against itself where the oracle cannot go): 10M vectors, hard
    distribution, batches up to 16 384 queries, 16 random knob sets against the default-knob answer, bit for bit."""
    from tests import fuzz_scale
    fuzz_scale.main(VECTORS=10_000_000, LISTS=1024, DIM=128, BATCH=16384, ROUNDS=16, SEED=5, HARD=1)


def test_arena_on_a_small_grid_where_everything_survives(rq, oracle):
    """Found by the fuzz driver (round 3, SEED=424242 N_MAX=40000, round 327; the generator state of that round is restored
    here): 700 queries one ulp off their centroids on sparse data at scale 3e4, heuristic ranker with top-256 and 70 probes
    -- thresholds stay loose, nearly every candidate of the probed lists survives -- on an index whose scan grid has ~130
    blocks, so only ~130 of the arena's 2048 shards are ever used: doubling the arena six times never made room and the call
    failed with RQ_ERR_OOM.  The retry now sizes the arena from the stage's exact survivor count."""
    from rabitq_amd import index as ix
    from tests import fuzz_parity as fz
    rng = np.random.default_rng(0)
    rng.bit_generator.state = {"bit_generator": "PCG64", "state": {"state": 39638530704376725464236549544941942162,
                                                                     "inc": 90750984832771704908184579979025356679},
                               "has_uint32": 0, "uinteger": 2370564739}
    x, centres, P, queries, desc = fz.make_case(rng, 327, 40000)
    assert (desc["n"], desc["d"], desc["k"], desc["nq"], desc["kind"]) == (33664, 128, 120, 700, "sparse"), desc
    knobs = {"base_device_mb": 0, "scan_tile_table": 2, "rerank_shadow": 0, "small_batch_span": 100, "scan_impl": 1, "survivor_segments": 1}
    oidx = oracle.OracleIndex.build(x, centres, P)
    try:
        for name, v in knobs.items():
            ix.set_option(name, v)
        gidx = rq.RaBitQ.build(x, centres, P)
        for probe, topk, heur in ((70, 256, True), (123, 200, False)):
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, heur)
        gidx.close()
    finally:
        for name, v in fz.KNOB_DEFAULTS.items():
            ix.set_option(name, v)
        oidx.close()


def test_arena_stages_equal_uniform_buffers_at_scale(rq):
    """The survivor arena at scale (no oracle at this size: the engine against itself): 8M vectors in 512 lists of
    Zipf-distributed sizes with overlapping clusters -- thousands of survivors for some queries, a handful for most, shards
    that run full so that the common area and the arena's growth are exercised --, 8 192 queries.  Arena stages + per-query
    segments + cell-bitmap ordering (survivor_segments = 2) must return, bit for bit, what the uniform buffers with overflow
    re-runs return (survivor_segments = 0), for both scan implementations."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    n, d, k, nq, probe, topk, sigma = 8_000_000, 128, 512, 8192, 32, 10, 0.5
    centres = synth.device_centres(k, d, dev, scale=sigma, seed=77)            # centre spacing ~ cluster radius
    wz = 1.0 / torch.arange(1, k + 1, device=dev, dtype=torch.float64) ** 0.9
    weights = (wz / wz.sum()).float()
    x = synth.device_mixture_chunk(centres, 0, n, sigma, 0, 4242, 0, k, weights)[0].contiguous()
    q = synth.device_queries(centres, nq, sigma, dev, seed=78, weights=weights)
    P = synth.random_orthogonal(d, seed=79)
    idx = rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=P)
    del x
    torch.cuda.empty_cache()

    def run():
        od = torch.full((nq, topk), -1.0, device=dev)
        oi = torch.zeros((nq, topk), device=dev, dtype=torch.int32)
        on = torch.zeros(nq, device=dev, dtype=torch.int32)
        idx.query_batch_device(q.data_ptr(), nq, d, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        return od.cpu().numpy().view(np.uint32), oi.cpu().numpy(), on.cpu().numpy(), ix.last_profile()

    try:
        for impl in (0, 2):
            ix.set_option("scan_impl", impl)
            ix.set_option("survivor_segments", 0)
            want = run()
            want = run()                       # (second call: capacities learnt)
            ix.set_option("survivor_segments", 2)
            got = run()
            got2 = run()                       # (arena sized from the first pass)
            for a, b in ((want, got), (want, got2)):
                assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
            assert want[3]["segmented_passes"] == 0 and got2[3]["segmented_passes"] == 1 and got2[3]["retries"] == 0, (want[3], got2[3])
    finally:
        ix.set_option("scan_impl", 0)
        ix.set_option("survivor_segments", 1)
        idx.close()


def test_segmented_final_stage_matches_oracle(rq, oracle):
    """Per-query survivor segments (option survivor_segments): a batch whose queries leave very different numbers of
    survivors -- most a few dozen, some tens of thousands (queries at the data's radius in one long list, deep top-k) -- gets
    stages that can exceed the uniform capacity appended to a shared arena and scattered into per-query segments sized by
    their exact counts, instead of one capacity for all.  Forced (2) from the first
    call and automatic (1: after the default capacity has overflowed once); both scan implementations; results bit-identical
    to the oracle in every mode.  (What the segments save is measured on the hard benchmark distribution: bench.py.)"""
    from rabitq_amd import index as ix
    n, d, k = 300_000, 64, 6
    rng = np.random.default_rng(33)
    centres = (rng.standard_normal((k, d)) * 4.0).astype(np.float32)
    sizes = np.array([0.8, 0.04, 0.04, 0.04, 0.04, 0.04])
    lab = rng.choice(k, n, p=sizes)
    x = (centres[lab] + rng.standard_normal((n, d))).astype(np.float32)
    P = synth.random_orthogonal(d, seed=34)
    oidx = oracle.OracleIndex.build(x, centres, P)
    nq = 300
    queries = (centres[rng.choice(k, nq, p=sizes)] + 0.2 * rng.standard_normal((nq, d))).astype(np.float32)
    queries[:40] = (x[lab == 0][:40] + 0.1 * rng.standard_normal((40, d))).astype(np.float32)   # at the radius of the long list: loose thresholds
    try:
        for impl in (1, 2):
            ix.set_option("scan_impl", impl)
            ix.set_option("survivor_segments", 2)
            gidx = rq.RaBitQ.build(x, centres, P)
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 100, False)   # (the stages before the final one may still overflow
            assert ix.last_profile()["segmented_passes"] == 1                        #  their uniform default here: re-runs, capacity learnt)
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 100, False)
            pr = ix.last_profile()
            assert pr["segmented_passes"] == 1 and pr["retries"] == 0, pr
            seg_bytes = pr["survivor_workspace_bytes"]
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, 3, 10, True)
            gidx.close()
            ix.set_option("survivor_segments", 1)        # automatic: uniform until the default capacity has overflowed once
            gidx = rq.RaBitQ.build(x, centres, P)
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 100, False)
            first = ix.last_profile()
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 100, False)
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 100, False)
            second = ix.last_profile()
            if first["retries"]:                          # the default capacity overflowed: from now on the final stage is segmented
                assert second["segmented_passes"] == 1 and second["retries"] == 0, (first, second)
            ix.set_option("survivor_segments", 0)
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, k, 100, False)
            uni = ix.last_profile()
            assert uni["segmented_passes"] == 0 and seg_bytes <= uni["survivor_workspace_bytes"]
            gidx.close()
    finally:
        ix.set_option("survivor_segments", 1)
        ix.set_option("scan_impl", 0)
    oidx.close()


def test_arena_allocation_failure_falls_back_to_uniform_buffers(rq):
    """A pass whose survivor arena cannot be had (out of memory) is repeated on the uniform buffers, results unchanged.  The
    allocation-failure injection is not in the shipped library (rq_set_option refuses it there): this runs the same workload in a
    child process on the developer build (librabitq_hip_dev.so, `make dev`; tests/dev_hooks_worker.py)."""
    from rabitq_amd import index as ix, _lib
    with pytest.raises(_lib.RabitqError):
        ix.set_option("survivor_segments", 3)             # the shipped library carries no failure injection
    dev = os.path.join(os.path.dirname(_lib.SO_PATH), "librabitq_hip_dev.so")
    assert os.path.exists(dev), "the developer build must be in the tree (__graft_entry__.build() makes it)"
    import subprocess, sys
    env = dict(os.environ, RABITQ_HIP_SO=dev)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev_hooks_worker.py"), "arena_failure"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "DEV_HOOK_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("dense_dir,scan_debug", [(0, 0), (1, 0), (0, 2048)], ids=["0", "1", "0-no_bitmap"])
def test_long_run_directories_large_batch(rq, oracle, dense_dir, scan_debug):
    """Loose thresholds (deep top-k, one long list) leave more than 512 survivor runs per query in a large batch.
    dense_dir = 0: runs are appended and the long directories ordered by sort_runs_mid_kernel, several stages in a row: by the
    cell bitmap (order_runs_bitmap), and under scan_debug = 2048, which withholds the bitmap, by its fall-backs -- the first
    call has no second directory buffer yet and sorts them bitonically in global memory, the later ones bucket the runs by probe
    slot and rank inside a bucket (sort_runs_by_slot; two probe slots: buckets beyond RQ_BUCKET_CHUNK runs, staged in chunks).
    dense_dir = 1 (default): the VALU stages write their runs into directories indexed by stream position (stage_fill_kernel:
    RQ_REC_CELL0) and nothing is sorted."""
    from rabitq_amd import index as ix
    n, d, k = 200_000, 64, 2
    rng = np.random.default_rng(15)
    centres = np.stack([np.zeros(d, np.float32), np.full(d, 5.0, np.float32)])
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:3000] += 5.0
    P = synth.random_orthogonal(d, seed=16)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    # queries at the data's own radius: their neighbours are spread over the whole (centre-distance ordered) list, so the
    # threshold learnt from the list's head stays loose and every later stage leaves thousands of sparse survivors
    queries = (x[rng.integers(3000, n, 260)] + 0.1 * rng.standard_normal((260, d))).astype(np.float32)
    try:
        ix.set_option("dense_dir", dense_dir)
        ix.set_option("scan_debug", scan_debug)
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, 2, 200, False)   # default buffers overflow: re-runs, capacity learnt
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, 2, 200, False)   # now the whole batch stays on the large-batch path
        pr = ix.last_profile()
        assert pr["retries"] == 0 and pr["rerank_candidates"] / 260 > 4096, (pr["retries"], pr["rerank_candidates"] / 260)
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, 1, 100, False)
        _compare_with_oracle(rq, oracle, oidx, gidx, queries, 2, 50, True)
    finally:
        ix.set_option("dense_dir", 1)
        ix.set_option("scan_debug", 0)
        gidx.close()
        oidx.close()


@pytest.mark.parametrize("tiered", [True, False])
@pytest.mark.parametrize("d,kind", [(128, "gauss"), (768, "gauss"), (128, "subnormal"), (128, "small_ints"), (64, "near_ties"), (128, "nan_row")])
def test_split_rows_keep_results_exact(rq, oracle, d, kind, tiered, tmp_path):
    """Indexes whose raw vectors leave no room for shadow rows (tiered ones; untiered ones that fill most of the HBM -- forced here
    with split_rows = 2) keep each row as two 16-bit planes: the upper halves of the f32 words
    rounded to nearest, then the lower halves.  Large batches re-rank through the first plane (accurate_split_kernel) and fetch the
    second one only when the first cannot PROVE accurate >= the stage's threshold; every word is restored exactly.  Ids, order and
    distances equal the oracle's bit for bit on data the first plane represents badly too (subnormal elements, near-equal
    distances, a NaN coordinate); the raw vectors read back unchanged; on ordinary data the test must reject rows; the plain layout
    (split_rows = 0) gives the same bits."""
    from rabitq_amd import index as ix
    n, k, nq = (40_000, 8, 300) if d < 768 else (12_000, 6, 280)
    rng = np.random.default_rng(7 * d + len(kind))
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=3 + d, centre_scale=0.6)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.7, seed=4 + d, centre_scale=0.6)
    if kind == "subnormal":      # tiny scales, and a twentieth of the elements subnormal f32 words
        x, centres, queries = x * 1e-6, centres * 1e-6, queries * 1e-6
        x = np.ascontiguousarray(x, np.float32)
        sub = rng.random(x.shape) < 0.05
        x.view(np.uint32)[sub] = (rng.integers(0, 1 << 23, int(sub.sum())) | (rng.integers(0, 2, int(sub.sum())) << 31)).astype(np.uint32)
    elif kind == "small_ints":
        x, centres, queries = np.rint(x * 40 + 128).clip(0, 255), np.rint(centres * 40 + 128), np.rint(queries * 40 + 128).clip(0, 255)
    elif kind == "near_ties":
        x[: n // 2] = x[:20].repeat(n // 40, axis=0) + 1e-4 * rng.standard_normal((n // 2, d))
        queries[:150] = x[rng.integers(0, n // 2, 150)] + 1e-4 * rng.standard_normal((150, d))
    x, centres, queries = (np.ascontiguousarray(a, np.float32) for a in (x, centres, queries))
    if kind == "nan_row":
        x[17, 5] = np.nan
    P = synth.random_orthogonal(d, seed=d)
    oidx = oracle.OracleIndex.build(x, centres, P)
    budget_mb = (n * d * 4 * 4 // 5) >> 20      # about four fifths of every list in HBM, the tails in pinned host memory
    ix.set_option("base_device_mb", budget_mb if tiered else -1)
    ix.set_option("split_rows", 1 if tiered else 2)
    ix.set_profiling(1)
    try:
        gidx = rq.RaBitQ.build(x, centres, P)
        assert (0 < gidx.n_hbm < n) if tiered else gidx.n_hbm == n
        assert gidx.split_rows
        with pytest.raises(rq.RabitqError) as e:   # no f32 device array of split rows
            gidx.device_ptr(0)
        assert e.value.status == -6
        assert_bits_equal(gidx.base, oidx.base, "raw vectors read back through the planes")
        for probe, topk, heur in [(8, 10, False), (3, 50, False), (8, 10, True)]:
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, heur)
            pr = ix.last_profile()
            assert pr["rerank_shadow_rejects"] <= pr["rerank_candidates"]
            if kind in ("gauss", "small_ints") and not heur:
                assert pr["rerank_shadow_rejects"] > pr["rerank_candidates"] // 8, (pr["rerank_shadow_rejects"], pr["rerank_candidates"])
        _compare_with_oracle(rq, oracle, oidx, gidx, queries[:40], 8, 10, False)    # small batch: the fused finish restores the words too
        ix.set_option("split_rows", 0)
        ix.set_option("rerank_shadow", 0)
        plain = rq.RaBitQ.build(x, centres, P)
        assert not plain.split_rows
        ix.set_option("rerank_shadow", 2)
        ix.set_option("split_rows", 1 if tiered else 2)
        a, b = gidx.query_batch(queries, 8, 10, False), plain.query_batch(queries, 8, 10, False)
        assert ix.last_profile()["rerank_shadow_rejects"] == 0
        for u, v in zip(a, b):
            assert_bits_equal(u, v, "split / plain rows")
        plain.close()
        if kind == "gauss" and d == 128:   # dump -> load and a carved shard go through the planes as well
            gidx.dump_to_dir(str(tmp_path / "idx"))
            oidx.dump_to_dir(str(tmp_path / "o"))
            assert (tmp_path / "idx" / "base.fvecs").read_bytes() == (tmp_path / "o" / "base.fvecs").read_bytes()
            loaded = rq.RaBitQ.load_from_dir(str(tmp_path / "idx"))
            assert (0 < loaded.n_hbm < n) if tiered else loaded.n_hbm == n
            c = loaded.query_batch(queries, 8, 10, False)
            assert ix.last_profile()["rerank_shadow_rejects"] > 0
            owner, _ = gidx.partition_lists(1)
            shard = gidx.shard(owner, 0)
            e = shard.query_batch(queries, 8, 10, False)
            for u, v, w in zip(a, c, e):
                assert_bits_equal(u, v, "loaded index")
                assert_bits_equal(u, w, "shard of everything")
            assert_bits_equal(shard.base, oidx.base, "shard rows")
            loaded.close()
            shard.close()
    finally:
        ix.set_profiling(0)
        ix.set_option("base_device_mb", -1)
        ix.set_option("split_rows", 1)
        ix.set_option("rerank_shadow", 2)
    gidx.close()
    oidx.close()


def test_split_rows_restore_every_bit_pattern(rq, oracle):
    """The two planes of a split row restore ANY 32-bit word: NaN payloads, infinities, subnormals, the words whose upper half
    rounds up into the next binade / to inf / wraps (0x7F7F8000.., 0xFFFF8000..).  An index loaded from arrays (no arithmetic on
    the raw vectors) with a third of every list in HBM reads back bit for bit; rq_rerank restores the words on the fly."""
    from rabitq_amd import index as ix
    n, d, k = 6000, 128, 6
    rng = np.random.default_rng(11)
    words = rng.integers(0, 1 << 32, (n, d), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7F7F8000, 0x7F7FFFFF, 0xFF7FC000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFFF8000, 0xFFFFFFFF, 0x00007FFF,
                        0x00008000, 0x8000FFFF, 0x00000000, 0x80000000, 0x3F7F8000, 0x3F7F7FFF, 0x007F8000], np.uint32)
    words[:, :16] = special[rng.integers(0, 16, (n, 16))]
    base = words.view(np.float32)
    offsets = np.linspace(0, n, k + 1).astype(np.uint32)
    P = synth.random_orthogonal(d, seed=3)
    centres = np.zeros((k, d), np.float32)
    ix.set_option("base_device_mb", 1)       # 2048 of the 6000 rows stay in HBM
    try:
        idx = rq.RaBitQ.from_arrays(base, P, centres, offsets, np.arange(n, dtype=np.uint32), np.zeros((n, d // 64), np.uint64),
                                    np.ones((n, 4), np.float32))
    finally:
        ix.set_option("base_device_mb", -1)
    assert 0 < idx.n_hbm < n
    assert_bits_equal(idx.base, base, "every word through the planes")
    fin = np.zeros((n, d), np.float32)
    fin[:] = rng.standard_normal((n, d)).astype(np.float32) * np.float32(3.0)
    idx.close()
    ix.set_option("base_device_mb", 1)
    try:
        idx = rq.RaBitQ.from_arrays(fin, P, centres, offsets, np.arange(n, dtype=np.uint32), np.zeros((n, d // 64), np.uint64),
                                    np.ones((n, 4), np.float32))
    finally:
        ix.set_option("base_device_mb", -1)
    q = rng.standard_normal(d).astype(np.float32)
    pos = np.arange(0, n, 7, dtype=np.uint32)
    want = np.array([oracle.l2_squared_distance(fin[p], q) for p in pos], np.float32)
    assert_bits_equal(rq.ops.rerank(idx, q, pos), want, "rq_rerank over split rows")
    idx.close()


@pytest.mark.parametrize("shadow", [2, 1])
@pytest.mark.parametrize("d,kind", [(128, "gauss"), (192, "gauss"), (128, "beyond_fp16"), (128, "fp16_subnormal"),
                                    (128, "small_ints"), (64, "near_ties"), (128, "nan_row"), (768, "gauss")])
def test_rerank_shadow_rows_keep_results_exact(rq, oracle, d, kind, shadow, tmp_path):
    """Large batches re-rank through shadow rows -- 8-bit codes with one affine map per list and a measured error bound
    (rerank_shadow = 2, the default: accurate_filtered8_kernel) or fp16 rows (1: accurate_filtered_kernel): a survivor is dropped
    without its f32 row being read only when the shadow PROVES accurate >= the stage's threshold.  Data the shadow represents
    badly (elements beyond the fp16 range -> inf / a list whose 8-bit step is huge, tiny scales, near-equal distances around
    the threshold, a NaN coordinate: that list is never filtered) must still give the oracle's ids and distances bit for
    bit; on ordinary data the test must actually reject rows."""
    from rabitq_amd import index as ix
    ix.set_option("rerank_shadow", shadow)
    n, k, nq = (40_000, 8, 300) if d < 768 else (12_000, 6, 280)
    rng = np.random.default_rng(d + len(kind))
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=3 + d, centre_scale=0.6)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.7, seed=4 + d, centre_scale=0.6)
    if kind == "beyond_fp16":      # a fifth of the rows carry elements the shadow can only store as inf
        big = rng.random(n) < 0.2
        x[big, rng.integers(0, d, int(big.sum()))] *= 1.0e5
        x *= 40.0
        centres, queries = centres * 40.0, queries * 40.0
    elif kind == "fp16_subnormal":
        x, centres, queries = x * 1e-6, centres * 1e-6, queries * 1e-6
    elif kind == "small_ints":     # SIFT-like
        x, centres, queries = np.rint(x * 40 + 128).clip(0, 255), np.rint(centres * 40 + 128), np.rint(queries * 40 + 128).clip(0, 255)
    elif kind == "near_ties":      # thousands of rows within 1e-4 of each other: distances crowd around every threshold
        x[: n // 2] = x[:20].repeat(n // 40, axis=0) + 1e-4 * rng.standard_normal((n // 2, d))
        queries[:150] = x[rng.integers(0, n // 2, 150)] + 1e-4 * rng.standard_normal((150, d))
    x, centres, queries = (np.ascontiguousarray(a, np.float32) for a in (x, centres, queries))
    if kind == "nan_row":
        x[17, 5] = np.nan
    P = synth.random_orthogonal(d, seed=d)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    ix.set_profiling(1)
    try:
        for probe, topk, heur in [(8, 10, False), (3, 50, False), (8, 10, True)]:
            _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, topk, heur)
            pr = ix.last_profile()
            assert pr["rerank_shadow_rejects"] <= pr["rerank_candidates"]
            if kind in ("gauss", "small_ints") and not heur:
                assert pr["rerank_shadow_rejects"] > pr["rerank_candidates"] // 8, (pr["rerank_shadow_rejects"], pr["rerank_candidates"])
        ix.set_option("rerank_shadow", 0)      # the same index without shadow rows: the plain exact re-ranker
        plain = rq.RaBitQ.build(x, centres, P)
        ix.set_option("rerank_shadow", shadow)
        a, b = gidx.query_batch(queries, 8, 10, False), plain.query_batch(queries, 8, 10, False)
        assert ix.last_profile()["rerank_shadow_rejects"] == 0
        for u, v in zip(a, b):
            assert_bits_equal(u, v, "with / without shadow rows")
        plain.close()
        if kind == "gauss" and d == 128:   # the shadow is derived state: a loaded index and a carved shard rebuild it
            gidx.dump_to_dir(str(tmp_path / "idx"))
            loaded = rq.RaBitQ.load_from_dir(str(tmp_path / "idx"))
            c = loaded.query_batch(queries, 8, 10, False)
            assert ix.last_profile()["rerank_shadow_rejects"] > 0
            owner, _ = gidx.partition_lists(1)
            shard = gidx.shard(owner, 0)
            e = shard.query_batch(queries, 8, 10, False)
            assert ix.last_profile()["rerank_shadow_rejects"] > 0
            for u, v, w in zip(a, c, e):
                assert_bits_equal(u, v, "loaded index")
                assert_bits_equal(u, w, "shard of everything")
            loaded.close()
            shard.close()
    finally:
        ix.set_profiling(0)
        ix.set_option("rerank_shadow", 2)
    gidx.close()
    oidx.close()


def test_rerank_prefilter_with_more_probed_lists_than_fit_in_lds(rq, oracle):
    """More than RQ_ACC8_LDS_PROBES (1024) probed lists: the 8-bit pre-filter reads its lists' maps, and the split-row pre-filter
    its lists' tier records, from global memory instead of LDS.  1100 lists, all probed, 256 queries (the smallest batch that takes
    the large-batch stages), both rankers, then one range search whose radii are the oracle's 10th distances (a range pass always
    runs the pre-filter: its radii are the thresholds) -- on the default index (rerank_shadow = 2) and on a tiered split-row one,
    everything bit for bit the oracle's, and every pass must have rejected rows through the pre-filter."""
    from rabitq_amd import index as ix
    from tests.models import Ref, run_range, same_range
    n, d, k, nq, probe = 110_000, 64, 1100, 256, 1100
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=61, centre_scale=0.6)
    queries, _, _ = synth.mixture(nq, d, k, sigma=0.7, seed=62, centre_scale=0.6)
    P = synth.random_orthogonal(d, seed=63)
    oidx = oracle.OracleIndex.build(x, centres, P)
    seen = []
    radii = want = None
    ix.set_profiling(1)
    try:
        for leg in ("8-bit shadow", "tiered split rows"):
            if leg == "tiered split rows":
                ix.set_option("base_device_mb", max(1, (n * d * 4 * 4 // 5) >> 20))   # split rows, list tails in host memory
            gidx = rq.RaBitQ.build(x, centres, P)
            assert (leg == "8-bit shadow") != (gidx.split_rows and gidx.n_hbm < gidx.n), leg
            for heur in (False, True):
                _compare_with_oracle(rq, oracle, oidx, gidx, queries, probe, 10, heur, seen=seen if radii is None and not heur else None)
                pr = ix.last_profile()
                print(leg, "heuristic" if heur else "heap", "rejects", pr["rerank_shadow_rejects"], "of", pr["rerank_candidates"])
                assert pr["rerank_shadow_rejects"] > 0, (leg, heur, pr)
            if radii is None:   # the oracle's side of the range search: once, for both legs
                radii = np.array([od.max() for od, _ in seen], dtype=np.float32)
                assert all(od.size == 10 for od, _ in seen)
                want = Ref(oracle, oidx).answer(queries, probe, radii)
            got, m, pr = run_range(rq, gidx, queries, probe, radii)
            same_range(got, want[:3], leg)
            assert (m["rough"], m["precise"], m["query"]) == (want[3]["rough"], want[3]["precise"], nq), (leg, m, want[3])
            print(leg, "range rejects", pr["rerank_shadow_rejects"], "of", pr["rerank_candidates"])
            assert pr["rerank_shadow_rejects"] > 0, (leg, pr)
            gidx.close()
    finally:
        ix.set_profiling(0)
        ix.set_option("base_device_mb", -1)
        oidx.close()


def test_dense_directory_falls_back_when_a_stage_has_more_cells_than_capacity(rq, oracle):
    """One list of 600 000 vectors, a large batch: the geometric stage [40 960, 327 680) spans 4 480 directory cells, more
    than the default survivor capacity (4 096), so that stage appends and sorts its runs while its neighbours use dense
    directories -- both forms inside one query pass."""
    n, d, nq = 600_000, 64, 260
    rng = np.random.default_rng(21)
    x = rng.standard_normal((n, d)).astype(np.float32)
    centres = np.zeros((1, d), np.float32)
    P = synth.random_orthogonal(d, seed=22)
    oidx = oracle.OracleIndex.build(x, centres, P)
    gidx = rq.RaBitQ.build(x, centres, P)
    queries = (x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d))).astype(np.float32)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 1, 10, False)
    _compare_with_oracle(rq, oracle, oidx, gidx, queries, 1, 10, True)
    gidx.close()
    oidx.close()


def test_json_persistence_round_trip(rq, oracle, tmp_path):
    """dump_to_json / load_from_json (src/rabitq.rs:72-81): the serde_json image of the struct (faer Mats as
    {"nrows","ncols","data": row-major}, base dim x n, centroids dim x k); every f32 survives the text bit for bit."""
    import json
    n, d, k = 300, 64, 5
    x, centres, _ = synth.mixture(n, d, k, sigma=0.8, seed=41, centre_scale=0.6)
    x[7] = centres[2]                          # a zero residual: non-normal norm -> default ip, factor edge values
    gidx = rq.RaBitQ.build(x, centres, synth.random_orthogonal(d, seed=42))
    gidx.dump_to_json(tmp_path / "idx.json")
    j = json.loads((tmp_path / "idx.json").read_text())
    assert list(j) == ["dim", "base", "orthogonal", "centroids", "rand_bias", "offsets", "map_ids", "x_binary_vec", "factors"]
    assert j["dim"] == d and (j["base"]["nrows"], j["base"]["ncols"]) == (d, n) and j["centroids"]["ncols"] == k
    assert np.array_equal(np.array(j["base"]["data"], np.float32).reshape(d, n).T, gidx.base)          # column j = vector j
    assert np.array_equal(np.array(j["centroids"]["data"], np.float32).reshape(d, k).T, gidx.centroids)
    assert np.array_equal(np.array(j["x_binary_vec"], np.uint64).reshape(n, d // 64), gidx.codes)
    assert list(j["factors"][0]) == ["factor_ip", "factor_ppc", "error_bound", "center_distance_square"]
    lidx = rq.RaBitQ.load_from_json(tmp_path / "idx.json")
    for name in ("base", "orthogonal", "centroids", "offsets", "map_ids", "codes", "factors"):
        assert_bits_equal(getattr(lidx, name), getattr(gidx, name), name)
    # key order and whitespace are free, unknown keys are skipped (serde's derive accepts any order)
    shuffled = {key: j[key] for key in reversed(list(j))}
    shuffled["extra"] = {"a": [1, 2, {"b": "x"}]}
    (tmp_path / "idx2.json").write_text(json.dumps(shuffled, indent=1))
    l2 = rq.RaBitQ.load_from_json(tmp_path / "idx2.json")
    assert_bits_equal(l2.factors, gidx.factors, "factors (shuffled text)")
    queries, _, _ = synth.mixture(20, d, k, sigma=0.8, seed=43, centre_scale=0.6)
    a, b = gidx.query_batch(queries, 3, 5), l2.query_batch(queries, 3, 5)
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))
    for g in (gidx, lidx, l2):
        g.close()


def test_fuzz_slice(rq, oracle):
    """A seeded, bounded slice of tests/fuzz_parity.py inside the suite: 60 random rounds (shapes, data families -- SIFT-like
    integers, 90 % sparse, Student-t tails, vectors on / next to their centroid, near-ties within a few ulp of the
    thresholds --, scales 1e-3 .. 3e4, query families, engine knobs incl. forced matrix-core scan and both small-batch
    settings), each compared with the oracle id for id, bit for bit, counters included."""
    from tests import fuzz_parity
    rng = np.random.default_rng(20261004)
    kinds, forced, exact_rounds = {}, 0, 0
    for it in range(60):
        desc = fuzz_parity.fuzz_round(rq, oracle, rng, it, nmax=5000)
        kinds[desc["kind"]] = kinds.get(desc["kind"], 0) + 1
        if desc["gate"] is not None and desc["gate"][0]:
            forced += 1
            exact_rounds += 1 if desc["gate"][1] else 0
    print(f"fuzz slice: families {kinds}; forced matrix-core rounds {forced}, of them with exact-path steps {exact_rounds}")
    assert len(kinds) >= 5 and forced >= 5
