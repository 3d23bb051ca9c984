"""The option sweep on indexes where an option's code path really runs (tests/test_option_paths_gpu.py), importable without a GPU:
the cases (data through tests/synth.py, batch, probe, topk, filter), the table of (option, value) rows, and the evidence a row's
`engaged` predicate reads.  tests/test_option_cases.py checks the table itself on the CPU.  Not a conftest: import it.

Evidence of one query_batch call, gathered by the GPU test:
  ev.passes   the plan trace (scan_debug bit 16384, host_plan.h): one dict of ints per pass -- nq nprobe large small will_list placed
              fin_additive qn_slots nstages seg_final sb_nstages sb_whole -- with "stages" (the launched stages: lo hi matrix
              cluster_major ranked additive arena placed table dense_cells slot_hi) and "sb_stages" (the stages a small batch runs
              inside its block per query: lo hi)
  ev.coarse   the coarse-ranking lines of the call: "exact" / "prefilter_regs" / "prefilter_tiled", and ev.coarse_kernels, the
              exact-order distance kernel where one ran ("sreg" / "lds8" / "lds4")
  ev.profile  rabitq_amd.index.last_profile()
  ev.info     what rq_info reports (n, n_hbm, split_rows, k, dim, max_list_len) plus min_list_len / lens from the index's offsets
  ev.stderr   the call's whole stderr
  ev.base     the same case's evidence under the default options (same ranker)

A predicate states which path the value must take ON ITS CASE; when it fails the shape is wrong (or the planner is): change the
shape, never the predicate.

The cases (list lengths from the engine's own offsets at run time; the figures here are what the CPU oracle's build gives):
  A  20 000 x 128, 32 lists of 574 .. 662, 2500 queries, probe 8, topk 10.  Default plan: [0, 160) and [160, 662) VALU list-major with
     dense directories, [662, end) on the matrix cores with the additive gate; qn_slots 2 of 8.
  S  A's index, 33 queries (the small-batch path); Sf: under a filter that admits a random half of the rows; Sx: probe 32 under a
     filter of 40 rows (one or two per list) -- too sparse for the automatic small-batch rule (16 x topk / density > 65 536).
  L  16 000 x 64, 4 lists of about 4000 rows (longer than the default small_batch_span), 33 queries.
  E  40 000 x 64, 2000 lists of about 20 rows, probe 16: E300 (300 queries, topk 1), E70 (70 queries), E2100 (2100 queries: the
     pre-filtered coarse ranking, 63 tiles of 32 lists >= probe).
  B192 / B256  dimensions without an additive-gate instantiation (192 has no lane-group quantisation kernel either)."""
from collections import namedtuple

import numpy as np

from tests import synth

Index = namedtuple("Index", "n d k seed")
Case = namedtuple("Case", "index nq probe topk filter")
INDEXES = {
    "A": Index(20000, 128, 32, 131),
    "E": Index(40000, 64, 2000, 141),
    "L": Index(16000, 64, 4, 151),
    "B192": Index(8000, 192, 12, 161),
    "B256": Index(8000, 256, 12, 171),
}
CASES = {
    "A": Case("A", 2500, 8, 10, None),
    "S": Case("A", 33, 8, 10, None),
    "Sf": Case("A", 33, 8, 10, "half"),
    "Sx": Case("A", 33, 32, 10, "sparse"),
    "L": Case("L", 33, 4, 10, None),
    "E300": Case("E", 300, 16, 1, None),
    "E70": Case("E", 70, 16, 10, None),
    "E2100": Case("E", 2100, 16, 10, None),
    "B192": Case("B192", 600, 6, 10, None),
    "B256": Case("B256", 600, 6, 10, None),
}
SIGMA, CENTRE_SCALE = 0.8, 0.6


def make_index(name):
    """-> x, centres, P of the index `name`."""
    n, d, k, seed = INDEXES[name]
    x, centres, _ = synth.mixture(n, d, k, sigma=SIGMA, seed=seed, centre_scale=CENTRE_SCALE)
    return x, centres, synth.random_orthogonal(d, seed=seed + 1)


def make_queries(name):
    """The queries of every case on index `name`: drawn like the rows; a case takes the first nq of them."""
    n, d, k, seed = INDEXES[name]
    nq = max(c.nq for c in CASES.values() if c.index == name)
    q, _, _ = synth.mixture(nq, d, k, sigma=SIGMA, seed=seed + 2, centre_scale=CENTRE_SCALE)
    return q


def make_filter(kind, map_ids, offsets):
    """-> bool mask over ids for an index with these map_ids / offsets (the oracle's and the engine's are the same arrays).
    half: a random 50 %; sparse: the first stored row of every list and eight more rows."""
    offs = np.asarray(offsets, dtype=np.int64)
    n = int(offs[-1])
    if kind == "half":
        return np.random.default_rng(7).random(n) < 0.5
    assert kind == "sparse"
    mask = np.zeros(n, dtype=bool)
    lens = np.diff(offs)
    mask[np.asarray(map_ids)[offs[:-1][lens > 0]]] = True
    mask[np.asarray(map_ids)[offs[:-1][lens > 1][:8] + 1]] = True
    return mask


class Answers:
    """A case's expected answers from the CPU oracle alone, computed once per (index, probe, topk, ranker, filter) for the longest
    batch on that index and shared by the cases (and by every option value): per query the count, the ids in order, the distance
    bits and the rough / precise counters."""

    def __init__(self, oracle):
        self.oracle, self.data, self.oidx, self.masks, self.cache = oracle, {}, {}, {}, {}

    def index(self, name):
        if name not in self.data:
            x, centres, P = make_index(name)
            self.data[name] = (x, centres, P, make_queries(name))
            self.oidx[name] = self.oracle.OracleIndex.build(x, centres, P)
        return self.data[name], self.oidx[name]

    def mask(self, name, kind):
        if (name, kind) not in self.masks:
            o = self.index(name)[1]
            self.masks[name, kind] = make_filter(kind, o.map_ids, o.offsets)
        return self.masks[name, kind]

    def queries(self, case):
        c = CASES[case]
        return np.ascontiguousarray(self.index(c.index)[0][3][:c.nq])

    def want(self, case, heur):
        """-> dict(cnt u32[nq], ids u32[nq, topk], dist f32[nq, topk], rough, precise) for the case's queries."""
        from tests.models import sub_arrays
        c = CASES[case]
        key = (c.index, c.probe, c.topk, bool(heur), c.filter)
        nq_max = max(o.nq for o in CASES.values() if (o.index, o.probe, o.topk, o.filter) == key[:3] + key[4:])
        if key not in self.cache:
            (_, _, _, queries), oidx = self.index(c.index)
            view = None
            if c.filter:
                view = oidx = self.oracle.OracleIndex.view(oidx.dim, *sub_arrays(oidx, self.mask(c.index, c.filter)))
            try:
                cnt = np.zeros(nq_max, np.uint32)
                ids = np.zeros((nq_max, c.topk), np.uint32)
                dist = np.zeros((nq_max, c.topk), np.float32)
                rough, precise = np.zeros(nq_max, np.int64), np.zeros(nq_max, np.int64)
                for i in range(nq_max):
                    self.oracle.metrics_reset()
                    od, oi = oidx.query(queries[i], c.probe, c.topk, bool(heur))   # (raises where the reference panics)
                    m = self.oracle.metrics()
                    cnt[i], ids[i, :oi.size], dist[i, :od.size], rough[i], precise[i] = oi.size, oi, od, m["rough"], m["precise"]
            finally:
                if view is not None:
                    view.close()
            self.cache[key] = dict(cnt=cnt, ids=ids, dist=dist, rough=rough, precise=precise)
        w = self.cache[key]
        return dict(cnt=w["cnt"][:c.nq], ids=w["ids"][:c.nq], dist=w["dist"][:c.nq], rough=int(w["rough"][:c.nq].sum()),
                    precise=int(w["precise"][:c.nq].sum()))

    def close(self):
        for o in self.oidx.values():
            o.close()
        self.oidx = {}


def same_answer(got, want, counters, what=""):
    """What tests/models.compare_with_oracle asserts, on whole arrays: counts, ids in order, distance bits, then the rough /
    precise / query counters.  No tolerance.  got: query_batch's (dist, ids, counts); counters: rabitq_amd.metrics() of the call."""
    d, ids, cnt = got
    assert np.array_equal(cnt, want["cnt"]), (what, "counts", np.nonzero(cnt != want["cnt"])[0][:5])
    live = np.arange(ids.shape[1])[None, :] < cnt[:, None]
    bad = np.nonzero((ids != want["ids"]) & live)
    assert bad[0].size == 0, (what, "ids", bad[0][:5], ids[bad[0][:1]], want["ids"][bad[0][:1]])
    bad = np.nonzero((d.view(np.uint32) != want["dist"].view(np.uint32)) & live)
    assert bad[0].size == 0, (what, "distance bits", bad[0][:5])
    assert (counters["rough"], counters["precise"], counters["query"]) == (want["rough"], want["precise"], len(cnt)), (what, counters, want["rough"], want["precise"])


# ---- the evidence ----------------------------------------------------------------------------------------------------------------
PREFIX = "[rabitq_hip] plan: "
PASS_KEYS = ("nq", "nprobe", "large", "small", "will_list", "placed", "fin_additive", "qn_slots", "nstages", "seg_final")
STAGE_KEYS = ("lo", "hi", "matrix", "cluster_major", "ranked", "additive", "arena", "placed", "table", "dense_cells", "slot_hi")
OPEN_END = 0xFFFFFFFF   # `hi` of a stage that runs to the end of every query's stream


class Evidence:
    def __init__(self, stderr="", profile=None, info=None, base=None):
        self.stderr, self.profile, self.info, self.base = stderr, profile or {}, info or {}, base
        self.passes, self.coarse, self.coarse_kernels = parse_trace(stderr)

    @property
    def stages(self):
        return [s for p in self.passes for s in p["stages"]]

    @property
    def sb_stages(self):
        return [s for p in self.passes for s in p["sb_stages"]]

    def valu(self):
        return [s for s in self.stages if not s["matrix"]]

    def matrix(self):
        return [s for s in self.stages if s["matrix"]]

    def early(self):
        return [s for s in self.stages if s["hi"] != OPEN_END]

    def final(self):
        return [s for s in self.stages if s["hi"] == OPEN_END]


def parse_trace(stderr):
    """-> passes, coarse, coarse_kernels from the `[rabitq_hip] plan:` lines (fixed key=value tokens)."""
    passes, coarse, kernels = [], [], []
    for line in stderr.splitlines():
        if not line.startswith(PREFIX):
            continue
        tok = line[len(PREFIX):].split()
        kv = dict(t.split("=", 1) for t in tok if "=" in t)
        if tok[0] == "pass":
            p = {key: int(v) for key, v in kv.items()}
            assert all(key in p for key in PASS_KEYS), line
            p["stages"], p["sb_stages"] = [], []
            passes.append(p)
        elif tok[0].startswith("stage="):
            s = {key: int(v) for key, v in kv.items()}
            assert all(key in s for key in STAGE_KEYS) and passes and s["stage"] == len(passes[-1]["stages"]), line
            passes[-1]["stages"].append(s)
        elif tok[0].startswith("sb_stage="):
            assert passes, line
            passes[-1]["sb_stages"].append({key: int(v) for key, v in kv.items()})
        elif tok[0].startswith("coarse="):
            coarse.append(kv["coarse"])
            if "kernel" in kv:
                kernels.append(kv["kernel"])
        else:
            raise AssertionError("unknown plan line: " + line)
    for p in passes:
        assert len(p["stages"]) == p["nstages"] and len(p["sb_stages"]) == p["sb_nstages"], p
    return passes, coarse, kernels


def stage_list(p):
    """A pass's plan as a hashable value (the planner grid counts distinct ones)."""
    return tuple((s["lo"], s["hi"], s["matrix"], s["cluster_major"], s["dense_cells"] > 0) for s in p["stages"])


# ---- predicates ------------------------------------------------------------------------------------------------------------------
def _all(items, pred):
    items = list(items)
    return bool(items) and all(pred(i) for i in items)


def staged(ev):
    """one staged (not small-batch) pass with at least an early and a final stage"""
    return len(ev.passes) == 1 and not ev.passes[0]["small"] and len(ev.early()) >= 1 and len(ev.final()) == 1


def default_plan_A(ev):
    """VALU list-major early stages with dense directories, one matrix-core final stage"""
    return (staged(ev) and ev.passes[0]["large"] == 1 and _all(ev.early(), lambda s: not s["matrix"] and s["cluster_major"] and s["dense_cells"] > 0)
            and _all(ev.final(), lambda s: s["matrix"]))


def final_lo_is(pct):
    def pred(ev):   # plan_stages: the early stages of a large batch end at (the longest list, capped at 16 averages) x pct / 100
        avg = max(1, ev.info["n"] // ev.info["k"])
        settle = max(avg, min(ev.info["max_list_len"], 16 * avg))
        return staged(ev) and ev.passes[0]["large"] == 1 and ev.final()[0]["lo"] == max(1, settle * pct // 100) and ev.final()[0]["matrix"] == 1
    return pred


def first_hi_is(hi):
    return lambda ev: staged(ev) and ev.stages[0]["lo"] == 0 and ev.stages[0]["hi"] == hi


def early_cluster_major(flag, small):
    def pred(ev):
        return (len(ev.passes) == 1 and ev.passes[0]["small"] == 0 and ev.passes[0]["large"] == (0 if small else 1) and len(ev.early()) >= 2
                and _all(ev.early(), lambda s: not s["matrix"] and s["cluster_major"] == flag)
                and (small or _all(ev.early(), lambda s: s["dense_cells"] > 0)))
    return pred


def coarse_is(kind, kernel=None):
    return lambda ev: ev.coarse == [kind] and (kernel is None or ev.coarse_kernels == [kernel])


def small_path(on):
    return lambda ev: len(ev.passes) == 1 and ev.passes[0]["small"] == on and ev.profile["small_batch_passes"] == on


def sb_span_pred(value):
    def pred(ev):
        if not small_path(1)(ev) or not ev.sb_stages:
            return False
        los = [s["lo"] for s in ev.sb_stages]
        if value == 64:         # the in-block early stages end behind the first one: [0, 160), then the rest
            return los == [0, 160]
        if value == 2560:       # ... at the span, which is shorter than the lists
            return max(los) == 2560 < ev.info["min_list_len"]
        return max(los) == ev.info["max_list_len"] > 2560   # ... where the threshold has settled: the longest list
    return pred


def tiers(kind):
    def pred(ev):
        n, hbm = ev.info["n"], ev.info["n_hbm"]
        return {"all": hbm == n, "none": hbm == 0, "some": 0 < hbm < n}[kind]
    return pred


Row = namedtuple("Row", "option value case engaged also covered_by", defaults=(None, None, None, None))


def R(option, value, case, engaged, **also):
    return Row(option, value, case, engaged, also, None)


def covered(option, value, test):
    return Row(option, value, None, None, None, test)


PARITY = "tests/test_gpu_parity.py::"
TABLE = [
    # -- the scan engines and their gate
    R("scan_impl", 0, "A", lambda ev: default_plan_A(ev) and 0 < ev.profile["matrix_launches"] < ev.profile["scan_launches"]),
    R("scan_impl", 1, "A", lambda ev: staged(ev) and not ev.matrix() and ev.profile["matrix_launches"] == 0 and ev.passes[0]["qn_slots"] == ev.passes[0]["nprobe"]),
    R("scan_impl", 2, "A", lambda ev: staged(ev) and not ev.valu() and ev.profile["matrix_launches"] == ev.profile["scan_launches"] > 0),
    R("scan_gate", 0, "A", lambda ev: default_plan_A(ev) and ev.final()[0]["additive"] == 1 and ev.profile["matrix_additive_launches"] > 0),
    R("scan_gate", 1, "A", lambda ev: default_plan_A(ev) and ev.final()[0]["additive"] == 0 and ev.profile["matrix_additive_launches"] == 0 < ev.profile["matrix_launches"]),
    R("scan_gate", 2, "A", lambda ev: default_plan_A(ev) and ev.final()[0]["additive"] == 1 and ev.profile["matrix_additive_launches"] > 0),
    R("scan_gate", 2, "B192", lambda ev: staged(ev) and ev.matrix() and _all(ev.stages, lambda s: s["additive"] == 0) and ev.profile["matrix_additive_launches"] == 0 < ev.profile["matrix_launches"]),
    R("scan_gate", 2, "B256", lambda ev: staged(ev) and ev.matrix() and _all(ev.stages, lambda s: s["additive"] == 0) and ev.profile["matrix_additive_launches"] == 0 < ev.profile["matrix_launches"]),
    # -- directories, grids, placement
    R("dense_dir", 1, "A", lambda ev: default_plan_A(ev)),
    R("dense_dir", 0, "A", lambda ev: staged(ev) and ev.passes[0]["large"] == 1 and ev.valu() and _all(ev.stages, lambda s: s["dense_cells"] == 0)),
    R("max_scan_blocks", 0, "A", lambda ev: default_plan_A(ev) and ev.profile["scan_launches"] == len(ev.stages)),
    R("max_scan_blocks", 1, "A", lambda ev: default_plan_A(ev) and ev.profile["scan_launches"] > ev.base.profile["scan_launches"] == len(ev.stages)),
    R("max_scan_blocks", 7, "A", lambda ev: default_plan_A(ev) and ev.profile["scan_launches"] > ev.base.profile["scan_launches"] == len(ev.stages)),
    R("scan_tile_table", 0, "A", lambda ev: default_plan_A(ev) and _all(ev.stages, lambda s: s["table"] == 0)),
    R("scan_tile_table", 1, "A", lambda ev: default_plan_A(ev) and _all(ev.stages, lambda s: s["table"] == 0)),   # (equal lists: the automatic rule keeps the plain grid)
    covered("scan_tile_table", 1, PARITY + "test_scan_grid_chunking_matches_oracle"),                                  # (one long list: it takes the table)
    R("scan_tile_table", 2, "A", lambda ev: default_plan_A(ev) and ev.final()[0]["table"] == 1),
    R("group_rank", 0, "A", lambda ev: default_plan_A(ev) and _all(ev.stages, lambda s: s["ranked"] == 0)),
    R("group_rank", 1, "A", lambda ev: default_plan_A(ev) and _all(ev.stages, lambda s: s["ranked"] == 0)),       # (20 000 pairs: below the automatic rule's 16 blocks)
    covered("group_rank", 1, PARITY + "test_ranked_group_placement_matches_oracle"),                                   # (9000 x 64 pairs: ranked the automatic way)
    R("group_rank", 2, "A", lambda ev: default_plan_A(ev) and _all(ev.stages, lambda s: s["ranked"] == 1)),
    R("prep_placement", 1, "A", lambda ev: default_plan_A(ev) and ev.passes[0]["placed"] == 1 and ev.final()[0]["placed"] == 1 and ev.passes[0]["fin_additive"] == 1,
      group_rank=2),
    R("prep_placement", 0, "A", lambda ev: default_plan_A(ev) and ev.passes[0]["placed"] == 0 and ev.final()[0]["ranked"] == 1 and not any(s["placed"] for s in ev.stages),
      group_rank=2),
    # -- survivors, rerank, where the rows live
    R("survivor_segments", 0, "A", lambda ev: default_plan_A(ev) and ev.passes[0]["seg_final"] == 0 and ev.profile["segmented_passes"] == 0),
    R("survivor_segments", 1, "A", lambda ev: default_plan_A(ev) and ev.passes[0]["seg_final"] == 0 and ev.profile["segmented_passes"] == 0),   # (nothing has overflowed)
    covered("survivor_segments", 1, PARITY + "test_arena_stages_equal_uniform_buffers_at_scale"),
    R("survivor_segments", 2, "A", lambda ev: staged(ev) and ev.passes[0]["seg_final"] == 1 and ev.final()[0]["arena"] == 1 and ev.profile["segmented_passes"] > 0),
    covered("survivor_segments", 3, PARITY + "test_arena_allocation_failure_falls_back_to_uniform_buffers"),         # (developer build)
    R("rerank_shadow", 0, "A", lambda ev: default_plan_A(ev) and ev.profile["rerank_shadow_rejects"] == 0),
    R("rerank_shadow", 1, "A", lambda ev: default_plan_A(ev) and ev.profile["rerank_shadow_rejects"] > 0),
    R("rerank_shadow", 2, "A", lambda ev: default_plan_A(ev) and ev.profile["rerank_shadow_rejects"] > 0),
    R("split_rows", 0, "A", lambda ev: tiers("some")(ev) and not ev.info["split_rows"], base_device_mb=1),
    R("split_rows", 1, "A", lambda ev: tiers("some")(ev) and ev.info["split_rows"] and ev.profile["rerank_shadow_rejects"] > 0, base_device_mb=1),
    R("split_rows", 2, "A", lambda ev: tiers("all")(ev) and ev.info["split_rows"] and ev.profile["rerank_shadow_rejects"] > 0),
    R("base_device_mb", -1, "A", tiers("all")),
    R("base_device_mb", 0, "A", tiers("none")),
    R("base_device_mb", 1, "A", tiers("some")),
    R("assign_impl", 0, "A", lambda ev: ev.info["dim"] // 64 in (1, 2, 3, 4, 6, 8, 12)),   # (the built arrays are compared for every row)
    R("assign_impl", 1, "A", lambda ev: ev.info["dim"] // 64 in (1, 2, 3, 4, 6, 8, 12)),
    # -- the planner's knobs
    R("large_batch_from", 256, "A", default_plan_A),
    R("large_batch_from", 100000, "A", lambda ev: staged(ev) and ev.passes[0]["large"] == 0 and _all(ev.stages, lambda s: s["dense_cells"] == 0) and ev.stages[0]["hi"] == 10),
    R("large_batch_from", 256, "S", lambda ev: len(ev.passes) == 1 and ev.passes[0]["small"] == 0 and ev.passes[0]["large"] == 0, small_batch=1),
    R("large_batch_from", 2, "S", lambda ev: len(ev.passes) == 1 and ev.passes[0]["small"] == 0 and ev.passes[0]["large"] == 1 and any(s["dense_cells"] > 0 for s in ev.stages),
      small_batch=1),
    R("stage_settle_pct", 25, "A", final_lo_is(25)),
    R("stage_settle_pct", 100, "A", final_lo_is(100)),
    R("stage_settle_pct", 400, "A", final_lo_is(400)),
    R("stage_growth", 0, "A", first_hi_is(160)),       # (below 32 768 queries the default growth is 16)
    covered("stage_growth", 0, PARITY + "test_call_of_several_passes_overlaps_them_with_the_same_results"),   # (from 32 768 queries on: 8)
    R("stage_growth", 2, "A", first_hi_is(20)),
    R("stage_growth", 16, "A", first_hi_is(160)),
    R("cluster_major_div", 2, "E300", early_cluster_major(0, small=False)),
    R("cluster_major_div", 32, "E300", early_cluster_major(1, small=False)),
    R("cluster_major_div", 1024, "E300", early_cluster_major(1, small=False)),
    R("cluster_major_div", 2, "E70", early_cluster_major(0, small=True), small_batch=1),
    R("cluster_major_div", 32, "E70", early_cluster_major(1, small=True), small_batch=1),
    R("cluster_major_div", 1024, "E70", early_cluster_major(1, small=True), small_batch=1),
    # -- coarse ranking
    R("coarse_impl", 0, "E2100", coarse_is("prefilter_regs")),
    R("coarse_impl", 1, "E2100", coarse_is("exact", "lds8")),
    R("coarse_impl", 2, "E2100", coarse_is("exact", "sreg")),
    R("coarse_impl", 3, "E2100", coarse_is("prefilter_regs")),
    R("coarse_impl", 4, "E2100", coarse_is("prefilter_tiled")),
    R("coarse_impl", 0, "E300", coarse_is("exact", "lds8")),
    R("coarse_tiled_from", 0, "E2100", coarse_is("prefilter_tiled")),
    R("coarse_tiled_from", 4096, "E2100", coarse_is("prefilter_regs")),
    R("coarse_tiled_from", 1000000, "E2100", coarse_is("prefilter_regs")),
    R("coarse_impl", 0, "A", coarse_is("exact", "sreg")),   # (32 lists: below the pre-filter's 64)
    # -- small batches
    R("small_batch", 0, "S", small_path(1)),
    R("small_batch", 1, "S", lambda ev: small_path(0)(ev) and len(ev.stages) >= 2),
    R("small_batch_span", 64, "L", sb_span_pred(64)),
    R("small_batch_span", 2560, "L", sb_span_pred(2560)),
    R("small_batch_span", 100000, "L", sb_span_pred(100000)),
    R("small_batch_filtered", 0, "Sf", small_path(0)),
    R("small_batch_filtered", 1, "Sf", small_path(1)),
    R("small_batch_filtered", 1, "Sx", small_path(0)),
    R("small_batch_filtered", 2, "Sx", small_path(1)),
    R("pair_split", 1, "Sf", lambda ev: small_path(0)(ev) and ev.passes[0]["will_list"] == 1, small_batch=1),
    R("pair_split", 0, "Sf", lambda ev: small_path(0)(ev) and ev.passes[0]["will_list"] == 0, small_batch=1),
    # -- measurement hooks (bit 16384 is set for every row: it is the trace)
    R("scan_debug", 0, "A", default_plan_A),
    R("scan_debug", 16384, "A", default_plan_A),
    R("scan_debug", 128, "A", lambda ev: default_plan_A(ev) and ev.profile["matrix_subtile_steps"] > 0),
    R("scan_debug", 512, "A", lambda ev: default_plan_A(ev) and ev.profile["rerank_shadow_rejects"] == 0 < ev.base.profile["rerank_shadow_rejects"]),
    R("scan_debug", 4096, "S", lambda ev: small_path(1)(ev) and "sb_query_kernel phases" in ev.stderr),
    R("scan_debug", 128 | 512 | 4096, "S", lambda ev: small_path(1)(ev) and "sb_query_kernel phases" in ev.stderr),
    covered("scan_debug", 2048, PARITY + "test_long_run_directories_large_batch"),                                      # (run directories beyond 512 runs)
    # -- paths that need shapes too big for this module
    covered("pass_overlap", 0, PARITY + "test_call_of_several_passes_overlaps_them_with_the_same_results"),           # (more than 65 536 queries)
    covered("pass_overlap", 1, PARITY + "test_call_of_several_passes_overlaps_them_with_the_same_results"),
    covered("shared_thresholds", 0, "tests/test_sharded_gpu.py::test_sharded_entry_through_rccl_world1"),               # (the sharded step)
    covered("shared_thresholds", 1, "tests/test_sharded_gpu.py::test_sharded_entry_through_rccl_world1"),
    covered("shared_thresholds", 2, "tests/test_sharded_gpu.py::test_sharded_entry_through_rccl_world1"),
]
ENGAGED = [r for r in TABLE if r.covered_by is None]

# every option rq_set_option knows and its default (the GPU test restores them all)
DEFAULTS = {"scan_impl": 0, "scan_gate": 0, "coarse_impl": 0, "coarse_tiled_from": 4096, "group_rank": 1, "scan_tile_table": 1, "dense_dir": 1,
            "small_batch": 0, "small_batch_span": 2560, "stage_growth": 0, "survivor_segments": 1, "max_scan_blocks": 0,
            "shared_thresholds": 1, "assign_impl": 0, "rerank_shadow": 2, "pair_split": 1, "scan_debug": 0,
            "split_rows": 1, "pass_overlap": 1, "large_batch_from": 256, "cluster_major_div": 32, "stage_settle_pct": 100,
            "prep_placement": 1, "small_batch_filtered": 1, "base_device_mb": -1}

# the planner grid on case A (tests/test_option_paths_gpu.py::test_planner_grid)
GRID = {"large_batch_from": (2, 256, 100000), "stage_settle_pct": (25, 100, 400), "stage_growth": (0, 2, 16), "cluster_major_div": (2, 32, 1024)}


def row_id(r):
    also = "".join(f"+{k}={v}" for k, v in (r.also or {}).items())
    return f"{r.option}={r.value}@{r.case}{also}"
