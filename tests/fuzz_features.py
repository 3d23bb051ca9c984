"""Randomised fuzz of the features built on the plain query -- in-place add / remove / update, filters made after a mutation,
range search without and with a filter, dump and reload -- on the GPU box, against the CPU oracle and the models of
tests/models.py built on it (never against the engine itself): arrays, ids in order, distance bits, lims, counts and the
rough / precise / query counters, no tolerance.

    ROUNDS=300 SEED=3 python tests/fuzz_features.py        (N_MAX = largest index, default 12000)

One round: a case of fuzz_parity.make_case (ten dims, seven data families, six scales, the query families), a knob set drawn as
fuzz_parity.fuzz_round draws it, an index built on a prefix of the rows, then three to five steps.  A step is one mutation
(MUTATIONS; new rows come from the case's own rows, so they are of its family and scale), after which the index's arrays must
equal the oracle's build of the live rows in id order, and the answers of plain query_batch (both rankers), of query_batch under
one filter made after the mutation (FILTERS), and of range_search without and with that filter (radii: RADII, cycled over the
queries) must equal the oracle's.  Once per round the index is dumped, loaded again and asked a plain and a range question.
base_device_mb is drawn but held at -1 and split_rows at 1 at the most: a tiered index and one that stores split rows refuse
mutation (RQ_ERR_UNSUPPORTED; test_mutable_gpu pins the refusal).

With rq = None a round runs its models alone: the same generator draws, the same oracle answers, no engine.  That is how
tests/test_fuzz_models.py shows, without a GPU, that the seeded slice of tests/test_fuzz_features_gpu.py tests what it claims
(Coverage.check)."""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MUTATIONS = ["none", "add", "add_ids", "remove", "update", "remove_list", "add_copies", "add_centroids"]
MUTATION_WEIGHTS = [1, 2, 4, 4, 2, 2, 2, 2]   # removes and explicit-id adds more often: an id has to be freed before it can be reused
FILTERS = ["all", "one", "half", "pct1", "lists", "nothing", "added", "beyond"]
RADII = ["zero", "neg", "nan", "inf", "fmax", "below", "kth", "kth115", "kth16", "kth3"]
RANGE_LIST_VISITS = 12000     # queries x probed lists of one range call: bounds the Python side of Ref.answer
DEFAULT_CAP = 4096            # candidates per query the engine's first range pass holds before it has learnt anything


class Coverage:
    """What the rounds exercised, judged from the oracle's answers alone (and, where an engine ran, `big_retried`: rounds in
    which a query with more than DEFAULT_CAP results was in a call whose profile showed retries)."""
    ROUND_CONDITIONS = ("tied", "empty", "big", "gated", "short_topk", "zero_residual", "reused_id")

    def __init__(self):
        self.kinds, self.dims, self.scales, self.mutations, self.filters = set(), set(), set(), set(), set()
        self.rounds = {name: set() for name in self.ROUND_CONDITIONS + ("big_retried",)}

    def hit(self, name, it):
        self.rounds[name].add(it)

    def summary(self):
        return (f"families {sorted(self.kinds)} dims {sorted(self.dims)} scales {sorted(self.scales)} "
                f"mutations {len(self.mutations)}/{len(MUTATIONS)} filters {len(self.filters)}/{len(FILTERS)} rounds with "
                + " ".join(f"{k}={len(v)}" for k, v in self.rounds.items()))

    def check(self, engine):
        assert len(self.kinds) >= 5, self.kinds
        assert len(self.dims - {64, 128}) >= 3, self.dims
        assert len(self.scales - {1.0}) >= 2, self.scales
        for name in self.ROUND_CONDITIONS + (("big_retried",) if engine else ()):
            assert len(self.rounds[name]) >= 3, (name, sorted(self.rounds[name]))
        assert self.mutations == set(MUTATIONS), set(MUTATIONS) - self.mutations
        assert self.filters == set(FILTERS), set(FILTERS) - self.filters


def _tolerated(e):
    """RQ_ERR_EMPTY from the engine / a reference panic reported by the oracle (heuristic ranker with no candidate): as
    fuzz_parity.fuzz_round, nothing more to compare in that batch."""
    return getattr(e, "status", None) == -7 or "reference panics" in str(e)


def feature_round(rq, oracle, rng, it, nmax=12000, cov=None):
    """One round (module docstring).  rq = None: the models alone.  -> the case's description with the step list."""
    from tests import fuzz_parity as fz
    from tests import models as mo
    engine = rq is not None
    if engine:
        from rabitq_amd import index as ix
    cov = cov if cov is not None else Coverage()
    state0 = rng.bit_generator.state
    x, centres, P, queries, desc = fz.make_case(rng, it, nmax)
    knobs = fz.draw_knobs(rng, it)
    knobs["base_device_mb"] = -1
    knobs["split_rows"] = min(knobs["split_rows"], 1)
    n, d, k, nq = desc["n"], desc["d"], desc["k"], desc["nq"]
    n0 = max(1, int(n * float(rng.choice([0.5, 0.7, 0.9, 1.0]))))
    nsteps = int(rng.integers(3, 6))
    reload_at = int(rng.integers(0, nsteps))
    live = mo.Live(np.arange(n0), x[:n0])
    pool = [r for r in x[n0:]]          # rows not in the index: the case's own family and scale
    freed, added_round, steps = [], set(), []
    g = oidx = None
    learnt = {}                         # id(index object) -> a range call on it may have taught it a capacity

    def take(m):
        """up to m rows that are not live (the pool; removed rows return to it); none left: copies of live rows."""
        if pool:
            out = [pool.pop() for _ in range(min(m, len(pool)))]
        else:
            cur = sorted(live.rows)
            out = [live.rows[cur[int(j)]] for j in rng.integers(0, len(cur), min(m, 50))]
        return np.array(out, dtype=np.float32).reshape(len(out), d)

    def canon(what):
        if engine:
            return mo.check_oracle(oracle, g, live, centres, P, what, keep=True)
        ids, rows = live.sorted()
        return oracle.OracleIndex.build(rows, centres, P), ids

    def topk(gi, probe, tk, heur, filt=None, allowed=None):
        """-> what the oracle answered ((distances, ids) per query, up to the first reference panic)."""
        seen = []
        try:
            if engine:
                mo.compare_with_oracle(rq, oracle, oidx, gi, queries, probe, tk, heur, ids=oids,
                                       filter=None if allowed is None else (filt, allowed), seen=seen)
            elif allowed is None:
                mo.oracle_topk(oracle, oidx, queries, probe, tk, heur, ids=oids, seen=seen)
            else:
                ov = oracle.OracleIndex.view(oidx.dim, *mo.sub_arrays(oidx, allowed, oids))
                try:
                    mo.oracle_topk(oracle, ov, queries, probe, tk, heur, seen=seen)
                finally:
                    ov.close()
        except RuntimeError as e:
            if not _tolerated(e):
                raise
        return seen

    def range_check(gi, probe, radii, kinds, filt=None, allowed=None):
        ov = None
        if allowed is None:
            ref = mo.Ref(oracle, oidx, oids)
        else:
            ov = oracle.OracleIndex.view(oidx.dim, *mo.sub_arrays(oidx, allowed, oids))
            ref = mo.Ref(oracle, ov)
        try:
            want = ref.answer(queries, probe, radii)
            counts = np.diff(want[0].astype(np.int64))
            if (counts == 0).any():
                cov.hit("empty", it)
            if (counts > DEFAULT_CAP).any():
                cov.hit("big", it)
            if mo.tied_entries(want[0], want[1]):
                cov.hit("tied", it)
            if it not in cov.rounds["gated"]:
                for b in [b for b in range(nq) if kinds[b] in ("kth", "kth115", "kth16")][:6]:
                    if ref.gated_rows(queries[b], probe, radii[b]):
                        cov.hit("gated", it)
                        break
            if engine:
                got, m, pr = mo.run_range(rq, gi, queries, probe, radii, filter=filt)
                mo.same_range(got, want[:3], ("range", "filtered" if filt is not None else "plain"))
                assert (m["rough"], m["precise"], m["query"]) == (want[3]["rough"], want[3]["precise"], nq), (m, want[3])
                if (counts > DEFAULT_CAP).any():
                    if not learnt.get(id(gi)):      # nothing learnt yet: such a query cannot fit the first pass
                        assert pr["retries"] > 0, pr
                    if pr["retries"] > 0:
                        cov.hit("big_retried", it)
                if (ref.candidates > DEFAULT_CAP).any():
                    learnt[id(gi)] = True
        finally:
            if ov is not None:
                ov.close()

    try:
        cov.kinds.add(desc["kind"]), cov.dims.add(d), cov.scales.add(desc["scale"])
        if engine:
            for name, v in knobs.items():
                ix.set_option(name, v)
            g = rq.RaBitQ.build(x[:n0], centres, P)
        oidx, oids = canon("build")
        for step in range(nsteps):
            kind = str(rng.choice(MUTATIONS, p=np.array(MUTATION_WEIGHTS) / sum(MUTATION_WEIGHTS)))
            cur = np.array(sorted(live.rows), dtype=np.int64)
            m = int(rng.integers(1, max(2, min(1500, n // 3))))
            new_ids = np.zeros(0, np.int64)
            if kind in ("add", "add_copies", "add_centroids"):
                if kind == "add":
                    rows = take(m)
                elif kind == "add_copies":
                    rows = np.array([live.rows[int(i)] for i in rng.choice(cur, min(m, 200))], dtype=np.float32).reshape(-1, d)
                else:
                    rows = np.ascontiguousarray(centres[rng.integers(0, k, min(m, 64))], dtype=np.float32)
                new_ids = int(cur.max()) + 1 + np.arange(len(rows), dtype=np.int64)
                if engine:
                    assert np.array_equal(g.add(rows), new_ids.astype(np.uint32)), (step, kind)
                live.add(new_ids, rows)
            elif kind == "add_ids":
                rows = take(m)
                freed = [f for f in freed if f not in live.rows]     # (a default-id add may have given a freed id out again)
                nf = min(len(freed), max(1, len(rows) // 2))
                new_ids = np.array(freed[:nf] + list(int(cur.max()) + 10 + 3 * np.arange(len(rows))), dtype=np.int64)
                new_ids = rng.permutation(new_ids)[:len(rows)]       # id order differs from storage order
                used = set(int(i) for i in new_ids)
                if used & set(freed):
                    cov.hit("reused_id", it)
                freed = [f for f in freed if f not in used]
                if engine:
                    assert np.array_equal(g.add(rows, ids=new_ids), new_ids.astype(np.uint32)), (step, kind)
                live.add(new_ids, rows)
            elif kind in ("remove", "remove_list"):
                ids = None
                if kind == "remove_list":
                    offs = oidx.offsets.astype(np.int64)
                    nonempty = np.nonzero(np.diff(offs))[0]
                    if nonempty.size >= 2:            # (never the last rows of the index)
                        c = int(rng.choice(nonempty))
                        ids = oids[oidx.map_ids[offs[c]:offs[c + 1]]].astype(np.int64)
                        absent = 0
                if ids is None:
                    ids = rng.choice(cur, size=min(m, cur.size // 2), replace=False)
                    ids = np.concatenate([ids, [cur.max() + 100]])            # one id the index does not hold: ignored
                    absent = 1
                if engine:
                    assert g.remove(ids=ids) == ids.size - absent, (step, kind)
                gone = [int(i) for i in ids[:ids.size - absent]]
                pool.extend(live.rows[i] for i in gone)
                live.remove(gone)
                freed += gone
                added_round -= set(gone)
            elif kind == "update":
                rows = take(min(m, cur.size))
                ids = rng.choice(cur, size=len(rows), replace=False)
                if engine:
                    g.update(ids, rows)
                pool.extend(live.rows[int(i)] for i in ids)
                live.remove(ids)
                live.add(ids, rows)
                new_ids = ids
            cov.mutations.add(kind)
            added_round |= set(int(i) for i in new_ids)
            steps.append((kind, m, int(len(live.rows))))
            oidx.close()
            oidx = None
            oidx, oids = canon((step, kind))
            cur = oids.astype(np.int64)
            if new_ids.size:
                zero = oids[oidx.map_ids[oidx.factors[:, 3] == 0]]     # center_distance_square == 0: the row IS its centroid
                if np.isin(zero, new_ids).any():
                    cov.hit("zero_residual", it)

            # plain top-k, both rankers
            probe = int(rng.choice([1, 2, max(1, k // 2), k, k + 3, 70]))
            tk = int(rng.choice([1, 5, 10, 63, 64, 65, 200, 256]))
            for heur in (False, True):
                topk(g, probe, tk, heur)

            # one filter made after the mutation
            fkind = str(rng.choice(FILTERS))
            cov.filters.add(fkind)
            M = int(cur.max()) + 1
            offs = oidx.offsets.astype(np.int64)
            if fkind == "all":
                allowed = np.ones(M, dtype=bool)
            elif fkind == "one":
                allowed = np.zeros(M, dtype=bool)
                allowed[int(rng.choice(cur))] = True
            elif fkind in ("half", "pct1"):
                allowed = rng.random(M) < (0.5 if fkind == "half" else 0.01)
            elif fkind == "lists":
                allowed = np.zeros(M, dtype=bool)
                for c in range(0, k, 4):
                    allowed[oids[oidx.map_ids[offs[c]:offs[c + 1]]]] = True
            elif fkind == "nothing":
                allowed = np.zeros(M, dtype=bool)
            elif fkind == "added":
                allowed = np.zeros(M, dtype=bool)
                allowed[np.array(sorted(added_round), dtype=np.int64)] = True
            else:                                       # "beyond": ids the index does not hold, above its largest, mixed in
                allowed = rng.random(M + 500) < 0.5
                allowed[M:M + 3] = True
            filt = None
            if engine:
                filt = g.make_filter(ids=np.nonzero(allowed)[0]) if fkind in ("one", "beyond") else g.make_filter(mask=allowed)
            try:
                for heur in (False, True):
                    for od, _ in topk(g, probe, tk, heur, filt, allowed):
                        if od.size < tk:
                            cov.hit("short_topk", it)

                # range search without and with the filter; radii from the oracle's own plain answer
                rprobe = int(rng.choice([1, 2, max(1, k // 2), k, k, k + 3]))
                if nq * min(rprobe, k) > RANGE_LIST_VISITS:
                    rprobe = max(1, RANGE_LIST_VISITS // nq)
                shift = int(rng.integers(len(RADII)))
                kinds = [RADII[(b + shift) % len(RADII)] for b in range(nq)]
                radii = np.empty(nq, dtype=np.float32)
                for b in range(nq):
                    od = oidx.query(queries[b], rprobe, 10)[0]
                    best, kth = (od.min(), od.max()) if od.size else (np.float32(0), np.float32(0))
                    radii[b] = {"zero": 0.0, "neg": -1.5, "nan": np.nan, "inf": np.inf, "fmax": mo.FMAX, "below": best * np.float32(0.99),
                                "kth": kth, "kth115": kth * np.float32(1.15), "kth16": kth * np.float32(1.6),
                                "kth3": kth * np.float32(3.0)}[kinds[b]]
                range_check(g, rprobe, radii, kinds)
                range_check(g, rprobe, radii, kinds, filt, allowed)
            finally:
                if filt is not None:
                    filt.close()
            steps[-1] += (fkind, probe, tk, rprobe)

            if step == reload_at and engine:
                with tempfile.TemporaryDirectory() as tmp:
                    g.dump_to_dir(os.path.join(tmp, "idx"))
                    h = rq.RaBitQ.load_from_dir(os.path.join(tmp, "idx"))
                    try:
                        topk(h, probe, tk, False)
                        range_check(h, rprobe, radii, kinds)
                    finally:
                        h.close()
    except BaseException:
        print(f"FEATURE FUZZ FAILURE round {it}: {desc} knobs={knobs} n0={n0} reload_at={reload_at} steps={steps} "
              f"generator state at the start of the round: {state0}", flush=True)
        raise
    finally:
        if engine:
            for name, v in fz.KNOB_DEFAULTS.items():
                ix.set_option(name, v)
            if g is not None:
                g.close()
        if oidx is not None:
            oidx.close()
    desc.update(knobs=list(knobs.values()), n0=n0, steps=steps)
    return desc


def run_rounds(rq, oracle, seed, rounds, nmax, log=None):
    """`rounds` rounds from default_rng(seed) -> Coverage."""
    rng = np.random.default_rng(seed)
    cov = Coverage()
    t0 = time.time()
    for it in range(rounds):
        desc = feature_round(rq, oracle, rng, it, nmax, cov)
        if log:
            log(f"[{it + 1}/{rounds}] {desc} ok  ({time.time() - t0:.0f}s)")
    return cov


def main():
    import oracle  # noqa: E402  (test infrastructure: this script is a test driver)
    rq = None
    if not os.environ.get("MODELS_ONLY"):       # MODELS_ONLY=1: no engine, the oracle's side alone (any machine)
        import rabitq_amd as rq  # noqa: E402
        from rabitq_amd import _lib
        _lib.check(_lib.lib().rq_init(0))
    rounds = int(os.environ.get("ROUNDS", 30))
    cov = run_rounds(rq, oracle, int(os.environ.get("SEED", 1)), rounds, int(os.environ.get("N_MAX", 12000)),
                     log=lambda s: print(s, flush=True))
    print(f"fuzz features: all {rounds} rounds identical to the oracle{'' if rq else ' (models only)'}; {cov.summary()}")


if __name__ == "__main__":
    main()
