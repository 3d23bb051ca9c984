"""The rerank pre-filter with its 8-bit shadow rows through the LDS ring (accurate_ring8_kernel) against the kernel that reads them
into registers (accurate_filtered8_kernel, scan_debug bit 32768): every case builds an index, runs one query_batch per ranker and
route, compares each answer with the CPU oracle bit for bit (counts, ids in order, distance bits, the rough / precise / query
counters), compares rerank_shadow_rejects and rerank_candidates of the two routes for equality, and reads the route the plan chose
from the trace (`rerank=ring` / `rerank=regs`, scan_debug bit 16384).  large_batch_from = 2, the smallest value the option takes: every batch here takes the large-batch path
(small_batch = 1: none the few-launch path).

Shapes: 24 000 vectors in 12 lists (2000 a list: the plan makes a first stage [0, 160) and two pre-filtered stages behind it), probe 4, topk 10 unless the case
says otherwise.  Dimensions 64, 128, 192, 256 have a ring instantiation (64: half-line rows; 192: 12 pieces, no measured row norms),
768 keeps the register kernel.  `overflow`: 96 000 rows around the origin in 24 lists and 6000 around a far centre in one, probe 25,
topk 250, half of the 12 queries at each place.  The first stage [0, 4000) (topk x stage_growth) fits the default capacity of 4096
survivors (what tests/fuzz_features.py calls DEFAULT_CAP); behind it the threshold lets a sixteenth through: some 5700 of the 92 000
rows around the origin, so the kernel meets n > cap for those queries (the call must report retries) and the re-run's blocks take
several rounds each, while for the far queries only the far list's rest competes and fits -- a re-run pass does not add to the
profile's rerank counters, the far queries' rejections are what they show.  That is the exact ranker's batch (6 retries, one per query
at the origin); the heuristic ranker's thresholds are tighter on this data and its batch stays inside the capacity (no retry), so the
case asks for an overflow under at least one ranker and for equal retry counts of the two routes under both.  `turnover`: 2100 queries, one block per query
(gx = 1), so a block works through every round of its query: the ring turns over (the heuristic ranker's looser thresholds leave
some 470 survivors per query and pre-filtered stage, 3.7 rounds).

A run that rejected nothing, or passed nothing on to the exact path, fails; so does the module when no ring case with one block per
query averaged 3 rounds' worth of survivors per query and pre-filtered stage, or none queued 128 survivors per query and
pre-filtered stage for the exact path.  Both figures leave out the first stage (its span is taken off: every candidate of it can
survive, none meets the pre-filter or this kernel's queue).  The CPU oracle has no model of the shadow rows, so it cannot say
which survivors the 8-bit test lets through; the figures are the GPU's own counters, asserted here.  `turnover` under the heuristic
ranker: 1100 candidates per query, 673 rejected, first stage [0, 160): 470 survivors and 133 queued per query and pre-filtered stage.

Run on the GPU box:  python -m pytest tests/test_rerank_ring_gpu.py -m gpu -x -q
"""
import re
from collections import namedtuple

import numpy as np
import pytest

from tests import option_cases as oc
from tests import synth
from tests.models import sub_arrays
from tests.test_gpu_parity import rq  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu
TRACE, REGS = 16384, 32768
ROUND = 128   # survivors per block and round: 128 lane pairs, one each (RQ_RING_V)

Case = namedtuple("Case", "dim nq topk filt shape expect")
CASES = {
    "d64-nq130": Case(64, 130, 10, None, "lists", "ring"),
    "d128-nq3": Case(128, 3, 10, None, "lists", "ring"),
    "d128-nq300": Case(128, 300, 10, None, "lists", "ring"),
    "d192-nq130": Case(192, 130, 10, None, "lists", "ring"),
    "d256-nq300": Case(256, 300, 10, None, "lists", "ring"),
    "d768-nq130": Case(768, 130, 10, None, "lists", "regs"),
    "d128-topk200": Case(128, 130, 200, None, "lists", "ring"),
    "d128-filter": Case(128, 130, 10, "half", "lists", "ring"),
    "d128-overflow": Case(128, 12, 250, None, "overflow", "ring"),
    "d128-turnover": Case(128, 2100, 10, None, "lists", "ring"),
}
PROBE = 4
seen = {}   # case -> (survivors per query and pre-filtered stage, exact-path survivors per query) under the ring


def make_data(c):
    if c.shape == "overflow":
        rng = np.random.default_rng(5 + c.dim)
        centres = (rng.standard_normal((25, c.dim)) * 0.05).astype(np.float32)
        centres[24] = 6.0
        x = rng.standard_normal((102000, c.dim)).astype(np.float32)
        x[96000:] += centres[24]
        queries = rng.standard_normal((c.nq, c.dim)).astype(np.float32) * 0.2
        queries[c.nq // 2:] += centres[24]
        return x, centres, synth.random_orthogonal(c.dim, seed=3), queries
    x, centres, _ = synth.mixture(24000, c.dim, 12, sigma=oc.SIGMA, seed=500 + c.dim, centre_scale=oc.CENTRE_SCALE)
    queries, _, _ = synth.mixture(2100, c.dim, 12, sigma=oc.SIGMA, seed=502 + c.dim, centre_scale=oc.CENTRE_SCALE)
    return x, centres, synth.random_orthogonal(c.dim, seed=501 + c.dim), queries


@pytest.fixture(scope="module")
def wanted(oracle):
    """The oracle's side, computed once per (shape, dim, topk, filter, ranker) for the longest batch and shared by the cases."""
    data, oidx, cache = {}, {}, {}

    def get(name, heur):
        c = CASES[name]
        dk = (c.shape, c.dim)
        if dk not in data:
            data[dk] = make_data(c)
            oidx[dk] = oracle.OracleIndex.build(*data[dk][:3])
        x, centres, P, queries = data[dk]
        o = oidx[dk]
        mask = oc.make_filter(c.filt, o.map_ids, o.offsets) if c.filt else None
        probe = 25 if c.shape == "overflow" else PROBE
        key = (dk, c.topk, c.filt, bool(heur))
        nq_max = max(v.nq for v in CASES.values() if ((v.shape, v.dim), v.topk, v.filt) == key[:3])
        if key not in cache:
            view = ov = None
            if mask is not None:
                view = ov = oracle.OracleIndex.view(o.dim, *sub_arrays(o, mask))
            try:
                cnt, ids, dist = np.zeros(nq_max, np.uint32), np.zeros((nq_max, c.topk), np.uint32), np.zeros((nq_max, c.topk), np.float32)
                rough, precise = np.zeros(nq_max, np.int64), np.zeros(nq_max, np.int64)
                for i in range(nq_max):
                    oracle.metrics_reset()
                    od, oi = (o if ov is None else ov).query(queries[i], probe, c.topk, bool(heur))
                    m = oracle.metrics()
                    cnt[i], ids[i, :oi.size], dist[i, :od.size], rough[i], precise[i] = oi.size, oi, od, m["rough"], m["precise"]
            finally:
                if view is not None:
                    view.close()
            cache[key] = (cnt, ids, dist, rough, precise)
        cnt, ids, dist, rough, precise = cache[key]
        n = c.nq
        want = dict(cnt=cnt[:n], ids=ids[:n], dist=dist[:n], rough=int(rough[:n].sum()), precise=int(precise[:n].sum()))
        return (x, centres, P, np.ascontiguousarray(queries[:n])), mask, probe, want

    yield get
    for o in oidx.values():
        o.close()


def run(rq, capfd, data, mask, probe, c, heur, ring, want, what):
    """A fresh index (what a batch teaches an index -- capacities, the gate -- must not differ between the routes), one batch."""
    from rabitq_amd import index as ix
    x, centres, P, queries = data
    gidx = filt = None
    try:
        ix.set_option("large_batch_from", 2)   # (the smallest value the option takes)
        ix.set_option("small_batch", 1)        # (... and none the few-launch path, which runs the stages inside one block per query)
        ix.set_option("scan_debug", TRACE | (0 if ring else REGS))
        gidx = rq.RaBitQ.build(x, centres, P)
        if mask is not None:
            filt = gidx.make_filter(mask=mask)
        capfd.readouterr()
        rq.metrics_reset()
        got = gidx.query_batch(queries, probe, c.topk, heur, filter=filt)
        counters, profile = rq.metrics(), ix.last_profile()
        err = capfd.readouterr().err
    finally:
        for name, v in oc.DEFAULTS.items():
            ix.set_option(name, v)
        if filt is not None:
            filt.close()
        if gidx is not None:
            gidx.close()
    oc.same_answer(got, want, counters, what)
    return profile, re.findall(r"stage \d+: rerank=(\w+)", err), err


@pytest.mark.parametrize("name", sorted(CASES))
def test_ring_and_registers_agree_with_the_oracle(rq, wanted, capfd, name):
    c = CASES[name]
    overflowed = False
    for heur in (False, True):
        data, mask, probe, want = wanted(name, heur)
        prof = {}
        for ring in (1, 0):
            prof[ring], tokens, err = run(rq, capfd, data, mask, probe, c, heur, ring, want, f"{name} heur={heur} ring={ring}")
            expect = c.expect if ring else "regs"
            assert tokens and set(tokens) == {expect}, (name, heur, ring, tokens, err[-2000:])
            cand, rej = prof[ring]["rerank_candidates"], prof[ring]["rerank_shadow_rejects"]
            with capfd.disabled():
                print(name, "heur", heur, "ring", ring, "route", tokens, "candidates", cand, "rejects", rej, "retries", prof[ring]["retries"],
                      "per query and pre-filtered stage", round(cand / c.nq / len(tokens), 1), "exact per query", round((cand - rej) / c.nq, 1))
            assert rej > 0, (name, heur, ring, "the pre-filter rejected nothing")
            assert cand - rej > 0, (name, heur, ring, "nothing went on to the exact path")
        overflowed = overflowed or prof[1]["retries"] > 0
        for key in ("rerank_shadow_rejects", "rerank_candidates", "retries"):
            assert prof[1][key] == prof[0][key], (name, heur, key, prof[1][key], prof[0][key])
        if c.expect == "ring":
            # rerank_candidates counts the first stage's survivors too, which meet no pre-filter: the first stage's span is taken off
            # (every candidate of it can survive), and the rest is spread over every pre-filtered stage of every pass.  The turn-over
            # figure is kept for the batches with one block per query only (gx = 1 from 2049 queries on): there a block sees every round.
            first_hi = oc.Evidence(err).passes[0]["stages"][0]["hi"]
            assert first_hi != oc.OPEN_END
            per_stage = (prof[1]["rerank_candidates"] / c.nq - first_hi) / len(tokens)
            # What the pre-filtered stages pass on to the queue: the first stage's survivors (never rejected, re-ranked by accurate_kernel,
            # not by this kernel's queue) are taken off here too.  Per query AND pre-filtered stage, under one block per query: at 128 or
            # more on average some block had 128 waiting inside its loop, i.e. ran a full exact pass between two rounds of a launch
            # whose threshold is finite (it rejected: copies in flight around the exact path's row loads).
            queued = ((prof[1]["rerank_candidates"] - prof[1]["rerank_shadow_rejects"]) / c.nq - first_hi) / len(tokens)
            with capfd.disabled():
                print(name, "heur", heur, "first stage", first_hi, "per query and pre-filtered stage: survivors", round(per_stage, 1), "queued", round(queued, 1))
            seen[name, heur] = (per_stage, queued) if c.nq >= 2049 else (0.0, 0.0)
    if c.shape == "overflow":
        assert overflowed, (name, "no batch of the case overflowed the default capacity: the kernel never met n > cap")


def test_the_ring_turned_over_and_the_queue_filled():
    """After the cases above (same module, same process): at least one ring case with one block per query averaged three rounds' worth
    of survivors per query and pre-filtered stage, and at least one such case queued 128 survivors per query and pre-filtered stage
    for the exact path (the first stage's survivors, which meet no pre-filter and no queue, counted out of both)."""
    assert seen, "run the whole module: this test reads what the cases recorded"
    assert max(v[0] for v in seen.values()) >= 3 * ROUND, seen
    assert max(v[1] for v in seen.values()) >= 128, seen
