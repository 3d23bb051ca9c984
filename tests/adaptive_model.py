"""Adaptive probing's rule in numpy -- the only statement of it in the tests -- and the data the adaptive tests run on.

The rule (include/rabitq_hip.h, rq_probe_rule_t).  d_0 <= d_1 <= ... <= d_{m-1}: a query's coarse distances in visiting order, m = min(probe, k).
    t = ratio * d_0                 one f32 multiplication, round to nearest (ratio = +inf: t = +inf)
    p = length of the longest prefix whose entries all satisfy d_j <= t       (a NaN compares false)
    n = min(cap, max(min_probe, p)) clamped to [1, m];   cap = the query's entry of the caps array clamped to [1, m], or m
"""
import numpy as np

from tests import synth


def probe_counts(dist, ratio, min_probe=1, caps=None):
    """dist: B x m f32 coarse distances, rows ascending -> uint32[B], the lists each query visits under the rule."""
    dist = np.asarray(dist, dtype=np.float32)
    assert dist.ndim == 2 and dist.shape[1] >= 1 and min_probe >= 1
    B, m = dist.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if np.isposinf(np.float32(ratio)):
            t = np.full(B, np.inf, dtype=np.float32)
        else:
            t = (np.float32(ratio) * dist[:, 0]).astype(np.float32)        # f32 x f32 -> f32, round to nearest
        ok = dist <= t[:, None]                                             # NaN on either side: False
    p = np.where(ok.all(axis=1), m, np.argmin(ok, axis=1))                  # first False, or m
    cap = np.full(B, m, dtype=np.int64) if caps is None else np.clip(np.asarray(caps, dtype=np.int64), 1, m)
    n = np.minimum(cap, np.maximum(int(min_probe), p.astype(np.int64)))
    return np.clip(n, 1, m).astype(np.uint32)


# ---- the worlds of tests/test_adaptive_probe_gpu.py (and what tests/test_adaptive_model.py checks about them) ----------------
# name -> rows x dim, lists, probe; sigma: spread of the rows around their centre; the rules (ratio, min_probe) the GPU tests use
WORLDS = {
    "d128": dict(n=20_000, d=128, k=64, probe=32, sigma=0.6, scale=0.5, seed=31, rules=((1.6, 1), (2.5, 2))),
    "d100": dict(n=5_000, d=100, k=16, probe=16, sigma=0.6, scale=0.5, seed=32, rules=((1.6, 1), (2.5, 2))),
    "k1024": dict(n=30_000, d=64, k=1024, probe=64, sigma=0.5, scale=0.5, seed=33, rules=((1.6, 1), (2.2, 3))),
    "d768": dict(n=4_000, d=768, k=64, probe=24, sigma=0.6, scale=0.5, seed=34, rules=((1.6, 1), (2.5, 2))),
}


def queries_of(centres, nq, sigma, seed):
    """Queries near a centre, between 2 .. 8 centres (their mean, plus noise) and far from every centre (so that all its coarse
    distances are alike), in equal parts and interleaved: the rule's counts then range from 1 to m."""
    rng = np.random.default_rng(seed)
    k, d = centres.shape
    q = np.empty((nq, d), dtype=np.float32)
    for i in range(nq):
        kind = i % 10
        if kind < 3:                                    # near one centre
            q[i] = centres[rng.integers(k)] + 0.3 * sigma * rng.standard_normal(d)
        elif kind < 9:                                  # between j centres, j = 2 .. 8 (never more than there are)
            j = min(k, int(rng.integers(2, 9)))
            q[i] = centres[rng.choice(k, size=j, replace=False)].mean(axis=0) + 0.2 * sigma * rng.standard_normal(d)
        else:                                           # far from all of them
            q[i] = 6.0 * np.abs(centres).max() * rng.standard_normal(d)
    return q


def world(name, nq=600):
    """-> (rows, centres, rotation, queries, spec) of a world; everything seeded."""
    w = WORLDS[name]
    x, centres, _ = synth.mixture(w["n"], w["d"], w["k"], sigma=w["sigma"], seed=w["seed"], centre_seed=w["seed"] + 100, centre_scale=w["scale"])
    P = synth.random_orthogonal((w["d"] + 63) // 64 * 64, seed=w["seed"] + 200)
    return x, centres, P, queries_of(centres, nq, w["sigma"], w["seed"] + 300), w


def oracle_coarse(oidx, queries, probe):
    """The oracle's coarse ranking of every query -> (clusters B x m u32, distances B x m f32)."""
    m = min(probe, oidx.k)
    cl = np.empty((len(queries), m), dtype=np.uint32)
    di = np.empty((len(queries), m), dtype=np.float32)
    for b, q in enumerate(queries):
        cl[b], di[b] = oidx.coarse_rank(oidx.rotate_query(q), probe)
    return cl, di
