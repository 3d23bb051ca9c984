"""Inputs for the per-instantiation tests of the two scan kernels (tests/test_scan_instantiations_gpu.py) and the conditions those
tests rely on (tests/test_scan_cases.py), built from tests/synth.py and numpy alone: no GPU, no engine.  Not a conftest: import it.

The data is made so that the FINAL stage of a query pass -- the one that runs on the matrix cores, and the arena stage under
survivor_segments = 2 -- decides part of every answer.  The wide-dimension cases elsewhere in the suite use
synth.mixture(..., sigma=0.8, centre_scale=0.6): at dim >= 192 those clusters do not overlap and no query returns a neighbour from
any list but its nearest (0 of 290 at dim 192 and at dim 1024), so a survivor that the final stage drops goes unnoticed.  With
centre_scale=0.05 the clusters overlap and 290 of 290 queries draw neighbours from several lists."""
import numpy as np

from tests import synth

WIDTHS = (1, 2, 3, 4, 6, 8, 12, 16)     # the fused scan instantiations: dim = 64 W
N, K_LONG, NQ = 9000, 4, 290            # 290 queries: nine full 32-query tiles + 2, so every list meets ten query tiles
SHORT_ROWS = 20                         # the fifth list: shorter than one candidate sub-tile (32 rows)
SIGMA, CENTRE_SCALE = 0.8, 0.05
DEFAULT_CAP = 4096                      # RQ_DEFAULT_CAP (host_plan.h): the uniform survivor capacity per query
QUERY_IS_ROW, QUERY_IS_CENTROID, QUERY_IS_SHORT_CENTROID = 2, 5, 7


def make_case(W):
    """-> x, centres, P, queries for dim = 64 W: four long overlapping lists, a fifth list of SHORT_ROWS rows, a sixth centroid that
    owns no row; queries[2] is a stored row, queries[5] a long list's centroid, queries[7] the short list's."""
    dim = 64 * W
    x, centres, _ = synth.mixture(N, dim, K_LONG, sigma=SIGMA, seed=700 + W, centre_scale=CENTRE_SCALE)
    rng = np.random.default_rng(900 + W)
    # a row of the mixture lies ~ SIGMA sqrt(dim) from every long centroid; the fifth centroid sits twice as far out, so a mixture
    # row would need a 2 sqrt(dim) >= 16 sigma excursion along one direction to be nearer to it than to its own centroid
    u = rng.standard_normal(dim)
    u /= np.linalg.norm(u)
    short_c = (2.0 * SIGMA * np.sqrt(dim) * u).astype(np.float32)
    short_rows = (short_c + 0.05 * SIGMA * rng.standard_normal((SHORT_ROWS, dim))).astype(np.float32)
    far_c = (-50.0 * SIGMA * np.sqrt(dim) * u).astype(np.float32)          # far from all the data: an empty list
    at = rng.choice(N, SHORT_ROWS, replace=False)                          # the short list's rows are spread over the ids
    x[at] = short_rows
    centres = np.ascontiguousarray(np.concatenate([centres, short_c[None], far_c[None]]), dtype=np.float32)
    P = synth.random_orthogonal(dim, seed=800 + W)
    queries, _, _ = synth.mixture(NQ, dim, K_LONG, sigma=SIGMA, seed=1000 + W, centre_scale=CENTRE_SCALE)
    queries[QUERY_IS_ROW] = x[11]
    queries[QUERY_IS_CENTROID] = centres[1]
    queries[QUERY_IS_SHORT_CENTROID] = short_c
    return np.ascontiguousarray(x), centres, P, np.ascontiguousarray(queries)


def make_filters(map_ids, offsets, seed=0):
    """name -> bool mask over ids, for an index with these map_ids / offsets (the oracle's and the engine's are the same arrays):
    half: a random 50 %; lists: the longest list excluded entirely, a random half of every other row -- the pairs of that list
    have nothing admitted."""
    offs = np.asarray(offsets, dtype=np.int64)
    n = int(offs[-1])
    rng = np.random.default_rng(seed)
    half = rng.random(n) < 0.5
    lists = rng.random(n) < 0.5
    c = int(np.argmax(np.diff(offs)))
    lists[np.asarray(map_ids)[offs[c]:offs[c + 1]]] = False
    return {"half": half, "lists": lists}


def final_span(max_list_len, nprobe):
    """Stream positions the final stage of a large-batch pass covers (host_plan.h, plan_stages / plan_pass): the early stages end
    where the threshold has settled, at the longest list's length, and the stream is at most nprobe lists long."""
    return nprobe * max_list_len - max_list_len


def spread(oidx, queries, answers, full=None):
    """Per query, from the oracle alone: (the answer holds a row outside the query's nearest list, the answer holds a row at a stream
    position the final stage scans).  answers: per query the ids returned; oidx: the index that answered (a view of a sub-index for
    a filtered case, `full` then being the whole index: a filtered pass keeps the whole index's stream positions and stage
    boundaries, and skips the lists that admit nothing)."""
    full = oidx if full is None else full
    offs, sub_offs = full.offsets.astype(np.int64), oidx.offsets.astype(np.int64)
    lens = np.diff(offs) * (np.diff(sub_offs) > 0)
    settle = int(np.diff(offs).max())
    pos_of = np.empty(full.n, dtype=np.int64)
    pos_of[full.map_ids] = np.arange(full.n)
    outside, final = [], []
    for q, ids in zip(queries, answers):
        order, _ = full.coarse_rank(full.rotate_query(q), full.k)
        begin = np.zeros(full.k, dtype=np.int64)
        begin[order] = np.concatenate([[0], np.cumsum(lens[order])[:-1]])
        pos = pos_of[np.asarray(ids, dtype=np.int64)]
        lst = np.searchsorted(offs, pos, side="right") - 1
        nearest = int(order[np.nonzero(lens[order] > 0)[0][0]])           # (the nearest list that admits anything)
        outside.append(bool((lst != nearest).any()))
        final.append(bool((begin[lst] + pos - offs[lst] >= settle).any()))
    return np.array(outside), np.array(final)
