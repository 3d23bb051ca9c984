"""Inputs of the pre-filtered coarse ranking tests (test_gpu_parity.test_prefiltered_coarse_ranking_equals_exact_order_kernels),
kept apart from the GPU test so that a CPU test (test_coarse_cases.py) can check what the inputs exercise."""
import numpy as np

# cases: (d, k, nq, probe, kind)
# a margin wide enough (dim 768) that the tile bound's candidates overflow the 256 slots while those of the row's own nprobe-th
# smallest value fit: the tiled selection's second collect and the bisection over collected keys (test_coarse_cases.py)
TILED_SECOND_COLLECT = (768, 1536, 64, 48, "mixture")
PREFILTER_CASES = [(128, 4096, 3000, 64, "mixture"), (128, 300, 2500, 64, "mixture"), (64, 1000, 2100, 33, "ties"),
                   (256, 700, 2100, 64, "equidistant"), (768, 260, 2100, 20, "mixture"),
                   (128, 5000, 2200, 64, "scaled"), (128, 130, 2100, 1, "nan"),
                   # more lists than one wave holds in registers (the ranking of a multi-GPU deployment is over
                   # all shards' lists): the tile-minima selection, its per-row fall-back included
                   (128, 9000, 2100, 64, "mixture"), (64, 33000, 2050, 33, "mixture"), (128, 20000, 2100, 64, "ties"),
                   (128, 10000, 2060, 64, "equidistant"), (128, 8300, 2100, 40, "nan"), (128, 16500, 2100, 64, "scaled"),
                   (64, 40001, 2050, 64, "mixture"), TILED_SECOND_COLLECT]


def prefilter_case(d, k, nq, kind):
    """-> (centres, queries, x) of one case.
    ties: duplicate centroids (exact ties at the selection threshold); equidistant: centroids on a sphere around the queries (more
    candidates than the refinement holds: the in-kernel exact fall-back); scaled: coordinates x 3e3; nan: a NaN query."""
    rng = np.random.default_rng(d + k)
    centres = rng.standard_normal((k, d)).astype(np.float32)
    queries = (centres[rng.integers(0, k, nq)] + 0.5 * rng.standard_normal((nq, d))).astype(np.float32)
    if kind == "ties":
        centres[k // 2:] = centres[: k - k // 2]            # every centroid twice
    elif kind == "equidistant":
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)
        queries = (1e-3 * rng.standard_normal((nq, d))).astype(np.float32)   # all lists at distance ~1: hundreds within the margin
    elif kind == "scaled":
        centres *= np.float32(3e3)
        queries *= np.float32(3e3)
    elif kind == "nan":
        queries[5, 3] = np.nan
    x = centres[rng.integers(0, k, 4 * k)] + 0.1 * rng.standard_normal((4 * k, d)).astype(np.float32)
    return centres, queries, x.astype(np.float32)
