"""Inputs of the matrix-free coarse ranking tests (test_coarse_fused_gpu.py: coarse_candidates_kernel + refine_candidates_kernel,
rabitq_amd/csrc/kernels_coarse.h), kept apart from the GPU test so that a CPU test (test_coarse_fused_cases.py) can check what the
mixed case exercises.  The other input kinds are those of tests/coarse_cases.py."""
import numpy as np

from tests import coarse_cases

CAND = 256      # RQ_COARSE_CAND: candidate slots of a row
WINDOW = 4      # RQ_FUSED_WINDOW: the bisection stops at any bound that selects nprobe .. nprobe + WINDOW tile keys
BAND = 32       # counts this close to CAND are not trusted: the model uses exact distances, the kernel bf16 approximations

# (d, k, nq, probe, kind): the smallest shapes at which each piece can go wrong -- whole and ragged list / query tiles, both ends of
# the route's list range, every dimension with an instantiation of its own, one and two query tiles per wave (dim <= 128 holds two
# up to 4544 lists, dim 64 up to 4800: launched_shape below; tests/test_kernel_shapes.py checks that the cases launch every shape
# of the kernel's list),
# probe counts 1 / 33 / 64, and the input kinds of coarse_cases at >= 4096 lists
CASES = [(128, 4096, 2048, 64, "mixture"), (128, 4100, 2048 + 37, 64, "mixture"), (128, 8192, 2048, 64, "mixture"),
         (64, 4096, 2048, 33, "mixture"), (64, 4832, 2048, 33, "mixture"), (256, 4096, 2048, 64, "mixture"), (192, 4128, 2050, 64, "mixture"), (128, 4096, 2048, 1, "mixture"),
         (64, 4096, 2100, 33, "ties"), (128, 5000, 2200, 64, "scaled"), (128, 4100, 2100, 40, "nan"), (128, 4096, 2060, 64, "equidistant"),
         (128, 4096, 2048, 64, "mixed")]

# the mixed case: CLUMP near-copies of one centroid (consecutive list ids from CLUMP_AT) beside an ordinary mixture; the first
# NEAR queries are drawn next to the copied centroid -- all CLUMP copies are within the margin of their nprobe-th nearest list, more
# than the slots hold --, the others around ordinary centroids
CLUMP, CLUMP_AT, NEAR = 400, 1000, 12


LDS_PER_BLOCK = 160 * 1024      # RQ_LDS_PER_BLOCK


def launched_shape(d, k, shapes):
    """-> (W, NT) of the coarse_candidates_kernel instantiation the route launches at this shape (launch_coarse_prefiltered,
    host_launch.h): the first of `shapes` (the kernel's (W, NT) list, in its order: two query tiles per wave before one) of this
    width whose two centroid-tile images and tile keys of 4 waves x NT x 32 queries fit in LDS; None: no such shape."""
    W, ntile = d // 64, (k + 31) // 32
    images = 2 * (32 * (64 * W * 2 + 16) + 128)
    return next(((w, nt) for w, nt in shapes if w == W and images + 4 * nt * 32 * ntile * 4 <= LDS_PER_BLOCK), None)


def case(d, k, nq, kind):
    """-> (centres, queries, x) of one case."""
    if kind != "mixed":
        return coarse_cases.prefilter_case(d, k, nq, kind)
    rng = np.random.default_rng(d + k + 1)
    centres = rng.standard_normal((k, d)).astype(np.float32)
    centres[CLUMP_AT:CLUMP_AT + CLUMP] = centres[CLUMP_AT] + 1e-3 * rng.standard_normal((CLUMP, d)).astype(np.float32)
    home = rng.integers(0, k, nq)
    home[(home >= CLUMP_AT) & (home < CLUMP_AT + CLUMP)] = 0
    queries = (centres[home] + 0.5 * rng.standard_normal((nq, d))).astype(np.float32)
    queries[:NEAR] = centres[CLUMP_AT] + 0.05 * rng.standard_normal((NEAR, d)).astype(np.float32)
    x = centres[rng.integers(0, k, 4 * k)] + 0.1 * rng.standard_normal((4 * k, d)).astype(np.float32)
    return centres, queries, x.astype(np.float32)


def model(centres, queries, probe):
    """Candidate counts of the route on exact distances -> (overflows for certain, fits for certain), one bool per row.  Per row the
    kernel bounds the nprobe-th smallest approximate distance by the nprobe-th smallest minimum of the 32-list tiles -- the bisection
    may stop at any bound that selects nprobe .. nprobe + WINDOW tiles -- and takes every list within 2 m of that bound; there is no
    second collect.  Each claim is taken at the end of the window that is worse for it, BAND away from the slot count."""
    c, q = centres.astype(np.float64), queries.astype(np.float64)
    k, d = c.shape
    nq = q.shape[0]
    e = (q * q).sum(1)[:, None] - 2.0 * q @ c.T + (c * c).sum(1)[None, :]            # nq x k exact distances
    ntile = (k + 31) // 32
    assert ntile >= probe                                                              # else the route is not taken
    pad = np.full((nq, ntile * 32 - k), np.inf)
    tmin = np.sort(np.concatenate([e, pad], axis=1).reshape(nq, ntile, 32).min(2), axis=1)
    cmax = np.sqrt((c * c).sum(1).max())
    m = (2.0 ** -8 + (2 * d + 64) * 2.0 ** -24) * 1.05 * (cmax + np.sqrt((q * q).sum(1))) ** 2     # prefilter_bound's m_x
    count = lambda bound: (e <= bound[:, None]).sum(1)
    tight, loose = tmin[:, probe - 1], tmin[:, min(probe + WINDOW, ntile - 1)]
    return count(tight + 2 * m) > CAND + BAND, count(loose + 2 * m) <= CAND - BAND
