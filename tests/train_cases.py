"""The fixtures of the centroid trainer's GPU tests (tests/test_train_gpu.py): name -> (base, k, points_per_centroid, iters) and
what each one must exercise, checked on the CPU model's own output.  All from tests/synth.mixture with sigma = 0.3.  Not a
conftest: import it."""
import numpy as np

from tests import synth

SIGMA = 0.3
# name: (n, d, k, points_per_centroid, iters)
SHAPES = {
    "A": (3000, 64, 16, 256, 20),      # ns = n, assign_regs_kernel<64>, early stop
    "B": (20_000, 128, 32, 64, 20),    # strata sampling (ns = 2048), assign_regs_kernel<128>
    "C": (5000, 100, 64, 32, 20),      # d padded to 128
    "D": (1600, 64, 16, 256, 20),      # rows 100, 200, 300 = row 0: duplicated initial centroids, three empties at iteration 0
    "E": (3000, 192, 16, 64, 20),      # the generic assign kernel, W = 3
    "F": (8192, 64, 8, 1024, 40),      # a cluster of thousands of members, the iteration cap
    "G": (2000, 768, 8, 64, 20),       # twelve 64-column slabs
}


def base_of(name):
    n, d, k, _, _ = SHAPES[name]
    if name == "F":   # 7000 rows of 0.3 N(0, I) plus 1192 of a 7-centre mixture, shuffled
        rng = np.random.default_rng(61)
        blob = (SIGMA * rng.standard_normal((7000, d))).astype(np.float32)
        mix, _, _ = synth.mixture(1192, d, 7, sigma=SIGMA, seed=62)
        return np.ascontiguousarray(np.concatenate([blob, mix])[rng.permutation(n)])
    # (C's seed: one whose model run has one-member clusters in every iteration, and splits)
    x, _, _ = synth.mixture(n, d, k, sigma=SIGMA, seed=105 if name == "C" else 50 + ord(name))
    if name == "D":
        x[[100, 200, 300]] = x[0]
    return x


def run_model(oracle, name, base=None, **kw):
    """The CPU model's run of a fixture (base: base_of(name) where the caller has it already)."""
    from tests import train_model
    _, _, k, ppc, iters = SHAPES[name]
    return train_model.train(oracle, base_of(name) if base is None else base, k, iters=iters, points_per_centroid=ppc, **kw)
