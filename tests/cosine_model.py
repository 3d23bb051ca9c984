"""The CPU model of the cosine metric: N(x) from the oracle's vector_dot_product, and the cosine oracle = the L2 oracle built on
normalised rows and asked normalised queries.  Nothing here asks the engine what the answer is.  Not a conftest: import it."""
import numpy as np

FLT_MIN = np.float32(np.finfo(np.float32).tiny)   # smallest normal f32


def pad64(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    dim = (x.shape[1] + 63) // 64 * 64
    out = np.zeros((x.shape[0], dim), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def normalize_rows(oracle, x):
    """N(x) row by row (include/rabitq_hip.h): pad, s = oracle.vector_dot_product(row, row), nrm = sqrt(s) in f32, row / nrm in f32
    where nrm is a normal number, the row itself otherwise."""
    p = pad64(x)
    out = p.copy()
    with np.errstate(all="ignore"):
        for i, row in enumerate(p):
            s = np.float32(oracle.vector_dot_product(row, row))
            nrm = np.sqrt(s, dtype=np.float32)
            if np.isfinite(nrm) and nrm >= FLT_MIN:
                out[i] = row / nrm
    return out


def cosine_oracle(oracle, base, centroids, P):
    """-> the oracle index a cosine index of (base, centroids, P) must equal."""
    return oracle.OracleIndex.build(normalize_rows(oracle, base), pad64(centroids), P)   # (zero-padded centroids: what the build makes of them)


def unit_error_bound(dim):
    """|N(x)| - 1 relative bound of the normalisation alone: dim/8 chained FMAs per lane + 3 adds of the fold (each <= 2^-24
    relative on a sum of non-negative terms), half of it through the square root, + sqrt's and the division's own roundings:
    <= (dim/8 + 3) * 2^-24 as include/rabitq_hip.h's contract states it."""
    return (dim / 8 + 3) * 2.0 ** -24
