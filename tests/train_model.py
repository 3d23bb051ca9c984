"""The CPU model of the centroid trainer's contract (include/rabitq_hip.h, "centroid training with a contract").
Labels and distances come from oracle.kmeans_nearest_cluster on the padded rows, the transforms from the models of the cosine /
inner-product / half / byte tests, the sums are explicit left-to-right f32 loops (np.sum is pairwise: not the contract).  Nothing
here asks the engine what the answer is.  Not a conftest: import it."""
from dataclasses import dataclass

import numpy as np

from tests import byte_model, cosine_model, half_model, ip_model

F32 = np.float32
M64 = (1 << 64) - 1
EPS = F32(2.0 ** -10)
UP, DOWN = F32(1.0) + EPS, F32(1.0) - EPS


def mix64(x):
    """splitmix64's finaliser (rq_mix64) on Python integers."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample_size(n, k, ppc):
    return min(n, max(ppc, 1) * k)


def sample_pos(r, n, ns, seed):
    if ns == n:
        return r
    lo, hi = r * n // ns, (r + 1) * n // ns
    return lo + mix64((seed * 0x100000001B3 + r) & M64) % (hi - lo)


def sample_positions(n, ns, seed):
    return np.array([sample_pos(r, n, ns, seed) for r in range(ns)], dtype=np.int64)


def widen(rows_array, rows):
    """W of a typed base (rows: "f32" / "f16" / "bf16" / "u8" / "i8") -> f32."""
    if rows == "f32":
        return np.ascontiguousarray(rows_array, dtype=np.float32)
    return (byte_model if rows in ("u8", "i8") else half_model).widen(rows_array, rows)


def transform(oracle, x, metric, S=None):
    """step 2 on f32 rows: N(x) / A(x; S) / zero padding, each to the padded length."""
    if metric == "cosine":
        return cosine_model.normalize_rows(oracle, x)
    if metric == "ip":
        return ip_model.augment_rows(oracle, x, S)
    return cosine_model.pad64(x)


@dataclass
class Trained:
    centroids: np.ndarray    # k x cols f32
    objective: np.ndarray    # iters_run f64
    iters_run: int
    sample_rows: int
    splits: int
    positions: np.ndarray    # the sample: rows of the base, ascending
    counts: list             # per iteration, the k member counts before the splits
    labels: np.ndarray       # of the last assignment


def lloyd(oracle, xs, k, iters):
    """steps 3 and 4 on the transformed sample xs (ns x dim f32) -> (padded centroids, objective, iters_run, splits, counts, labels)."""
    ns, dim = xs.shape
    cent = np.stack([xs[j * ns // k] for j in range(k)]).astype(np.float32)
    prev, labels = None, np.zeros(ns, np.int64)
    objective, counts_log, splits, iters_run = [], [], 0, iters
    for t in range(iters):
        labels = np.empty(ns, np.int64)
        dist = np.empty(ns, np.float32)
        for i in range(ns):
            labels[i], dist[i] = oracle.kmeans_nearest_cluster(cent, xs[i])
        if t > 0 and np.array_equal(labels, prev):
            iters_run = t
            break
        prev = labels
        count = [0] * k
        acc = np.zeros((k, dim), np.float32)
        part = [0.0] * k                       # Python floats are f64
        for i in range(ns):                    # ascending sample position: per cluster, strictly left to right
            j = labels[i]
            acc[j] = acc[j] + xs[i]
            part[j] = part[j] + float(dist[i])
            count[j] += 1
        for j in range(k):
            if count[j]:
                cent[j] = acc[j] / F32(count[j])
        obj = 0.0
        for j in range(k):
            obj = obj + part[j]
        objective.append(obj)
        counts_log.append(list(count))
        even = (np.arange(dim) % 2) == 0
        for e in range(k):
            if count[e]:
                continue
            donor = max(range(k), key=lambda j: (count[j], -j))
            if count[donor] < 2:
                continue
            v = cent[donor].copy()
            cent[e] = v * np.where(even, UP, DOWN).astype(np.float32)
            cent[donor] = v * np.where(even, DOWN, UP).astype(np.float32)
            count[e] = count[donor] // 2
            count[donor] -= count[e]
            splits += 1
    return cent, np.array(objective, dtype=np.float64), iters_run, splits, counts_log, labels


def train(oracle, base, k, iters=20, points_per_centroid=256, seed=0, metric="l2", max_sq_norm=None, rows="f32"):
    """The whole contract on a base of any row type.  Raises ValueError where the contract refuses."""
    base = np.asarray(base)
    n, d = base.shape
    if n < k:
        raise ValueError("n < k")
    cols = d + 1 if metric == "ip" else d
    dim = (cols + 63) // 64 * 64
    ns = sample_size(n, k, points_per_centroid)
    if ns * dim > 1 << 31:
        raise ValueError("sample too large")
    S = None
    if metric == "ip":
        S = ip_model.auto_bound(oracle, widen(base, rows)) if max_sq_norm is None else F32(max_sq_norm)
    pos = sample_positions(n, ns, seed)
    w = widen(base[pos], rows)
    if not np.isfinite(w).all():
        raise ValueError("non-finite sample row")
    if metric == "ip" and ip_model.invalid_rows(oracle, w, S).any():
        raise ValueError("a sample row exceeds the bound")
    xs = transform(oracle, w, metric, S)
    cent, obj, iters_run, splits, counts, labels = lloyd(oracle, xs, k, iters)
    return Trained(np.ascontiguousarray(cent[:, :cols]), obj, iters_run, ns, splits, pos, counts, labels)
