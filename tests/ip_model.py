"""The CPU model of the inner-product metric (include/rabitq_hip.h, RQ_METRIC_IP): A(x; S) from the oracle's vector_dot_product,
and the IP oracle = the L2 oracle built on augmented rows and asked zero-extended queries.  Nothing here asks the engine what the
answer is.  Not a conftest: import it."""
import numpy as np

F32 = np.float32


def ip_dim(d):
    return (d + 1 + 63) // 64 * 64


def pad_cols(x, dim):
    """x zero-extended to dim columns: Q(q) for queries, and what the build makes of centroids."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    out = np.zeros((x.shape[0], dim), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def sqnorms(oracle, x):
    """s = vector_dot_product(row, row) of every row, on the row zero-padded to ip_dim(d) -- f32[n]."""
    p = pad_cols(x, ip_dim(np.asarray(x).shape[-1]))
    return np.array([oracle.vector_dot_product(r, r) for r in p], dtype=np.float32)


def invalid_rows(oracle, x, S):
    """bool[n]: rows the contract refuses for the bound S (s not finite, or s > S in f32)."""
    s = sqnorms(oracle, x)
    with np.errstate(all="ignore"):
        return ~(np.isfinite(s) & (s <= F32(S)))


def auto_bound(oracle, x):
    """The automatic S: the largest s of the input, bit for bit (0 for no rows)."""
    s = sqnorms(oracle, x)
    return F32(s.max()) if s.size else F32(0.0)


def augment_rows(oracle, x, S):
    """A(x; S) row by row: x_i bit for bit, slot d = sqrtf(S - s) (one f32 subtraction, a correctly rounded root), zeros after."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    d = x.shape[1]
    out = pad_cols(x, ip_dim(d))
    with np.errstate(all="ignore"):
        out[:, d] = np.sqrt(F32(S) - sqnorms(oracle, x), dtype=np.float32)
    return out


def ip_oracle(oracle, base, centroids, P, S):
    """-> the oracle index an inner-product index of (base, centroids, P, S) must equal."""
    dim = ip_dim(np.asarray(base).shape[1])
    return oracle.OracleIndex.build(augment_rows(oracle, base, S), pad_cols(centroids, dim), P)


def ip_from_dist(oracle, S, queries, dist):
    """ip = 0.5f * ((S + s_q) - D), every operation in f32; dist is nq x topk."""
    c = (F32(S) + sqnorms(oracle, queries)).astype(np.float32)
    return (F32(0.5) * (c[:, None] - np.asarray(dist, dtype=np.float32))).astype(np.float32)


def ip_radius(oracle, S, queries, min_ip):
    """radius = (S + s_q) - 2.0f * min_ip in f32, one per query."""
    c = (F32(S) + sqnorms(oracle, queries)).astype(np.float32)
    return (c - F32(2.0) * np.asarray(min_ip, dtype=np.float32)).astype(np.float32)


def sq_error_bound(dim):
    """Relative bound on s against the exact sum of squares: dim/8 chained FMAs per lane + the 3 adds of the fold, each at most
    2^-24 relative on a sum of non-negative terms (the bound tests/cosine_model.py states for the same chain)."""
    return (dim / 8 + 3) * 2.0 ** -24


def aug_sq_error_bound(dim):
    """|A(x)|^2 against S, relative to S, in exact arithmetic on the f32 row: A_d^2 = (S - s)(1 + e1)(1 + e2)^2 with e1 the
    subtraction's and e2 the root's rounding (each <= 2^-24), so |A|^2 - S = (|x|^2 - s) + (S - s) * (3 * 2^-24 + ...), and
    | |x|^2 - s | <= sq_error_bound * s with s <= S: at most (dim/8 + 3 + 3.01) * 2^-24 of S."""
    return sq_error_bound(dim) + 3.01 * 2.0 ** -24
