"""Inputs for the per-instantiation tests of the exact scan (tests/test_exact_scan_instantiations_gpu.py: exact_scan_kernel<RT, PRE,
RANGE> of rabitq_amd/csrc/kernels_exact.h) and the conditions those tests rely on (tests/test_exact_scan_cases.py), built from
tests/synth.py, the row models and numpy alone: no GPU, no engine.  Not a conftest: import it.

Two kinds of data.  parity_case / typed_case: small clustered mixtures at every tile height of the scan (RT = 4, 2, 1 sub-tiles of 32
rows per block, and 0 = the tile does not fit and the scan runs without its pre-filter) -- three full row tiles and a ragged fourth,
five query tiles.  margin_case: rows and queries on which the scan's bf16 approximation is as wrong as it can be.  On a mixture the
bf16 rounding errors of a product's terms cancel and the approximation stays within a sixth of the margin m the kernel allows
(kernels_exact.h, "Approximation"); a margin half as wide would go unnoticed.  Here every coordinate is s_j (1 + 2^-8 - 2^-20) or twice
that: just below the midpoint of two bf16 values, so bf16 rounds every operand DOWN by almost 2^-8 of itself, every term of <x, q> is
positive, and nothing cancels: the approximation sits 0.88 to 0.94 of m above the exact distance."""
import numpy as np

from tests import byte_model as bm
from tests import half_model as hm
from tests import synth

# ---- the tile table (kernels_exact.h: exact_scan_lds_bytes, exact_scan_subtiles) ------------------------------------------------
LDS_HALF, LDS_MAX = 64 * 1024, 156 * 1024       # two blocks per CU (RT = 4, 2); one block per CU (RT = 1)
DIMS = (64, 192, 256, 448, 512, 2432, 2496)     # the first and last dimension of every tile height, and the first without a tile
NQ_SMALL, NQ = 33, 160                          # one query tile + 1; five query tiles: wave 0 of a block streams two of them
K = 4
QUERY_IS_ROW, QUERY_IS_ZERO = 0, 1


def lds_bytes(rt, dim):
    """Dynamic LDS of exact_scan_kernel<rt> as the header states it: the bf16 tile image (row stride 2 dim + 16 bytes), then |x|^2,
    its scaled root and the admitted flag of every row."""
    return rt * 32 * (2 * dim + 16) + rt * 32 * 12


def expected_rt(dim):
    """32-row sub-tiles per block at this dim; 0 = no tile fits: the scan runs without the pre-filter."""
    if lds_bytes(4, dim) <= LDS_HALF:
        return 4
    if lds_bytes(2, dim) <= LDS_HALF:
        return 2
    return 1 if lds_bytes(1, dim) <= LDS_MAX else 0


def tile_rows(dim):
    """Rows of one block of the scan the fixtures are laid out for (a dim without a tile runs the RT = 4 form of the no-pre-filter scan)."""
    return 32 * (expected_rt(dim) or 4)


def rows_of(dim):
    """Three full row tiles, then a ragged one: one full 32-row sub-tile and five rows of the next."""
    return 3 * tile_rows(dim) + 37


def rotation(dim, seed):
    """P.  Nothing in the exact search reads it; from dim 512 on the identity (a QR of 2432^2 is wasted time)."""
    return np.eye(dim, dtype=np.float32) if dim >= 512 else synth.random_orthogonal(dim, seed=seed)


# ---- mixtures -------------------------------------------------------------------------------------------------------------------
def parity_case(dim):
    """-> dict(x, centres, P, q, n): a clustered mixture of rows_of(dim) rows in K lists and NQ queries of the same mixture; query 0 is
    a stored row, query 1 is zero."""
    n = rows_of(dim)
    x, centres, _ = synth.mixture(n, dim, K, sigma=0.3, seed=4000 + dim, centre_scale=1.0)
    q, _, _ = synth.mixture(NQ, dim, K, sigma=0.3, seed=5000 + dim, centre_scale=1.0)
    q[QUERY_IS_ROW] = x[7]
    q[QUERY_IS_ZERO] = 0.0
    return dict(x=x, centres=centres, P=rotation(dim, 6000 + dim), q=np.ascontiguousarray(q), n=n)


def filters(map_ids, n, rt):
    """name -> bool mask over ids for an index of n rows with these map_ids, laid out on the scan's tiles of 32 rt POSITIONS:
    third: every third id; hole: every row but those of the second tile -- a block with nothing admitted between two live ones (the
    scan's early return); tail: only the ragged last tile; straddle: positions 30 .. 34, across a word boundary of the bitmap."""
    map_ids = np.asarray(map_ids, dtype=np.int64)
    tile = 32 * rt

    def at(positions):
        mask = np.zeros(n, dtype=bool)
        mask[map_ids[positions]] = True
        return mask

    pos = np.arange(n)
    return {"third": np.arange(n) % 3 == 0,
            "hole": at(pos[(pos < tile) | (pos >= 2 * tile)]),
            "tail": at(pos[pos >= (n - 1) // tile * tile]),
            "straddle": at(pos[30:35])}


def typed_case(rows, dim, nq=NQ_SMALL):
    """-> dict(typed, wide, centres, P, q, n): the recipe of test_typed_rows_equal_the_f32_index_of_the_widened_rows at rows_of(dim)
    rows.  typed: what RaBitQ.build(rows=) takes; wide: the same rows widened to f32."""
    n = rows_of(dim)
    seed = 7000 + dim
    if rows in bm.TYPES:
        b, centres, marks = bm.byte_data(rows, n, dim, K, seed=seed)
        wide, q, typed = bm.widen(b, rows), bm.byte_queries(rows, b, marks, nq, dim, K, seed=seed + 1), b
    else:
        x, centres, _ = synth.mixture(n, dim, K, sigma=0.3, seed=seed)
        q, _, _ = synth.mixture(nq, dim, K, sigma=0.3, seed=seed + 1)
        h = hm.narrow(x, rows)
        wide = hm.widen(h, rows)
        typed = h.view(np.float16) if rows == "f16" else h
    return dict(typed=typed, wide=wide, centres=centres, P=rotation(dim, seed + 2), q=np.ascontiguousarray(q), n=n)


# ---- the adversarial fixture ----------------------------------------------------------------------------------------------------
V = np.float32(1.0) + np.float32(2.0 ** -8) - np.float32(2.0 ** -20)    # just below the midpoint of the bf16 values 1 and 1 + 2^-7
MARGIN_DIMS = (128, 448, 768, 2432)
MARGIN_NQ = 32                                                         # one query tile
CLASSES = 9                                                            # rows differ from query 0 in 0 .. 8 coordinates


def margin_case(dim):
    """-> dict(x, centres, P, q, n, cls).  Query 0 is V s for a fixed sign pattern s; row i is query 0 with c_i of its coordinates
    doubled (c_i in 0 .. 8, the coordinates at random); queries 1 .. 31 are query 0 with one to three coordinates doubled.  V and 2 V
    are rounded down by bf16 with the same relative error, almost 2^-8.  cls[b, i] = the number of coordinates in which row i and
    query b differ: their exact distance is cls V^2, so the rows of one class tie (to the rounding of the f32 chain).  Four arbitrary
    centroids that equal no row."""
    n = rows_of(dim)
    rng = np.random.default_rng(8000 + dim)
    s = np.where(rng.random(dim) < 0.5, np.float32(-1.0), np.float32(1.0)).astype(np.float32)

    def doubled(counts):
        mask = np.zeros((len(counts), dim), dtype=bool)
        for i, c in enumerate(counts):
            mask[i, rng.choice(dim, int(c), replace=False)] = True
        return mask

    dx = doubled(rng.integers(0, CLASSES, n))
    dq = doubled(np.concatenate([[0], rng.integers(1, 4, MARGIN_NQ - 1)]))
    x = np.where(dx, np.float32(2.0) * V, V).astype(np.float32) * s
    q = np.where(dq, np.float32(2.0) * V, V).astype(np.float32) * s
    cls = (dq[:, None, :] != dx[None, :, :]).sum(axis=2)
    centres = rng.standard_normal((K, dim)).astype(np.float32)
    return dict(x=np.ascontiguousarray(x), centres=centres, P=np.eye(dim, dtype=np.float32), q=np.ascontiguousarray(q), n=n, cls=cls)


def bf16_round(x):
    """f32 -> the nearest bf16 (ties to even, on the f32 bits), as f32."""
    return hm.widen(hm.narrow(x, "bf16"), "bf16")


def approx_and_margin(x, q, dim):
    """The scan's approximation and margin of every (query, row) pair as the header's comment states them, in float64:
    a = |x|^2 + |q|^2 - 2 <x~, q~> with x~, q~ the operands rounded to bf16, m = (2^-8 + (2 dim + 64) 2^-24) 1.05 (|x| + |q|)^2
    -> (a, m), nq x n each.  For the fixtures' own conditions only: never compared with an engine result."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    assert x.shape[1] == q.shape[1] == dim
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    xn, qn = (x64 * x64).sum(axis=1), (q64 * q64).sum(axis=1)
    dot = bf16_round(q).astype(np.float64) @ bf16_round(x).astype(np.float64).T
    a = xn[None, :] + qn[:, None] - 2.0 * dot
    m = (2.0 ** -8 + (2 * dim + 64) * 2.0 ** -24) * 1.05 * (np.sqrt(xn)[None, :] + np.sqrt(qn)[:, None]) ** 2
    return a, m


def exact64(x, q):
    """|x - q|^2 of every (query, row) pair in float64, nq x n."""
    x64, q64 = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return ((q64[:, None, :] - x64[None, :, :]) ** 2).sum(axis=2)


def class_radii(dist, cls, c):
    """Per query, the f32 just above the largest model distance of the rows of classes <= c (dist: nq x n f32, position-aligned with
    cls); a query without such a row gets half of V^2: below every row that differs from it."""
    big = np.where(cls <= c, dist, np.float32(-1.0)).max(axis=1).astype(np.float32)
    r = np.nextafter(big, np.float32(np.inf))
    return np.where(big < 0, np.float32(0.5) * V * V, r).astype(np.float32)


def cut_inside_class(cls_row, c):
    """A topk whose cut falls in the middle of class c of one query's rows."""
    counts = np.bincount(cls_row, minlength=c + 1)
    assert counts[c] >= 2
    return int(counts[:c].sum() + counts[c] // 2)
