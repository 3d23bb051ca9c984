"""The CPU model of byte rows (include/rabitq_hip.h, "Byte rows"): the widening W of both row types in numpy, the padding of the
stored rows, and the maker of the test data.  Nothing here asks the engine what the answer is.  Not a conftest: import it.

Rows travel as uint8 ("u8") / int8 ("i8") arrays; as_bytes() gives either as raw uint8 for comparisons."""
import numpy as np

from tests import synth

TYPES = ("u8", "i8")
NP_DTYPE = {"u8": np.uint8, "i8": np.int8}   # what RaBitQ.build(rows=) takes and RaBitQ.base_rows returns
RANGE = {"u8": (0, 255), "i8": (-128, 127)}


def as_bytes(b):
    """uint8 / int8 -> the raw bytes as uint8."""
    b = np.ascontiguousarray(b)
    assert b.dtype.itemsize == 1, b.dtype
    return b.view(np.uint8)


def typed(b, rows):
    """raw bytes -> the array type of the row type (the same bytes)."""
    return as_bytes(b).view(NP_DTYPE[rows])


def widen(b, rows):
    """W: u8 -> the integer as f32; i8 -> the two's-complement integer as f32.  Written on the bits, not with astype: bit 7 of an
    i8 pattern weighs -128."""
    u = as_bytes(b).astype(np.int32)
    if rows == "i8":
        u = u - ((u & 0x80) << 1)
    out = np.zeros(u.shape, dtype=np.float32)
    for bit in range(8):   # (every partial sum is a small integer: exact in f32)
        out += ((np.abs(u) >> bit) & 1).astype(np.float32) * np.float32(1 << bit)
    return np.where(u < 0, -out, out).astype(np.float32)


def pad_bits(b, dim):
    """n x d bytes -> n x dim raw bytes, the padding 0x00."""
    b = as_bytes(b)
    out = np.zeros((b.shape[0], dim), dtype=np.uint8)
    out[:, :b.shape[1]] = b
    return out


def scale_into(x, rows):
    """f32 mixture coordinates (roughly N(0, 1)) -> f32 coordinates inside the type's range, not yet rounded: what the centroids and
    the queries of a byte data set are."""
    lo, hi = RANGE[rows]
    return np.clip(x * np.float32(32.0) + np.float32((lo + hi + 1) // 2), lo, hi).astype(np.float32)


def byte_data(rows, n, d, k, seed):
    """-> (b: n x d of the row type, centres: k x d f32, marks).  synth.mixture scaled into the type's range, rounded and clipped,
    with injected rows: all 0; all 255 (i8: -128, 127 alternating); one row repeated three times under different ids; and a block of
    rows drawn from {0, 1} -- integer data makes exact-distance ties dense, which float data never did.  marks: where they are."""
    x, centres, _ = synth.mixture(n, d, k, sigma=0.7, seed=seed, centre_scale=0.6)
    lo, hi = RANGE[rows]
    v = np.rint(scale_into(x, rows)).astype(np.int32)
    rng = np.random.default_rng(seed + 500)
    nblock = min(200, n // 10)
    at = rng.choice(n, size=5 + nblock, replace=False)
    v[at[0]] = 0
    if rows == "u8":
        v[at[1]] = 255
    else:
        v[at[1], 0::2] = -128
        v[at[1], 1::2] = 127
    v[at[3]] = v[at[2]]
    v[at[4]] = v[at[2]]
    v[at[5:]] = rng.integers(0, 2, size=(nblock, d))
    assert v.min() >= lo and v.max() <= hi
    b = np.ascontiguousarray(v.astype(NP_DTYPE[rows]))
    marks = dict(zero=int(at[0]), extreme=int(at[1]), repeated=[int(i) for i in at[2:5]], block=at[5:].copy())
    return b, np.ascontiguousarray(scale_into(centres, rows)), marks


def byte_queries(rows, b, marks, nq, d, k, seed):
    """nq f32 queries for byte_data's rows: the mixture scaled as the rows were (not rounded), and in front four that sit on the
    ties -- the repeated row itself (three ids at distance 0), a row of the {0, 1} block, 0.5 everywhere (every row of the block at
    exactly d / 4) and the all-zero row."""
    q, _, _ = synth.mixture(nq, d, k, sigma=0.7, seed=seed, centre_scale=0.6)
    q = scale_into(q, rows)
    w = widen(b, rows)
    q[0] = w[marks["repeated"][0]]
    if nq >= 4:
        q[1] = w[marks["block"][0]]
        q[2] = np.float32(0.5)
        q[3] = 0.0
    return np.ascontiguousarray(q)
