"""The CPU model of half-precision rows (include/rabitq_hip.h, "half-precision rows"): the widening W and the rounding R_t of both
row types in numpy, on bit patterns, and the rows a cosine index of half rows stores, built on tests/cosine_model.py.  Nothing here
asks the engine what the answer is.  Not a conftest: import it.

Rows travel as uint16 bit patterns throughout ("f16": IEEE binary16, "bf16": the upper half of an f32)."""
import numpy as np

from tests import cosine_model as cm

TYPES = ("f16", "bf16")
NP_DTYPE = {"f16": np.float16, "bf16": np.uint16}   # what RaBitQ.base_rows returns


def as_bits(h):
    """float16 values or uint16 bit patterns -> uint16 bit patterns."""
    h = np.ascontiguousarray(h)
    return h.view(np.uint16) if h.dtype == np.float16 else h.astype(np.uint16, copy=False)


def widen(h, rows):
    """W: bit patterns -> f32.  f16: the exact IEEE conversion (numpy's); bf16: bits << 16."""
    h = as_bits(h)
    if rows == "f16":
        return h.view(np.float16).astype(np.float32)
    return (h.astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow(x, rows):
    """R_t: f32 -> bit patterns, round to nearest even.  f16: numpy's conversion (subnormal results kept, overflow to inf).
    bf16: r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the f32 bits u of a non-NaN value; a NaN keeps its upper half and stays a NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if rows == "f16":
        with np.errstate(all="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((u[nan] >> np.uint64(16)) | np.where((u[nan] & np.uint64(0xFFFF)) != 0, np.uint64(0x40), np.uint64(0))).astype(np.uint16)
    return r


def nan_patterns(rows):
    """bool[65536]: the bit patterns of the type that are NaNs."""
    h = np.arange(65536, dtype=np.uint32)
    return ((h & 0x7C00) == 0x7C00) & ((h & 0x3FF) != 0) if rows == "f16" else ((h & 0x7F80) == 0x7F80) & ((h & 0x7F) != 0)


def pad_bits(h, dim):
    """n x d bit patterns -> n x dim, the padding +0."""
    h = as_bits(h)
    out = np.zeros((h.shape[0], dim), dtype=np.uint16)
    out[:, :h.shape[1]] = h
    return out


def cosine_stored_bits(oracle, h, rows):
    """The rows a cosine index of the half rows h stores: R_t(N(W(h))), n x ceil64(d) bit patterns."""
    return narrow(cm.normalize_rows(oracle, widen(h, rows)), rows)


def cosine_l2_rows(oracle, h, rows):
    """W(R_t(N(W(h)))): the f32 rows whose L2 index the cosine index of h equals."""
    return widen(cosine_stored_bits(oracle, h, rows), rows)
