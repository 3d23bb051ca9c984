"""fvecs / ivecs / u64vecs / bvecs framing used by the reference's datasets and index directory
(src/utils.rs:280-364): records of [u32 LE count][count x element LE].  Host-side plumbing for
callers that keep their data in those files; the index directory itself is read and written by the
C++ side (rq_load_dir / rq_dump_dir)."""
from __future__ import annotations

import numpy as np


def read_vecs(path, dtype=np.float32) -> list:
    """utils.rs:280-303 (`read_vecs`) / :309-330 (`read_u64_vecs`): a list of 1-D arrays."""
    raw = np.fromfile(path, dtype=np.uint8)
    dtype = np.dtype(dtype)
    out, off = [], 0
    while off + 4 <= raw.size:
        cnt = int(raw[off:off + 4].view("<u4")[0])
        off += 4
        nbytes = cnt * dtype.itemsize
        out.append(raw[off:off + nbytes].view(dtype).copy())
        off += nbytes
    return out


def read_matrix(path, dtype=np.float32) -> np.ndarray:
    """utils.rs:44-49 (`matrix_from_fvecs`): all records have the same length."""
    recs = read_vecs(path, dtype)
    return np.stack(recs) if recs else np.zeros((0, 0), dtype=dtype)


def write_vecs(path, records) -> None:
    """utils.rs:350-364 (`write_vecs`) and :333-347 (`write_matrix`, one record per row)."""
    with open(path, "wb") as f:
        for r in records:
            r = np.ascontiguousarray(r)
            f.write(np.uint32(r.size).tobytes())
            f.write(r.tobytes())


def write_ivecs(path, rows) -> None:
    """n x m integer rows (ids) -> an .ivecs file: records of [u32 LE m][m x i32 LE], one per row (a ground-truth file).
    The format's elements are i32: a uint32 id of 2^31 or more is stored as its two's-complement bit pattern (read it back with
    read_vecs(path, np.int32) and .view(np.uint32))."""
    a = np.asarray(rows)
    if a.ndim != 2 or a.dtype.kind not in "iu":
        raise ValueError("write_ivecs takes a 2-D integer array")
    write_vecs(path, list(a.astype("<i4")))


def read_bvecs(path, dtype=np.uint8) -> np.ndarray:
    """A .bvecs file (SIFT1B / BIGANN): records of [u32 LE dim][dim x one byte], all of the same dim -> n x dim, uint8 (or int8:
    the same bytes read as two's complement).  What RaBitQ.build(rows="u8" / "i8") takes."""
    dtype = np.dtype(dtype)
    if dtype.itemsize != 1:
        raise ValueError(f"a bvecs element is one byte, not {dtype}")
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size == 0:
        return np.zeros((0, 0), dtype=dtype)
    if raw.size < 4:
        raise ValueError(f"{path}: truncated bvecs header")
    d = int(raw[:4].view("<u4")[0])
    if raw.size % (4 + d) != 0:
        raise ValueError(f"{path}: {raw.size} bytes are not a whole number of {4 + d}-byte records")
    recs = raw.reshape(-1, 4 + d)
    if not (recs[:, :4] == recs[0, :4]).all():
        raise ValueError(f"{path}: records of different dimensions")
    return np.ascontiguousarray(recs[:, 4:]).view(dtype)


def write_bvecs(path, rows) -> None:
    """n x d uint8 / int8 rows -> a .bvecs file, one record per row."""
    a = np.ascontiguousarray(rows)
    if a.ndim != 2 or a.dtype.itemsize != 1:
        raise ValueError("write_bvecs takes a 2-D array of one-byte elements")
    out = np.empty((a.shape[0], 4 + a.shape[1]), dtype=np.uint8)
    out[:, :4] = np.frombuffer(np.uint32(a.shape[1]).astype("<u4").tobytes(), dtype=np.uint8)
    out[:, 4:] = a.view(np.uint8)
    out.tofile(path)
