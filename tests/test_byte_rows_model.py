"""Byte rows without a GPU: the numpy model of the widening (tests/byte_model.py) against numpy's own conversion on every pattern,
the header / package mirror of the two new row types, the bvecs framing, and the CPU oracle on the tie-heavy data the GPU tests use.

Run:  python -m pytest tests/test_byte_rows_model.py -m "not gpu" -q
"""
import os
import re

import numpy as np
import pytest

from tests import byte_model as bm
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rows", bm.TYPES)
def test_widening_is_numpys_conversion_on_all_patterns(rows):
    pat = np.arange(256, dtype=np.uint8)
    w = bm.widen(pat, rows)
    assert w.dtype == np.float32
    assert np.array_equal(w.view(np.uint32), bm.typed(pat, rows).astype(np.float32).view(np.uint32))
    lo, hi = bm.RANGE[rows]
    assert (w.min(), w.max()) == (lo, hi) and np.unique(w).size == 256
    # the package takes the names and mirrors the header's values
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"RQ_ROWS_U8\s*=\s*4\s*,\s*RQ_ROWS_I8\s*=\s*5\b", hdr)
    assert (_lib.ROWS_U8, _lib.ROWS_I8) == (4, 5)
    assert _lib.row_type_id(rows) == {"u8": 4, "i8": 5}[rows] and _lib.ROW_TYPE_NAMES[_lib.row_type_id(rows)] == rows
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+4\b", hdr) and _lib.ABI_VERSION == 4


def test_pad_bits():
    b = np.arange(6, dtype=np.int8).reshape(2, 3) - 3
    p = bm.pad_bits(b, 64)
    assert p.shape == (2, 64) and p.dtype == np.uint8
    assert np.array_equal(p[:, :3], b.view(np.uint8)) and not p[:, 3:].any()


@pytest.mark.parametrize("rows", bm.TYPES)
def test_bvecs_round_trip(tmp_path, rows):
    from rabitq_amd import vecs
    b, _, _ = bm.byte_data(rows, 50, 37, 4, seed=3)
    path = str(tmp_path / "x.bvecs")
    vecs.write_bvecs(path, b)
    raw = np.fromfile(path, dtype=np.uint8)
    assert raw.size == 50 * (4 + 37)                                      # a 4-byte little-endian dim, then d bytes per record
    assert raw[:4].tolist() == [37, 0, 0, 0] and raw[41:45].tolist() == [37, 0, 0, 0]
    assert np.array_equal(raw[4:41], bm.as_bytes(b[0]))
    back = vecs.read_bvecs(path, bm.NP_DTYPE[rows])
    assert back.dtype == b.dtype and np.array_equal(back, b)
    assert np.array_equal(vecs.read_bvecs(path), bm.as_bytes(b))         # the default reads uint8
    # the generic record reader sees the same records
    recs = vecs.read_vecs(path, np.uint8)
    assert len(recs) == 50 and np.array_equal(np.stack(recs), bm.as_bytes(b))
    with open(path, "ab") as f:
        f.write(b"\x01")
    with pytest.raises(ValueError):
        vecs.read_bvecs(path)
    empty = str(tmp_path / "empty.bvecs")
    vecs.write_bvecs(empty, np.zeros((0, 8), np.uint8))
    assert vecs.read_bvecs(empty).shape[0] == 0
    with pytest.raises(ValueError):
        vecs.write_bvecs(path, np.zeros((2, 3), np.float32))


@pytest.mark.parametrize("rows", bm.TYPES)
def test_data_maker(rows):
    n, d, k = 3000, 100, 8
    b, centres, marks = bm.byte_data(rows, n, d, k, seed=5)
    assert b.dtype == bm.NP_DTYPE[rows] and b.shape == (n, d) and centres.dtype == np.float32 and centres.shape == (k, d)
    w = bm.widen(b, rows)
    assert not w[marks["zero"]].any()
    if rows == "u8":
        assert (w[marks["extreme"]] == 255).all()
    else:
        assert (w[marks["extreme"], 0::2] == -128).all() and (w[marks["extreme"], 1::2] == 127).all()
    r = marks["repeated"]
    assert len(set(r)) == 3 and np.array_equal(b[r[0]], b[r[1]]) and np.array_equal(b[r[0]], b[r[2]])
    blk = w[marks["block"]]
    assert blk.shape[0] == 200 and set(np.unique(blk).tolist()) == {0.0, 1.0}
    q = bm.byte_queries(rows, b, marks, 16, d, k, seed=6)
    # the ties the data is made for: three ids at distance 0, and every row of the block at exactly d / 4 from the 0.5 query
    assert (((w[r] - q[0]) ** 2).sum(axis=1) == 0).all()
    assert (((blk - q[2]) ** 2).sum(axis=1) == np.float32(d / 4)).all()


@pytest.mark.parametrize("rows", bm.TYPES)
def test_the_oracle_is_deterministic_on_the_tie_heavy_data(oracle, rows):
    """Two builds of the oracle on W(b) hold the same arrays and answer every query -- the tie queries included -- identically."""
    n, d, k = 3000, 100, 8
    b, centres, marks = bm.byte_data(rows, n, d, k, seed=5)
    q = bm.byte_queries(rows, b, marks, 40, d, k, seed=6)
    P = synth.random_orthogonal(128, seed=7)
    wx = bm.widen(b, rows)
    o1 = oracle.OracleIndex.build(wx, centres, P)
    o2 = oracle.OracleIndex.build(wx.copy(), centres.copy(), P.copy())
    try:
        for name in ("base", "codes", "factors", "offsets", "map_ids"):
            assert np.array_equal(np.asarray(getattr(o1, name)).view(np.uint8), np.asarray(getattr(o2, name)).view(np.uint8)), name
        ties = 0
        for heur in (False, True):
            for topk in (1, 10, 100):
                for qi in q:
                    d1, i1 = o1.query(qi, 4, topk, heur)
                    d2, i2 = o2.query(qi, 4, topk, heur)
                    assert np.array_equal(i1, i2) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
                    ties += int(d1.size - np.unique(d1).size)
        assert ties > 0   # the data does what it is made for: results with equal distances
        # the repeated row: the answer of the query that sits on it holds its three ids at distance 0 (in the reference's order, unsorted)
        d1, i1 = o1.query(q[0], 4, 10, False)
        assert set(i1[d1 == 0].tolist()) == set(marks["repeated"])
    finally:
        o1.close()
        o2.close()
