"""tests/adaptive_model.py: the properties of the rule's numpy statement, and that the data of tests/test_adaptive_probe_gpu.py
makes the rule cut unevenly (otherwise the GPU tests would only show uniform cuts).  No GPU needed."""
import numpy as np
import pytest

from tests import adaptive_model as am

F32 = np.float32


def rows(*r):
    return np.array(r, dtype=F32)


def test_prefix_not_count():
    """The cut is the longest PREFIX under the threshold: an entry over it ends the prefix even if later ones are under it again
    (rows are ascending in the engine; the model does not rely on it)."""
    d = rows([1, 1.5, 3, 1.2, 1.1], [1, 1, 1, 1, 1], [2, 5, 6, 7, 8])
    assert am.probe_counts(d, 2.0).tolist() == [2, 5, 1]
    assert am.probe_counts(d, 1.0).tolist() == [1, 5, 1]      # d_0 <= 1 * d_0 always holds for a finite d_0


def test_threshold_is_one_f32_multiplication():
    """t = f32(ratio) * d_0 rounded to f32: an entry one ulp above it is cut, the entry equal to it is kept."""
    d0 = F32(3.1234567)
    ratio = F32(1.7)
    t = F32(ratio * d0)
    assert t == F32(np.float64(ratio) * np.float64(d0))        # (the f64 product of two f32 rounds once)
    d = rows([d0, t, np.nextafter(t, F32(np.inf))], [d0, np.nextafter(t, F32(0)), t])
    assert am.probe_counts(d, float(ratio)).tolist() == [2, 3]


def test_min_probe_and_caps_and_clamps():
    d = rows([1, 2, 3, 4, 5, 6], [1, 1, 1, 1, 9, 9], [1, 9, 9, 9, 9, 9])
    assert am.probe_counts(d, 3.0).tolist() == [3, 4, 1]
    assert am.probe_counts(d, 3.0, min_probe=2).tolist() == [3, 4, 2]
    assert am.probe_counts(d, 3.0, min_probe=100).tolist() == [6, 6, 6]             # min_probe >= m: nothing is cut
    assert am.probe_counts(d, 3.0, caps=[2, 100, 0]).tolist() == [2, 4, 1]          # caps are clamped to [1, m]
    assert am.probe_counts(d, 3.0, min_probe=5, caps=[2, 3, 6]).tolist() == [2, 3, 5]   # the cap wins over min_probe
    assert am.probe_counts(d, np.inf, caps=[1, 4, 6]).tolist() == [1, 4, 6]         # per-query nprobe
    assert am.probe_counts(d, 0.0).tolist() == [1, 1, 1]                            # never below 1
    assert am.probe_counts(d[:, :1], 5.0, min_probe=3, caps=[7, 7, 7]).tolist() == [1, 1, 1]   # m = 1


def test_ratio_inf_cuts_nothing():
    d = rows([1, 2, 3], [0, 0, 5], [0, 1, np.inf])
    assert am.probe_counts(d, np.inf).tolist() == [3, 3, 3]
    assert am.probe_counts(d, np.inf, min_probe=2).tolist() == [3, 3, 3]


def test_d0_zero():
    """d_0 = 0: t = 0 for every finite ratio, the prefix is the run of zeros."""
    d = rows([0, 0, 1e-30, 1], [0, 1, 2, 3])
    assert am.probe_counts(d, 1e30).tolist() == [2, 1]
    assert am.probe_counts(d, 2.0, min_probe=3).tolist() == [3, 3]


def test_nan_gives_min_probe():
    """A NaN compares false: a row of NaNs (a query holding a NaN) has an empty prefix at every ratio, +inf included."""
    nan = np.nan
    d = rows([nan, nan, nan, nan], [1, nan, 1, 1], [1, 1.5, nan, 1])
    assert am.probe_counts(d, 2.0).tolist() == [1, 1, 2]
    assert am.probe_counts(d, np.inf, min_probe=3).tolist() == [3, 3, 3]
    assert am.probe_counts(d, np.inf).tolist() == [1, 1, 2]
    assert am.probe_counts(d, 2.0, min_probe=2, caps=[1, 4, 4]).tolist() == [1, 2, 2]


def test_overflowing_threshold():
    """ratio * d_0 beyond f32::MAX is +inf: everything finite (and +inf) is under it."""
    d = rows([1e30, 2e30, 3e38, np.inf])
    assert am.probe_counts(d, 1e30).tolist() == [4]


@pytest.mark.parametrize("name", sorted(am.WORLDS))
def test_gpu_worlds_cut_unevenly(oracle, name):
    """For every world and rule of the GPU file: the counts the model derives from the oracle's coarse distances take at least four
    distinct values, min_probe and m among them.  (The coarse ranking reads the centroids and the rotation only: the oracle index
    here holds a few rows of the world, its coarse distances are those of the whole world.)"""
    x, centres, P, queries, w = am.world(name)
    oidx = oracle.OracleIndex.build(x[:4 * w["k"]], centres, P)
    try:
        _, dist = am.oracle_coarse(oidx, queries, w["probe"])
    finally:
        oidx.close()
    m = min(w["probe"], w["k"])
    assert dist.shape == (len(queries), m) and len(queries) >= 500
    assert (np.diff(dist, axis=1) >= 0).all()
    for ratio, min_probe in w["rules"]:
        n = am.probe_counts(dist, ratio, min_probe)
        vals = set(n.tolist())
        assert len(vals) >= 4 and min_probe in vals and m in vals, (name, ratio, min_probe, sorted(vals))
