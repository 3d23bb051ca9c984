"""The CPU model of the exact search (tests/exact_model.py) against float64 numpy brute force, its tie / NaN / inf rules on hand-made
rows, and the boundary: the header declares the entries, the built library exports them, the ctypes mirror has their structs'
layout.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import exact_model, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rq_exact_search", "rq_exact_search_device", "rq_last_exact_stats")


def test_ord32_is_the_oracles(oracle):
    vals = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, 0.5, 2.5e-7, 123456.78],
                    dtype=np.float32)
    rng = np.random.default_rng(3)
    vals = np.concatenate([vals, rng.standard_normal(200).astype(np.float32) * np.float32(1e3)])
    got = exact_model.ord32(vals)
    assert [int(v) for v in got] == [oracle.ord32_from_f32(v) for v in vals]
    order = np.lexsort((~np.signbit(vals), vals))                 # (-0.0 before +0.0: the one pair "<" does not separate)
    assert np.all(np.diff(got[order].astype(np.int64)) >= 0)      # monotone: sorting the keys sorts the floats


@pytest.mark.parametrize("d,topk", [(64, 10), (100, 1), (128, 100)])
def test_model_matches_float64_brute_force(oracle, d, topk):
    n, nq, k = 2000, 24, 16
    x, _, _ = synth.mixture(n, d, k, sigma=0.6, seed=5, centre_scale=0.5)
    q, _, _ = synth.mixture(nq, d, k, sigma=0.6, seed=6, centre_scale=0.5)
    ids_of = np.random.default_rng(1).permutation(n).astype(np.uint32)       # positions are not ids
    base = exact_model.cosine_model.pad64(x)
    qp = exact_model.transformed_queries(oracle, q, "l2", base.shape[1])
    dist, ids, cnt = exact_model.exact_batch(oracle, base, ids_of, qp, topk)
    assert np.all(cnt == topk)
    d64 = ((q[:, None, :].astype(np.float64) - x[None, :, :].astype(np.float64)) ** 2).sum(-1)
    for b in range(nq):
        order = np.argsort(d64[b], kind="stable")
        np.testing.assert_allclose(dist[b], d64[b][order[:topk]], rtol=1e-5)
        gap = (d64[b][order[topk]] - d64[b][order[topk - 1]]) / d64[b][order[topk]]
        if gap > 1e-4:                                                        # not a near-tie at the cut: the sets are equal
            assert set(ids[b].tolist()) == set(ids_of[order[:topk]].tolist())
        assert np.all(np.diff(dist[b].astype(np.float64)) >= 0)


def test_filter_variant_takes_a_mask_over_ids(oracle):
    n, d = 300, 64
    rng = np.random.default_rng(8)
    base = rng.standard_normal((n, d)).astype(np.float32)
    ids_of = (rng.permutation(n) * 3).astype(np.uint32)                       # sparse ids, some past the mask's end
    mask = np.zeros(500, dtype=bool)
    mask[::2] = True
    q = rng.standard_normal((3, d)).astype(np.float32)
    dist, ids, cnt = exact_model.exact_batch(oracle, base, ids_of, q, 400, mask)
    admitted = {int(i) for i in ids_of if i < 500 and mask[i]}
    for b in range(3):
        assert cnt[b] == len(admitted) and set(ids[b, :cnt[b]].tolist()) == admitted
        assert np.all(ids[b, cnt[b]:] == exact_model.NO_ID) and np.all(np.isnan(dist[b, cnt[b]:]))
    none = exact_model.exact_batch(oracle, base, ids_of, q, 5, np.zeros(10, dtype=bool))
    assert np.all(none[2] == 0)


def test_ties_nan_and_inf_rows_by_hand(oracle):
    d = 64
    base = np.zeros((8, d), dtype=np.float32)
    base[0, 0] = 2.0                      # e = 4
    base[1, 0] = 1.0                      # e = 1
    base[2, 1] = 1.0                      # e = 1: an exact tie with row 1
    base[3, 0] = np.nan                   # never returned
    base[4, 0] = np.inf                   # never returned
    base[5, :] = 3.0e19                   # |x|^2 overflows: e = inf, never returned
    base[6, 2] = -1.0                     # e = 1: third member of the tie
    # row 7 is the query itself: e = 0
    ids_of = np.array([10, 7, 3, 1, 0, 2, 5, 9], dtype=np.uint32)
    q = np.zeros(d, dtype=np.float32)
    dist, ids = exact_model.exact_one(oracle, base, ids_of, q, 8)
    assert ids.tolist() == [9, 3, 5, 7, 10]                                  # the tie at e = 1 goes by id; NaN / inf rows are absent
    assert dist.tolist() == [0.0, 1.0, 1.0, 1.0, 4.0]
    dist, ids = exact_model.exact_one(oracle, base, ids_of, q, 2)            # the cut falls inside the tie: the lower id stays
    assert ids.tolist() == [9, 3]
    # -0.0 sorts before +0.0 under Ord32, and a distance is never negative: the keys of 0.0 are the smallest
    assert exact_model.ord32(np.float32([0.0]))[0] == 0
    # a row at exactly f32::MAX is out ("below f32::MAX")
    big = np.zeros((1, d), dtype=np.float32)
    big[0, 0] = np.sqrt(exact_model.F32_MAX, dtype=np.float32)
    e = oracle.l2_squared_distance_rows(q, big, [0])
    got = exact_model.exact_one(oracle, big, np.uint32([0]), q, 1)[0]
    assert got.size == (1 if e[0] < exact_model.F32_MAX else 0)


def test_transformed_queries_follow_the_metric(oracle):
    q = np.arange(1, 101, dtype=np.float32)[None, :] / 7
    l2 = exact_model.transformed_queries(oracle, q, "l2", 128)
    assert l2.shape == (1, 128) and np.array_equal(l2[0, :100], q[0]) and not l2[0, 100:].any()
    cs = exact_model.transformed_queries(oracle, q, "cosine", 128)
    assert abs(float(np.linalg.norm(cs[0].astype(np.float64))) - 1.0) < 1e-5
    ip = exact_model.transformed_queries(oracle, q[:, :64], "ip", 128)
    assert ip.shape == (1, 128) and np.array_equal(ip[0, :64], q[0, :64]) and not ip[0, 64:].any()


def test_header_declares_and_library_exports_the_entries():
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\brq_status\s+%s\s*\(" % name, plain), name
        assert name in _lib.EXPORTS
    assert "rq_exact_params_t" in plain and "rq_exact_stats_t" in plain
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+4\b", plain)              # additions only
    _lib.build()
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name


def test_exact_structs_match_the_compiled_header(tmp_path):
    from rabitq_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "rabitq_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu\\n", sizeof(rq_exact_params_t), offsetof(rq_exact_params_t, seed_probe), offsetof(rq_exact_params_t, cand_per_query), offsetof(rq_exact_params_t, flags));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rq_exact_stats_t), offsetof(rq_exact_stats_t, ms_seed), offsetof(rq_exact_stats_t, seed_unfilled),
           offsetof(rq_exact_stats_t, reruns), offsetof(rq_exact_stats_t, candidates), offsetof(rq_exact_stats_t, row_bytes_read), offsetof(rq_exact_stats_t, scan_launches),
           offsetof(rq_exact_stats_t, scan_subtiles));
    return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(v) for v in ln.split()] for ln in subprocess.check_output([str(exe)]).decode().splitlines()]
    P, S = _lib.ExactParamsT, _lib.ExactStatsT
    assert rows[0] == [C.sizeof(P), P.seed_probe.offset, P.cand_per_query.offset, P.flags.offset]
    assert rows[1] == [C.sizeof(S), S.ms_seed.offset, S.seed_unfilled.offset, S.reruns.offset, S.candidates.offset,
                       S.row_bytes_read.offset, S.scan_launches.offset, S.scan_subtiles.offset]
    assert S.scan_subtiles.offset == 60 and C.sizeof(S) == 64                # the word that was reserved0: the layout did not move


def test_write_ivecs_roundtrip(tmp_path):
    from rabitq_amd import vecs
    ids = np.arange(12, dtype=np.uint32).reshape(3, 4)
    p = str(tmp_path / "t.ivecs")
    vecs.write_ivecs(p, ids)
    back = vecs.read_vecs(p, np.int32)
    assert len(back) == 3 and all(np.array_equal(back[i], ids[i].astype(np.int32)) for i in range(3))
    with pytest.raises(ValueError):
        vecs.write_ivecs(p, np.zeros((2, 2), dtype=np.float32))


def test_cli_has_the_make_truth_flag():
    from rabitq_amd import cli
    ap = cli.build_parser()
    base = ["-b", "b", "-c", "c", "-q", "q", "-t", "t", "-s", "s"]
    assert ap.parse_args(base).make_truth is False
    assert ap.parse_args(base + ["--make-truth"]).make_truth is True
