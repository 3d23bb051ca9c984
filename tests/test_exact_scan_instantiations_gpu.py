"""Every instantiation of the exact scan (exact_scan_kernel<RT, PRE, RANGE>, rabitq_amd/csrc/kernels_exact.h) against the CPU model:
every tile height (RT = 4, 2, 1 sub-tiles of 32 rows per block, by dimension) and the scan without its pre-filter, in the top-k form
and the range form, with and without a filter, over f32 / f16 / bf16 / u8 / i8 rows -- and the scan's margin on data where its bf16
approximation is as wrong as it can be (tests/exact_scan_cases.py; the fixtures' own conditions: tests/test_exact_scan_cases.py).

Ids, distance bits, counts and lims are compared BIT FOR BIT with tests/exact_model.py / tests/exact_range_model.py; no tolerance
appears.  After every call rq_last_exact_stats must show the form that was meant: scan_subtiles = the RT of the dimension (0 = no
pre-filter), every admitted pair a candidate where the pre-filter did not run, fewer where it did and the data lets it prune.

Run on the GPU box:  python -m pytest tests/test_exact_scan_instantiations_gpu.py -m gpu -q
"""
import contextlib
import os

import numpy as np
import pytest

from tests import exact_model as em
from tests import exact_range_model as erm
from tests import exact_scan_cases as xc
from tests import half_model as hm
from tests.models import bits

pytestmark = pytest.mark.gpu
F32 = np.float32
NO_PREFILTER = 2
BYTES = {"f32": 4, "f16": 2, "bf16": 2, "u8": 1, "i8": 1}


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


# ---- the model's whole ranking, cut ---------------------------------------------------------------------------------------------
def restrict(full, mask):
    """The whole ranking of the rows a filter admits, from the whole ranking of all rows: every query's entries whose id the mask
    admits, in the order they have (every id occurs once per query, so every query keeps the same number)."""
    fd, fi, fc = full
    assert np.all(fc == fd.shape[1])
    keep = np.asarray(mask, dtype=bool)[fi]
    m = int(keep[0].sum())
    assert np.all(keep.sum(axis=1) == m)
    return fd[keep].reshape(len(fd), m), fi[keep].reshape(len(fd), m), np.full(len(fd), m, dtype=np.uint32)


def expect_topk(full, nq, topk):
    """The first nq queries of a whole ranking cut at topk, in RaBitQ.exact_search's layout."""
    fd, fi, fc = full
    w = min(topk, fd.shape[1])
    dist = np.full((nq, topk), np.nan, dtype=np.float32)
    ids = np.full((nq, topk), em.NO_ID, dtype=np.uint32)
    dist[:, :w], ids[:, :w] = fd[:nq, :w], fi[:nq, :w]
    return dist, ids, np.minimum(fc[:nq], topk).astype(np.uint32)


def same_topk(got, want, what):
    (gd, gi, gc), (wd, wi, wc) = got, want
    assert np.array_equal(gc, wc), (what, "counts", gc[:8], wc[:8])
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert bad.size == 0, (what, "ids", int(bad[0]), gi[bad[0]][:12], wi[bad[0]][:12])
    assert np.array_equal(bits(gd), bits(wd)), (what, "distance bits")


def same_range(got, want, what):
    (gl, gd, gi), (wl, wd, wi) = got, want
    assert gl.dtype == np.uint64 and gl[0] == 0 and gd.size == gi.size == int(gl[-1]), what
    assert np.array_equal(gl, wl), (what, "lims", np.diff(gl)[:8], np.diff(wl)[:8])
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, (what, "ids", int(bad[0]), gi[bad[0]:bad[0] + 8], wi[bad[0]:bad[0] + 8])
    assert np.array_equal(bits(gd), bits(wd)), (what, "distance bits")


def check_form(rq, what, rt, pre, nq, admitted, n, dim, rows="f32", prunes=False):
    """The last call ran the form it was meant to.  pre: the pre-filter was asked for (it runs where the dimension has a tile).
    prunes: the data is a mixture and the answer a small part of the admitted rows -- the scan must have dropped pairs."""
    st = rq.last_exact_stats()
    assert st["scan_subtiles"] == (rt if pre else 0), (what, st)
    assert st["scan_launches"] == 1 + st["reruns"], (what, st)
    assert st["row_bytes_read"] == st["scan_launches"] * n * dim * BYTES[rows], (what, st)
    if pre and rt:
        assert st["candidates"] <= nq * admitted, (what, st)
        if prunes:
            assert st["candidates"] < nq * admitted, (what, st)
    else:
        assert st["candidates"] == nq * admitted, (what, st)
    return st


def kth_of(admitted, kth):
    """The neighbour a range radius is taken from: the kth (10th, 200th), or the middle one where fewer rows are admitted."""
    if kth <= 10:
        return min(kth, admitted)
    return kth if admitted >= 2 * kth else max(1, admitted // 2)


def filter_of(g, mask):
    return contextlib.nullcontext(None) if mask is None else g.make_filter(mask=mask)


def run_both_forms(rq, g, full, q, nq, rt, flt, admitted, what, rows="f32", mixture=True, topks=(10, 64), kths=(10, 200)):
    """The top-k form at every topk and the range form at the radii of every kth neighbour, with default parameters and (the top-k
    form, and the range form at the first kth) without the pre-filter, against the whole ranking `full` of the admitted rows."""
    n, dim = g.n, g.dim
    for topk in topks:
        for pre in (True, False):
            got = g.exact_search(q[:nq], topk, filter=flt, params=None if pre else dict(flags=NO_PREFILTER))
            same_topk(got, expect_topk(full, nq, topk), (what, nq, "topk", topk, pre))
            check_form(rq, (what, nq, "topk", topk, pre), rt, pre, nq, admitted, n, dim, rows, prunes=mixture and admitted >= 4 * topk)
    for j, kth in enumerate(kths):
        kth = kth_of(admitted, kth)
        radii = full[0][:nq, kth - 1].copy()
        want = erm.cut_full(full, radii, nq)
        for pre in (True, False)[:2 if j == 0 else 1]:
            got = g.exact_range_search(q[:nq], radii, filter=flt, params=None if pre else dict(flags=NO_PREFILTER))
            same_range(got, want, (what, nq, "range", kth, pre))
            check_form(rq, (what, nq, "range", kth, pre), rt, pre, nq, admitted, n, dim, rows, prunes=mixture and admitted >= 4 * kth)


# ---- f32 rows: every tile height x form x filter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", xc.DIMS)
def test_every_tile_height_and_form(rq, oracle, dim):
    """exact_scan_kernel<RT, PRE, RANGE> for the RT of this dimension (0: only PRE = false exists), PRE true and false, RANGE false
    and true; 33 queries (a ragged second query tile) and 160 (five tiles over four waves); no filter and the four filters of
    exact_scan_cases.filters; at dims 256 and 512 also the range form's arena re-run."""
    c = xc.parity_case(dim)
    n, rt = c["n"], xc.expected_rt(dim)
    g = rq.RaBitQ.build(c["x"], c["centres"], c["P"])
    try:
        assert g.n == n and g.dim == dim
        mids = g.map_ids
        assert np.array_equal(g.base, c["x"][mids])                          # the stored rows are the rows given, in cluster order
        whole = em.exact_batch(oracle, c["x"][mids], mids, em.transformed_queries(oracle, c["q"], "l2", dim), n)
        assert whole[0][xc.QUERY_IS_ROW, 0] == 0.0
        masks = {"none": None, **xc.filters(mids, n, rt or 4)}
        for name, mask in masks.items():
            full = whole if mask is None else restrict(whole, mask)
            admitted = n if mask is None else int(mask.sum())
            with filter_of(g, mask) as f:
                for nq in (xc.NQ_SMALL, xc.NQ):
                    run_both_forms(rq, g, full, c["q"], nq, rt, f, admitted, (dim, name))
        if dim in (256, 512):                                                # one record per query: the launch overflows and runs again
            radii = whole[0][:xc.NQ, 9].copy()
            got = g.exact_range_search(c["q"], radii, params=dict(cand_per_query=1))
            same_range(got, erm.cut_full(whole, radii, xc.NQ), (dim, "arena re-run"))
            assert check_form(rq, (dim, "arena re-run"), rt, True, xc.NQ, n, n, dim, prunes=True)["reruns"] >= 1
    finally:
        g.close()


# ---- typed rows at every tile height ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [192, 448, 512, 2496])
@pytest.mark.parametrize("rows", ["f16", "bf16", "u8", "i8"])
def test_typed_rows_at_every_tile_height(rq, oracle, rows, dim):
    """2-byte and 1-byte rows through the tile load of RT = 4, 2, 1 and through the scan without the pre-filter, both forms, with
    and without a filter, against the model on the widened rows."""
    c = xc.typed_case(rows, dim)
    n, rt = c["n"], xc.expected_rt(dim)
    g = rq.RaBitQ.build(c["typed"], c["centres"], c["P"], rows=rows)
    try:
        assert g.n == n and g.dim == dim and g.row_type == rows
        mids = g.map_ids
        assert np.array_equal(bits(g.base), bits(c["wide"][mids]))           # index.base: the widened rows, in cluster order
        whole = em.exact_batch(oracle, c["wide"][mids], mids, em.transformed_queries(oracle, c["q"], "l2", dim), n)
        third = xc.filters(mids, n, rt or 4)["third"]
        for name, mask in (("none", None), ("third", third)):
            full = whole if mask is None else restrict(whole, mask)
            with filter_of(g, mask) as f:
                run_both_forms(rq, g, full, c["q"], xc.NQ_SMALL, rt, f, n if mask is None else int(mask.sum()), (rows, dim, name),
                               rows=rows, mixture=rows in hm.TYPES)
    finally:
        g.close()


@pytest.mark.parametrize("rows", ["f16", "bf16"])
def test_cosine_half_rows(rq, oracle, rows):
    """A cosine index of half rows at dim 448 (RT = 2): the model runs on the rows the index stores -- normalised, rounded to the row
    type, widened (tests/half_model.py) -- and the normalised queries."""
    dim = 448
    c = xc.typed_case(rows, dim)
    n = c["n"]
    scale = np.random.default_rng(9).uniform(0.5, 2.0, (n, 1)).astype(np.float32)     # norms that the normalisation has to remove
    h = hm.narrow(hm.widen(c["typed"], rows) * scale, rows)
    g = rq.RaBitQ.build(h.view(np.float16) if rows == "f16" else h, c["centres"], c["P"], metric="cosine", rows=rows)
    try:
        mids = g.map_ids
        stored = hm.cosine_l2_rows(oracle, h, rows)[mids]
        assert np.array_equal(bits(g.base), bits(stored))
        whole = em.exact_batch(oracle, stored, mids, em.transformed_queries(oracle, c["q"], "cosine", dim), n)
        run_both_forms(rq, g, whole, c["q"], xc.NQ_SMALL, 2, None, n, ("cosine", rows), rows=rows)
    finally:
        g.close()


# ---- the margin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", xc.MARGIN_DIMS)
def test_margin_holds_where_bf16_is_worst(rq, oracle, dim):
    """margin_case: the approximation of every pair lies 0.88 to 0.94 of the margin above its exact distance, the rows of a class tie,
    and every cut falls among them.  Range form: the radius just above class c's distance returns every row of classes <= c.  Top-k
    form: topk cuts inside a class; with the whole index as the bound's sample the bound is the true topk-th distance, so nothing but
    the margin keeps the rows at the cut.  The pre-filter runs (scan_subtiles = RT); it rightly prunes next to nothing here."""
    c = xc.margin_case(dim)
    n, rt, nq = c["n"], xc.expected_rt(dim), xc.MARGIN_NQ
    g = rq.RaBitQ.build(c["x"], c["centres"], c["P"])
    try:
        assert rt > 0 and g.n == n and g.dim == dim
        mids = g.map_ids
        assert np.array_equal(g.base, c["x"][mids])
        full = em.exact_batch(oracle, c["x"][mids], mids, c["q"], n)
        assert np.all(full[2] == n)
        by_id = np.empty((nq, n), dtype=np.float32)                          # the model's distance of (query, id)
        np.put_along_axis(by_id, full[1].astype(np.int64), full[0], axis=1)
        cls = c["cls"]
        for k in range(1, xc.CLASSES):
            radii = xc.class_radii(by_id, cls, k)
            got = g.exact_range_search(c["q"], radii)
            check_form(rq, (dim, "class", k), rt, True, nq, n, n, dim)
            same_range(got, erm.cut_full(full, radii), (dim, "class", k))
            for b in range(nq):                                              # every row of classes <= k, with its distance bits
                lo, hi = int(got[0][b]), int(got[0][b + 1])
                want_ids = np.flatnonzero(cls[b] <= k)
                assert np.array_equal(np.sort(got[2][lo:hi]), want_ids), (dim, k, b)
                assert np.array_equal(bits(got[1][lo:hi]), bits(by_id[b, got[2][lo:hi]])), (dim, k, b)
        for k in (2, 5):
            topk = xc.cut_inside_class(cls[0], k)
            want = expect_topk(full, nq, topk)
            assert cls[0][want[1][0, topk - 1]] == k and cls[0][full[1][0, topk]] == k      # the cut is inside class k of query 0
            got = g.exact_search(c["q"], topk, params=dict(seed_probe=(n + topk - 1) // topk))
            st = check_form(rq, (dim, "topk", topk, "whole sample"), rt, True, nq, n, n, dim)
            assert st["seed_probe"] == n and st["seed_unfilled"] == 0, st    # the sample is every row: the bound is the topk-th distance
            same_topk(got, want, (dim, "topk", topk, "whole sample"))
            same_topk(g.exact_search(c["q"], topk), want, (dim, "topk", topk, "defaults"))
            check_form(rq, (dim, "topk", topk, "defaults"), rt, True, nq, n, n, dim)
    finally:
        g.close()
