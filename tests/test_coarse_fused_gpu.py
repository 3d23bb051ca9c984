"""The coarse ranking without the nq x k matrix of approximate distances (coarse_candidates_kernel + refine_candidates_kernel,
rabitq_amd/csrc/kernels_coarse.h: the automatic route of big batches at 4096 .. 8192 lists, dim <= 256) returns what the other
routes return: list ids and distance bits of every row against the plain exact-order kernels (rq.ops.coarse_rank) and against the
two-kernel pre-filter it replaces (scan_debug bit 65536), with the route of each leg read from the plan trace (scan_debug bit 16384).
The inputs are in tests/coarse_fused_cases.py; tests/test_coarse_fused_cases.py shows on the CPU what the mixed case exercises."""
import re

import numpy as np
import pytest

from tests import coarse_fused_cases as cf
from tests import synth
from tests.test_gpu_parity import rq  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu
TRACE, TWO_KERNELS = 16384, 65536


def _routes(err):
    return re.findall(r"plan: coarse=(\w+)", err)


@pytest.mark.parametrize("d,k,nq,probe,kind", cf.CASES, ids=lambda v: str(v))
def test_fused_route_equals_exact_order_kernels_and_two_kernel_route(rq, capfd, d, k, nq, probe, kind):
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    centres, queries, x = cf.case(d, k, nq, kind)
    idx = rq.RaBitQ.build(x.astype(np.float32), centres, synth.random_orthogonal(d, seed=9))
    _, want_cl, want_cd = rq.ops.coarse_rank(idx, queries, probe)          # the plain exact-order kernels + selection
    q = torch.from_numpy(queries).to(dev)
    try:
        for bits, route in ((0, "prefilter_fused"), (TWO_KERNELS, "prefilter_tiled")):
            ix.set_option("scan_debug", TRACE | bits)
            pc = torch.zeros((nq, probe), device=dev, dtype=torch.int32)
            pdd = torch.zeros((nq, probe), device=dev, dtype=torch.float32)
            capfd.readouterr()
            idx.coarse_topk_device(q.data_ptr(), nq, d, 0, k, probe, pc.data_ptr(), pdd.data_ptr())
            err = capfd.readouterr().err
            assert _routes(err) == [route], (route, err[-1000:])
            got_cl, got_cd = pc.cpu().numpy().view(np.uint32), pdd.cpu().numpy()
            # (the NaN row included: no finite margin, so the row goes to the exact-order fall-back and the block-per-query selection)
            assert np.array_equal(got_cl, want_cl), (route, np.argwhere(got_cl != want_cl)[:5])
            assert np.array_equal(got_cd.view(np.uint32), want_cd.view(np.uint32)), route
    finally:
        ix.set_option("scan_debug", 0)
        idx.close()


@pytest.mark.parametrize("kind", ["mixture", "mixed", "equidistant"])
def test_query_batch_is_the_same_under_both_routes(rq, capfd, kind):
    """query_batch_device at 4096 lists: distances, ids and counts byte for byte under the default options and under bit 65536; the
    fall-back counter of the matrix-free route is 0 on the mixture, the modelled count on the mixed case (the CPU model leaves no row
    of it undecided: test_coarse_fused_cases.py) and every row on the equidistant case."""
    import torch
    from rabitq_amd import index as ix
    dev = torch.device("cuda", 0)
    d, k, nq, probe, topk = 128, 4096, 2048, 64, 10
    centres, queries, x = cf.case(d, k, nq, kind)
    if kind == "mixed":
        over, fits = cf.model(centres, queries, probe)
        assert (over | fits).all()
        want_fallback = int(over.sum())
    else:
        want_fallback = {"mixture": 0, "equidistant": nq}[kind]
    idx = rq.RaBitQ.build(x.astype(np.float32), centres, synth.random_orthogonal(d, seed=9))
    q = torch.from_numpy(queries).to(dev)
    out = {}
    try:
        ix.set_profiling(1)
        for bits, route in ((0, "prefilter_fused"), (TWO_KERNELS, "prefilter_tiled")):
            ix.set_option("scan_debug", TRACE | bits)
            od = torch.zeros((nq, topk), device=dev, dtype=torch.float32)
            oi = torch.zeros((nq, topk), device=dev, dtype=torch.int32)
            on = torch.zeros(nq, device=dev, dtype=torch.int32)
            capfd.readouterr()
            idx.query_batch_device(q.data_ptr(), nq, d, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
            torch.cuda.synchronize()
            err = capfd.readouterr().err
            assert _routes(err) == [route], (route, err[-1000:])
            out[route] = (od.cpu().numpy().tobytes(), oi.cpu().numpy().tobytes(), on.cpu().numpy().tobytes(), ix.last_profile()["coarse_fallback_rows"])
    finally:
        ix.set_profiling(0)
        ix.set_option("scan_debug", 0)
        idx.close()
    with capfd.disabled():
        print(kind, "fall-back rows: fused", out["prefilter_fused"][3], "two kernels", out["prefilter_tiled"][3], "modelled", want_fallback)
    assert out["prefilter_fused"][:3] == out["prefilter_tiled"][:3]
    assert out["prefilter_fused"][3] == want_fallback, (out["prefilter_fused"][3], want_fallback)
