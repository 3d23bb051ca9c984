"""What the mixed case of the matrix-free coarse ranking test exercises (no GPU): a numpy model of the candidate counts of
coarse_candidates_kernel (rabitq_amd/csrc/kernels_coarse.h) on exact distances."""
import numpy as np

from tests import coarse_fused_cases as cf


def test_mixed_case_overflows_a_few_rows_and_fits_the_rest():
    """The route has one collect and 256 slots per row: a row with more candidates goes to the exact-order fall-back.  The mixed case
    must send a few rows there and keep most on the candidate path, and -- so that the GPU test can pin the fall-back counter -- leave
    no row in the band where exact distances cannot tell.  With these inputs: 21 rows overflow (the 12 drawn next to the clump and 9 ordinary ones near enough to it), 2027 fit."""
    d, k, nq, probe, kind = cf.CASES[-1]
    assert kind == "mixed"
    centres, queries, _ = cf.case(d, k, nq, kind)
    over, fits = cf.model(centres, queries, probe)
    print(f"overflow for certain {int(over.sum())} of {nq} rows, fit for certain {int(fits.sum())}")
    assert over.sum() >= 4, int(over.sum())
    assert fits.sum() >= nq // 2, int(fits.sum())
    assert not (over & fits).any() and (over | fits).all(), np.flatnonzero(~(over | fits))[:10]
    assert over[:cf.NEAR].all()


def test_mixture_rows_fit():
    """The headline mixture at the smallest shape of the route: every row fits for certain (the end-to-end test expects no fall-back)."""
    d, k, nq, probe, kind = cf.CASES[0]
    assert kind == "mixture"
    centres, queries, _ = cf.case(d, k, nq, kind)
    over, fits = cf.model(centres, queries, probe)
    assert fits.all(), int((~fits).sum())
