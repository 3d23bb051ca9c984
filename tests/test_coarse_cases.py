"""What the inputs of the pre-filtered coarse ranking test exercise (no GPU): a numpy model of the candidate counts of the tiled
selection (select_refine_tiled_kernel, rabitq_amd/csrc/kernels_coarse.h) on the case added for its second collect."""
import numpy as np

from tests import coarse_cases

CAND = 256      # RQ_COARSE_CAND: candidate slots of a row
WINDOW = 12     # the loose bisection stops at any bound that selects nprobe .. nprobe + WINDOW keys
BAND = 32       # counts this close to CAND are not trusted: the model uses exact distances, the kernel bf16 approximations


def test_tiled_second_collect_case_takes_the_middle_path():
    """Per row, the kernel (1) bounds the nprobe-th smallest approximate distance by the nprobe-th smallest minimum of the 32-list
    tiles and collects the lists within the margin 2 m of that bound; (2) if those overflow the CAND slots, collects the lists at or
    below the bound itself (the second collect), bisects over THEIR keys for the row's own nprobe-th smallest value and collects
    within 2 m of that; (3) if the second or the third collect overflows as well, hands the row to the exact-order fall-back.
    Every earlier tiled case has dim <= 128, where (1) fits or, for "equidistant", (1) and (2) both fail.  Here most rows must pass
    through (2) and a few must fall back.  Either bisection may stop anywhere in its window, so every count is taken at the end of
    the window that is worse for the claim.  With these inputs: 40 of 64 rows on the middle path, 5 fall back."""
    d, k, nq, probe, kind = coarse_cases.TILED_SECOND_COLLECT
    centres, queries, _ = coarse_cases.prefilter_case(d, k, nq, kind)
    c, q = centres.astype(np.float64), queries.astype(np.float64)
    e = (q * q).sum(1)[:, None] - 2.0 * q @ c.T + (c * c).sum(1)[None, :]            # nq x k exact distances
    ntile = (k + 31) // 32
    assert k % 32 == 0 and ntile >= probe                                             # else the tiled selection is not taken
    tmin = np.sort(e.reshape(nq, ntile, 32).min(2), axis=1)
    es = np.sort(e, axis=1)
    cmax = np.sqrt((c * c).sum(1).max())
    m = (2.0 ** -8 + (2 * d + 64) * 2.0 ** -24) * 1.05 * (cmax + np.sqrt((q * q).sum(1))) ** 2     # prefilter_bound's m_x
    count = lambda bound: (e <= bound[:, None]).sum(1)
    lo_end, hi_end = probe - 1, lambda n: min(probe + WINDOW, n - 1)                  # sorted index of a window's two ends
    # (1) overflows for certain: even the tightest tile bound collects more than CAND + BAND
    first_overflows = count(tmin[:, lo_end] + 2 * m) > CAND + BAND
    # (2) the lists at or below the loosest tile bound fit, and so do those within the margin of the loosest row bound
    below_fits = count(tmin[:, hi_end(ntile)]) <= CAND - BAND
    second_fits = count(es[:, hi_end(k)] + 2 * m) <= CAND - BAND
    # (3) the second collect overflows for certain: more than CAND + BAND lists at or below even the tightest tile bound
    below_overflows = count(tmin[:, lo_end]) > CAND + BAND
    middle = int((first_overflows & below_fits & second_fits).sum())
    fallback = int((first_overflows & below_overflows).sum())
    print(f"middle path {middle} of {nq} rows, fall-back {fallback}")
    assert middle >= 32, middle
    assert fallback >= 4, fallback
