"""A seeded, bounded slice of tests/fuzz_features.py inside the suite: mutated, filtered and range-searched indexes of every data
family against the CPU oracle, bit for bit.  The slice must not be able to pass without having tested anything: what it covered
is accumulated from the oracle's answers alone (fuzz_features.Coverage) and asserted at the end; tests/test_fuzz_models.py
replays the same generator without the engine and asserts the same conditions where there is no GPU.

Run on the GPU box:  python -m pytest tests/test_fuzz_features_gpu.py -m gpu -q -s
"""
import os
import time

import pytest

pytestmark = pytest.mark.gpu

SLICE_SEED, SLICE_ROUNDS, SLICE_NMAX = 6, 32, 5000      # (nmax as in test_gpu_parity.py::test_fuzz_slice)


@pytest.fixture(scope="module")
def rq():
    import rabitq_amd
    from rabitq_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "librabitq_hip.so must be built in-tree"
    _lib.check(_lib.lib().rq_init(0))
    return rabitq_amd


def test_feature_fuzz_slice(rq, oracle):
    """SLICE_ROUNDS rounds of fuzz_features.feature_round: after every mutation the arrays, plain and filtered top-k (both
    rankers) and plain and filtered range answers equal the oracle's; once per round after a dump and reload as well.  At the
    end: at least 5 families, 3 dims outside {64, 128}, 2 scales other than 1; at least 3 rounds each with tied distance bits
    inside a range result, an empty range result, a range result beyond 4096 entries whose call re-ran queries, a row the gate
    leaves out (accurate < r <= rough), a filtered top-k answer shorter than topk, an added row with zero residual, a freed id
    given out again; every mutation kind and every filter kind."""
    from tests import fuzz_features as ff
    t0 = time.time()
    cov = ff.run_rounds(rq, oracle, SLICE_SEED, SLICE_ROUNDS, SLICE_NMAX)
    print(f"feature fuzz slice: {SLICE_ROUNDS} rounds in {time.time() - t0:.0f} s; {cov.summary()}")
    cov.check(engine=True)
