"""CPU-side checks of the MaxSim-by-postings entries (include/rabitq_hip.h, 0.21.0): exports, arity, and the refusals that need
no device -- they come before the index or the postings are read, so a non-null address that is never dereferenced stands in."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -6
NAMES = ["rq_maxsim_scores_keyed", "rq_maxsim_scores_keyed_device", "rq_query_batch_maxsim_keyed", "rq_query_batch_maxsim_keyed_device"]


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def test_exports_and_arity(L):
    from rabitq_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == (12 if "scores" in name else 14)


WHATS = [("index", INVALID), ("postings", INVALID), ("params", INVALID), ("tokens", INVALID), ("out", INVALID), ("keys", INVALID),
         ("struct_size", INVALID), ("flags", INVALID), ("doc_stride", INVALID), ("T0", INVALID), ("T257", INVALID), ("topk0", UNSUPPORTED),
         ("topk2049", UNSUPPORTED), ("source", UNSUPPORTED)]
# (topk and fetch are not read by the scoring entries)
CASES = [(n, w, s) for n in NAMES for w, s in WHATS if not ("scores" in n and w in ("topk0", "topk2049", "source"))]


@pytest.mark.parametrize("name,what,status", CASES)
def test_deviceless_refusals(L, name, what, status):
    buf = (C.c_uint8 * 64)()
    junk = C.c_void_p(C.addressof(buf))
    scores = "scores" in name
    from rabitq_amd import _lib
    bad = {"flags": dict(flags=2), "doc_stride": dict(doc_stride=40), "T0": dict(tokens=0), "T257": dict(tokens=257),
           "topk0": dict(topk=0), "topk2049": dict(topk=2049), "source": dict(fetch=65)}.get(what, {})
    prm = _lib.MaxsimParamsT(**{**dict(tokens=32, doc_stride=0, topk=10, fetch=8, flags=0), **bad})
    if what == "struct_size":
        prm.struct_size = 8
    pp = None if what == "params" else C.byref(prm)
    idx, post = (None if what == "index" else junk), (None if what == "postings" else junk)
    tok = None if what == "tokens" else junk
    if scores:       # (idx, postings, tokens, n_tokens, nq, len, keys, cand_n, ncand, params, out_score, out_rows)
        got = getattr(L, name)(idx, post, tok, None, 2, 64, None if what == "keys" else junk, None, 3, pp, None if what == "out" else junk, junk)
    else:            # (idx, postings, filter, tokens, n_tokens, nq, len, probe, heuristic, params, out_dist, out_keys, out_n, out_candidates)
        got = getattr(L, name)(idx, post, None, tok, None, 2, 64, 4, 0, pp, junk, None if what in ("out", "keys") else junk, junk, None)
    assert got == status, (name, what, L.rq_last_error())
