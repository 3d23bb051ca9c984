"""CPU-side checks of the exact multi-vector entries (include/rabitq_hip.h, 0.23.0): exports, arity, struct sizes and the refusals
that need no device -- they come before the index or the postings are read, so a non-null address that is never dereferenced stands in."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -6
NAMES = ["rq_exact_search_maxsim", "rq_exact_search_maxsim_device"]


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def test_exports_arity_and_struct_sizes(L):
    from rabitq_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == 10
    assert "rq_last_maxsim_exact_stats" in _lib.EXPORTS and C.sizeof(_lib.MaxsimExactStatsT) == 80 and C.sizeof(_lib.MaxsimParamsT) == 24
    st = _lib.MaxsimExactStatsT()
    assert L.rq_last_maxsim_exact_stats(C.byref(st)) == 0 and L.rq_last_maxsim_exact_stats(None) == INVALID


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("what,status", [
    ("index", INVALID), ("postings", INVALID), ("params", INVALID), ("tokens", INVALID), ("out", INVALID), ("keys", INVALID),
    ("struct_size", INVALID), ("flags", INVALID), ("doc_stride", INVALID), ("fetch", INVALID), ("T0", INVALID), ("T257", INVALID),
    ("topk0", UNSUPPORTED), ("topk2049", UNSUPPORTED)])
def test_deviceless_refusals(L, name, what, status):
    from rabitq_amd import _lib
    buf = (C.c_uint8 * 64)()
    junk = C.c_void_p(C.addressof(buf))
    bad = {"flags": dict(flags=2), "doc_stride": dict(doc_stride=40), "fetch": dict(fetch=8), "T0": dict(tokens=0), "T257": dict(tokens=257),
           "topk0": dict(topk=0), "topk2049": dict(topk=2049)}.get(what, {})
    prm = _lib.MaxsimParamsT(**{**dict(tokens=32, doc_stride=0, topk=10, fetch=0, flags=0), **bad})
    if what == "struct_size":
        prm.struct_size = 8
    # (idx, postings, tokens, n_tokens, nq, len, params, out_dist, out_keys, out_n)
    got = getattr(L, name)(None if what == "index" else junk, None if what == "postings" else junk, None if what == "tokens" else junk, None,
                           2, 64, None if what == "params" else C.byref(prm), None if what == "out" else junk,
                           None if what == "keys" else junk, junk)
    assert got == status, (name, what, L.rq_last_error())
