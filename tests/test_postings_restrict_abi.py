"""CPU-side checks of rq_postings_restrict and the filtered exact multi-vector entries (include/rabitq_hip.h, 0.24.0): exports, arity
and the refusals that need no device, as tests/test_maxsim_exact_abi.py checks the unfiltered entries' (a non-null address that is
never dereferenced stands in; the filter is one of them: a null filter is no refusal, it is the unfiltered entry)."""
import ctypes as C

import pytest

from tests.test_maxsim_exact_abi import INVALID, UNSUPPORTED, L  # noqa: F401

NAMES = ["rq_exact_search_maxsim_filtered", "rq_exact_search_maxsim_filtered_device"]


def test_exports_and_arity(L):
    from rabitq_amd import _lib
    for name, arity in [("rq_postings_restrict", 3)] + [(n, 11) for n in NAMES]:
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == arity


@pytest.mark.parametrize("what", ["postings", "filter", "out"])
def test_restrict_refuses_nulls(L, what):
    buf = (C.c_uint8 * 64)()
    junk, out = C.c_void_p(C.addressof(buf)), C.c_void_p()
    got = L.rq_postings_restrict(None if what == "postings" else junk, None if what == "filter" else junk, None if what == "out" else C.byref(out))
    assert got == INVALID and not out.value, (what, L.rq_last_error())


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("filt", ["junk", "null"])
@pytest.mark.parametrize("what,status", [
    ("index", INVALID), ("postings", INVALID), ("params", INVALID), ("tokens", INVALID), ("out", INVALID), ("keys", INVALID),
    ("struct_size", INVALID), ("flags", INVALID), ("doc_stride", INVALID), ("fetch", INVALID), ("T0", INVALID), ("T257", INVALID),
    ("topk0", UNSUPPORTED), ("topk2049", UNSUPPORTED)])
def test_deviceless_refusals(L, name, filt, what, status):
    from rabitq_amd import _lib
    buf = (C.c_uint8 * 64)()
    junk = C.c_void_p(C.addressof(buf))
    bad = {"flags": dict(flags=2), "doc_stride": dict(doc_stride=40), "fetch": dict(fetch=8), "T0": dict(tokens=0), "T257": dict(tokens=257),
           "topk0": dict(topk=0), "topk2049": dict(topk=2049)}.get(what, {})
    prm = _lib.MaxsimParamsT(**{**dict(tokens=32, doc_stride=0, topk=10, fetch=0, flags=0), **bad})
    if what == "struct_size":
        prm.struct_size = 8
    # (idx, postings, filter, tokens, n_tokens, nq, len, params, out_dist, out_keys, out_n)
    got = getattr(L, name)(None if what == "index" else junk, None if what == "postings" else junk, junk if filt == "junk" else None,
                           None if what == "tokens" else junk, None, 2, 64, None if what == "params" else C.byref(prm),
                           None if what == "out" else junk, None if what == "keys" else junk, junk)
    assert got == status, (name, what, L.rq_last_error())
