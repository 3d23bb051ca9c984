"""CPU-side checks of rq_exact_search_keyed_tiered* (include/rabitq_hip.h, 0.25.0): the ctypes mirror lists both with the keyed
entries' twelve arguments, the built library exports them, and the refusals that need no device are made before one is looked for."""
import ctypes as C

import pytest

INVALID = -1
PAIRS = {"rq_exact_search_keyed_tiered": "rq_exact_search_keyed", "rq_exact_search_keyed_tiered_device": "rq_exact_search_keyed_device"}


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("name", list(PAIRS))
def test_exported_with_the_keyed_entry_s_arguments(L, name):
    from rabitq_amd import _lib
    assert name in _lib.EXPORTS
    assert len(getattr(L, name).argtypes) == 12 and getattr(L, name).argtypes == getattr(L, PAIRS[name]).argtypes


@pytest.mark.parametrize("name", list(PAIRS))
def test_null_arguments_are_refused_before_a_device_is_looked_for(L, name):
    buf = (C.c_uint8 * 64)()
    junk = C.c_void_p(C.addressof(buf))   # a non-null address that is never dereferenced: the null argument is checked first
    fn = getattr(L, name)
    assert fn(None, None, None, junk, 1, 64, junk, 10, None, junk, junk, junk) == INVALID      # no index
    assert fn(junk, None, None, junk, 1, 64, junk, 10, None, junk, junk, junk) == INVALID      # no postings
    assert b"null" in L.rq_last_error()
