"""Filtered small batches and filtered tickets, the part that needs no GPU: the new export is declared, exported and mirrored,
it refuses a NULL out_ticket before any device work, and the option "small_batch_filtered" takes 0, 1 and 2 only."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rq_query_batch_device_begin_filtered"


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def test_export_is_declared_exported_and_mirrored(L):
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, code)
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    assert "#define RQ_ABI_VERSION 4" in hdr and L.rq_abi_version() == 4 and "rq_query_batch_device_begin_filtered, option" in hdr
    # the unfiltered _begin's signature with `const rq_filter *filter` after the index
    sig = lambda n: re.sub(r"\s+", "", re.search(r"rq_status %s\((.*?)\);" % n, code, flags=re.S).group(1))
    assert sig(NAME).replace("constrq_filter*filter,", "") == sig("rq_query_batch_device_begin")
    assert len(getattr(L, NAME).argtypes) == len(L.rq_query_batch_device_begin.argtypes) + 1


def test_null_out_ticket_is_refused_before_any_device_work(L):
    # (no index, no filter, no device: the ticket pointer is looked at first)
    assert getattr(L, NAME)(None, None, None, 1, 64, 1, 1, 0, None, None, None, None) == -1
    assert b"null" in L.rq_last_error()
    assert L.rq_query_batch_device_begin(None, None, 1, 64, 1, 1, 0, None, None, None, None) == -1


def test_option_values(L):
    try:
        for v in (0, 1, 2):
            assert L.rq_set_option(b"small_batch_filtered", v) == 0, v
        for v in (3, -1):
            assert L.rq_set_option(b"small_batch_filtered", v) == -1, v
    finally:
        assert L.rq_set_option(b"small_batch_filtered", 1) == 0


def test_python_begin_takes_a_filter():
    import inspect
    from rabitq_amd.index import RaBitQ
    p = inspect.signature(RaBitQ.query_batch_device_begin).parameters
    assert "filter" in p and p["filter"].default is None
