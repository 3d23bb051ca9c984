"""CPU-side checks of in-place mutation (rq_add / rq_remove): the header declares the entries and the library exports them, the
Python layer refuses bad shapes and dtypes before it reaches the library, and without a device the entries answer
RQ_ERR_NO_DEVICE (there is no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def test_header_declares_and_library_exports(L):
    from rabitq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rabitq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"rq_status\s+rq_add\s*\(\s*rq_index\s*\*\s*idx\s*,\s*const float\s*\*\s*rows\s*,\s*uint64_t m\s*,\s*uint32_t d\s*,"
                     r"\s*const uint32_t\s*\*\s*ids\s*,\s*int rows_on_device\s*,\s*uint32_t\s*\*\s*out_first_id\s*\)", code)
    assert re.search(r"rq_status\s+rq_remove\s*\(\s*rq_index\s*\*\s*idx\s*,\s*const uint32_t\s*\*\s*id_bits\s*,\s*uint64_t nbits\s*,"
                     r"\s*int bits_on_device\s*,\s*uint64_t\s*\*\s*out_removed\s*\)", code)
    assert "0.7.0" in hdr
    for name in ("rq_add", "rq_remove"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    assert b"0.7.0" in L.rq_version()


def _no_device(L):
    return L.rq_init(0) != 0


def test_entries_without_a_device_say_so(L):
    if not _no_device(L):
        pytest.skip("a device is visible: the device-less answer is not observable here")
    rows = np.zeros((2, 64), dtype=np.float32)
    first = C.c_uint32()
    assert L.rq_add(None, rows.ctypes.data, 2, 64, None, 0, C.byref(first)) == -5
    words = np.ones(1, dtype=np.uint32)
    removed = C.c_uint64()
    assert L.rq_remove(None, words.ctypes.data, 32, 0, C.byref(removed)) == -5


def _fake(dim=128):
    """A RaBitQ whose handle is never used: every refusal must come before the library is called."""
    from rabitq_amd.index import RaBitQ
    r = RaBitQ.__new__(RaBitQ)
    r._h = None
    r.dim, r.k, r.n = dim, 4, 10
    return r


@pytest.mark.parametrize("bad,exc", [
    (np.zeros((3,), np.float32), ValueError),                 # 1-D
    (np.zeros((2, 3, 128), np.float32), ValueError),          # 3-D
    (np.zeros((2, 200), np.float32), "dim"),                  # pads to 256, not 128
    (np.zeros((2, 0), np.float32), "dim"),
    (np.zeros((2, 128), np.complex64), TypeError),
    (np.array([["a"] * 128] * 2), TypeError),
    (np.zeros((2, 128), dtype=object), TypeError),
])
def test_add_rejects_bad_rows_before_the_library(bad, exc, monkeypatch):
    from rabitq_amd import _lib
    from rabitq_amd import index as ix

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(ix, "lib", boom)
    r = _fake()
    if exc == "dim":
        with pytest.raises(_lib.RabitqError) as e:
            r.add(bad)
        assert e.value.status == -2
    else:
        with pytest.raises(exc):
            r.add(bad)


@pytest.mark.parametrize("ids,exc", [
    (np.arange(3), ValueError),                              # 3 ids for 2 rows
    (np.arange(2, dtype=np.float32), TypeError),
    (np.array([[0, 1]]), ValueError),
    (np.array([-1, 2]), ValueError),
    (np.array([0, 1 << 32], dtype=np.int64), ValueError),
])
def test_add_rejects_bad_ids_before_the_library(ids, exc, monkeypatch):
    from rabitq_amd import index as ix

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(ix, "lib", boom)
    with pytest.raises(exc):
        _fake().add(np.zeros((2, 100), np.float32), ids=ids)


@pytest.mark.parametrize("kw,exc", [
    ({}, ValueError),                                        # neither ids nor mask
    ({"ids": [1], "mask": [True]}, ValueError),              # both
    ({"ids": np.array([1.5])}, TypeError),
    ({"ids": np.array([-3])}, ValueError),
    ({"ids": np.array([1 << 33], dtype=np.uint64)}, ValueError),   # past 2^32 bits
])
def test_remove_rejects_bad_ids_before_the_library(kw, exc, monkeypatch):
    from rabitq_amd import index as ix

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(ix, "lib", boom)
    with pytest.raises(exc):
        _fake().remove(**kw)


def test_update_checks_both_arguments_before_removing(monkeypatch):
    from rabitq_amd import index as ix

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(ix, "lib", boom)
    r = _fake()
    with pytest.raises(ValueError):
        r.update(np.array([1, 1]), np.zeros((2, 128), np.float32))     # repeated id
    with pytest.raises(ValueError):
        r.update(np.array([1, 2, 3]), np.zeros((2, 128), np.float32))  # one id per row
    with pytest.raises(ValueError):
        r.update(np.array([1, 2]), np.zeros((128,), np.float32))


def test_mutate_stats_layout_matches_the_header(tmp_path):
    """rq_mutate_stats_t as gcc lays it out from include/rabitq_hip.h == the ctypes mirror."""
    import subprocess
    from rabitq_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "rabitq_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\\n", sizeof(rq_mutate_stats_t), offsetof(rq_mutate_stats_t, ms_keys), offsetof(rq_mutate_stats_t, ms_total),
           offsetof(rq_mutate_stats_t, rows_before), offsetof(rq_mutate_stats_t, gather_bytes));
    return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    M = _lib.MutateStatsT
    assert got == [C.sizeof(M), M.ms_keys.offset, M.ms_total.offset, M.rows_before.offset, M.gather_bytes.offset]


def test_mutate_stats_refuse_an_unset_struct_size(L):
    from rabitq_amd import _lib
    st = _lib.MutateStatsT()
    assert L.rq_last_mutate_stats(C.byref(st)) == 0
    st.struct_size = 0
    assert L.rq_last_mutate_stats(C.byref(st)) == -1
