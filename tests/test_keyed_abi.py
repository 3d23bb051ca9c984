"""CPU-side checks of the postings and keyed-search entries (include/rabitq_hip.h, 0.19.0): the refusals that need no device, and
the sized structs as gcc lays them out against the ctypes mirror."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    return _lib.lib()


def test_null_arguments_are_refused_before_a_device_is_looked_for(L):
    from rabitq_amd import _lib
    h, n, buf = C.c_void_p(), C.c_uint64(), (C.c_uint8 * 64)()
    junk = C.c_void_p(C.addressof(buf))   # a non-null address that is never dereferenced: the null argument is checked first
    assert L.rq_postings_create(None, b"tenant", C.byref(h)) == INVALID and not h.value
    assert L.rq_postings_create(junk, b"tenant", None) == INVALID
    assert L.rq_postings_info(None, C.byref(_lib.PostingsInfoT())) == INVALID
    assert L.rq_postings_values(None, None, None, 0) == INVALID
    assert L.rq_postings_counts(None, None, 0, None) == INVALID
    assert L.rq_postings_positions_device(None, 0, None, 0, C.byref(n)) == INVALID
    assert L.rq_exact_search_keyed(None, None, None, junk, 1, 64, junk, 10, None, junk, junk, junk) == INVALID
    assert L.rq_exact_search_keyed_device(junk, None, None, junk, 1, 64, junk, 10, None, junk, junk, junk) == INVALID
    assert b"null" in L.rq_last_error()
    L.rq_postings_free(None)
    assert L.rq_last_keyed_stats(None) == INVALID
    st = _lib.KeyedStatsT()
    st.struct_size = 0
    assert L.rq_last_keyed_stats(C.byref(st)) == INVALID


def test_struct_sizes_match_the_compiled_header(tmp_path):
    from rabitq_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "rabitq_hip.h"
int main(void) {
    printf("%zu %zu %zu\\n", sizeof(rq_postings_info_t), offsetof(rq_postings_info_t, values), offsetof(rq_postings_info_t, bytes));
    printf("%zu %zu %zu %zu\\n", sizeof(rq_keyed_stats_t), offsetof(rq_keyed_stats_t, ms_plan), offsetof(rq_keyed_stats_t, reruns), offsetof(rq_keyed_stats_t, items));
    printf("%zu\\n", sizeof(rq_attr_value_t));
    return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(v) for v in ln.split()] for ln in subprocess.check_output([str(exe)]).decode().splitlines()]
    P, S = _lib.PostingsInfoT, _lib.KeyedStatsT
    assert rows[0] == [C.sizeof(P), P.values.offset, P.bytes.offset] and rows[0][0] == 32
    assert rows[1] == [C.sizeof(S), S.ms_plan.offset, S.reruns.offset, S.items.offset] and rows[1][0] == 80
    assert rows[2] == [C.sizeof(_lib.AttrValue)] == [8]
