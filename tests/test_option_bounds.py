"""Every option's bounds and refusal text, through rq_set_option itself (no GPU: the call stores a value and touches no device).

For each option: the lowest and the highest accepted value are taken, one below and one above are refused with the exact message,
and the options whose rule is not a plain range -- stage_growth, survivor_segments, scan_debug, max_scan_blocks -- are probed at
their special values.  The bounds and the messages are written out here, not read from the source: they are the library's
behaviour as it shipped, and the option table of rabitq_amd/csrc/host_options.h has to reproduce them.  The shipped library is the
ordinary build, so the developer-only values are refused.
"""
import pytest

from tests import option_cases as oc

OK, INVALID = 0, -1
INT_MAX = 2 ** 31 - 1

# name -> (lowest accepted, highest accepted or None where only the lower side is bounded, the refusal's text)
BOUNDS = {
    "scan_impl": (0, 2, "scan_impl must be 0 (auto), 1 (valu) or 2 (mfma)"),
    "cluster_major_div": (1, 4096, "cluster_major_div must be in [1, 4096]"),
    "large_batch_from": (2, 1 << 20, "large_batch_from must be in [2, 2^20]"),
    "stage_settle_pct": (1, 400, "stage_settle_pct must be in [1, 400]"),
    "stage_growth": (0, 64, "stage_growth must be 0 or in [2, 64]"),
    "base_device_mb": (-1, None, "base_device_mb must be >= -1"),
    "pass_overlap": (0, 1, "pass_overlap must be 0 or 1"),
    "split_rows": (0, 2, "split_rows must be 0, 1 or 2"),
    "scan_tile_table": (0, 2, "scan_tile_table must be 0 (never), 1 (auto) or 2 (always)"),
    "max_scan_blocks": (0, None, "max_scan_blocks must be >= 0"),
    "pair_split": (0, 1, "pair_split must be 0 or 1"),
    "coarse_tiled_from": (0, None, "coarse_tiled_from must be >= 0"),
    "coarse_impl": (0, 4, "coarse_impl must be 0, 1, 2, 3 or 4"),
    "survivor_segments": (0, 2, "survivor_segments must be 0, 1 or 2"),
    "assign_impl": (0, 1, "assign_impl must be 0 or 1"),
    "small_batch_span": (1, None, "small_batch_span must be >= 1"),
    "small_batch": (0, 1, "small_batch must be 0 or 1"),
    "small_batch_filtered": (0, 2, "small_batch_filtered must be 0, 1 or 2"),
    "dense_dir": (0, 1, "dense_dir must be 0 or 1"),
    "shared_thresholds": (0, 2, "shared_thresholds must be 0, 1 or 2"),
    "group_rank": (0, 2, "group_rank must be 0, 1 or 2"),
    "prep_placement": (0, 1, "prep_placement must be 0 or 1"),
    "rerank_shadow": (0, 2, "rerank_shadow must be 0 (never), 1 (fp16 rows when they fit) or 2 (8-bit rows when they fit)"),
    "scan_gate": (0, 2, "scan_gate must be 0, 1 or 2"),
}
SCAN_DEBUG_BITS = 128 | 512 | 2048 | 4096 | 16384 | 32768 | 65536
SCAN_DEBUG_TEXT = "scan_debug: this bit exists in the developer build only (librabitq_hip_dev.so)"
SEGMENTS_3_TEXT = "survivor_segments = 3 (allocation-failure injection) exists in the developer build only (make dev)"


@pytest.fixture(scope="module")
def L():
    from rabitq_amd import _lib
    _lib.build()
    lib = _lib.lib()
    try:
        yield lib
    finally:
        for name, v in oc.DEFAULTS.items():
            assert lib.rq_set_option(name.encode(), v) == OK, name


def taken(L, name, value):
    assert L.rq_set_option(name.encode(), value) == OK, (name, value, L.rq_last_error())


def refused(L, name, value, text):
    assert L.rq_set_option(None if name is None else name.encode(), value) == INVALID, (name, value)
    assert L.rq_last_error().decode() == text, (name, value)


def test_the_table_here_names_every_option():
    assert set(BOUNDS) | {"scan_debug"} == set(oc.DEFAULTS)
    for name, (lo, hi, _) in BOUNDS.items():
        assert lo <= oc.DEFAULTS[name] <= (INT_MAX if hi is None else hi), name


@pytest.mark.parametrize("name", sorted(BOUNDS))
def test_bounds(L, name):
    lo, hi, text = BOUNDS[name]
    try:
        taken(L, name, lo)
        taken(L, name, INT_MAX if hi is None else hi)
        refused(L, name, lo - 1, text)
        refused(L, name, -INT_MAX - 1, text)
        if hi is not None and name != "survivor_segments":     # (its 3 has a text of its own: below)
            refused(L, name, hi + 1, text)
            refused(L, name, INT_MAX, text)
        taken(L, name, oc.DEFAULTS[name])     # (a refusal leaves the option settable)
    finally:
        assert L.rq_set_option(name.encode(), oc.DEFAULTS[name]) == OK


def test_stage_growth_is_zero_or_a_range(L):
    try:
        for v in (0, 2, 64):
            taken(L, "stage_growth", v)
        for v in (1, 65, -1):
            refused(L, "stage_growth", v, BOUNDS["stage_growth"][2])
    finally:
        assert L.rq_set_option(b"stage_growth", oc.DEFAULTS["stage_growth"]) == OK


def test_survivor_segments_3_is_the_developer_builds(L):
    try:
        refused(L, "survivor_segments", 3, SEGMENTS_3_TEXT)
        refused(L, "survivor_segments", 4, BOUNDS["survivor_segments"][2])
        refused(L, "survivor_segments", INT_MAX, BOUNDS["survivor_segments"][2])
    finally:
        assert L.rq_set_option(b"survivor_segments", oc.DEFAULTS["survivor_segments"]) == OK


def test_scan_debug_is_a_mask(L):
    try:
        for v in (0, 128 | 512, SCAN_DEBUG_BITS, 16384, 65536):
            taken(L, "scan_debug", v)
        for v in (1, 2, 4, 64, 256, 1024, 8192, 128 | 1, SCAN_DEBUG_BITS + 1, 131072, INT_MAX, -1, -INT_MAX - 1):
            refused(L, "scan_debug", v, SCAN_DEBUG_TEXT)
    finally:
        assert L.rq_set_option(b"scan_debug", oc.DEFAULTS["scan_debug"]) == OK


def test_max_scan_blocks_zero_is_the_hardware_bound(L):
    try:
        for v in (0, 1, 7, (1 << 23) - 1, 1 << 23, INT_MAX):     # (values beyond the hardware bound are clamped to it, not refused)
            taken(L, "max_scan_blocks", v)
        refused(L, "max_scan_blocks", -1, BOUNDS["max_scan_blocks"][2])
    finally:
        assert L.rq_set_option(b"max_scan_blocks", oc.DEFAULTS["max_scan_blocks"]) == OK


def test_unknown_and_null_names(L):
    refused(L, "no_such_option", 0, "unknown option no_such_option")
    refused(L, "scan_impl ", 0, "unknown option scan_impl ")
    refused(L, "", 0, "unknown option ")
    refused(L, "SCAN_IMPL", 0, "unknown option SCAN_IMPL")
    refused(L, None, 0, "null option name")
