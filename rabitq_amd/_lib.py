"""ctypes loader for librabitq_hip.so (the C ABI in include/rabitq_hip.h).

There is no CPU fallback: if the shared library is missing or no gfx950 device is usable, every
operation raises.  Build it with `make -C rabitq_amd/csrc` (or `__graft_entry__.build()`).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import NamedTuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("RABITQ_HIP_SO") or os.path.join(_HERE, "librabitq_hip.so")   # (override: kernel experiments)
CSRC = os.path.join(_HERE, "csrc")

RQ_OK = 0
RQ_ERR_EMPTY = -7
STATUS_NAMES = {0: "RQ_OK", -1: "RQ_ERR_INVALID", -2: "RQ_ERR_DIM_MISMATCH", -3: "RQ_ERR_IO", -4: "RQ_ERR_HIP",
                -5: "RQ_ERR_NO_DEVICE", -6: "RQ_ERR_UNSUPPORTED", -7: "RQ_ERR_EMPTY", -8: "RQ_ERR_OOM"}

# every symbol include/rabitq_hip.h declares (checked by tests/test_abi.py against the header)
EXPORTS = [
    "rq_version", "rq_abi_version", "rq_last_error", "rq_init", "rq_normalize", "rq_normalize_device", "rq_build_ip", "rq_build_device_ip", "rq_build_from_path_ip", "rq_builder_create_ip", "rq_from_arrays_ip",
    "rq_ip_params", "rq_augment", "rq_augment_device", "rq_row_sqnorm_max", "rq_row_sqnorm_max_device", "rq_ip_from_dist", "rq_ip_from_dist_device", "rq_ip_radius", "rq_ip_radius_device", "rq_build", "rq_build_device", "rq_build_from_path",
    "rq_build_metric", "rq_build_device_metric", "rq_build_from_path_metric", "rq_builder_create_metric", "rq_from_arrays_metric", "rq_kmeans_device", "rq_builder_create", "rq_builder_assign_chunk", "rq_builder_order", "rq_builder_place_chunk", "rq_builder_finish", "rq_builder_free", "rq_builder_stats", "rq_load_dir",
    "rq_dump_dir", "rq_load_json", "rq_dump_json", "rq_free", "rq_from_arrays", "rq_info", "rq_get_array", "rq_get_device_ptr", "rq_query",
    "rq_query_batch", "rq_query_batch_device", "rq_query_batch_device_begin", "rq_query_batch_device_end", "rq_filter_create", "rq_filter_rows", "rq_filter_free", "rq_query_batch_filtered", "rq_query_batch_device_filtered", "rq_query_batch_device_begin_filtered", "rq_range_search", "rq_range_search_device", "rq_range_result_info", "rq_range_result_device_ptrs", "rq_range_result_copy", "rq_range_result_free", "rq_add", "rq_remove", "rq_last_mutate_stats", "rq_coarse_topk_device", "rq_merge_smallest_u64_device", "rq_query_batch_device_probed", "rq_query_batch_device_seeded", "rq_partition_lists", "rq_shard_index", "rq_query_batch_sharded_device", "rq_set_collectives", "rq_metrics", "rq_metrics_reset", "rq_rotate", "rq_rotate_device",
    "rq_quantize_pack",
    "rq_coarse_rank", "rq_query_prep", "rq_scan", "rq_rerank", "rq_set_profiling", "rq_set_option", "rq_last_profile",
    "rq_build_rows", "rq_build_device_rows", "rq_builder_create_rows", "rq_builder_assign_chunk_rows", "rq_builder_place_chunk_rows",
    "rq_from_arrays_rows", "rq_row_type", "rq_widen", "rq_widen_device",
    "rq_exact_search", "rq_exact_search_device", "rq_last_exact_stats",
    "rq_exact_range_search", "rq_exact_range_search_device",
    "rq_query_batch_adaptive", "rq_query_batch_device_adaptive", "rq_probe_counts_device",
    "rq_train_centroids", "rq_train_centroids_device",
    "rq_merge_from", "rq_extract",
    "rq_remove_lazy", "rq_compact", "rq_pending_removals",
    "rq_locate", "rq_locate_device", "rq_fetch_rows", "rq_fetch_rows_device", "rq_fetch_stored", "rq_fetch_stored_device",
    "rq_pair_distances", "rq_pair_distances_device", "rq_neighbours_of", "rq_neighbours_of_device", "rq_neighbours_of_exact",
    "rq_neighbours_of_exact_device", "rq_last_by_id_stats",
    "rq_attr_create", "rq_attr_drop", "rq_attr_count", "rq_attr_info", "rq_attr_index", "rq_attr_set", "rq_attr_set_device",
    "rq_attr_get", "rq_attr_get_device", "rq_attr_get_array", "rq_filter_create_where", "rq_last_where_stats",
    "rq_filter_combine", "rq_filter_id_bits", "rq_filter_ids_device",
    "rq_query_batch_grouped", "rq_query_batch_grouped_device", "rq_exact_search_grouped", "rq_exact_search_grouped_device",
    "rq_group_results", "rq_group_results_device", "rq_last_group_stats",
    "rq_query_batch_diverse", "rq_query_batch_diverse_device", "rq_exact_search_diverse", "rq_exact_search_diverse_device",
    "rq_diversify_results", "rq_diversify_results_device", "rq_last_diverse_stats",
]


class RabitqError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


METRIC_L2, METRIC_COSINE = 0, 1   # RQ_METRIC_*
METRIC_IP = 2
METRICS = {"l2": METRIC_L2, "cosine": METRIC_COSINE, "ip": METRIC_IP}
METRIC_NAMES = {v: k for k, v in METRICS.items()}
MERGE_IDS_KEEP, MERGE_IDS_SHIFT, MERGE_IDS_APPEND = 0, 1, 2   # RQ_MERGE_IDS_*
EXTRACT_ALL_IDS = 0xFFFFFFFFFFFFFFFF   # RQ_EXTRACT_ALL_IDS


def metric_id(metric) -> int:
    """"l2" / "cosine" / "ip" (or an RQ_METRIC_* value) -> the C ABI's metric id."""
    if isinstance(metric, str):
        if metric.lower() not in METRICS:
            raise ValueError(f"metric must be one of {sorted(METRICS)}, not {metric!r}")
        return METRICS[metric.lower()]
    return int(metric)


class RowType(NamedTuple):
    """One row type (RQ_ROWS_* of include/rabitq_hip.h), as the Python layer sees it."""
    name: str          # the rows= argument and RaBitQ.row_type
    id: int            # the C ABI's row_type
    takes: tuple       # numpy dtypes an array of these rows may have (f32: anything, it is converted)
    returns: type      # numpy dtype base_rows returns
    elem_bytes: int


# the one table of row types: everything below, index.py and cli.py read it
ROW_TABLE = (
    RowType("f32", 0, (), np.float32, 4),
    RowType("f16", 1, (np.float16, np.uint16), np.float16, 2),   # (uint16: bit patterns)
    RowType("bf16", 2, (np.uint16,), np.uint16, 2),              # bit patterns only: numpy has no bfloat16
    RowType("u8", 4, (np.uint8,), np.uint8, 1),
    RowType("i8", 5, (np.int8,), np.int8, 1),
)
ROWS_F32, ROWS_F16, ROWS_BF16, ROWS_U8, ROWS_I8 = (t.id for t in ROW_TABLE)   # RQ_ROWS_*
ROW_TYPES = {t.name: t.id for t in ROW_TABLE}
ROW_TYPE_NAMES = {t.id: t.name for t in ROW_TABLE}
ROW_TYPE_BY_ID = {t.id: t for t in ROW_TABLE}
ROW_TYPE_BY_NAME = {t.name: t for t in ROW_TABLE}


def row_type_id(rows) -> int:
    """"f32" / "f16" / "bf16" / "u8" / "i8" (or an RQ_ROWS_* value) -> the C ABI's row_type."""
    if isinstance(rows, str):
        if rows.lower() not in ROW_TYPES:
            raise ValueError(f"rows must be one of {sorted(ROW_TYPES)}, not {rows!r}")
        return ROW_TYPES[rows.lower()]
    return int(rows)


ABI_VERSION = 4   # RQ_ABI_VERSION of include/rabitq_hip.h this mirror was written against


class _Sized(C.Structure):
    """Out-struct versioned by size: `struct_size` is set to the mirror's sizeof before every call."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(type(self))


class Info(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("dim", C.c_uint32), ("k", C.c_uint32), ("max_list_len", C.c_uint32),
                ("n", C.c_uint64), ("n_hbm", C.c_uint64), ("split_rows", C.c_uint32), ("metric", C.c_uint32)]


class MetricsT(C.Structure):
    _fields_ = [("rough", C.c_uint64), ("precise", C.c_uint64), ("query", C.c_uint64), ("miss", C.c_uint64)]


class BuildStatsT(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("ms_rotate", C.c_float), ("ms_assign", C.c_float), ("ms_quantize", C.c_float),
                ("rows_assigned", C.c_uint64), ("rows_in_hbm", C.c_uint64), ("rows_in_host_memory", C.c_uint64),
                ("rows_exact_redo", C.c_uint64)]


class ProfileT(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("coarse_fallback_rows", C.c_uint32)] + [(n, C.c_float) for n in ("ms_rotate", "ms_coarse", "ms_select", "ms_prep", "ms_group", "ms_scan",
                                         "ms_rerank", "ms_sort", "ms_replay", "ms_total")] + [
        ("scan_bytes", C.c_uint64), ("scan_candidates", C.c_uint64), ("rerank_candidates", C.c_uint64),
        ("scan_launches", C.c_uint32), ("retries", C.c_uint32),
        ("ms_scan_matrix", C.c_float), ("matrix_launches", C.c_uint32), ("matrix_pairs", C.c_uint64),
        ("matrix_subtile_steps", C.c_uint64), ("matrix_exact_steps", C.c_uint64),
        ("rerank_shadow_rejects", C.c_uint64), ("ms_early", C.c_float), ("small_batch_passes", C.c_uint32),
        ("survivor_workspace_bytes", C.c_uint64), ("segmented_passes", C.c_uint32), ("matrix_additive_launches", C.c_uint32)]


class MutateStatsT(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32)] + [(n, C.c_float) for n in (
        "ms_keys", "ms_assign", "ms_alloc", "ms_merge", "ms_gather", "ms_derive", "ms_free", "ms_total")] + [
        ("rows_before", C.c_uint64), ("rows_after", C.c_uint64), ("gather_bytes", C.c_uint64)]


class ExactParamsT(_Sized):
    """rq_exact_params_t: test hooks of the exact search (zero = automatic; results never depend on them)."""
    _fields_ = [("struct_size", C.c_uint32), ("seed_probe", C.c_uint32), ("cand_per_query", C.c_uint32), ("flags", C.c_uint32)]


EXACT_NO_SEED, EXACT_NO_PREFILTER = 1, 2   # rq_exact_params_t.flags


class ExactStatsT(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("seed_probe", C.c_uint32)] + [(n, C.c_float) for n in (
        "ms_seed", "ms_scan", "ms_exact", "ms_select")] + [
        ("seed_unfilled", C.c_uint32), ("reruns", C.c_uint32), ("candidates", C.c_uint64), ("exact", C.c_uint64),
        ("row_bytes_read", C.c_uint64), ("scan_launches", C.c_uint32), ("scan_subtiles", C.c_uint32)]


class ProbeRuleT(_Sized):
    """rq_probe_rule_t: adaptive probing's cut rule (max_probe: a raw address, device or host as the entry says; 0 = none)."""
    _fields_ = [("struct_size", C.c_uint32), ("min_probe", C.c_uint32), ("ratio", C.c_float), ("reserved", C.c_uint32),
                ("max_probe", C.c_void_p)]


class TrainParamsT(_Sized):
    """rq_train_params_t: what the centroid trainer is asked for (sq_bound: the inner-product metric's S, NaN = automatic)."""
    _fields_ = [("struct_size", C.c_uint32), ("iters", C.c_uint32), ("points_per_centroid", C.c_uint32), ("seed", C.c_uint64),
                ("metric", C.c_uint32), ("row_type", C.c_uint32), ("sq_bound", C.c_float)]


class TrainStatsT(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("iters_run", C.c_uint32), ("sample_rows", C.c_uint32), ("splits", C.c_uint32)]


POS_ABSENT = 0xFFFFFFFF   # RQ_POS_ABSENT
DIRECTORY_FORMS = {0: "none", 1: "dense", 2: "hash"}   # RQ_DIRECTORY_*


class ByIdStatsT(_Sized):
    """rq_by_id_stats_t: the calling thread's last by-id call (locate / fetch / distances_to / neighbours_of)."""
    _fields_ = [("struct_size", C.c_uint32), ("form", C.c_uint32), ("directory_bytes", C.c_uint64), ("ms_build", C.c_float),
                ("longest_chain", C.c_uint32), ("found", C.c_uint64), ("absent", C.c_uint64), ("gather_bytes", C.c_uint64),
                ("ms_gather", C.c_float), ("ms_lookup", C.c_float), ("built", C.c_uint32), ("reserved0", C.c_uint32)]


class AttrType(NamedTuple):
    """One attribute column type (RQ_ATTR_* of include/rabitq_hip.h)."""
    name: str        # the dtype= argument of create_attr
    id: int
    dtype: type      # numpy dtype of the column's values
    elem_bytes: int


ATTR_TABLE = (
    AttrType("u32", 0, np.uint32, 4), AttrType("i32", 1, np.int32, 4), AttrType("f32", 2, np.float32, 4),
    AttrType("u64", 3, np.uint64, 8), AttrType("i64", 4, np.int64, 8),
)
ATTR_BY_NAME = {t.name: t for t in ATTR_TABLE}
ATTR_BY_ID = {t.id: t for t in ATTR_TABLE}
ATTR_MAX_COLUMNS = 16                                    # RQ_ATTR_MAX_COLUMNS
FILTER_AND, FILTER_OR, FILTER_ANDNOT, FILTER_NOT = range(4)   # RQ_FILTER_*


class AttrValue(C.Union):
    """rq_attr_value_t: 8 bytes, a 4-byte value in the low 4.  (ctypes passes no union by value: the entries that take one by value
    are declared with its u64 image, which the x86-64 and aarch64 calling conventions pass the same way.)"""
    _fields_ = [("u32", C.c_uint32), ("i32", C.c_int32), ("f32", C.c_float), ("u64", C.c_uint64), ("i64", C.c_int64)]


class AttrInfoT(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("type", C.c_uint32), ("name", C.c_char * 32), ("fill", AttrValue), ("bytes", C.c_uint64)]


class WhereTermT(C.Structure):
    """rq_where_term_t: one comparison of a column (its index in rq_attr_info order) with constants; `set`: a host address."""
    _fields_ = [("column", C.c_uint32), ("op", C.c_uint32), ("a", AttrValue), ("b", AttrValue), ("set", C.c_void_p),
                ("set_count", C.c_uint32), ("reserved0", C.c_uint32)]


class WhereStatsT(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("columns", C.c_uint32), ("rows", C.c_uint64), ("admitted", C.c_uint64),
                ("bytes_read", C.c_uint64), ("ms_eval", C.c_float), ("ms_finish", C.c_float)]


class GroupParamsT(_Sized):
    """rq_group_params_t: topk groups of at most group_size rows, out of `fetch` candidates per query."""
    _fields_ = [("struct_size", C.c_uint32), ("topk", C.c_uint32), ("group_size", C.c_uint32), ("fetch", C.c_uint32), ("flags", C.c_uint32)]


class GroupStatsT(_Sized):
    """rq_group_stats_t: the calling thread's last grouped call."""
    _fields_ = [("struct_size", C.c_uint32), ("fetch", C.c_uint32), ("ms_source", C.c_float), ("ms_group", C.c_float),
                ("candidates", C.c_uint64), ("absent", C.c_uint64), ("kept", C.c_uint64), ("groups", C.c_uint64),
                ("directory_built", C.c_uint32), ("reserved0", C.c_uint32)]


GROUP_MAX_FETCH = 2048   # RQ_MAX_TOPK: the most candidates per query a grouped call takes


def default_group_fetch(topk: int, group_size: int) -> int:
    """fetch=None of the grouped calls: min(2048, max(64, 4 * topk * group_size)) -- a default, not a guarantee."""
    return min(GROUP_MAX_FETCH, max(64, 4 * int(topk) * int(group_size)))


class DiverseParamsT(_Sized):
    """rq_diverse_params_t: the topk rows maximal marginal relevance takes out of `fetch` candidates per query."""
    _fields_ = [("struct_size", C.c_uint32), ("topk", C.c_uint32), ("fetch", C.c_uint32), ("lambda_", C.c_float), ("flags", C.c_uint32)]


class DiverseStatsT(_Sized):
    """rq_diverse_stats_t: the calling thread's last diverse call."""
    _fields_ = [("struct_size", C.c_uint32), ("fetch", C.c_uint32), ("ms_source", C.c_float), ("ms_select", C.c_float),
                ("candidates", C.c_uint64), ("absent", C.c_uint64), ("skipped", C.c_uint64), ("taken", C.c_uint64),
                ("pair_distances", C.c_uint64), ("directory_built", C.c_uint32), ("reserved0", C.c_uint32)]


def default_diverse_fetch(topk: int) -> int:
    """fetch=None of the diverse calls: min(2048, max(64, 4 * topk)) -- a default, not a guarantee."""
    return min(GROUP_MAX_FETCH, max(64, 4 * int(topk)))


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return SO_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RabitqError(-5, f"{SO_PATH} not built (run `make -C rabitq_amd/csrc`); there is no CPU fallback")
    # A process that also uses PyTorch must load torch's bundled ROCm runtime BEFORE this library pulls in the system
    # one: the other way round torch later reports "No HIP GPUs are available" (measured on this image).  The library
    # itself does not need torch; the import only fixes the load order when torch is installed.  Hosts that never use
    # torch set RABITQ_NO_TORCH_PRELOAD=1 and skip the (heavy) import ("Loading order").
    import importlib.util
    import sys
    if (not os.environ.get("RABITQ_NO_TORCH_PRELOAD") and "torch" not in sys.modules
            and importlib.util.find_spec("torch") is not None):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(SO_PATH)
    vp, f32p, u32p, u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p  # raw addresses (host or device)
    u32, u64, i32, flt = C.c_uint32, C.c_uint64, C.c_int32, C.c_float
    pp = C.POINTER(C.c_void_p)
    sig = {
        "rq_version": (C.c_char_p, []),
        "rq_abi_version": (C.c_uint32, []),
        "rq_last_error": (C.c_char_p, []),
        "rq_init": (i32, [C.c_int]),
        "rq_build": (i32, [f32p, u64, u32, f32p, u32, f32p, u64, pp]),
        "rq_build_device": (i32, [f32p, u64, u32, f32p, u32, f32p, u64, pp]),
        "rq_build_from_path": (i32, [C.c_char_p, C.c_char_p, f32p, u64, pp]),
        "rq_normalize": (i32, [f32p, u64, u32, f32p]),
        "rq_normalize_device": (i32, [f32p, u64, u32, f32p]),
        "rq_build_metric": (i32, [f32p, u64, u32, f32p, u32, f32p, u64, u32, pp]),
        "rq_build_device_metric": (i32, [f32p, u64, u32, f32p, u32, f32p, u64, u32, pp]),
        "rq_build_from_path_metric": (i32, [C.c_char_p, C.c_char_p, f32p, u64, u32, pp]),
        "rq_builder_create_metric": (i32, [u64, u32, f32p, u32, f32p, u64, u64, u32, pp]),
        "rq_from_arrays_metric": (i32, [u32, u64, u32, f32p, f32p, f32p, u32p, u32p, u64p, vp, u32, pp]),
        "rq_build_ip": (i32, [f32p, u64, u32, f32p, u32, f32p, u64, u32, flt, pp]),
        "rq_build_device_ip": (i32, [f32p, u64, u32, f32p, u32, f32p, u64, u32, flt, pp]),
        "rq_build_from_path_ip": (i32, [C.c_char_p, C.c_char_p, f32p, u64, flt, pp]),
        "rq_builder_create_ip": (i32, [u64, u32, f32p, u32, f32p, u64, u64, u32, flt, pp]),
        "rq_from_arrays_ip": (i32, [u32, u64, u32, f32p, f32p, f32p, u32p, u32p, u64p, vp, u32, flt, pp]),
        "rq_ip_params": (i32, [vp, C.POINTER(u32), C.POINTER(flt)]),
        "rq_augment": (i32, [f32p, u64, u32, flt, f32p]),
        "rq_augment_device": (i32, [f32p, u64, u32, flt, f32p]),
        "rq_row_sqnorm_max": (i32, [f32p, u64, u32, C.POINTER(flt)]),
        "rq_row_sqnorm_max_device": (i32, [f32p, u64, u32, C.POINTER(flt)]),
        "rq_ip_from_dist": (i32, [vp, f32p, u32, u32, f32p, u32, u32p, f32p]),
        "rq_ip_from_dist_device": (i32, [vp, f32p, u32, u32, f32p, u32, u32p, f32p]),
        "rq_ip_radius": (i32, [vp, f32p, u32, u32, f32p, f32p]),
        "rq_ip_radius_device": (i32, [vp, f32p, u32, u32, f32p, f32p]),
        "rq_kmeans_device": (i32, [f32p, u64, u32, u32, u32, u32, u64, f32p]),
        "rq_builder_create": (i32, [u64, u32, f32p, u32, f32p, u64, u64, pp]),
        "rq_builder_assign_chunk": (i32, [vp, f32p, u64, u64]),
        "rq_builder_order": (i32, [vp]),
        "rq_builder_place_chunk": (i32, [vp, f32p, u64, u64]),
        "rq_builder_finish": (i32, [vp, pp]),
        "rq_builder_free": (None, [vp]),
        "rq_builder_stats": (i32, [vp, C.POINTER(BuildStatsT)]),
        "rq_load_dir": (i32, [C.c_char_p, pp]),
        "rq_dump_dir": (i32, [vp, C.c_char_p]),
        "rq_load_json": (i32, [C.c_char_p, pp]),
        "rq_dump_json": (i32, [vp, C.c_char_p]),
        "rq_free": (None, [vp]),
        "rq_from_arrays": (i32, [u32, u64, u32, f32p, f32p, f32p, u32p, u32p, u64p, vp, pp]),
        "rq_info": (i32, [vp, C.POINTER(Info)]),
        "rq_get_array": (i32, [vp, C.c_int, vp, u64]),
        "rq_get_device_ptr": (i32, [vp, C.c_int, pp, C.POINTER(u64)]),
        "rq_query": (i32, [vp, f32p, u32, u32, u32, C.c_int, f32p, u32p, u32p]),
        "rq_query_batch": (i32, [vp, f32p, u32, u32, u32, u32, C.c_int, f32p, u32p, u32p]),
        "rq_query_batch_device": (i32, [vp, f32p, u32, u32, u32, u32, C.c_int, f32p, u32p, u32p]),
        "rq_query_batch_device_begin": (i32, [vp, f32p, u32, u32, u32, u32, C.c_int, f32p, u32p, u32p, pp]),
        "rq_query_batch_device_end": (i32, [vp]),
        "rq_filter_create": (i32, [vp, u32p, u64, C.c_int, pp]),
        "rq_filter_rows": (i32, [vp, C.POINTER(u64)]),
        "rq_filter_free": (None, [vp]),
        "rq_query_batch_filtered": (i32, [vp, vp, f32p, u32, u32, u32, u32, C.c_int, f32p, u32p, u32p]),
        "rq_query_batch_device_filtered": (i32, [vp, vp, f32p, u32, u32, u32, u32, C.c_int, f32p, u32p, u32p]),
        "rq_query_batch_device_begin_filtered": (i32, [vp, vp, f32p, u32, u32, u32, u32, C.c_int, f32p, u32p, u32p, pp]),
        "rq_range_search": (i32, [vp, vp, f32p, u32, u32, u32, f32p, pp]),
        "rq_range_search_device": (i32, [vp, vp, f32p, u32, u32, u32, f32p, pp]),
        "rq_range_result_info": (i32, [vp, C.POINTER(u32), C.POINTER(u64)]),
        "rq_range_result_device_ptrs": (i32, [vp, pp, pp, pp]),
        "rq_range_result_copy": (i32, [vp, u64p, f32p, u32p]),
        "rq_range_result_free": (None, [vp]),
        "rq_add": (i32, [vp, f32p, u64, u32, u32p, C.c_int, u32p]),
        "rq_remove": (i32, [vp, u32p, u64, C.c_int, u64p]),
        "rq_last_mutate_stats": (i32, [C.POINTER(MutateStatsT)]),
        "rq_merge_from": (i32, [vp, vp, u32, u32, u32p]),
        "rq_extract": (i32, [vp, u32p, u64, C.c_int, pp]),
        "rq_remove_lazy": (i32, [vp, u32p, u64, C.c_int, u64p]),
        "rq_compact": (i32, [vp, u64p]),
        "rq_pending_removals": (i32, [vp, u64p]),
        "rq_coarse_topk_device": (i32, [vp, f32p, u32, u32, u32, u32, u32, u32p, f32p]),
        "rq_merge_smallest_u64_device": (i32, [vp, u32, u32, u32, u32, vp]),
        "rq_query_batch_device_probed": (i32, [vp, f32p, u32, u32, u32p, f32p, u32, u32, C.c_int, f32p, u32p, u32p]),
        "rq_query_batch_device_seeded": (i32, [vp, f32p, u32, u32, u32p, f32p, u32, u32, C.c_int, f32p, f32p, u32p, u32p]),
        "rq_partition_lists": (i32, [vp, u32, u32p, u64p]),
        "rq_shard_index": (i32, [vp, u32p, u32, pp]),
        "rq_query_batch_sharded_device": (i32, [vp, vp, u32, u32, f32p, u32, u32, u32, u32, C.c_int, f32p, u32p, u32p]),
        "rq_set_collectives": (i32, [vp]),
        "rq_metrics": (i32, [C.POINTER(MetricsT)]),
        "rq_metrics_reset": (i32, []),
        "rq_rotate": (i32, [f32p, u64, u32, f32p, C.c_int, f32p]),
        "rq_rotate_device": (i32, [vp, f32p, u64, f32p, C.POINTER(C.c_float)]),
        "rq_quantize_pack": (i32, [f32p, u64, u32, f32p, u32, u32p, f32p, u64p, vp]),
        "rq_coarse_rank": (i32, [vp, f32p, u32, u32, u32, f32p, u32p, f32p]),
        "rq_query_prep": (i32, [vp, f32p, u32, u32p, f32p, f32p, u32p, u64p]),
        "rq_scan": (i32, [vp, u32, flt, u64p, flt, flt, flt, f32p]),
        "rq_rerank": (i32, [vp, f32p, u32p, u32, f32p]),
        "rq_set_profiling": (i32, [C.c_int]),
        "rq_set_option": (i32, [C.c_char_p, C.c_int]),
        "rq_last_profile": (i32, [C.POINTER(ProfileT)]),
        "rq_build_rows": (i32, [vp, u64, u32, f32p, u32, f32p, u64, u32, u32, pp]),
        "rq_build_device_rows": (i32, [vp, u64, u32, f32p, u32, f32p, u64, u32, u32, pp]),
        "rq_builder_create_rows": (i32, [u64, u32, f32p, u32, f32p, u64, u64, u32, u32, pp]),
        "rq_builder_assign_chunk_rows": (i32, [vp, vp, u64, u64]),
        "rq_builder_place_chunk_rows": (i32, [vp, vp, u64, u64]),
        "rq_from_arrays_rows": (i32, [u32, u64, u32, vp, f32p, f32p, u32p, u32p, u64p, vp, u32, u32, pp]),
        "rq_row_type": (i32, [vp, C.POINTER(u32)]),
        "rq_widen": (i32, [vp, u32, u64, f32p]),
        "rq_widen_device": (i32, [vp, u32, u64, f32p]),
        "rq_exact_search": (i32, [vp, vp, f32p, u32, u32, u32, C.POINTER(ExactParamsT), f32p, u32p, u32p]),
        "rq_exact_search_device": (i32, [vp, vp, f32p, u32, u32, u32, C.POINTER(ExactParamsT), f32p, u32p, u32p]),
        "rq_last_exact_stats": (i32, [C.POINTER(ExactStatsT)]),
        "rq_exact_range_search": (i32, [vp, vp, f32p, u32, u32, f32p, C.POINTER(ExactParamsT), pp]),
        "rq_exact_range_search_device": (i32, [vp, vp, f32p, u32, u32, f32p, C.POINTER(ExactParamsT), pp]),
        "rq_query_batch_adaptive": (i32, [vp, vp, f32p, u32, u32, u32, u32, C.c_int, C.POINTER(ProbeRuleT), f32p, u32p, u32p, u32p]),
        "rq_query_batch_device_adaptive": (i32, [vp, vp, f32p, u32, u32, u32, u32, C.c_int, C.POINTER(ProbeRuleT), f32p, u32p, u32p, u32p]),
        "rq_probe_counts_device": (i32, [vp, f32p, u32, u32, u32, C.POINTER(ProbeRuleT), u32p]),
        "rq_train_centroids": (i32, [vp, u64, u32, u32, C.POINTER(TrainParamsT), f32p, vp, C.POINTER(TrainStatsT)]),
        "rq_train_centroids_device": (i32, [vp, u64, u32, u32, C.POINTER(TrainParamsT), f32p, vp, C.POINTER(TrainStatsT)]),
        "rq_locate": (i32, [vp, u32p, u64, u32p]),
        "rq_locate_device": (i32, [vp, u32p, u64, u32p]),
        "rq_fetch_rows": (i32, [vp, u32p, u64, f32p, u32p]),
        "rq_fetch_rows_device": (i32, [vp, u32p, u64, f32p, u32p]),
        "rq_fetch_stored": (i32, [vp, u32p, u64, vp, u32p]),
        "rq_fetch_stored_device": (i32, [vp, u32p, u64, vp, u32p]),
        "rq_pair_distances": (i32, [vp, f32p, u32, u32, u32p, u32, f32p]),
        "rq_pair_distances_device": (i32, [vp, f32p, u32, u32, u32p, u32, f32p]),
        "rq_neighbours_of": (i32, [vp, u32p, u32, u32, u32, C.c_int, vp, f32p, u32p, u32p]),
        "rq_neighbours_of_device": (i32, [vp, u32p, u32, u32, u32, C.c_int, vp, f32p, u32p, u32p]),
        "rq_neighbours_of_exact": (i32, [vp, u32p, u32, u32, vp, C.POINTER(ExactParamsT), f32p, u32p, u32p]),
        "rq_neighbours_of_exact_device": (i32, [vp, u32p, u32, u32, vp, C.POINTER(ExactParamsT), f32p, u32p, u32p]),
        "rq_last_by_id_stats": (i32, [C.POINTER(ByIdStatsT)]),
        "rq_attr_create": (i32, [vp, C.c_char_p, u32, u64]),   # (fill: the union's u64 image, see AttrValue)
        "rq_attr_drop": (i32, [vp, C.c_char_p]),
        "rq_attr_count": (i32, [vp, C.POINTER(u32)]),
        "rq_attr_info": (i32, [vp, u32, C.POINTER(AttrInfoT)]),
        "rq_attr_index": (i32, [vp, C.c_char_p, C.POINTER(u32)]),
        "rq_attr_set": (i32, [vp, C.c_char_p, u32p, vp, u64, C.POINTER(u64)]),
        "rq_attr_set_device": (i32, [vp, C.c_char_p, u32p, vp, u64, C.POINTER(u64)]),
        "rq_attr_get": (i32, [vp, C.c_char_p, u32p, u64, vp, u32p]),
        "rq_attr_get_device": (i32, [vp, C.c_char_p, u32p, u64, vp, u32p]),
        "rq_attr_get_array": (i32, [vp, C.c_char_p, vp, u64]),
        "rq_filter_create_where": (i32, [vp, C.POINTER(WhereTermT), u32, vp, u32, pp]),
        "rq_last_where_stats": (i32, [C.POINTER(WhereStatsT)]),
        "rq_filter_combine": (i32, [vp, vp, vp, u32, pp]),
        "rq_filter_id_bits": (i32, [vp, u32p, u64, C.c_int]),
        "rq_filter_ids_device": (i32, [vp, u32p, u64, C.POINTER(u64)]),
        "rq_query_batch_grouped": (i32, [vp, vp, f32p, u32, u32, u32, C.c_int, C.c_char_p, C.POINTER(GroupParamsT), f32p, u32p, u64p, u32p, u32p, u32p]),
        "rq_query_batch_grouped_device": (i32, [vp, vp, f32p, u32, u32, u32, C.c_int, C.c_char_p, C.POINTER(GroupParamsT), f32p, u32p, u64p, u32p, u32p, u32p]),
        "rq_exact_search_grouped": (i32, [vp, vp, f32p, u32, u32, C.POINTER(ExactParamsT), C.c_char_p, C.POINTER(GroupParamsT), f32p, u32p, u64p, u32p, u32p, u32p]),
        "rq_exact_search_grouped_device": (i32, [vp, vp, f32p, u32, u32, C.POINTER(ExactParamsT), C.c_char_p, C.POINTER(GroupParamsT), f32p, u32p, u64p, u32p, u32p, u32p]),
        "rq_group_results": (i32, [vp, f32p, u32p, u32p, u32, C.c_char_p, C.POINTER(GroupParamsT), f32p, u32p, u64p, u32p, u32p]),
        "rq_group_results_device": (i32, [vp, f32p, u32p, u32p, u32, C.c_char_p, C.POINTER(GroupParamsT), f32p, u32p, u64p, u32p, u32p]),
        "rq_last_group_stats": (i32, [C.POINTER(GroupStatsT)]),
        "rq_query_batch_diverse": (i32, [vp, vp, f32p, u32, u32, u32, C.c_int, C.POINTER(DiverseParamsT), f32p, u32p, f32p, u32p, u32p]),
        "rq_query_batch_diverse_device": (i32, [vp, vp, f32p, u32, u32, u32, C.c_int, C.POINTER(DiverseParamsT), f32p, u32p, f32p, u32p, u32p]),
        "rq_exact_search_diverse": (i32, [vp, vp, f32p, u32, u32, C.POINTER(ExactParamsT), C.POINTER(DiverseParamsT), f32p, u32p, f32p, u32p, u32p]),
        "rq_exact_search_diverse_device": (i32, [vp, vp, f32p, u32, u32, C.POINTER(ExactParamsT), C.POINTER(DiverseParamsT), f32p, u32p, f32p, u32p, u32p]),
        "rq_diversify_results": (i32, [vp, f32p, u32p, u32p, u32, C.POINTER(DiverseParamsT), f32p, u32p, f32p, u32p]),
        "rq_diversify_results_device": (i32, [vp, f32p, u32p, u32p, u32, C.POINTER(DiverseParamsT), f32p, u32p, f32p, u32p]),
        "rq_last_diverse_stats": (i32, [C.POINTER(DiverseStatsT)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if L.rq_abi_version() != ABI_VERSION:
        raise RabitqError(-6, f"{SO_PATH} has ABI revision {L.rq_abi_version()}, this mirror expects {ABI_VERSION}: rebuild "
                              "(make -C rabitq_amd/csrc)")
    _lib = L
    return L


def check(status: int):
    if status != RQ_OK:
        raise RabitqError(status, lib().rq_last_error().decode(errors="replace"))
