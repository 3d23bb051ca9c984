"""`RaBitQ`: host-side mirror of the reference's index type (src/rabitq.rs:57-68, :70-333).

Same method names, argument meaning and error behaviour as the crate: where the reference panics
(`expect` / `assert!`), these raise `RabitqError`.  Everything is delegated to librabitq_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import BuildStatsT, Info, MetricsT, ProfileT, check, lib

ARR_BASE, ARR_ORTHOGONAL, ARR_CENTROIDS, ARR_OFFSETS, ARR_MAP_IDS, ARR_CODES, ARR_FACTORS, ARR_BASE_ROWS = range(8)


def _addr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _sq_bound(max_sq_norm) -> float:
    """max_sq_norm= of the inner-product constructors -> the C ABI's sq_bound (None: NaN, the largest squared norm of the input)."""
    return float("nan") if max_sq_norm is None else float(max_sq_norm)


def _f32(a):
    """-> contiguous f32 (float16 input is widened here, on the host: exact)."""
    return np.ascontiguousarray(a, dtype=np.float32)


def _typed_rows(base, rows):
    """(base, rows=) of the constructors -> (contiguous array as the library reads it, RQ_ROWS_* id).  rows=None: float16 arrays
    are f16 rows, everything else f32 (a uint8 array too: it is converted).  rows="f16" takes float16 (or uint16 bit patterns),
    rows="bf16" uint16 bit patterns, rows="u8" a uint8 array, rows="i8" an int8 array (_lib.ROW_TABLE)."""
    a = np.asarray(base)
    rt = (_lib.ROWS_F16 if a.dtype == np.float16 else _lib.ROWS_F32) if rows is None else _lib.row_type_id(rows)
    if rt == _lib.ROWS_F32:
        return _f32(a), rt
    t = _lib.ROW_TYPE_BY_ID.get(rt)
    if a.dtype not in (t.takes if t else (np.uint16,)):   # (an id the table does not know: the library refuses it)
        if t and t.elem_bytes == 1:
            raise TypeError(f"rows={t.name!r} takes a {np.dtype(t.returns).name} array, not {a.dtype}")
        raise TypeError(f"rows={_lib.ROW_TYPE_NAMES.get(rt, rt)!r} takes a uint16 array of bit patterns"
                        + (" or a float16 array" if rt == _lib.ROWS_F16 else "") + f", not {a.dtype}")
    return np.ascontiguousarray(a), rt


def widen(x, rows="f16"):
    """W(x): f16 / bf16 elements (float16, or uint16 bit patterns) or, rows="u8" / "i8", uint8 / int8 elements -> f32, on the GPU
    (rq_widen); any shape."""
    a, rt = _typed_rows(x, rows)
    if rt == _lib.ROWS_F32:
        return a
    out = np.empty(a.shape, dtype=np.float32)
    check(lib().rq_widen(_addr(a), rt, a.size, _addr(out)))
    return out


class TrainStats:
    """What a training run did (rq_train_stats_t + the objective): `iters_run` iterations updated the centroids (== iters when the
    cap ended it), on `sample_rows` rows, with `splits` empty-cluster splits; `objective[t]` is iteration t's sum of squared
    distances of the sample rows to their centroids (f64), one entry per iteration run."""

    def __init__(self, iters_run: int, sample_rows: int, splits: int, objective):
        self.iters_run, self.sample_rows, self.splits, self.objective = iters_run, sample_rows, splits, objective

    def __repr__(self):
        return f"TrainStats(iters_run={self.iters_run}, sample_rows={self.sample_rows}, splits={self.splits}, objective={self.objective!r})"


def _train_call(entry, rows_addr, n, d, k, out_addr, iters, points_per_centroid, seed, metric, max_sq_norm, rt) -> TrainStats:
    p = _lib.TrainParamsT(iters=iters, points_per_centroid=points_per_centroid, seed=seed, metric=_lib.metric_id(metric), row_type=rt,
                          sq_bound=_sq_bound(max_sq_norm))
    st = _lib.TrainStatsT()
    obj = np.zeros(max(iters, 1), dtype=np.float64)
    check(entry(rows_addr, n, d, k, C.byref(p), out_addr, _addr(obj), C.byref(st)))
    return TrainStats(int(st.iters_run), int(st.sample_rows), int(st.splits), obj[:st.iters_run].copy())


def train_centroids(base, k: int, iters: int = 20, points_per_centroid: int = 256, seed: int = 0, metric="l2", max_sq_norm=None,
                    rows=None, return_stats: bool = False):
    """Train the k centroids a build of (base, metric, rows) takes: deterministic k-means on the GPU (rq_train_centroids), the same
    bits for the same arguments on every run.  base: n x d as RaBitQ.build takes it (rows= too).  -> k x d f32 (metric="ip":
    k x (d + 1), the centroids of the augmented rows, S = max_sq_norm or the largest squared row norm); with return_stats also a
    TrainStats."""
    base, rt = _typed_rows(base, rows)
    if base.ndim != 2:
        raise _lib.RabitqError(-2, "base must be 2-D (n x d)")
    n, d = base.shape
    out = np.empty((k, d + 1 if _lib.metric_id(metric) == _lib.METRIC_IP else d), dtype=np.float32)
    st = _train_call(lib().rq_train_centroids, _addr(base), n, d, k, _addr(out), iters, points_per_centroid, seed, metric, max_sq_norm, rt)
    return (out, st) if return_stats else out


def train_centroids_device(base_ptr: int, n: int, d: int, k: int, out_ptr: int, iters: int = 20, points_per_centroid: int = 256,
                           seed: int = 0, metric="l2", max_sq_norm=None, rows="f32") -> TrainStats:
    """train_centroids on device-resident rows (raw addresses): base_ptr holds n x d elements of `rows`, out_ptr receives k x d f32
    (metric="ip": k x (d + 1))."""
    return _train_call(lib().rq_train_centroids_device, C.c_void_p(base_ptr), n, d, k, C.c_void_p(out_ptr), iters, points_per_centroid,
                       seed, metric, max_sq_norm, _lib.row_type_id(rows))


def pack_filter_bits(ids=None, mask=None, nbits=None):
    """An allow-list as the bitmap rq_filter_create reads -> (words u32, nbits): bit (id & 31) of word id >> 5 set = id admitted.
    `ids`: admitted ids (any order, repeats allowed; ids >= nbits are dropped -- the library never admits them); nbits defaults to
    max(ids) + 1.  `mask`: a boolean mask over ids (nbits = its length).  Exactly one of the two."""
    if (ids is None) == (mask is None):
        raise ValueError("give exactly one of ids / mask")
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=bool).reshape(-1)
        nb = m.size
    else:
        a = np.asarray(ids).reshape(-1)
        if a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < 0):
            raise ValueError("ids must be non-negative integers")
        a = a.astype(np.uint64, copy=False)
        nb = int(a.max()) + 1 if nbits is None and a.size else int(nbits or 0)
        m = np.zeros(nb, dtype=bool)
        m[a[a < nb].astype(np.int64)] = True
    if nbits is not None and mask is not None and int(nbits) != nb:
        raise ValueError("nbits must equal the mask's length")
    if nb > (1 << 32):
        raise ValueError("ids are u32: nbits <= 2^32")
    nwords = (nb + 31) // 32
    packed = np.packbits(m, bitorder="little")
    buf = np.zeros(nwords * 4, dtype=np.uint8)
    buf[:packed.size] = packed
    return buf.view(np.uint32), nb


class Filter:
    """A query-time allow-list of one index (rq_filter_create): made once, passed as `filter=` to the query methods.  Holds a
    reference to its index, so the index outlives it."""

    def __init__(self, index: "RaBitQ", handle):
        self.index = index
        self._h = handle
        rows = C.c_uint64()
        check(lib().rq_filter_rows(self._h, C.byref(rows)))
        self.rows = int(rows.value)   # rows of the index the filter admits

    def close(self):
        if getattr(self, "_h", None):
            lib().rq_filter_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- set algebra (rq_filter_combine): new filters of the same index, made on the device ----
    def _combine(self, other, op):
        if op != _lib.FILTER_NOT:
            if not isinstance(other, Filter):
                return NotImplemented
            if other.index is not self.index:
                raise ValueError("the two filters belong to different indexes")
        h = C.c_void_p()
        check(lib().rq_filter_combine(self.index._h, self._h, _fh(other), op, C.byref(h)))
        return Filter(self.index, h)

    def __and__(self, other):
        """Rows both filters admit."""
        return self._combine(other, _lib.FILTER_AND)

    def __or__(self, other):
        """Rows either filter admits."""
        return self._combine(other, _lib.FILTER_OR)

    def __sub__(self, other):
        """Rows this filter admits and `other` does not."""
        return self._combine(other, _lib.FILTER_ANDNOT)

    def __invert__(self):
        """The live rows this filter does not admit."""
        return self._combine(None, _lib.FILTER_NOT)

    def ids_device(self, out_ptr: int, cap: int) -> int:
        """The admitted ids in position order into device memory at out_ptr (room for cap u32); -> rows admitted (rq_filter_ids_device)."""
        count = C.c_uint64()
        check(lib().rq_filter_ids_device(self._h, C.c_void_p(out_ptr), cap, C.byref(count)))
        return int(count.value)

    def ids(self) -> np.ndarray:
        """The admitted ids (u32) in position order, compacted on the device; the array travels through torch."""
        if self.rows == 0:
            return np.empty(0, dtype=np.uint32)
        import torch
        out = torch.empty(self.rows, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        got = self.ids_device(out.data_ptr(), self.rows)
        return out[:got].cpu().numpy().view(np.uint32)

    def id_bits(self, nbits=None) -> np.ndarray:
        """The admitted ids as a boolean mask over ids (rq_filter_id_bits), the `mask=` remove(), extract() and make_filter() take:
        `index.remove(mask=index.where(expr).id_bits())` is "delete where".  nbits: the mask's length, ids at or past it are left
        out; default 1 + the largest admitted id."""
        if nbits is None:
            ids = self.ids()
            nbits = int(ids.max()) + 1 if ids.size else 0
        nbits = int(nbits)
        if not 0 <= nbits <= (1 << 32):
            raise ValueError("ids are u32: 0 <= nbits <= 2^32")
        words = np.zeros((nbits + 31) // 32, dtype=np.uint32)
        check(lib().rq_filter_id_bits(self._h, _addr(words), nbits, 0))
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:nbits].astype(bool)


def _fh(filter):
    return filter._h if filter is not None else None


class RangeResult:
    """The answer of a range search (rq_range_search*), owned by the library and resident on the device: `nq` queries, `total`
    (distance, id) entries, query b's at [lims[b], lims[b + 1]) ascending by (distance, id).  Holds a reference to its index, so
    the index outlives it; close() (or the context manager) frees the device arrays."""

    def __init__(self, index: "RaBitQ", handle):
        self.index = index
        self._h = handle
        nq, total = C.c_uint32(), C.c_uint64()
        check(lib().rq_range_result_info(self._h, C.byref(nq), C.byref(total)))
        self.nq, self.total = int(nq.value), int(total.value)

    def device_ptrs(self):
        """-> (lims, dist, ids) raw device addresses: nq + 1 u64, total f32, total u32; valid until close()."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().rq_range_result_device_ptrs(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value or 0, b.value or 0, c.value or 0

    def to_host(self):
        """-> (lims u64[nq + 1], dist f32[total], ids u32[total]) as numpy arrays."""
        lims = np.empty(self.nq + 1, dtype=np.uint64)
        dist = np.empty(self.total, dtype=np.float32)
        ids = np.empty(self.total, dtype=np.uint32)
        check(lib().rq_range_result_copy(self._h, _addr(lims), _addr(dist), _addr(ids)))
        return lims, dist, ids

    def close(self):
        if getattr(self, "_h", None):
            lib().rq_range_result_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DiverseResult:
    """What a host-form diverse call returns.  dist / ids / div: B x topk in SELECTION order, padded with NaN / 0xFFFFFFFF / NaN
    (dist: the source's distance; div: the smallest pair distance to the rows taken before, +inf for the first); counts: rows taken
    per query; fetched: candidates the source call gave per query (None from diversify_results)."""
    __slots__ = ("dist", "ids", "div", "counts", "fetched")

    def __init__(self, dist, ids, div, counts, fetched):
        self.dist, self.ids, self.div, self.counts, self.fetched = dist, ids, div, counts, fetched

    def __repr__(self):
        return f"DiverseResult(queries={self.counts.size}, topk={self.ids.shape[1]})"


class GroupedResult:
    """What a host-form grouped call returns.  dist / ids: B x topk x group_size, group-major, padded with NaN / 0xFFFFFFFF; keys
    (the column's dtype) and group_counts (rows kept per group): B x topk, padded with 0; counts: groups per query; fetched:
    candidates the source call gave per query (None from group_results)."""
    __slots__ = ("dist", "ids", "keys", "group_counts", "counts", "fetched")

    def __init__(self, dist, ids, keys, group_counts, counts, fetched):
        self.dist, self.ids, self.keys, self.group_counts, self.counts, self.fetched = dist, ids, keys, group_counts, counts, fetched

    def __repr__(self):
        return f"GroupedResult(queries={self.counts.size}, topk={self.keys.shape[1]}, group_size={self.ids.shape[2]})"


class RaBitQ:
    """Device-resident RaBitQ index.  Construct with `from_path`, `build`, `load_from_dir` or
    `from_arrays`; query with `query` (one vector, like the crate) or `query_batch`."""

    def __init__(self, handle):
        self._h = handle
        self._refresh()

    def _refresh(self):
        info = Info()
        check(lib().rq_info(self._h, C.byref(info)))
        self.dim, self.k, self.n, self.max_list_len = int(info.dim), int(info.k), int(info.n), int(info.max_list_len)
        self.n_hbm = int(info.n_hbm)      # raw vectors in HBM; the other n - n_hbm live in pinned host memory
        self.split_rows = bool(info.split_rows)   # raw vectors stored as two 16-bit planes per row (option "split_rows")
        self.metric = _lib.METRIC_NAMES.get(int(info.metric), "l2")   # a cosine index normalises rows and queries itself; an "ip" index augments rows
        self._ip_d = self.ip_params[0] if self.metric == "ip" else 0   # the raw row length add() and the queries must have
        rt = C.c_uint32()
        check(lib().rq_row_type(self._h, C.byref(rt)))
        self.row_type = _lib.ROW_TYPE_NAMES.get(int(rt.value), "f32")   # "f16" / "bf16" / "u8" / "i8": the raw vectors are stored in that type, 2*dim / dim bytes each
        dead = C.c_uint64()
        check(lib().rq_pending_removals(self._h, C.byref(dead)))
        self.pending_removals = int(dead.value)   # stored rows marked dead by remove(lazy=True) and not compacted yet (n counts them)

    @property
    def live_n(self) -> int:
        """Rows a query can return: n - pending_removals."""
        return self.n - self.pending_removals

    # ---- RaBitQ::from_path (src/rabitq.rs:159) ------------------------------------------------
    @classmethod
    def from_path(cls, base_path, centroid_path, orthogonal=None, seed: int = 0, metric="l2", max_sq_norm=None) -> "RaBitQ":
        """Build from base.fvecs + centroids.fvecs.  `orthogonal` (dim x dim, P[r][c]) fixes the
        rotation the reference draws unseeded (src/utils.rs:16-20); None = seeded Gaussian-QR.
        metric: "l2" (the reference) or "cosine": rows and queries are normalised on the GPU, distances are 2 - 2 cos; or "ip":
        maximum inner product search, rows get one more coordinate sqrt(S - |x|^2) (index dim = ceil64(d + 1)), distances are
        S + |q|^2 - 2<x, q> (inner_product() converts), S = max_sq_norm (None: the largest squared row norm)."""
        h = C.c_void_p()
        P = _f32(orthogonal) if orthogonal is not None else None
        if _lib.metric_id(metric) == _lib.METRIC_IP:
            check(lib().rq_build_from_path_ip(os.fsencode(base_path), os.fsencode(centroid_path), _addr(P), seed,
                                              _sq_bound(max_sq_norm), C.byref(h)))
            return cls(h)
        check(lib().rq_build_from_path_metric(os.fsencode(base_path), os.fsencode(centroid_path), _addr(P), seed,
                                              _lib.metric_id(metric), C.byref(h)))
        return cls(h)

    @classmethod
    def build(cls, base, centroids, orthogonal=None, seed: int = 0, metric="l2", max_sq_norm=None, rows=None) -> "RaBitQ":
        """from_path on in-memory arrays (base n x d, centroids k x d; metric="ip": k x c with d <= c <= ceil64(d + 1), missing
        columns are zero).  A float16 `base` (or rows="f16" / rows="bf16" with a uint16 array of bit patterns) makes a half-precision
        index: the rows are stored as given, 2*dim bytes each.  rows="u8" with a uint8 array / rows="i8" with an int8 array makes a
        byte-row index (L2 only), dim bytes each; without rows= such an array is converted to f32.
        centroids=<int>: that many lists are trained first (train_centroids with this build's metric, rows, max_sq_norm and seed)."""
        if isinstance(centroids, (int, np.integer)) and not isinstance(centroids, bool):
            centroids = train_centroids(base, int(centroids), seed=seed, metric=metric, max_sq_norm=max_sq_norm, rows=rows)
        base, rt = _typed_rows(base, rows)
        centroids = _f32(centroids)
        if rt != _lib.ROWS_F32:
            if base.ndim != 2 or centroids.ndim != 2 or base.shape[1] != centroids.shape[1]:
                raise _lib.RabitqError(-2, "base and centroids must be 2-D with the same dimension (rabitq.rs:165)")
            P = _f32(orthogonal) if orthogonal is not None else None
            h = C.c_void_p()
            check(lib().rq_build_rows(_addr(base), base.shape[0], base.shape[1], _addr(centroids), centroids.shape[0], _addr(P),
                                      seed, _lib.metric_id(metric), rt, C.byref(h)))
            return cls(h)
        if _lib.metric_id(metric) == _lib.METRIC_IP:
            if base.ndim != 2 or centroids.ndim != 2:
                raise _lib.RabitqError(-2, "base and centroids must be 2-D")
            P = _f32(orthogonal) if orthogonal is not None else None
            h = C.c_void_p()
            check(lib().rq_build_ip(_addr(base), base.shape[0], base.shape[1], _addr(centroids), centroids.shape[0], _addr(P),
                                    seed, centroids.shape[1], _sq_bound(max_sq_norm), C.byref(h)))
            return cls(h)
        if base.ndim != 2 or centroids.ndim != 2 or base.shape[1] != centroids.shape[1]:
            raise _lib.RabitqError(-2, "base and centroids must be 2-D with the same dimension (rabitq.rs:165)")
        P = _f32(orthogonal) if orthogonal is not None else None
        h = C.c_void_p()
        check(lib().rq_build_metric(_addr(base), base.shape[0], base.shape[1], _addr(centroids), centroids.shape[0], _addr(P),
                                    seed, _lib.metric_id(metric), C.byref(h)))
        return cls(h)

    @classmethod
    def build_device(cls, base_ptr: int, n: int, d: int, centroids_ptr: int, k: int, orthogonal=None,
                     seed: int = 0, metric="l2", max_sq_norm=None, centroid_cols: int = None, rows="f32") -> "RaBitQ":
        """Build from device-resident arrays (raw HIP device addresses, e.g. torch.Tensor.data_ptr()).  metric="ip": the
        centroids are k x centroid_cols (None: d).  rows="f16" / "bf16" / "u8" / "i8": base_ptr holds n x d elements of that type.
        centroids_ptr=None: k lists are trained on the device first (train_centroids_device with this build's metric, rows,
        max_sq_norm and seed; the centroid buffer is a torch tensor that lives for the call)."""
        if centroids_ptr is None:
            import torch
            ip = _lib.metric_id(metric) == _lib.METRIC_IP
            learnt = torch.empty((k, d + 1 if ip else d), dtype=torch.float32, device="cuda")
            train_centroids_device(base_ptr, n, d, k, learnt.data_ptr(), seed=seed, metric=metric, max_sq_norm=max_sq_norm, rows=rows)
            centroids_ptr, centroid_cols = learnt.data_ptr(), (d + 1 if ip else None)
        P = _f32(orthogonal) if orthogonal is not None else None
        h = C.c_void_p()
        if _lib.row_type_id(rows) != _lib.ROWS_F32:
            check(lib().rq_build_device_rows(C.c_void_p(base_ptr), n, d, C.c_void_p(centroids_ptr), k, _addr(P), seed,
                                             _lib.metric_id(metric), _lib.row_type_id(rows), C.byref(h)))
            return cls(h)
        if _lib.metric_id(metric) == _lib.METRIC_IP:
            check(lib().rq_build_device_ip(C.c_void_p(base_ptr), n, d, C.c_void_p(centroids_ptr), k, _addr(P), seed,
                                           d if centroid_cols is None else centroid_cols, _sq_bound(max_sq_norm), C.byref(h)))
            return cls(h)
        check(lib().rq_build_device_metric(C.c_void_p(base_ptr), n, d, C.c_void_p(centroids_ptr), k, _addr(P), seed,
                                           _lib.metric_id(metric), C.byref(h)))
        return cls(h)

    @classmethod
    def builder(cls, n: int, d: int, centroids_ptr: int, k: int, orthogonal=None, seed: int = 0,
                max_device_base_bytes: int = 0, metric="l2", max_sq_norm=None, centroid_cols: int = None, rows="f32") -> "Builder":
        """Streamed two-pass build for inputs that are not resident (include/rabitq_hip.h: rq_builder_*).  metric="ip" needs
        max_sq_norm (the largest row_sqnorm_max over the chunks): the streamed build has no automatic bound.  rows="f16" /
        "bf16" / "u8" / "i8": the chunks hold elements of that type."""
        return Builder(n, d, centroids_ptr, k, orthogonal, seed, max_device_base_bytes, metric, max_sq_norm, centroid_cols, rows)

    # ---- load_from_dir / dump_to_dir (src/rabitq.rs:84, :128) ---------------------------------
    @classmethod
    def load_from_dir(cls, path) -> "RaBitQ":
        h = C.c_void_p()
        check(lib().rq_load_dir(os.fsencode(path), C.byref(h)))
        return cls(h)

    def dump_to_dir(self, path) -> None:
        """Refused (RQ_ERR_UNSUPPORTED) while removals are pending: a dump would bring the dead rows back -- compact() first."""
        check(lib().rq_dump_dir(self._h, os.fsencode(path)))

    # ---- load_from_json / dump_to_json (src/rabitq.rs:72-81) -------------------------------------
    @classmethod
    def load_from_json(cls, path) -> "RaBitQ":
        h = C.c_void_p()
        check(lib().rq_load_json(os.fsencode(path), C.byref(h)))
        return cls(h)

    def dump_to_json(self, path) -> None:
        """Refused (RQ_ERR_UNSUPPORTED) while removals are pending: a dump would bring the dead rows back -- compact() first."""
        check(lib().rq_dump_json(self._h, os.fsencode(path)))

    @classmethod
    def from_arrays(cls, base, orthogonal, centroids, offsets, map_ids, codes, factors, metric="l2", max_sq_norm=None,
                    d: int = None, rows=None) -> "RaBitQ":
        """From the reference's in-memory arrays (what load_from_dir produces).  The arrays are taken as they are; metric="cosine"
        only marks the index, so that its queries and added rows are normalised (`base` then holds normalised rows already).
        A float16 `base` (or rows="f16" / "bf16" with uint16 bit patterns), n x dim, makes a half-precision index; rows="u8" /
        "i8" with a uint8 / int8 array a byte-row index."""
        base, rt = _typed_rows(base, rows)
        orthogonal, centroids, factors = _f32(orthogonal), _f32(centroids), _f32(factors)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        map_ids = np.ascontiguousarray(map_ids, dtype=np.uint32)
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        h = C.c_void_p()
        if rt != _lib.ROWS_F32:
            check(lib().rq_from_arrays_rows(orthogonal.shape[0], map_ids.size, offsets.size - 1, _addr(base), _addr(orthogonal),
                                            _addr(centroids), _addr(offsets), _addr(map_ids), _addr(codes), _addr(factors),
                                            _lib.metric_id(metric), rt, C.byref(h)))
            return cls(h)
        if metric == "ip" and max_sq_norm is not None:   # an inner-product index: `base` holds augmented rows, d = the raw row length
            if d is None:
                raise ValueError('from_arrays(metric="ip") needs d, the raw row length')
            check(lib().rq_from_arrays_ip(orthogonal.shape[0], map_ids.size, offsets.size - 1, _addr(base), _addr(orthogonal),
                                          _addr(centroids), _addr(offsets), _addr(map_ids), _addr(codes), _addr(factors),
                                          int(d), float(max_sq_norm), C.byref(h)))
            return cls(h)
        check(lib().rq_from_arrays_metric(orthogonal.shape[0], map_ids.size, offsets.size - 1, _addr(base), _addr(orthogonal),
                                          _addr(centroids), _addr(offsets), _addr(map_ids), _addr(codes), _addr(factors),
                                          _lib.metric_id(metric), C.byref(h)))
        return cls(h)

    def rotate_device(self, x_ptr: int, n: int, out_ptr: int) -> float:
        """X' = X P on device-resident rows (MFMA kernel); returns the kernel time in ms (HIP events)."""
        ms = C.c_float()
        check(lib().rq_rotate_device(self._h, C.c_void_p(x_ptr), n, C.c_void_p(out_ptr), C.byref(ms)))
        return float(ms.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().rq_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- arrays (copies to host) ----------------------------------------------------------------
    def _get(self, which, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        check(lib().rq_get_array(self._h, which, _addr(out), out.nbytes))
        return out

    @property
    def base(self):
        """The raw vectors as f32, cluster order (a half-precision or byte-row index: its rows widened)."""
        return self._get(ARR_BASE, (self.n, self.dim), np.float32)

    @property
    def base_rows(self):
        """The raw vectors in the type the index stores: float32, float16, (bf16) uint16 bit patterns, uint8 or int8."""
        if self.row_type == "f32":
            return self.base
        return self._get(ARR_BASE_ROWS, (self.n, self.dim), _lib.ROW_TYPE_BY_NAME[self.row_type].returns)

    @property
    def orthogonal(self):
        return self._get(ARR_ORTHOGONAL, (self.dim, self.dim), np.float32)

    @property
    def centroids(self):
        return self._get(ARR_CENTROIDS, (self.k, self.dim), np.float32)

    @property
    def offsets(self):
        return self._get(ARR_OFFSETS, (self.k + 1,), np.uint32)

    @property
    def map_ids(self):
        return self._get(ARR_MAP_IDS, (self.n,), np.uint32)

    @property
    def codes(self):
        return self._get(ARR_CODES, (self.n, self.dim // 64), np.uint64)

    @property
    def factors(self):
        return self._get(ARR_FACTORS, (self.n, 4), np.float32)

    def device_ptr(self, which):
        p, nbytes = C.c_void_p(), C.c_uint64()
        check(lib().rq_get_device_ptr(self._h, which, C.byref(p), C.byref(nbytes)))
        return p.value, nbytes.value

    # ---- filters: answer from a subset of the index --------------------------------------------
    def make_filter(self, ids=None, mask=None) -> Filter:
        """A filter admitting the original ids `ids` (an id array) or those where `mask` (a boolean mask over ids) is set;
        packed on the host (pack_filter_bits), turned into the index's terms on the device once."""
        words, nbits = pack_filter_bits(ids=ids, mask=mask)
        h = C.c_void_p()
        check(lib().rq_filter_create(self._h, _addr(words), nbits, 0, C.byref(h)))
        return Filter(self, h)

    def make_filter_device(self, bits_ptr: int, nbits: int) -> Filter:
        """A filter from an id bitmap already in device memory (bit (id & 31) of u32 word id >> 5)."""
        h = C.c_void_p()
        check(lib().rq_filter_create(self._h, C.c_void_p(bits_ptr), nbits, 1, C.byref(h)))
        return Filter(self, h)

    # ---- attribute columns: per-row values in position order, predicates over them as filters -------
    def create_attr(self, name: str, dtype, fill=0) -> None:
        """A new column `name` of dtype "u32" / "i32" / "f32" / "u64" / "i64" (or the numpy dtype), every row holding `fill`
        (rq_attr_create).  At most 16 columns; a name is 1-31 bytes of [A-Za-z0-9_]."""
        t = self._attr_type(dtype)
        image = int(np.array([fill]).astype(t.dtype).view(np.uint32 if t.elem_bytes == 4 else np.uint64)[0])
        check(lib().rq_attr_create(self._h, name.encode(), t.id, image))

    def drop_attr(self, name: str) -> None:
        check(lib().rq_attr_drop(self._h, name.encode()))

    @staticmethod
    def _attr_type(dtype):
        if isinstance(dtype, str) and dtype in _lib.ATTR_BY_NAME:
            return _lib.ATTR_BY_NAME[dtype]
        for t in _lib.ATTR_TABLE:
            if not isinstance(dtype, str) and np.dtype(dtype) == np.dtype(t.dtype):
                return t
        raise ValueError(f"dtype must be one of {sorted(_lib.ATTR_BY_NAME)} or their numpy dtypes, not {dtype!r}")

    def attrs(self) -> list:
        """The columns in rq_attr_info order: [{"name", "dtype", "fill", "bytes"}]."""
        cnt = C.c_uint32()
        check(lib().rq_attr_count(self._h, C.byref(cnt)))
        out = []
        for i in range(cnt.value):
            info = _lib.AttrInfoT()
            check(lib().rq_attr_info(self._h, i, C.byref(info)))
            t = _lib.ATTR_BY_ID[int(info.type)]
            fill = np.array([info.fill.u64], dtype=np.uint64).view(t.dtype)[0]
            out.append({"name": info.name.decode(), "dtype": t.name, "fill": fill.item(), "bytes": int(info.bytes)})
        return out

    def _attr(self, name):
        for a in self.attrs():
            if a["name"] == name:
                return _lib.ATTR_BY_NAME[a["dtype"]]
        raise _lib.RabitqError(-1, f"the index has no column named {name}")

    def set_attr(self, name: str, ids, values) -> int:
        """values[i] becomes the value of the row with id ids[i] (rq_attr_set); a scalar `values` goes to every id.  Ids the index
        does not hold (or dead ones) are skipped -> how many were.  Where an id repeats, its last value wins.  Positions do not
        change: existing filters stay valid and keep the rows they selected."""
        t = self._attr(name)
        idv = self._id_list(ids)
        vals = np.asarray(values)
        if vals.ndim == 0:
            vals = np.full(idv.shape, vals)
        vals = np.ascontiguousarray(vals.astype(t.dtype, copy=False))
        if vals.shape != idv.shape:
            raise ValueError(f"values must have one value per id ({idv.size}), not shape {vals.shape}")
        absent = C.c_uint64()
        check(lib().rq_attr_set(self._h, name.encode(), _addr(idv), _addr(vals), idv.size, C.byref(absent)))
        return int(absent.value)

    def get_attr(self, name: str, ids):
        """-> (values in the column's dtype, found bool): the value of each id; an absent id gives the fill value and False."""
        t = self._attr(name)
        idv = self._id_list(ids)
        vals = np.empty(idv.size, dtype=t.dtype)
        found = np.zeros(idv.size, dtype=np.uint32)
        check(lib().rq_attr_get(self._h, name.encode(), _addr(idv), idv.size, _addr(vals), _addr(found)))
        return vals, found.astype(bool)

    def attr_array(self, name: str) -> np.ndarray:
        """The whole column in position order: element p belongs to the row whose id is map_ids[p] (rq_attr_get_array)."""
        t = self._attr(name)
        self._refresh()
        out = np.empty(self.n, dtype=t.dtype)
        check(lib().rq_attr_get_array(self._h, name.encode(), _addr(out), out.nbytes))
        return out

    def where(self, expr) -> Filter:
        """A filter of the rows a predicate over the columns holds for, evaluated on the device (rq_filter_create_where):
        `idx.where((col("tenant") == 7) & (col("ts") >= t0))`.  See rabitq_amd/where.py for the expression forms."""
        from . import where as W
        terms, program = W.compile_expr(expr)
        cols = {a["name"]: (i, _lib.ATTR_BY_NAME[a["dtype"]]) for i, a in enumerate(self.attrs())}
        arr = (_lib.WhereTermT * max(len(terms), 1))()
        keep = []   # the sets' host arrays, alive until the call returns
        for i, t in enumerate(terms):
            if t.column not in cols:
                raise _lib.RabitqError(-1, f"the index has no column named {t.column}")
            ci, at = cols[t.column]
            view = np.uint32 if at.elem_bytes == 4 else np.uint64
            image = lambda v: int(self._attr_const(v, at).view(view)[0])
            arr[i].column, arr[i].op = ci, t.op
            arr[i].a.u64, arr[i].b.u64 = image(t.a), image(t.b)
            if t.op == W.OP_IN:
                vals = np.concatenate([self._attr_const(v, at) for v in t.values]) if t.values else np.empty(0, dtype=at.dtype)
                keep.append(vals)
                arr[i].set, arr[i].set_count = vals.ctypes.data, vals.size
        prog = np.asarray(program, dtype=np.uint8)
        h = C.c_void_p()
        check(lib().rq_filter_create_where(self._h, arr, len(terms), _addr(prog), prog.size, C.byref(h)))
        return Filter(self, h)

    @staticmethod
    def _attr_const(v, at):
        """A predicate's constant in the column's type, as a 1-element array: exact, or ValueError (an integer the type cannot
        hold, a fraction for an integer column)."""
        if at.name == "f32":
            return np.array([v], dtype=np.float32)
        if isinstance(v, (float, np.floating)) and not float(v).is_integer():
            raise ValueError(f"{v!r} is not a value of an integer ({at.name}) column")
        iv = int(v)
        info = np.iinfo(at.dtype)
        if not info.min <= iv <= info.max:
            raise ValueError(f"{iv} is not a value of a {at.name} column")
        return np.array([iv], dtype=at.dtype)

    @staticmethod
    def last_where_stats() -> dict:
        return last_where_stats()

    # ---- in-place mutation: the index afterwards equals a fresh build of its live rows -------------
    def _rows(self, vectors):
        v = np.asarray(vectors)
        if v.dtype.kind not in "fiu":
            raise TypeError(f"vectors must be real numbers, not {v.dtype}")
        if v.ndim != 2:
            raise ValueError(f"vectors must be 2-D (m x d), not {v.ndim}-D")
        if getattr(self, "_ip_d", 0):   # rows of an inner-product index's own d: rq_add augments them
            if v.shape[1] != self._ip_d:
                raise _lib.RabitqError(-2, f"row length {v.shape[1]} is not the inner-product index's row length {self._ip_d}")
        elif v.shape[1] == 0 or (v.shape[1] + 63) // 64 * 64 != self.dim:
            raise _lib.RabitqError(-2, f"row length {v.shape[1]} does not pad to index dim {self.dim}")
        return _f32(v)

    @staticmethod
    def _ids(ids, m):
        a = np.asarray(ids)
        if a.dtype.kind not in "iu":
            raise TypeError(f"ids must be integers, not {a.dtype}")
        if a.ndim != 1 or a.size != m:
            raise ValueError(f"ids must be 1-D with one id per row ({m}), not shape {a.shape}")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("ids are u32: 0 <= id < 2^32")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def add(self, vectors, ids=None) -> np.ndarray:
        """Insert rows (m x d, d padding to dim) -> the u32 ids they got: `ids` (absent from the index, unique), or by default
        the next ids after the largest the index holds.  One relayout (include/rabitq_hip.h: rq_add); filters made before it
        are refused afterwards.  With removals pending the index is compacted first (one more relayout): the id of a dead row
        is free again, and the next ids follow the largest LIVE id."""
        rows = self._rows(vectors)
        m = rows.shape[0]
        idv = self._ids(ids, m) if ids is not None else None
        first = C.c_uint32()
        check(lib().rq_add(self._h, _addr(rows), m, rows.shape[1], _addr(idv), 0, C.byref(first)))
        self._refresh()
        return idv.copy() if idv is not None else np.arange(m, dtype=np.uint64).astype(np.uint32) + np.uint32(first.value)

    def add_device(self, rows_ptr: int, m: int, d: int, ids_ptr: int = None) -> int:
        """rq_add on device-resident rows (raw HIP device addresses, as build_device takes); ids_ptr: m u32 ids on the device,
        None = the next ids.  -> the first id given (default ids: ids first .. first + m - 1)."""
        first = C.c_uint32()
        check(lib().rq_add(self._h, C.c_void_p(rows_ptr), m, d, C.c_void_p(ids_ptr or 0), 1, C.byref(first)))
        self._refresh()
        return int(first.value)

    def remove(self, ids=None, mask=None, lazy: bool = False) -> int:
        """Remove the ids `ids` (an id array) or those where `mask` (a boolean mask over ids) is set; ids not in the index are
        ignored.  -> rows removed.  One relayout (rq_remove) unless nothing matched; it drops pending removals too.
        lazy=True (rq_remove_lazy): the rows are only marked dead -- no relayout, no second copy of the arrays, and it works on
        typed, tiered and split-row indexes too.  Every query answers as after the eager removal, through the filtered pass,
        until compact(); -> rows newly dead (ids already dead are ignored).  Filters made before a call that marks anything
        are refused afterwards."""
        if ids is not None:
            a = np.asarray(ids)
            if a.size and a.dtype.kind not in "iu":
                raise TypeError(f"ids must be integers, not {a.dtype}")
        words, nbits = pack_filter_bits(ids=ids, mask=mask)
        removed = C.c_uint64()
        entry = lib().rq_remove_lazy if lazy else lib().rq_remove
        check(entry(self._h, _addr(words), nbits, 0, C.byref(removed)))
        self._refresh()
        return int(removed.value)

    def compact(self) -> int:
        """Drop the pending removals in one relayout (rq_compact) -> rows dropped; 0 and no change when none is pending.  An index
        that cannot be mutated eagerly (typed, tiered or split rows) answers RQ_ERR_UNSUPPORTED and keeps its pending removals."""
        removed = C.c_uint64()
        check(lib().rq_compact(self._h, C.byref(removed)))
        self._refresh()
        return int(removed.value)

    def update(self, ids, vectors, lazy: bool = False) -> None:
        """Give the ids `ids` the rows `vectors` (ids not in the index are inserted): remove followed by add with those ids --
        two relayouts, not one.  `lazy` goes to the remove (the add then compacts first: still two relayouts, no eager scan)."""
        rows = self._rows(vectors)
        idv = self._ids(ids, rows.shape[0])
        if np.unique(idv).size != idv.size:
            raise ValueError("ids must be unique")
        self.remove(ids=idv, lazy=lazy)
        self.add(rows, idv)

    # ---- merge / extract: stored rows move as they stand, nothing is quantised again ----------------
    def merge_from(self, other: "RaBitQ", ids="append") -> int:
        """Take in the live rows of `other`, an index over the same rotation, centroids, metric and dim (rq_merge_from): this
        index afterwards equals a fresh build of both row sets.  ids: "append" = other's ids + (1 + the largest id held here),
        "keep" = other's ids as they are (none may be held here), or an int shift added to other's ids.  -> the shift applied.
        `other` is not changed and stays usable; filters made on this index before are refused afterwards.  With removals
        pending here the index is compacted first; with removals pending in `other` the call is refused (RQ_ERR_UNSUPPORTED):
        compact `other`, or extract its live rows, first."""
        if not isinstance(other, RaBitQ):
            raise TypeError(f"other must be a RaBitQ index, not {type(other).__name__}")
        if other is self:
            raise ValueError("an index cannot be merged into itself")
        if isinstance(ids, str):
            modes = {"append": _lib.MERGE_IDS_APPEND, "keep": _lib.MERGE_IDS_KEEP}
            if ids not in modes:
                raise ValueError(f'ids must be "append", "keep" or an int shift, not {ids!r}')
            mode, shift = modes[ids], 0
        elif isinstance(ids, (int, np.integer)) and not isinstance(ids, bool):
            if not 0 <= int(ids) <= 0xFFFFFFFF:
                raise ValueError("ids are u32: 0 <= shift < 2^32")
            mode, shift = _lib.MERGE_IDS_SHIFT, int(ids)
        else:
            raise TypeError(f'ids must be "append", "keep" or an int shift, not {type(ids).__name__}')
        applied = C.c_uint32()
        check(lib().rq_merge_from(self._h, other._h, mode, shift, C.byref(applied)))
        self._refresh()
        return int(applied.value)

    def extract(self, ids=None, mask=None) -> "RaBitQ":
        """A new index holding the rows whose ids are in `ids` (an id array) or where `mask` (a boolean mask over ids) is set, ids
        kept (rq_extract): what remove() of the complement would leave, without touching this index.  Rows marked dead by
        remove(lazy=True) are never taken."""
        if ids is not None:
            a = np.asarray(ids)
            if a.size and a.dtype.kind not in "iu":
                raise TypeError(f"ids must be integers, not {a.dtype}")
        words, nbits = pack_filter_bits(ids=ids, mask=mask)
        h = C.c_void_p()
        check(lib().rq_extract(self._h, _addr(words), nbits, 0, C.byref(h)))
        return type(self)(h)

    def copy(self) -> "RaBitQ":
        """A second index equal to this one: extract() with every id (no bitmap is made: RQ_EXTRACT_ALL_IDS).  With removals
        pending the copy holds the live rows only -- it is this index compacted."""
        h = C.c_void_p()
        check(lib().rq_extract(self._h, None, _lib.EXTRACT_ALL_IDS, 0, C.byref(h)))
        return type(self)(h)

    # ---- RaBitQ::query (src/rabitq.rs:268) ------------------------------------------------------
    def query(self, query, probe: int, topk: int, heuristic_rank: bool = False, filter: Filter = None):
        """-> list of (distance, original id), at most topk, in the reference's (unspecified,
        heap-internal) order.  filter: only its rows can be returned (the filtered batch entry with one query)."""
        q = _f32(query).reshape(-1)
        d = np.empty(max(topk, 1), dtype=np.float32)
        ids = np.empty(max(topk, 1), dtype=np.uint32)
        n = C.c_uint32()
        if filter is None:
            check(lib().rq_query(self._h, _addr(q), q.size, probe, topk, int(heuristic_rank), _addr(d), _addr(ids),
                                 C.cast(C.byref(n), C.c_void_p)))
        else:
            check(lib().rq_query_batch_filtered(self._h, _fh(filter), _addr(q), 1, q.size, probe, topk, int(heuristic_rank),
                                                _addr(d), _addr(ids), C.cast(C.byref(n), C.c_void_p)))
        return [(float(d[i]), int(ids[i])) for i in range(n.value)]

    def query_batch(self, queries, probe: int, topk: int, heuristic_rank: bool = False, filter: Filter = None):
        """B queries at once -> (dist B x topk f32, ids B x topk u32, counts B u32)."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        B = q.shape[0]
        d = np.full((B, max(topk, 1)), np.nan, dtype=np.float32)
        ids = np.full((B, max(topk, 1)), 0xFFFFFFFF, dtype=np.uint32)
        cnt = np.zeros(B, dtype=np.uint32)
        if filter is None:
            st = lib().rq_query_batch(self._h, _addr(q), B, q.shape[1], probe, topk, int(heuristic_rank), _addr(d),
                                      _addr(ids), _addr(cnt))
        else:
            st = lib().rq_query_batch_filtered(self._h, _fh(filter), _addr(q), B, q.shape[1], probe, topk, int(heuristic_rank),
                                               _addr(d), _addr(ids), _addr(cnt))
        if st != _lib.RQ_ERR_EMPTY:
            check(st)
        return d, ids, cnt

    def query_batch_device(self, q_ptr: int, nq: int, length: int, probe: int, topk: int, out_dist_ptr: int,
                           out_id_ptr: int, out_n_ptr: int, heuristic_rank: bool = False, filter: Filter = None):
        """Queries and outputs already in device memory (raw addresses)."""
        if filter is None:
            check(lib().rq_query_batch_device(self._h, C.c_void_p(q_ptr), nq, length, probe, topk, int(heuristic_rank),
                                              C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr), C.c_void_p(out_n_ptr)))
        else:
            check(lib().rq_query_batch_device_filtered(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length, probe, topk,
                                                       int(heuristic_rank), C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr),
                                                       C.c_void_p(out_n_ptr)))

    # ---- exact search: brute-force top-k over the stored rows (rq_exact_search*) -----------------
    @staticmethod
    def _exact_params(params):
        """None, an ExactParamsT, or a dict of its fields (seed_probe, cand_per_query, flags: test hooks, result-neutral)."""
        if params is None or isinstance(params, _lib.ExactParamsT):
            return params
        return _lib.ExactParamsT(**params)

    def exact_search(self, queries, topk: int, filter: Filter = None, params=None):
        """The true topk nearest stored rows of every query, on the GPU -> (dist B x topk f32, ids B x topk u32, counts B u32),
        ascending by (distance, id); slots past a query's count hold NaN / 0xFFFFFFFF.  filter: only its rows can be returned."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        B = q.shape[0]
        d = np.full((B, max(topk, 1)), np.nan, dtype=np.float32)
        ids = np.full((B, max(topk, 1)), 0xFFFFFFFF, dtype=np.uint32)
        cnt = np.zeros(B, dtype=np.uint32)
        prm = self._exact_params(params)
        check(lib().rq_exact_search(self._h, _fh(filter), _addr(q), B, q.shape[1], topk, C.byref(prm) if prm is not None else None,
                                    _addr(d), _addr(ids), _addr(cnt)))
        return d, ids, cnt

    def exact_search_device(self, q_ptr: int, nq: int, length: int, topk: int, out_dist_ptr: int, out_id_ptr: int, out_n_ptr: int,
                            filter: Filter = None, params=None):
        """exact_search with queries and outputs already in device memory (raw addresses)."""
        prm = self._exact_params(params)
        check(lib().rq_exact_search_device(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length, topk,
                                           C.byref(prm) if prm is not None else None, C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr),
                                           C.c_void_p(out_n_ptr)))

    # ---- rows by id: locate, fetch, exact distances to known ids, neighbours of stored rows (rq_locate ...) ----
    @staticmethod
    def _id_list(ids):
        """ids of a by-id call -> contiguous u32 array (any shape; the result keeps it)."""
        a = np.asarray(ids)
        if a.dtype.kind not in "iu":
            raise TypeError(f"ids must be integers, not {a.dtype}")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("ids are u32: 0 <= id < 2^32")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def locate(self, ids) -> np.ndarray:
        """Cluster-order positions of `ids` (u32, the shape of ids): what rq_rerank takes and base / map_ids are ordered by;
        0xFFFFFFFF for an id the index does not hold or whose row is dead.  Valid until the next relayout."""
        a = self._id_list(ids)
        out = np.empty(a.shape, dtype=np.uint32)
        check(lib().rq_locate(self._h, _addr(a), a.size, _addr(out)))
        return out

    def contains(self, ids) -> np.ndarray:
        """Boolean, the shape of ids: the index holds a live row with that id."""
        return self.locate(ids) != np.uint32(_lib.POS_ABSENT)

    def fetch(self, ids, stored: bool = False, raw: bool = True):
        """The rows of `ids` (1-D) -> (rows, found): rows[i] is the row `base` holds for ids[i], bit for bit (f32, m x dim); with
        stored=True the row as `base_rows` holds it, in the index's row type (an f32 index raises, as base_rows' array id does).
        raw=True cuts the rows of an inner-product index to its d (the augmented coordinate and the padding off); the rows of
        other indexes keep dim.  An absent id gives a row of zeros and found[i] == False."""
        a = self._id_list(ids).reshape(-1)
        found = np.zeros(a.size, dtype=np.uint32)
        if stored:
            rows = np.zeros((a.size, self.dim), dtype=_lib.ROW_TYPE_BY_NAME[self.row_type].returns)
            check(lib().rq_fetch_stored(self._h, _addr(a), a.size, _addr(rows), _addr(found)))
        else:
            rows = np.zeros((a.size, self.dim), dtype=np.float32)
            check(lib().rq_fetch_rows(self._h, _addr(a), a.size, _addr(rows), _addr(found)))
        if raw and self._ip_d:
            rows = np.ascontiguousarray(rows[:, :self._ip_d])
        return rows, found.astype(bool)

    def fetch_device(self, ids_ptr: int, m: int, out_rows_ptr: int, out_found_ptr: int = 0, stored: bool = False) -> None:
        """fetch with ids and outputs in device memory (raw addresses; rows m x dim f32, or m x dim elements with stored=True;
        16-byte aligned; found m x u32, 0 = not wanted)."""
        fn = lib().rq_fetch_stored_device if stored else lib().rq_fetch_rows_device
        check(fn(self._h, C.c_void_p(ids_ptr), m, C.c_void_p(out_rows_ptr), C.c_void_p(out_found_ptr)))

    def locate_device(self, ids_ptr: int, m: int, out_pos_ptr: int) -> None:
        """locate with ids and positions in device memory (raw addresses)."""
        check(lib().rq_locate_device(self._h, C.c_void_p(ids_ptr), m, C.c_void_p(out_pos_ptr)))

    def distances_to(self, queries, ids) -> np.ndarray:
        """Exact distances from query i (B x d, raw: transformed and padded as in query_batch) to its own ids[i] (B x c) -> B x c
        f32, bit for bit the rerank's value for that row; +inf for an absent id.  (An "ip" index: inner_product() converts.)"""
        q = _f32(queries)
        a = self._id_list(ids)
        if q.ndim != 2 or a.ndim != 2 or a.shape[0] != q.shape[0]:
            raise _lib.RabitqError(-1, "queries must be B x d and ids B x c")
        out = np.empty(a.shape, dtype=np.float32)
        check(lib().rq_pair_distances(self._h, _addr(q), q.shape[0], q.shape[1], _addr(a), a.shape[1], _addr(out)))
        return out

    def neighbours_of(self, ids, probe: int, topk: int, filter: Filter = None, heuristic_rank: bool = False, exact: bool = False):
        """The neighbours of stored rows -> (dist m x topk, ids m x topk, found m): row i is what query_batch (exact=True:
        exact_search; probe is not used) returns at topk + 1 for the stored row of ids[i] (fetch(ids)[0][i]) without the row
        itself -- the first entry with id ids[i] is removed, or the last entry if the row is not among them (outside the
        probed lists or the filter).  Short rows are padded with NaN / 0xFFFFFFFF; an absent id gives such a row and
        found[i] == False.  One call on the GPU: lookup, gather, the query, the removal."""
        a = self._id_list(ids).reshape(-1)
        m = a.size
        d = np.full((m, max(topk, 1)), np.nan, dtype=np.float32)
        out = np.full((m, max(topk, 1)), 0xFFFFFFFF, dtype=np.uint32)
        found = np.zeros(m, dtype=np.uint32)
        if exact:
            st = lib().rq_neighbours_of_exact(self._h, _addr(a), m, topk, _fh(filter), None, _addr(d), _addr(out), _addr(found))
        else:
            st = lib().rq_neighbours_of(self._h, _addr(a), m, probe, topk, int(heuristic_rank), _fh(filter), _addr(d), _addr(out),
                                        _addr(found))
        if st != _lib.RQ_ERR_EMPTY:
            check(st)
        return d, out, found.astype(bool)

    def neighbours_of_device(self, ids_ptr: int, m: int, probe: int, topk: int, out_dist_ptr: int, out_id_ptr: int, out_found_ptr: int,
                             filter: Filter = None, heuristic_rank: bool = False, exact: bool = False) -> None:
        """neighbours_of with ids and outputs in device memory (raw addresses)."""
        if exact:
            st = lib().rq_neighbours_of_exact_device(self._h, C.c_void_p(ids_ptr), m, topk, _fh(filter), None, C.c_void_p(out_dist_ptr),
                                                     C.c_void_p(out_id_ptr), C.c_void_p(out_found_ptr))
        else:
            st = lib().rq_neighbours_of_device(self._h, C.c_void_p(ids_ptr), m, probe, topk, int(heuristic_rank), _fh(filter),
                                               C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr), C.c_void_p(out_found_ptr))
        if st != _lib.RQ_ERR_EMPTY:
            check(st)

    def knn_graph(self, probe: int, topk: int, exact: bool = False, chunk: int = 65536):
        """The k-NN graph of the index -> (ids, neigh_dist, neigh_ids): every live id in ascending order and, through
        neighbours_of in chunks of `chunk` ids, its topk neighbours (n_live x topk; padded as neighbours_of pads)."""
        ids = np.sort(self.map_ids)
        ids = ids[self.contains(ids)] if self.pending_removals else ids
        nd = np.full((ids.size, max(topk, 1)), np.nan, dtype=np.float32)
        ni = np.full((ids.size, max(topk, 1)), 0xFFFFFFFF, dtype=np.uint32)
        for i0 in range(0, ids.size, max(int(chunk), 1)):
            sl = slice(i0, i0 + max(int(chunk), 1))
            nd[sl], ni[sl], _ = self.neighbours_of(ids[sl], probe, topk, exact=exact)
        return ids, nd, ni

    @staticmethod
    def last_by_id_stats() -> dict:
        """The calling thread's last by-id call (include/rabitq_hip.h: rq_by_id_stats_t); form as "dense" / "hash"."""
        return last_by_id_stats()

    # ---- grouped search: at most group_size rows per value of a column, the topk nearest values (rq_*_grouped, rq_group_results) ----
    @staticmethod
    def _group_params(topk, group_size, fetch):
        f = _lib.default_group_fetch(topk, group_size) if fetch is None else int(fetch)
        return _lib.GroupParamsT(topk=int(topk), group_size=int(group_size), fetch=f, flags=0)

    def _grouped_host(self, call, B, prm, group_by, with_fetched):
        """The outputs of a host-form grouped call, made, filled by call(addresses...) and wrapped."""
        t = self._attr(group_by)
        cells = (B, max(prm.topk, 1), max(prm.group_size, 1))
        d = np.full(cells, np.nan, dtype=np.float32)
        ids = np.full(cells, 0xFFFFFFFF, dtype=np.uint32)
        keys = np.zeros(cells[:2], dtype=np.uint64)
        gn = np.zeros(cells[:2], dtype=np.uint32)
        cnt = np.zeros(B, dtype=np.uint32)
        fetched = np.zeros(B, dtype=np.uint32) if with_fetched else None
        st = call(_addr(d), _addr(ids), _addr(keys), _addr(gn), _addr(cnt), *([_addr(fetched)] if with_fetched else []))
        if st != _lib.RQ_ERR_EMPTY:
            check(st)
        if t.elem_bytes == 4:
            keys = keys.astype(np.uint32)   # (the u64 image of a 4-byte value is zero-extended)
        return GroupedResult(d, ids, keys.view(t.dtype), gn, cnt, fetched)

    def query_batch_grouped(self, queries, probe: int, topk: int, group_by: str, group_size: int = 1, fetch=None,
                            heuristic_rank: bool = False, filter: Filter = None) -> "GroupedResult":
        """The topk nearest VALUES of the integer column `group_by`, at most group_size rows each, out of what query_batch returns
        at topk = fetch -- grouped on the GPU, nothing travels to the host in between.  Groups come in order of their nearest row,
        rows inside a group ascending by (distance, id).  fetch=None means min(2048, max(64, 4 * topk * group_size)): a default, not
        a guarantee -- result.fetched[b] == fetch says query b may have more to give (raise fetch)."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        prm = self._group_params(topk, group_size, fetch)
        return self._grouped_host(lambda *out: lib().rq_query_batch_grouped(
            self._h, _fh(filter), _addr(q), q.shape[0], q.shape[1], probe, int(heuristic_rank), group_by.encode(), C.byref(prm), *out),
            q.shape[0], prm, group_by, True)

    def exact_search_grouped(self, queries, topk: int, group_by: str, group_size: int = 1, fetch=None, filter: Filter = None,
                             params=None) -> "GroupedResult":
        """query_batch_grouped over exact_search at topk = fetch.  Where result.fetched[b] < fetch the answer is the true grouped
        answer over all admitted rows; with group_size == 1, counts[b] == topk proves it too."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        prm = self._group_params(topk, group_size, fetch)
        ex = self._exact_params(params)
        return self._grouped_host(lambda *out: lib().rq_exact_search_grouped(
            self._h, _fh(filter), _addr(q), q.shape[0], q.shape[1], C.byref(ex) if ex is not None else None, group_by.encode(),
            C.byref(prm), *out), q.shape[0], prm, group_by, True)

    def group_results(self, dist, ids, counts, topk: int, group_by: str, group_size: int = 1) -> "GroupedResult":
        """The selection alone over result rows the caller has (dist / ids B x fetch, counts B; fetch = their width): those of
        tickets, the adaptive call, neighbours_of or the sharded step.  The order inside a row does not matter; an id without a
        live row is skipped (last_group_stats()["absent"])."""
        d = np.ascontiguousarray(dist, dtype=np.float32)
        i = self._id_list(ids)
        c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if d.ndim != 2 or i.shape != d.shape or c.size != d.shape[0]:
            raise _lib.RabitqError(-1, "dist and ids must be B x fetch and counts B")
        prm = self._group_params(topk, group_size, d.shape[1])
        return self._grouped_host(lambda *out: lib().rq_group_results(
            self._h, _addr(d), _addr(i), _addr(c), d.shape[0], group_by.encode(), C.byref(prm), *out), d.shape[0], prm, group_by, False)

    def query_batch_grouped_device(self, q_ptr: int, nq: int, length: int, probe: int, topk: int, group_by: str, out_dist_ptr: int,
                                   out_id_ptr: int, out_key_ptr: int, out_group_n_ptr: int, out_n_ptr: int, out_fetched_ptr: int = 0,
                                   group_size: int = 1, fetch=None, heuristic_rank: bool = False, filter: Filter = None) -> None:
        """query_batch_grouped with queries and outputs in device memory (raw addresses; dist / ids nq x topk x group_size, keys u64
        and group counts nq x topk, counts and fetched nq; fetched 0 = not wanted)."""
        prm = self._group_params(topk, group_size, fetch)
        st = lib().rq_query_batch_grouped_device(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length, probe, int(heuristic_rank),
                                                 group_by.encode(), C.byref(prm), C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr),
                                                 C.c_void_p(out_key_ptr), C.c_void_p(out_group_n_ptr), C.c_void_p(out_n_ptr),
                                                 C.c_void_p(out_fetched_ptr))
        if st != _lib.RQ_ERR_EMPTY:
            check(st)

    def exact_search_grouped_device(self, q_ptr: int, nq: int, length: int, topk: int, group_by: str, out_dist_ptr: int, out_id_ptr: int,
                                    out_key_ptr: int, out_group_n_ptr: int, out_n_ptr: int, out_fetched_ptr: int = 0, group_size: int = 1,
                                    fetch=None, filter: Filter = None, params=None) -> None:
        """exact_search_grouped with queries and outputs in device memory (raw addresses, as query_batch_grouped_device)."""
        prm = self._group_params(topk, group_size, fetch)
        ex = self._exact_params(params)
        check(lib().rq_exact_search_grouped_device(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length,
                                                   C.byref(ex) if ex is not None else None, group_by.encode(), C.byref(prm),
                                                   C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr), C.c_void_p(out_key_ptr),
                                                   C.c_void_p(out_group_n_ptr), C.c_void_p(out_n_ptr), C.c_void_p(out_fetched_ptr)))

    def group_results_device(self, dist_ptr: int, id_ptr: int, cnt_ptr: int, nq: int, fetch: int, topk: int, group_by: str,
                             out_dist_ptr: int, out_id_ptr: int, out_key_ptr: int, out_group_n_ptr: int, out_n_ptr: int,
                             group_size: int = 1) -> None:
        """group_results with the rows (stride fetch) and outputs in device memory (raw addresses)."""
        prm = self._group_params(topk, group_size, fetch)
        check(lib().rq_group_results_device(self._h, C.c_void_p(dist_ptr), C.c_void_p(id_ptr), C.c_void_p(cnt_ptr), nq, group_by.encode(),
                                            C.byref(prm), C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr), C.c_void_p(out_key_ptr),
                                            C.c_void_p(out_group_n_ptr), C.c_void_p(out_n_ptr)))

    @staticmethod
    def last_group_stats() -> dict:
        """The calling thread's last grouped call (include/rabitq_hip.h: rq_group_stats_t)."""
        return last_group_stats()

    # ---- diverse search: the topk rows MMR takes out of `fetch` candidates (rq_*_diverse, rq_diversify_results) ----
    @staticmethod
    def _diverse_params(topk, lam, fetch):
        f = _lib.default_diverse_fetch(topk) if fetch is None else int(fetch)
        return _lib.DiverseParamsT(topk=int(topk), fetch=f, lambda_=float(lam), flags=0)

    @staticmethod
    def _diverse_host(call, B, prm, with_fetched):
        """The outputs of a host-form diverse call, made, filled by call(addresses...) and wrapped."""
        cells = (B, max(prm.topk, 1))
        d = np.full(cells, np.nan, dtype=np.float32)
        ids = np.full(cells, 0xFFFFFFFF, dtype=np.uint32)
        div = np.full(cells, np.nan, dtype=np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        fetched = np.zeros(B, dtype=np.uint32) if with_fetched else None
        st = call(_addr(d), _addr(ids), _addr(div), _addr(cnt), *([_addr(fetched)] if with_fetched else []))
        if st != _lib.RQ_ERR_EMPTY:
            check(st)
        return DiverseResult(d, ids, div, cnt, fetched)

    def query_batch_diverse(self, queries, probe: int, topk: int, lam: float = 0.5, fetch=None, heuristic_rank: bool = False,
                            filter: Filter = None) -> "DiverseResult":
        """The topk rows that maximal marginal relevance takes, greedily, out of what query_batch returns at topk = fetch --
        selected on the GPU, no row travels to the host.  Each step takes the candidate with the smallest
        lam * distance - (1 - lam) * (smallest pair distance to the rows already taken); lam = 1 is the plain call's order, lam = 0
        diversity alone.  The pair distance is the engine's squared L2 between STORED rows (2 - 2 cos on a cosine index, the
        augmented space's distance on an inner-product index).  fetch=None means min(2048, max(64, 4 * topk)): a default, not a
        guarantee -- the selection sees no row beyond the first `fetch`."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        prm = self._diverse_params(topk, lam, fetch)
        return self._diverse_host(lambda *out: lib().rq_query_batch_diverse(
            self._h, _fh(filter), _addr(q), q.shape[0], q.shape[1], probe, int(heuristic_rank), C.byref(prm), *out), q.shape[0], prm, True)

    def exact_search_diverse(self, queries, topk: int, lam: float = 0.5, fetch=None, filter: Filter = None, params=None) -> "DiverseResult":
        """query_batch_diverse over exact_search at topk = fetch."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        prm = self._diverse_params(topk, lam, fetch)
        ex = self._exact_params(params)
        return self._diverse_host(lambda *out: lib().rq_exact_search_diverse(
            self._h, _fh(filter), _addr(q), q.shape[0], q.shape[1], C.byref(ex) if ex is not None else None, C.byref(prm), *out),
            q.shape[0], prm, True)

    def diversify_results(self, dist, ids, counts, topk: int, lam: float = 0.5) -> "DiverseResult":
        """The selection alone over result rows the caller has (dist / ids B x fetch, counts B; fetch = their width).  The order
        inside a row does not matter; an id without a live row is skipped (last_diverse_stats()["absent"]), and so is a distance
        that is not finite (["skipped"])."""
        d = np.ascontiguousarray(dist, dtype=np.float32)
        i = self._id_list(ids)
        c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if d.ndim != 2 or i.shape != d.shape or c.size != d.shape[0]:
            raise _lib.RabitqError(-1, "dist and ids must be B x fetch and counts B")
        prm = self._diverse_params(topk, lam, d.shape[1])
        return self._diverse_host(lambda *out: lib().rq_diversify_results(
            self._h, _addr(d), _addr(i), _addr(c), d.shape[0], C.byref(prm), *out), d.shape[0], prm, False)

    def query_batch_diverse_device(self, q_ptr: int, nq: int, length: int, probe: int, topk: int, out_dist_ptr: int, out_id_ptr: int,
                                   out_div_ptr: int, out_n_ptr: int, out_fetched_ptr: int = 0, lam: float = 0.5, fetch=None,
                                   heuristic_rank: bool = False, filter: Filter = None) -> None:
        """query_batch_diverse with queries and outputs in device memory (raw addresses; dist / ids / div nq x topk, counts and
        fetched nq; fetched 0 = not wanted)."""
        prm = self._diverse_params(topk, lam, fetch)
        st = lib().rq_query_batch_diverse_device(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length, probe, int(heuristic_rank),
                                                 C.byref(prm), C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr), C.c_void_p(out_div_ptr),
                                                 C.c_void_p(out_n_ptr), C.c_void_p(out_fetched_ptr))
        if st != _lib.RQ_ERR_EMPTY:
            check(st)

    def exact_search_diverse_device(self, q_ptr: int, nq: int, length: int, topk: int, out_dist_ptr: int, out_id_ptr: int, out_div_ptr: int,
                                    out_n_ptr: int, out_fetched_ptr: int = 0, lam: float = 0.5, fetch=None, filter: Filter = None,
                                    params=None) -> None:
        """exact_search_diverse with queries and outputs in device memory (raw addresses, as query_batch_diverse_device)."""
        prm = self._diverse_params(topk, lam, fetch)
        ex = self._exact_params(params)
        check(lib().rq_exact_search_diverse_device(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length,
                                                   C.byref(ex) if ex is not None else None, C.byref(prm), C.c_void_p(out_dist_ptr),
                                                   C.c_void_p(out_id_ptr), C.c_void_p(out_div_ptr), C.c_void_p(out_n_ptr),
                                                   C.c_void_p(out_fetched_ptr)))

    def diversify_results_device(self, dist_ptr: int, id_ptr: int, cnt_ptr: int, nq: int, fetch: int, topk: int, out_dist_ptr: int,
                                 out_id_ptr: int, out_div_ptr: int, out_n_ptr: int, lam: float = 0.5) -> None:
        """diversify_results with the rows (stride fetch) and outputs in device memory (raw addresses)."""
        prm = self._diverse_params(topk, lam, fetch)
        check(lib().rq_diversify_results_device(self._h, C.c_void_p(dist_ptr), C.c_void_p(id_ptr), C.c_void_p(cnt_ptr), nq, C.byref(prm),
                                                C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr), C.c_void_p(out_div_ptr),
                                                C.c_void_p(out_n_ptr)))

    @staticmethod
    def last_diverse_stats() -> dict:
        """The calling thread's last diverse call (include/rabitq_hip.h: rq_diverse_stats_t)."""
        return last_diverse_stats()

    @staticmethod
    def _recall_of(ids, cnt, exact_ids, exact_cnt) -> float:
        """mean over the queries with a non-empty exact answer of |query ids n exact ids| / exact count"""
        vals = [len(np.intersect1d(ids[b, :cnt[b]], exact_ids[b, :exact_cnt[b]])) / int(exact_cnt[b])
                for b in range(len(exact_cnt)) if exact_cnt[b]]
        return float(np.mean(vals)) if vals else 1.0

    def recall(self, queries, probe: int, topk: int, filter: Filter = None, heuristic_rank: bool = False) -> float:
        """What fraction of the true topk neighbours query_batch(queries, probe, topk) returns: the mean over the queries of
        |query ids n exact ids| / exact count (queries whose exact answer is empty are left out; none left: 1.0)."""
        _, eids, ecnt = self.exact_search(queries, topk, filter)
        _, ids, cnt = self.query_batch(queries, probe, topk, heuristic_rank, filter)
        return self._recall_of(ids, cnt, eids, ecnt)

    def tune_nprobe(self, queries, topk: int, target_recall: float, filter: Filter = None):
        """The smallest nprobe whose recall on these queries reaches target_recall -> (nprobe, recall); (k, recall at k) when the
        target is out of reach.  The exact answer is computed once; every probe value tried is one query_batch: doubling from 1
        until the target is met, then bisection between the last miss and the first hit."""
        _, eids, ecnt = self.exact_search(queries, topk, filter)
        seen = {}

        def at(p):
            if p not in seen:
                _, ids, cnt = self.query_batch(queries, p, topk, False, filter)
                seen[p] = self._recall_of(ids, cnt, eids, ecnt)
            return seen[p]

        lo, hi = 0, 1                      # lo: the largest value known to miss (0: none), hi: the value being tried
        while at(hi) < target_recall:
            if hi >= self.k:
                return self.k, at(self.k)
            lo, hi = hi, min(2 * hi, self.k)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if at(mid) >= target_recall:
                hi = mid
            else:
                lo = mid
        return hi, at(hi)

    # ---- adaptive probing: each query's probe list cut by centroid distance (rq_probe_rule_t) ----
    @staticmethod
    def _probe_rule(ratio, min_probe, caps_addr):
        """-> the rq_probe_rule_t of (ratio, min_probe) with max_probe at the raw address caps_addr (None: no array)."""
        return _lib.ProbeRuleT(min_probe=int(min_probe), ratio=float(ratio), reserved=0, max_probe=caps_addr)

    @staticmethod
    def _caps(max_probe, B):
        """max_probe= -> None, or a contiguous uint32[B] (a scalar is one cap for every query)."""
        if max_probe is None:
            return None
        return np.array(np.broadcast_to(np.asarray(max_probe, dtype=np.uint32), (B,)), dtype=np.uint32, order="C")   # (a writable copy)

    def query_batch_adaptive(self, queries, probe: int, topk: int, ratio: float = float("inf"), min_probe: int = 1, max_probe=None,
                             heuristic_rank: bool = False, filter: Filter = None):
        """query_batch with every query's probe list cut by centroid distance -> (dist, ids, counts, nprobe uint32[B]).
        With d_0 <= d_1 <= ... the query's coarse distances over its min(probe, k) nearest lists, the query visits
        n = min(cap, max(min_probe, p)) of them, p = the longest prefix with d_j <= ratio * d_0 (f32) and cap = its entry of
        max_probe (None: no cap); its row is exactly that of query_batch(probe=n).  ratio=inf cuts nothing; max_probe with
        ratio=inf is a per-query nprobe."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        B = q.shape[0]
        d = np.full((B, max(topk, 1)), np.nan, dtype=np.float32)
        ids = np.full((B, max(topk, 1)), 0xFFFFFFFF, dtype=np.uint32)
        cnt = np.zeros(B, dtype=np.uint32)
        npr = np.zeros(B, dtype=np.uint32)
        caps = self._caps(max_probe, B)
        rule = self._probe_rule(ratio, min_probe, caps.ctypes.data if caps is not None else None)
        st = lib().rq_query_batch_adaptive(self._h, _fh(filter), _addr(q), B, q.shape[1], probe, topk, int(heuristic_rank),
                                           C.byref(rule), _addr(d), _addr(ids), _addr(cnt), _addr(npr))
        if st != _lib.RQ_ERR_EMPTY:
            check(st)
        return d, ids, cnt, npr

    def query_batch_adaptive_device(self, q_ptr: int, nq: int, length: int, probe: int, topk: int, out_dist_ptr: int,
                                    out_id_ptr: int, out_n_ptr: int, out_nprobe_ptr: int = None, ratio: float = float("inf"),
                                    min_probe: int = 1, max_probe_ptr: int = None, heuristic_rank: bool = False, filter: Filter = None):
        """query_batch_adaptive with queries, caps (max_probe_ptr: uint32[nq] or None) and outputs already in device memory (raw
        addresses; out_nprobe_ptr may be None)."""
        rule = self._probe_rule(ratio, min_probe, max_probe_ptr)
        check(lib().rq_query_batch_device_adaptive(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length, probe, topk,
                                                   int(heuristic_rank), C.byref(rule), C.c_void_p(out_dist_ptr),
                                                   C.c_void_p(out_id_ptr), C.c_void_p(out_n_ptr), C.c_void_p(out_nprobe_ptr)))

    def probe_counts(self, queries, probe: int, ratio: float, min_probe: int = 1, max_probe=None) -> np.ndarray:
        """How many lists each query would visit under the rule of query_batch_adaptive -> uint32[B].  Runs only the query
        transform, the rotation, the coarse ranking and the cut (rq_probe_counts_device); the arrays travel through torch."""
        import torch
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        B = q.shape[0]
        _lib.check(lib().rq_init(0))
        dq = torch.from_numpy(q).cuda()
        caps = self._caps(max_probe, B)
        dcaps = torch.from_numpy(caps.view(np.int32)).cuda() if caps is not None else None
        out = torch.zeros(max(B, 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rule = self._probe_rule(ratio, min_probe, dcaps.data_ptr() if dcaps is not None else None)
        check(lib().rq_probe_counts_device(self._h, C.c_void_p(dq.data_ptr()), B, q.shape[1], probe, C.byref(rule),
                                           C.c_void_p(out.data_ptr())))
        return out[:B].cpu().numpy().view(np.uint32).copy()

    def tune_probe_ratio(self, queries, probe: int, topk: int, target_recall: float, min_probe: int = 1, filter: Filter = None):
        """A ratio for query_batch_adaptive(queries, probe, topk, ratio, min_probe) whose recall on these queries reaches
        target_recall -> (ratio, recall, mean_nprobe).  The exact answer is computed once.  If ratio=inf (no cut) misses the target:
        (inf, that recall, min(probe, k)).  Otherwise 12 steps of geometric bisection on the ratio between 1 and the largest finite
        d_{m-1} / d_0 of the batch; the smallest ratio tried that meets the target is returned.  As with tune_nprobe, recall is
        only nearly monotone in the ratio: a smaller ratio than the one returned may also meet the target."""
        _, eids, ecnt = self.exact_search(queries, topk, filter)
        m = min(int(probe), self.k)

        def at(r):
            _, ids, cnt, npr = self.query_batch_adaptive(queries, probe, topk, r, min_probe, None, False, filter)
            return self._recall_of(ids, cnt, eids, ecnt), float(np.mean(npr)) if len(npr) else float(m)

        rec_inf, _ = at(float("inf"))
        if rec_inf < target_recall:
            return float("inf"), rec_inf, float(m)
        q = _f32(queries)
        cd = np.empty((q.shape[0], m), dtype=np.float32)
        cc = np.empty((q.shape[0], m), dtype=np.uint32)
        check(lib().rq_coarse_rank(self._h, _addr(q), q.shape[0], q.shape[1], m, _addr(None), _addr(cc), _addr(cd)))
        with np.errstate(divide="ignore", invalid="ignore"):
            spread = cd[:, -1].astype(np.float64) / cd[:, 0].astype(np.float64)
        spread = spread[np.isfinite(spread)]
        hi = float(np.float32(max(1.0, float(spread.max()) if spread.size else 1.0)) * np.float32(1.0 + 2.0 ** -20))
        rec_hi, mean_hi = at(hi)
        if rec_hi < target_recall:          # (rows whose d_0 is 0 or not finite are cut by every finite ratio)
            return float("inf"), rec_inf, float(m)
        best = (hi, rec_hi, mean_hi)
        lo = 1.0
        for _ in range(12):
            mid = float(np.sqrt(lo * hi))
            rec, mean = at(mid)
            if rec >= target_recall:
                hi, best = mid, (mid, rec, mean)
            else:
                lo = mid
        return best

    # ---- range search: every neighbour within a per-query radius --------------------------------
    @property
    def ip_params(self):
        """(d, S) of an inner-product index: the raw row length and the bound on the squared row norms."""
        d, s = C.c_uint32(), C.c_float()
        check(lib().rq_ip_params(self._h, C.byref(d), C.byref(s)))
        return int(d.value), np.float32(s.value)

    def inner_product(self, dist, queries, counts=None):
        """The inner products an "ip" index's distances stand for: ip = 0.5 * ((S + |q|^2) - dist), in f32 on the GPU.  dist is
        B x topk as query_batch returns it; with counts (its third result) the slots past a query's count get -inf."""
        q, dist = _f32(queries), _f32(dist)
        if q.ndim != 2 or dist.ndim != 2 or dist.shape[0] != q.shape[0]:
            raise _lib.RabitqError(-1, "queries must be B x d and dist B x topk")
        n = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        out = np.empty_like(dist)
        check(lib().rq_ip_from_dist(self._h, _addr(q), q.shape[0], q.shape[1], _addr(dist), dist.shape[1], _addr(n), _addr(out)))
        return out

    def ip_radius(self, queries, min_ip):
        """The range_search radius that stands for "inner product above min_ip" on an "ip" index, one per query."""
        q = _f32(queries)
        m = np.asarray(min_ip, dtype=np.float32)
        m = np.full(q.shape[0], m, dtype=np.float32) if m.ndim == 0 else np.ascontiguousarray(m.reshape(-1))
        if q.ndim != 2 or m.size != q.shape[0]:
            raise _lib.RabitqError(-1, "queries must be B x d and min_ip a scalar or one value per query")
        out = np.empty(q.shape[0], np.float32)
        check(lib().rq_ip_radius(self._h, _addr(q), q.shape[0], q.shape[1], _addr(m), _addr(out)))
        return out

    def range_search(self, queries, probe: int, radius=None, filter: Filter = None, min_ip=None):
        """B queries -> (lims u64[B + 1], dist f32[total], ids u32[total]): query b's neighbours with estimate and exact squared
        distance both strictly below radius[b] (a scalar = the same radius for every query), among the rows of its `probe` nearest
        lists, at [lims[b], lims[b + 1]) ascending by (distance, id).  filter: only its rows can be returned.
        min_ip (an "ip" index, instead of radius): the neighbours whose inner product is above min_ip[b] (ip_radius)."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        if (radius is None) == (min_ip is None):
            raise _lib.RabitqError(-1, "give either radius or min_ip")
        if min_ip is not None:
            radius = self.ip_radius(q, min_ip)
        r = np.asarray(radius, dtype=np.float32)
        r = np.full(q.shape[0], r, dtype=np.float32) if r.ndim == 0 else np.ascontiguousarray(r.reshape(-1))
        if r.size != q.shape[0]:
            raise _lib.RabitqError(-1, f"radius must be a scalar or one value per query ({q.shape[0]}), not {r.size}")
        h = C.c_void_p()
        check(lib().rq_range_search(self._h, _fh(filter), _addr(q), q.shape[0], q.shape[1], probe, _addr(r), C.byref(h)))
        with RangeResult(self, h) as res:
            return res.to_host()

    def range_search_device(self, q_ptr: int, nq: int, length: int, probe: int, radius_ptr: int, filter: Filter = None) -> RangeResult:
        """Queries (nq x length) and radii (nq f32) already in device memory (raw addresses) -> a RangeResult whose arrays stay
        on the device."""
        h = C.c_void_p()
        check(lib().rq_range_search_device(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length, probe, C.c_void_p(radius_ptr),
                                           C.byref(h)))
        return RangeResult(self, h)

    # ---- exact range search: every stored row within a per-query radius (rq_exact_range_search*) ----
    def _radii(self, q, radius, min_ip):
        """One f32 radius per query from radius= (a scalar or one per query) or min_ip= (an "ip" index: ip_radius)."""
        if (radius is None) == (min_ip is None):
            raise _lib.RabitqError(-1, "give either radius or min_ip")
        if min_ip is not None:
            radius = self.ip_radius(q, min_ip)
        r = np.asarray(radius, dtype=np.float32)
        r = np.full(q.shape[0], r, dtype=np.float32) if r.ndim == 0 else np.ascontiguousarray(r.reshape(-1))
        if r.size != q.shape[0]:
            raise _lib.RabitqError(-1, f"radius must be a scalar or one value per query ({q.shape[0]}), not {r.size}")
        return r

    def exact_range_search(self, queries, radius=None, filter: Filter = None, min_ip=None, params=None):
        """B queries -> (lims u64[B + 1], dist f32[total], ids u32[total]): EVERY stored row whose exact squared distance is strictly
        below radius[b] (a scalar = the same radius for every query), at [lims[b], lims[b + 1]) ascending by (distance, id): what
        range_search is measured against.  filter: only its rows can be returned.  min_ip (an "ip" index, instead of radius): the rows
        whose inner product is above min_ip[b] (ip_radius).  params: the exact search's test hooks (result-neutral)."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        r = self._radii(q, radius, min_ip)
        prm = self._exact_params(params)
        h = C.c_void_p()
        check(lib().rq_exact_range_search(self._h, _fh(filter), _addr(q), q.shape[0], q.shape[1], _addr(r),
                                          C.byref(prm) if prm is not None else None, C.byref(h)))
        with RangeResult(self, h) as res:
            return res.to_host()

    def exact_range_search_device(self, q_ptr: int, nq: int, length: int, radius_ptr: int, filter: Filter = None, params=None) -> RangeResult:
        """exact_range_search with queries (nq x length) and radii (nq f32) already in device memory (raw addresses) -> a
        RangeResult whose arrays stay on the device."""
        prm = self._exact_params(params)
        h = C.c_void_p()
        check(lib().rq_exact_range_search_device(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length, C.c_void_p(radius_ptr),
                                                 C.byref(prm) if prm is not None else None, C.byref(h)))
        return RangeResult(self, h)

    def range_recall(self, queries, probe: int, radius=None, filter: Filter = None, min_ip=None) -> float:
        """What fraction of the exact range answer range_search(queries, probe, ...) returns, pooled over the queries:
        sum_b |A_b n E_b| / sum_b |E_b| (A: the approximate answer's ids, E: the exact one's); 1.0 when E is empty everywhere."""
        q = _f32(queries)
        if q.ndim != 2:
            raise _lib.RabitqError(-1, "queries must be 2-D")
        r = self._radii(q, radius, min_ip)
        el, _, ei = self.exact_range_search(q, radius=r, filter=filter)
        al, _, ai = self.range_search(q, probe, radius=r, filter=filter)
        if int(el[-1]) == 0:
            return 1.0
        found = sum(len(np.intersect1d(ai[int(al[b]):int(al[b + 1])], ei[int(el[b]):int(el[b + 1])])) for b in range(q.shape[0]))
        return found / int(el[-1])

    def query_batch_device_begin(self, q_ptr: int, nq: int, length: int, probe: int, topk: int, out_dist_ptr: int,
                                 out_id_ptr: int, out_n_ptr: int, heuristic_rank: bool = False, filter: Filter = None):
        """Enqueue a device-resident batch and return a ticket; finish it with query_batch_device_end(ticket).
        Batches begun back to back overlap on the device (each has its own workspace and stream).
        filter: only its rows can be returned; it must stay open until the ticket has been ended."""
        t = C.c_void_p()
        if filter is None:
            check(lib().rq_query_batch_device_begin(self._h, C.c_void_p(q_ptr), nq, length, probe, topk, int(heuristic_rank),
                                                    C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr), C.c_void_p(out_n_ptr),
                                                    C.byref(t)))
        else:
            check(lib().rq_query_batch_device_begin_filtered(self._h, _fh(filter), C.c_void_p(q_ptr), nq, length, probe, topk,
                                                             int(heuristic_rank), C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr),
                                                             C.c_void_p(out_n_ptr), C.byref(t)))
        return t

    @staticmethod
    def query_batch_device_end(ticket) -> None:
        check(lib().rq_query_batch_device_end(ticket))


    # ---- sharded deployments ---------------------------------------------------------------------
    def coarse_topk_device(self, q_ptr: int, nq: int, length: int, list_lo: int, list_hi: int, probe: int,
                           out_cluster_ptr: int, out_dist_ptr: int) -> None:
        """The `probe` nearest lists among [list_lo, list_hi) per query (device buffers nq x probe)."""
        check(lib().rq_coarse_topk_device(self._h, C.c_void_p(q_ptr), nq, length, list_lo, list_hi, probe,
                                          C.c_void_p(out_cluster_ptr), C.c_void_p(out_dist_ptr)))

    def query_batch_device_probed(self, q_ptr: int, nq: int, length: int, probe_cluster_ptr: int, probe_dist_ptr: int,
                                  probe: int, topk: int, out_dist_ptr: int, out_id_ptr: int, out_n_ptr: int,
                                  heuristic_rank: bool = False) -> None:
        """query_batch_device with caller-supplied probe lists (nq x probe, visiting order)."""
        check(lib().rq_query_batch_device_probed(self._h, C.c_void_p(q_ptr), nq, length, C.c_void_p(probe_cluster_ptr),
                                                 C.c_void_p(probe_dist_ptr), probe, topk, int(heuristic_rank),
                                                 C.c_void_p(out_dist_ptr), C.c_void_p(out_id_ptr), C.c_void_p(out_n_ptr)))


    def query_batch_device_seeded(self, q_ptr: int, nq: int, length: int, probe_cluster_ptr: int, probe_dist_ptr: int,
                                  probe: int, topk: int, thr_init_ptr: int, out_dist_ptr: int, out_id_ptr: int,
                                  out_n_ptr: int, heuristic_rank: bool = False) -> None:
        """query_batch_device_probed with per-query initial thresholds (nq floats on the device, f32 max = none)."""
        check(lib().rq_query_batch_device_seeded(self._h, C.c_void_p(q_ptr), nq, length, C.c_void_p(probe_cluster_ptr),
                                                 C.c_void_p(probe_dist_ptr), probe, topk, int(heuristic_rank),
                                                 C.c_void_p(thr_init_ptr), C.c_void_p(out_dist_ptr),
                                                 C.c_void_p(out_id_ptr), C.c_void_p(out_n_ptr)))

    def partition_lists(self, world: int):
        """Greedy-by-length assignment of whole lists to `world` shards -> (owner u32[k], load u64[world])."""
        owner = np.zeros(self.k, dtype=np.uint32)
        load = np.zeros(world, dtype=np.uint64)
        check(lib().rq_partition_lists(self._h, world, _addr(owner), _addr(load)))
        return owner, load

    def shard(self, owner, rank: int) -> "RaBitQ":
        """The shard of `rank`: same centroids and rotation, only the lists with owner[c] == rank (original ids kept).
        Refused (RQ_ERR_UNSUPPORTED) while removals are pending: compact() first.  A shard itself refuses remove(lazy=True)."""
        owner = np.ascontiguousarray(owner, dtype=np.uint32)
        assert owner.size == self.k
        h = C.c_void_p()
        check(lib().rq_shard_index(self._h, _addr(owner), rank, C.byref(h)))
        return RaBitQ(h)

    def query_batch_sharded_device(self, comm: int, world: int, id_offset: int, q_ptr: int, nq: int, length: int,
                                   probe: int, topk: int, out_dist_ptr: int, out_id_ptr: int, out_n_ptr: int,
                                   heuristic_rank: bool = False) -> None:
        """The multi-GPU step through the C ABI: local shard query, ONE ncclAllGather on `comm` (an ncclComm_t address;
        0 when world == 1), k-way merge.  Every rank gets the same global top-k."""
        check(lib().rq_query_batch_sharded_device(self._h, C.c_void_p(comm), world, id_offset, C.c_void_p(q_ptr), nq, length,
                                                  probe, topk, int(heuristic_rank), C.c_void_p(out_dist_ptr),
                                                  C.c_void_p(out_id_ptr), C.c_void_p(out_n_ptr)))


class Builder:
    """assign_chunk every row -> order() -> place_chunk every row -> finish() -> RaBitQ.  Chunks are device pointers."""

    def __init__(self, n, d, centroids_ptr, k, orthogonal=None, seed=0, max_device_base_bytes=0, metric="l2", max_sq_norm=None,
                 centroid_cols=None, rows="f32"):
        P = _f32(orthogonal) if orthogonal is not None else None
        self._b = C.c_void_p()
        self._typed = _lib.row_type_id(rows) != _lib.ROWS_F32   # chunks of the builder's row type go through the _rows calls
        if self._typed:
            check(lib().rq_builder_create_rows(n, d, C.c_void_p(centroids_ptr), k, _addr(P), seed, max_device_base_bytes,
                                               _lib.metric_id(metric), _lib.row_type_id(rows), C.byref(self._b)))
            return
        if _lib.metric_id(metric) == _lib.METRIC_IP:
            check(lib().rq_builder_create_ip(n, d, C.c_void_p(centroids_ptr), k, _addr(P), seed, max_device_base_bytes,
                                             d if centroid_cols is None else centroid_cols, _sq_bound(max_sq_norm), C.byref(self._b)))
            return
        check(lib().rq_builder_create_metric(n, d, C.c_void_p(centroids_ptr), k, _addr(P), seed, max_device_base_bytes,
                                             _lib.metric_id(metric), C.byref(self._b)))

    def assign_chunk(self, rows_ptr: int, i0: int, m: int) -> None:
        fn = lib().rq_builder_assign_chunk_rows if self._typed else lib().rq_builder_assign_chunk
        check(fn(self._b, C.c_void_p(rows_ptr), i0, m))

    def order(self) -> None:
        check(lib().rq_builder_order(self._b))

    def place_chunk(self, rows_ptr: int, i0: int, m: int) -> None:
        fn = lib().rq_builder_place_chunk_rows if self._typed else lib().rq_builder_place_chunk
        check(fn(self._b, C.c_void_p(rows_ptr), i0, m))

    def stats(self) -> dict:
        st = BuildStatsT()
        check(lib().rq_builder_stats(self._b, C.byref(st)))
        return {name: getattr(st, name) for name, _ in BuildStatsT._fields_ if name != "struct_size"}

    def finish(self) -> RaBitQ:
        h = C.c_void_p()
        b, self._b = self._b, None
        check(lib().rq_builder_finish(b, C.byref(h)))
        return RaBitQ(h)

    def __del__(self):
        if getattr(self, "_b", None):
            lib().rq_builder_free(self._b)
            self._b = None


# ---- METRICS (src/metrics.rs) --------------------------------------------------------------------
def metrics() -> dict:
    m = MetricsT()
    check(lib().rq_metrics(C.byref(m)))
    return {"query": m.query, "rough": m.rough, "precise": m.precise, "miss": m.miss}


def metrics_reset() -> None:
    check(lib().rq_metrics_reset())


def metrics_str() -> str:
    """Metrics::to_str, src/metrics.rs:30-41."""
    m = metrics()
    ratio = m["rough"] / m["precise"] if m["precise"] else float("nan")
    return (f"query: {m['query']}, rough: {m['rough']}, precise: {m['precise']}, ratio: {ratio:.2f}, "
            f"cache miss: {m['miss']}")


def set_profiling(level) -> None:
    """0/False = off, 1/True = HIP events around every kernel group, 2 = around the scan launches only."""
    check(lib().rq_set_profiling(int(level)))


def set_option(name: str, value: int) -> None:
    """Engine options (include/rabitq_hip.h: rq_set_option), e.g. set_option("scan_impl", 1)."""
    check(lib().rq_set_option(name.encode(), int(value)))


def last_profile() -> dict:
    p = ProfileT()
    check(lib().rq_last_profile(C.byref(p)))
    return {name: getattr(p, name) for name, _ in ProfileT._fields_ if name != "struct_size"}


def last_mutate_stats() -> dict:
    """The calling thread's last add / remove / merge_from / extract by phase (include/rabitq_hip.h: rq_last_mutate_stats)."""
    st = _lib.MutateStatsT()
    check(lib().rq_last_mutate_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _lib.MutateStatsT._fields_ if name not in ("struct_size", "reserved0")}


def last_exact_stats() -> dict:
    """The calling thread's last exact search (include/rabitq_hip.h: rq_last_exact_stats)."""
    st = _lib.ExactStatsT()
    check(lib().rq_last_exact_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _lib.ExactStatsT._fields_ if name not in ("struct_size", "reserved0")}


def last_by_id_stats() -> dict:
    """The calling thread's last by-id call (include/rabitq_hip.h: rq_last_by_id_stats)."""
    st = _lib.ByIdStatsT()
    check(lib().rq_last_by_id_stats(C.byref(st)))
    out = {name: getattr(st, name) for name, _ in _lib.ByIdStatsT._fields_ if name not in ("struct_size", "reserved0")}
    out["form"] = _lib.DIRECTORY_FORMS.get(out["form"], out["form"])
    return out


def last_where_stats() -> dict:
    """The calling thread's last where() (include/rabitq_hip.h: rq_last_where_stats)."""
    st = _lib.WhereStatsT()
    check(lib().rq_last_where_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _lib.WhereStatsT._fields_ if name != "struct_size"}


def last_diverse_stats() -> dict:
    """The calling thread's last diverse call (include/rabitq_hip.h: rq_last_diverse_stats)."""
    st = _lib.DiverseStatsT()
    check(lib().rq_last_diverse_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _lib.DiverseStatsT._fields_ if name not in ("struct_size", "reserved0")}


def last_group_stats() -> dict:
    """The calling thread's last grouped call (include/rabitq_hip.h: rq_last_group_stats)."""
    st = _lib.GroupStatsT()
    check(lib().rq_last_group_stats(C.byref(st)))
    return {name: getattr(st, name) for name, _ in _lib.GroupStatsT._fields_ if name not in ("struct_size", "reserved0")}


def calculate_recall(truth, res, topk: int) -> float:
    """src/utils.rs:367-379 (host-side bookkeeping of the CLI harness, crates/cli/src/main.rs:73-74)."""
    res = list(res)
    assert len(res) == topk
    t = list(truth)[:topk]
    return sum(1 for r in res if r in t) / topk
