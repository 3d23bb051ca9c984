"""rabitq_amd -- MI355X (gfx950) engine for the RaBitQ build/query hot path of kemingy/rabitq.

Host-side mirror of the crate's public surface (`pub use rabitq::RaBitQ`, src/lib.rs:12) over the
C ABI in include/rabitq_hip.h.  All arithmetic runs in hand-written HIP kernels
(rabitq_amd/csrc); there is no CPU fallback.
"""
from .index import RaBitQ, Filter, RangeResult, pack_filter_bits, widen, metrics, metrics_reset, metrics_str, calculate_recall, last_exact_stats, last_by_id_stats, last_where_stats, last_group_stats, GroupedResult, last_diverse_stats, DiverseResult, train_centroids, train_centroids_device, TrainStats  # noqa: F401
from . import ops, vecs, where  # noqa: F401
from .where import col  # noqa: F401
from .ops import normalize, cosine_similarity, augment, row_sqnorm_max  # noqa: F401
from ._lib import RabitqError, build  # noqa: F401

__all__ = ["RaBitQ", "Filter", "RangeResult", "pack_filter_bits", "widen", "metrics", "metrics_reset", "metrics_str", "calculate_recall", "last_exact_stats", "last_by_id_stats", "last_where_stats", "last_group_stats", "GroupedResult", "last_diverse_stats", "DiverseResult", "col", "where", "train_centroids", "train_centroids_device", "TrainStats", "normalize", "cosine_similarity", "augment", "row_sqnorm_max", "ops", "vecs", "RabitqError",
           "build"]
