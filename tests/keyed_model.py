"""The model of the keyed exact search (include/rabitq_hip.h, "KEYED EXACT SEARCH"): query b is answered by the existing
idx.exact_search under idx.where(col(column) == keys[b]) [& extra] -- a path pinned to the oracle by tests/test_exact_search_gpu.py
and tests/test_attr_gpu.py.  A key no live row holds gives count 0 and untouched slots.  Not a conftest: import it."""
import numpy as np

from rabitq_amd import col


def keyed_reference(idx, column, queries, keys, topk, extra=None, live_values=None):
    """-> (dist, ids, counts) as exact_search_keyed returns them.  live_values: the column's values of the live rows when the postings
    were made (default: as they are now); a key outside them is absent."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    B = q.shape[0]
    dist = np.full((B, topk), np.nan, dtype=np.float32)
    ids = np.full((B, topk), 0xFFFFFFFF, dtype=np.uint32)
    cnt = np.zeros(B, dtype=np.uint32)
    held = set(np.unique(idx.attr_array(column) if live_values is None else live_values).tolist())
    filters = {}
    for b in range(B):
        key = int(keys[b])
        if key not in held:
            continue
        if key not in filters:
            f = idx.where(col(column) == key)
            filters[key] = f & extra if extra is not None else f
        dist[b], ids[b], cnt[b:b + 1] = (a[0] for a in idx.exact_search(q[b:b + 1], topk, filter=filters[key]))
    return dist, ids, cnt


def same_bits(got, want):
    """dist, ids and counts bit for bit (NaN padding included)."""
    return (np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2], want[2]))
