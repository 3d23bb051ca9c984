"""A numpy model of the per-list merge behind rq_merge_from / rq_extract (kernels_relayout.h: merge_lists_kernel), written the way the
kernel places rows -- by ranks and counts, never by sorting -- so that tests/test_merge_model.py can hold it against a plain sort.

An index is (offsets[k + 1], key words[n], ids[n]); inside a list the rows ascend by the 64-bit key (key word << 32 | id).  Not a
test module and not a conftest: import it."""
import numpy as np


def keys64(words, ids, shift=0):
    return (np.asarray(words, dtype=np.uint64) << np.uint64(32)) | (np.asarray(ids, dtype=np.uint64) + np.uint64(shift))


def merge_lists(off_a, words_a, ids_a, off_b, words_b, ids_b, shift=0):
    """-> (offsets of the merged index, src_of_dst): src_of_dst[dst] = a position of A (< n_a) or n_a + a position of B, whose
    ids count with `shift` added.  A row of A lands at (its rank in its list) + (keys of B's list below its key), a row of B
    symmetrically; keys must not tie across the two (ids are unique after the collision check)."""
    off_a, off_b = np.asarray(off_a, dtype=np.int64), np.asarray(off_b, dtype=np.int64)
    k, n_a = off_a.size - 1, int(off_a[-1])
    ka, kb = keys64(words_a, ids_a), keys64(words_b, ids_b, shift)
    out_off = off_a + off_b
    src_of_dst = np.full(int(out_off[-1]), 0xFFFFFFFF, dtype=np.uint32)
    for c in range(k):
        a, b = ka[off_a[c]:off_a[c + 1]], kb[off_b[c]:off_b[c + 1]]
        ra = np.arange(a.size) + np.searchsorted(b, a, side="left")     # keys of B below each key of A
        rb = np.arange(b.size) + np.searchsorted(a, b, side="left")
        src_of_dst[out_off[c] + ra] = off_a[c] + np.arange(a.size)
        src_of_dst[out_off[c] + rb] = n_a + off_b[c] + np.arange(b.size)
    return out_off.astype(np.uint32), src_of_dst


def extract_lists(off, ids, allowed):
    """-> (offsets of the sub-index, src_of_dst): the rows whose id is below allowed.size with allowed[id] set, every list in its
    stored order (a kept row's place is its rank among its list's kept rows: the merge with an empty other side)."""
    off, ids = np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    allowed = np.asarray(allowed, dtype=bool)
    keep = np.zeros(ids.size, dtype=bool)
    inr = ids < allowed.size
    keep[inr] = allowed[ids[inr]]
    k = off.size - 1
    out_off = np.zeros(k + 1, dtype=np.int64)
    src_of_dst = np.full(int(keep.sum()), 0xFFFFFFFF, dtype=np.uint32)
    for c in range(k):
        kept = keep[off[c]:off[c + 1]]
        out_off[c + 1] = out_off[c] + int(kept.sum())
        rank = np.cumsum(kept) - 1                                      # rank among the list's kept rows
        src_of_dst[out_off[c] + rank[kept]] = off[c] + np.nonzero(kept)[0]
    return out_off.astype(np.uint32), src_of_dst
