"""Numpy model of the rows-by-id layer (rabitq_amd/csrc/kernels_directory.h, host_directory.h): the rule between the
two directory forms, the hash function and a table builder, locate, and drop_self.  Pure numpy; the tests of both files use it."""
import numpy as np

ABSENT = 0xFFFFFFFF          # RQ_POS_ABSENT, and the padding id of a neighbour row
HASH_MUL = 0x9E3779B1        # home(id) = ((id * HASH_MUL) mod 2^32) >> (32 - log2(cap))
EMPTY = 0xFFFFFFFFFFFFFFFF   # an empty slot of the hash form (slots are id << 32 | pos)


def is_dense(top: int, n: int) -> bool:
    """The form rule: the dense array over [0, top) where it is at most 4 entries per row plus 65536; top = 1 + the largest id."""
    return top <= 4 * n + 65536


def hash_bits(n: int) -> int:
    """log2 of the hash table's capacity: the power of two >= max(2 n, 16)."""
    bits = 4
    while (1 << bits) < 2 * n:
        bits += 1
    return bits


def home(ids, bits: int):
    """Home slot of every id in a table of 2^bits slots."""
    ids = np.asarray(ids, dtype=np.uint64)
    return (((ids * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)).astype(np.int64)


def build_table(map_ids, bits: int = None):
    """The hash form of map_ids (position p holds id map_ids[p]), rows inserted in position order with linear probing ->
    (slots u64[2^bits], chain[p] = slots insertion p looked at).  The GPU inserts in another order: the occupied set and every
    lookup agree with this table, the slot of an id inside a run and the chain lengths need not."""
    map_ids = np.asarray(map_ids, dtype=np.uint64)
    bits = hash_bits(len(map_ids)) if bits is None else bits
    cap = 1 << bits
    assert len(map_ids) < cap
    slots = np.full(cap, EMPTY, dtype=np.uint64)
    chain = np.zeros(len(map_ids), dtype=np.int64)
    for p, (i, s) in enumerate(zip(map_ids.tolist(), home(map_ids, bits).tolist())):
        c = 1
        while slots[s] != np.uint64(EMPTY):
            s = (s + 1) & (cap - 1)
            c += 1
        slots[s] = np.uint64((i << 32) | p)
        chain[p] = c
    return slots, chain


def table_lookup(slots, ids):
    """ids -> positions through a table of build_table (ABSENT where the walk meets an empty slot first)."""
    cap = len(slots)
    bits = cap.bit_length() - 1
    out = np.full(len(ids), ABSENT, dtype=np.uint32)
    for j, (i, s) in enumerate(zip(np.asarray(ids, dtype=np.uint64).tolist(), home(ids, bits).tolist())):
        for _ in range(cap):
            v = int(slots[s])
            if v == EMPTY:
                break
            if v >> 32 == i:
                out[j] = v & 0xFFFFFFFF
                break
            s = (s + 1) & (cap - 1)
    return out


def colliding_ids(bits: int, slot: int, count: int, lo: int = 0, hi: int = 1 << 32, taken=()):
    """`count` ascending ids in [lo, hi) whose home slot in a table of 2^bits slots is `slot`, none of them in `taken`."""
    taken = set(int(t) for t in taken)
    out, start, step = [], lo, 1 << 22
    while len(out) < count and start < hi:
        cand = np.arange(start, min(start + step, hi), dtype=np.uint64)
        for c in cand[home(cand, bits) == slot].tolist():
            if c not in taken:
                out.append(c)
                if len(out) == count:
                    break
        start += step
    assert len(out) == count, (bits, slot, count)
    return np.array(out, dtype=np.uint32)


def locate(map_ids, ids, live=None):
    """ids -> positions in map_ids (ABSENT for an id that is not there, or whose position is not live)."""
    map_ids = np.asarray(map_ids, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.uint32)
    order = np.argsort(map_ids, kind="stable")
    sorted_ids = map_ids[order]
    at = np.searchsorted(sorted_ids, ids)
    at_c = np.minimum(at, max(len(map_ids) - 1, 0))
    hit = (at < len(map_ids)) & (sorted_ids[at_c] == ids) if len(map_ids) else np.zeros(ids.shape, dtype=bool)
    pos = np.where(hit, order[at_c] if len(map_ids) else 0, ABSENT).astype(np.uint32)
    if live is not None:
        live = np.asarray(live, dtype=bool)
        dead = hit & ~live[np.where(hit, pos, 0).astype(np.int64)]
        pos[dead] = ABSENT
    return pos


def drop_self(dist, ids, cnt, self_ids, found=None):
    """Rows of a plain call at topk + 1 (dist, ids: m x (topk + 1); cnt: valid entries per row) -> (dist, ids) m x topk: per row
    the first entry whose id is self_ids[i] leaves, or the last valid entry if there is none; the others keep their order and the
    slots behind them hold NaN / ABSENT.  found[i] == False: the whole row is padding."""
    dist, ids = np.asarray(dist, dtype=np.float32), np.asarray(ids, dtype=np.uint32)
    m, w = ids.shape
    topk = w - 1
    od = np.full((m, topk), np.nan, dtype=np.float32)
    oi = np.full((m, topk), ABSENT, dtype=np.uint32)
    for i in range(m):
        n = min(int(cnt[i]), w)
        if n == 0 or (found is not None and not found[i]):
            continue
        hits = np.nonzero(ids[i, :n] == np.uint32(self_ids[i]))[0]
        drop = int(hits[0]) if hits.size else n - 1
        keep = [e for e in range(n) if e != drop][:topk]
        od[i, :len(keep)] = dist[i, keep]
        oi[i, :len(keep)] = ids[i, keep]
    return od, oi
