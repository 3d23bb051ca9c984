"""A numpy model of multi-vector search over documents named by a column (include/rabitq_hip.h, "MaxSim by postings"; DESIGN
§4.26).  The score is tests/maxsim_model.py's chamfer; what differs is the document: the document of key v is the set of positions
that held v in the column when the postings were made (`segs`: {value as a Python int: positions}, the snapshot).  A key without a
segment is a document without a row.  End to end, a result row's document is its column value AS IT IS NOW (`column_now`, position
order); a value without a segment is no candidate; ties of the sum go by the column type's own ascending order of the keys, which
is the order of Python ints of that dtype.
"""
import numpy as np

from tests.maxsim_model import NAN_BITS, chamfer, chamfer_f64, ord32_biased  # noqa: F401


def segments(column, live=None):
    """the postings of `column` (position order; live: bool mask or None) -> {value: positions}"""
    segs = {}
    for p, v in enumerate(column):
        if live is None or live[p]:
            segs.setdefault(int(v), []).append(p)
    return segs


def scores(tok, n_tokens, keys, counts, segs, base):
    """rq_maxsim_scores_keyed -> (score bits B x C u32, rows B x C u32)."""
    B, C = keys.shape
    sb = np.full((B, C), NAN_BITS, dtype=np.uint32)
    rows = np.zeros((B, C), dtype=np.uint32)
    for b in range(B):
        nt = tok.shape[1] if n_tokens is None else min(int(n_tokens[b]), tok.shape[1])
        for c in range(C if counts is None else min(int(counts[b]), C)):
            pos = segs.get(int(keys[b, c]))
            if pos:
                sb[b, c] = np.array([chamfer(tok[b], nt, base, pos)], dtype=np.float32).view(np.uint32)[0]
                rows[b, c] = len(pos)
    return sb, rows


def search(tok, n_tokens, src_ids, src_cnt, topk, posmap, column_now, segs, base):
    """rq_query_batch_maxsim_keyed, fed the plain call's rows of the B T tokens at topk = fetch
    -> (dist bits B x topk, keys B x topk in the column's dtype padded with 0, counts B, candidates B)."""
    B, T = tok.shape[:2]
    db = np.full((B, topk), NAN_BITS, dtype=np.uint32)
    keys = np.zeros((B, topk), dtype=column_now.dtype)
    cnt, ncand = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
    for b in range(B):
        nt = T if n_tokens is None else min(int(n_tokens[b]), T)
        ids = [i for t in range(nt) for i in src_ids[b * T + t, :src_cnt[b * T + t]]]
        cand = sorted({int(column_now[posmap[int(i)]]) for i in ids} & segs.keys())
        if not cand:
            continue
        sb, _ = scores(tok[b:b + 1], [nt], np.array([cand], dtype=column_now.dtype), None, segs, base)
        order = sorted(range(len(cand)), key=lambda c: (int(ord32_biased(sb[0, c:c + 1].view(np.float32))[0]), cand[c]))[:topk]
        db[b, :len(order)], keys[b, :len(order)] = sb[0, order], [cand[c] for c in order]
        cnt[b], ncand[b] = len(order), len(cand)
    return db, keys, cnt, ncand
