"""A numpy model of multi-vector search (include/rabitq_hip.h, "multi-vector search").  Input: the PREPARED tokens
(B x T x dim f32: transformed and padded, as the rerank sees a query), the widened stored rows `base` (f32, position order) and a map
{id: position} of the ids that have a live row.  The document of id i is i // S; d(t, x) = oracle.l2_squared_distance_rows; a
token's minimum is the value with the smallest ord32_biased image, a NaN of any sign and payload counted as 0x7FC00000 (what a
NaN operand leaves behind is the hardware's: the engine's exact distance to a NaN token is 0xFFC00000 on gfx950, the oracle's
0x7FC00000 on x86); the sum runs in f32 from +0.0 in ascending t, a NaN sum written as 0x7FC00000.
"""
import numpy as np

import oracle
from tests.diverse_model import ord32_biased, posmap_of  # noqa: F401  (the same ordered image and id map)

NAN_BITS = 0x7FC00000
PAD_DOC = 0xFFFFFFFF
NAN = np.array([NAN_BITS], dtype=np.uint32).view(np.float32)[0]


def doc_positions(posmap, doc, S):
    return [posmap[i] for i in range(int(doc) * S, int(doc) * S + S) if i in posmap]


def chamfer(tok, n_tok, base, positions):
    """-> the f32 Chamfer sum of the first n_tok tokens against the rows at `positions` (non-empty)."""
    s = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(int(n_tok)):
            d = oracle.l2_squared_distance_rows(tok[t], base, positions)
            d[np.isnan(d)] = NAN                              # a NaN of any sign and payload counts as 0x7FC00000
            s = np.float32(s + d[np.argmin(ord32_biased(d))])
    return NAN if np.isnan(s) else s


def scores(tok, n_tokens, cand, counts, S, posmap, base):
    """rq_maxsim_scores -> (score bits B x C u32, rows B x C u32)."""
    B, C = cand.shape
    sb = np.full((B, C), NAN_BITS, dtype=np.uint32)
    rows = np.zeros((B, C), dtype=np.uint32)
    for b in range(B):
        nt = tok.shape[1] if n_tokens is None else min(int(n_tokens[b]), tok.shape[1])
        for c in range(C if counts is None else min(int(counts[b]), C)):
            pos = doc_positions(posmap, cand[b, c], S)
            if pos:
                sb[b, c] = np.array([chamfer(tok[b], nt, base, pos)], dtype=np.float32).view(np.uint32)[0]
                rows[b, c] = len(pos)
    return sb, rows


def search(tok, n_tokens, src_ids, src_cnt, S, topk, posmap, base):
    """rq_query_batch_maxsim, fed the plain call's rows of the B T tokens at topk = fetch (src_ids B T x fetch, src_cnt B T)
    -> (dist bits B x topk, docs B x topk, counts B, candidates B)."""
    B, T = tok.shape[:2]
    db = np.full((B, topk), NAN_BITS, dtype=np.uint32)
    docs = np.full((B, topk), PAD_DOC, dtype=np.uint32)
    cnt, ncand = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
    for b in range(B):
        nt = T if n_tokens is None else min(int(n_tokens[b]), T)
        ids = [src_ids[b * T + t, :src_cnt[b * T + t]] for t in range(nt)]
        cand = np.unique(np.concatenate(ids) // S).astype(np.uint32) if ids else np.zeros(0, dtype=np.uint32)
        sb, rows = scores(tok[b:b + 1], [nt], cand[None, :], None, S, posmap, base)
        live = np.flatnonzero(rows[0])
        key = (ord32_biased(sb[0, live].view(np.float32)).astype(np.uint64) << np.uint64(32)) | cand[live].astype(np.uint64)
        order = live[np.argsort(key, kind="stable")][:topk]
        db[b, :order.size], docs[b, :order.size] = sb[0, order], cand[order]
        cnt[b], ncand[b] = order.size, cand.size
    return db, docs, cnt, ncand


def chamfer_f64(tok, n_tok, base, positions):
    """The plain sum in f64: sum_t min_x |x - q_t|^2."""
    x = base[np.asarray(positions, dtype=np.int64)].astype(np.float64)
    q = tok[:int(n_tok)].astype(np.float64)
    return float(((x[None, :, :] - q[:, None, :]) ** 2).sum(axis=2).min(axis=1).sum()) if len(q) else 0.0
