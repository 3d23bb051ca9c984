"""A numpy model of exact multi-vector search (include/rabitq_hip.h, "exact multi-vector search"): every segment of
the postings scored by tests/maxsim_model.py's chamfer, ordered by (ord32_biased(score), key in the column type's order -- the order
of Python ints), the first topk taken.  bounds() restates the bound pass's lo / hi in float64 (operands rounded to bf16; the
accumulation order is free, the margin covers it): L <= chamfer <= U is what lets the engine leave documents unscored."""
import numpy as np

from tests.exact_scan_cases import approx_and_margin
from tests.maxsim_keyed_model import NAN_BITS, chamfer, ord32_biased, segments  # noqa: F401


def search(tok, n_tokens, topk, segs, base, dtype):
    """rq_exact_search_maxsim -> (dist bits B x topk, keys B x topk in `dtype` padded with 0, counts B)."""
    B, T = tok.shape[:2]
    keys = sorted(segs)
    db = np.full((B, topk), NAN_BITS, dtype=np.uint32)
    out = np.zeros((B, topk), dtype=dtype)
    cnt = np.zeros(B, dtype=np.uint32)
    for b in range(B):
        nt = T if n_tokens is None else min(int(n_tokens[b]), T)
        s = np.array([chamfer(tok[b], nt, base, segs[k]) for k in keys], dtype=np.float32)
        order = sorted(range(len(keys)), key=lambda c: (int(ord32_biased(s[c:c + 1])[0]), keys[c]))[:topk]
        db[b, :len(order)], out[b, :len(order)], cnt[b] = s[order].view(np.uint32), [keys[c] for c in order], len(order)
    return db, out, cnt


def bounds(tok, n_tok, base, positions):
    """-> (L, U) of one document for finite operands: the sums over the tokens of min_x (a - m) and of min_x (a + m)."""
    a, m = approx_and_margin(base[np.asarray(positions, dtype=np.int64)], tok[:int(n_tok)], tok.shape[1])
    return float((a - m).min(axis=1).sum()), float((a + m).min(axis=1).sum())
