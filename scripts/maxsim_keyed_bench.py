"""Multi-vector search by postings against the stride form, at §4.23's configuration (100M x 128, 4096 lists, T 32, documents of 128
consecutive ids, fetch 64), in one session on one index that carries a u32 column doc = id // stride.  Prints ONE
JSON line (and appends it to --out).  Per batch of --batches: the stride form (the code path of §4.23, unchanged) and the keyed form
alternated, medians of --steps calls after a warm-up; per form ms_score (HIP events around the scoring launch), (token, row) pairs
per second, gathered TB/s, and the stride form's own run-to-run spread (max - min of its ms_score) -- the yardstick of the claim
"the keyed walk is not slower than the stride walk by more than that spread".  Both forms must return the same sums and the same
documents.  --slab-dim 64 adds, on a second index of that dim and --slab-vectors rows, one slab against two (rq_keyed_tuning's
slabs = 1 / 0), alternated --slab-rounds times.

  python scripts/maxsim_keyed_bench.py [--vectors 100000000] [--out profiles/maxsim_keyed_bench_100M.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--stride", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--fetch", type=int, default=64)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batches", default="16,256,4096")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--slab-dim", type=int, default=64)
    ap.add_argument("--slab-vectors", type=int, default=20_000_000)
    ap.add_argument("--slab-batch", type=int, default=256)
    ap.add_argument("--slab-rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib, index as ix
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    k, T, S, F = args.lists, args.tokens, args.stride, args.fetch

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def med(v):
        return round(float(np.median(v)), 3)

    def make(n, d):
        """-> (index with the column, its postings, the centres, ms of the postings' creation)"""
        x, centres = synth.device_mixture(n, d, k, args.sigma, dev)
        g = rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=synth.random_orthogonal((d + 63) // 64 * 64, seed=99))
        del x
        torch.cuda.empty_cache()
        g.create_attr("doc", "u32", fill=0)
        ids = np.arange(n, dtype=np.uint32)
        g.set_attr("doc", ids, ids // np.uint32(S))
        p, post_ms = timed(lambda: g.postings("doc"))
        return g, p, centres, post_ms

    def run(g, p, centres, d, B, forms, steps):
        """forms: (name, by, slabs knob) alternated -> {name: record}; every form's outputs must equal the first one's"""
        q = synth.device_queries(centres, B * T, args.sigma, dev)
        od = {f[0]: torch.empty((B, args.topk), device=dev, dtype=torch.float32) for f in forms}
        oi = {f[0]: torch.zeros((B, args.topk), device=dev, dtype=torch.int64) for f in forms}
        on = {f[0]: torch.empty(B, device=dev, dtype=torch.int32) for f in forms}

        def call(name, by, slabs):
            _lib.check(_lib.lib().rq_keyed_tuning(0, 0, slabs))
            g.query_batch_maxsim_device(q.data_ptr(), 0, B, T, d, args.nprobe, args.topk, None if by else S, F, od[name].data_ptr(),
                                        oi[name].data_ptr(), on[name].data_ptr(), by=p if by else None)
        for f in forms + forms:
            timed(lambda: call(*f))
        score, st = {f[0]: [] for f in forms}, {}
        for _ in range(steps):
            for f in forms:
                timed(lambda: call(*f))
                st[f[0]] = ix.last_maxsim_stats()
                score[f[0]].append(st[f[0]]["ms_score"])
        _lib.check(_lib.lib().rq_keyed_tuning(0, 0, 0))
        first, recs = forms[0][0], {}
        held = torch.arange(args.topk, device=dev)[None, :] < on[first][:, None]
        # (the stride form writes B x topk u32 document numbers at the start of the same buffer)
        docs = lambda name, by: (oi[name] if by else oi[name].view(torch.int32).reshape(-1)[:B * args.topk].reshape(B, args.topk).to(torch.int64) & 0xFFFFFFFF)
        for name, by, _ in forms:
            ms = med(score[name]) * 1e-3
            s = st[name]
            same = bool((od[name].view(torch.int32) == od[first].view(torch.int32)).all().item() and (on[name] == on[first]).all().item()
                        and (docs(name, by)[held] == docs(first, forms[0][1])[held]).all().item())
            recs[name] = {"ms_score": med(score[name]), "ms_score_spread": round(max(score[name]) - min(score[name]), 3), "pairs": s["pairs"],
                          "pairs_per_s": round(s["pairs"] / ms, 1), "rows_gathered": s["rows_gathered"],
                          "gather_TBps": round(s["rows_gathered"] * g.dim * 4 / ms / 1e12, 3), "exact_distances": s["exact_distances"],
                          "lds_bytes": s["lds_bytes"], "same_outputs_as_" + first: same}
        return recs

    out = {"vectors": args.vectors, "dim": args.dim, "lists": k, "nprobe": args.nprobe, "stride": S, "tokens": T, "fetch": F, "topk": args.topk,
           "steps": args.steps, "runs": []}
    g, p, centres, post_ms = make(args.vectors, args.dim)
    out["postings_ms"], out["postings_values"], out["postings_bytes"] = round(post_ms, 1), len(p.values), p.bytes
    for B in (int(v) for v in args.batches.split(",")):
        rec = {"batch": B, **run(g, p, centres, args.dim, B, [("stride", False, 0), ("keyed", True, 0)], args.steps)}
        rec["keyed_minus_stride_ms"] = round(rec["keyed"]["ms_score"] - rec["stride"]["ms_score"], 3)
        out["runs"].append(rec)
        print(rec, file=sys.stderr, flush=True)
    p.close(), g.close()
    del g, p
    torch.cuda.empty_cache()
    if args.slab_dim:
        g, p, centres, _ = make(args.slab_vectors, args.slab_dim)
        out["slabs"] = {"vectors": args.slab_vectors, "dim": args.slab_dim, "batch": args.slab_batch, "rounds": []}
        for _ in range(args.slab_rounds):
            rec = run(g, p, centres, args.slab_dim, args.slab_batch, [("one_slab", True, 1), ("two_slabs", True, 0)], args.steps)
            out["slabs"]["rounds"].append({name: {f: r[f] for f in ("ms_score", "ms_score_spread", "lds_bytes", "same_outputs_as_one_slab")}
                                           for name, r in rec.items()})
            print(out["slabs"]["rounds"][-1], file=sys.stderr, flush=True)
        p.close(), g.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
