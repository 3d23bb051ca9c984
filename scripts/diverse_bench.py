"""Diverse search at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, the synthetic mixture of tests/synth.py), in
one session on one index.  Prints ONE JSON line (and appends it to --out).  Per (topk, fetch) of --cases and per
batch of --batches, medians of --steps calls after a warm-up, the two calls alternated so that both see the same machine:
  diverse     wall ms of rq_query_batch_diverse_device at --lam
  plain       wall ms of rq_query_batch_device at topk = fetch: what a caller had before, and the yardstick
  ms_select   device ms of the selection kernel (rq_last_diverse_stats, HIP events), its share of the diverse call, and ms_source
  row_GBps    pair_distances x row bytes / ms_select: the rate at which the selection reads candidate rows (mostly from the L2:
              a query's candidates are read again at every step), beside the by-id gather's HBM rate of DESIGN §4.19
  taken, candidates, pair_distances   the call's totals

  python scripts/diverse_bench.py [--vectors 100000000] [--out profiles/diverse_bench_100M.json]
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
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--cases", default="10:64,10:128,100:1024")
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib, index as ix
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    n, d, k = args.vectors, args.dim, args.lists
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=99)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def spread(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}

    x, centres = synth.device_mixture(n, d, k, args.sigma, dev)
    g, build_ms = timed(lambda: rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=P))
    del x
    torch.cuda.empty_cache()
    row_bytes = g.dim * 4
    out = {"vectors": n, "dim": d, "lists": k, "nprobe": args.nprobe, "lambda": args.lam, "steps": args.steps, "build_ms": round(build_ms, 1),
           "row_bytes": row_bytes, "runs": []}
    for B in (int(v) for v in args.batches.split(",")):
        q = synth.device_queries(centres, B, args.sigma, dev)
        for case in args.cases.split(","):
            topk, fetch = (int(v) for v in case.split(":"))
            pd = torch.empty((B, fetch), device=dev, dtype=torch.float32)
            pi = torch.empty((B, fetch), device=dev, dtype=torch.int32)
            pn = torch.empty(B, device=dev, dtype=torch.int32)
            od = torch.empty((B, topk), device=dev, dtype=torch.float32)
            oi = torch.empty((B, topk), device=dev, dtype=torch.int32)
            ov = torch.empty((B, topk), device=dev, dtype=torch.float32)
            on = torch.empty(B, device=dev, dtype=torch.int32)
            of = torch.empty(B, device=dev, dtype=torch.int32)
            plain = lambda: g.query_batch_device(q.data_ptr(), B, d, args.nprobe, fetch, pd.data_ptr(), pi.data_ptr(), pn.data_ptr())
            diverse = lambda: g.query_batch_diverse_device(q.data_ptr(), B, d, args.nprobe, topk, od.data_ptr(), oi.data_ptr(), ov.data_ptr(),
                                                           on.data_ptr(), of.data_ptr(), lam=args.lam, fetch=fetch)
            for call in (plain, plain, diverse, diverse):   # warm-up: the first calls learn the survivor-buffer capacity
                timed(call)
            tp, tv, ms_sel, ms_src = [], [], [], []
            for _ in range(args.steps):
                tp.append(timed(plain)[1])
                tv.append(timed(diverse)[1])
                st = ix.last_diverse_stats()
                ms_sel.append(st["ms_select"])
                ms_src.append(st["ms_source"])
            assert bool((of == pn).all().item()) and int(on.sum().item()) == st["taken"]
            sel = float(np.median(ms_sel))
            rec = {"batch": B, "topk": topk, "fetch": fetch, "plain_at_fetch": spread(tp), "diverse": spread(tv), "ms_select": spread(ms_sel),
                   "ms_source": spread(ms_src), "candidates": st["candidates"], "absent": st["absent"], "skipped": st["skipped"],
                   "taken": st["taken"], "pair_distances": st["pair_distances"],
                   "overhead_ms": round(float(np.median(tv) - np.median(tp)), 3),
                   "selection_share_of_diverse": round(sel / float(np.median(tv)), 4),
                   "row_GBps": round(st["pair_distances"] * row_bytes / (sel * 1e-3) / 1e9, 1)}
            out["runs"].append(rec)
            print(rec, file=sys.stderr, flush=True)
            del pd, pi, pn, od, oi, ov, on, of
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
