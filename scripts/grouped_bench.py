"""Grouped search at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, the synthetic mixture of tests/synth.py), in
one session on one index with one u32 column of ~10 rows per key.  Prints ONE JSON line (and appends it to --out).
Per (topk, group_size, fetch) of --cases and per batch of --batches, medians of --steps calls after a warm-up, the two calls
alternated so that both see the same machine:
  grouped     wall ms of rq_query_batch_grouped_device
  plain       wall ms of rq_query_batch_device at topk = fetch: what a caller had before, and the yardstick
  ms_group    device ms of the selection kernel (rq_last_group_stats, HIP events), its share of the grouped call, and ms_source
  kept, groups, candidates   the call's totals

  python scripts/grouped_bench.py [--vectors 100000000] [--out profiles/grouped_bench_100M.json]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--rows-per-key", type=int, default=10)
    ap.add_argument("--cases", default="10:1:64,10:3:128,100:1:1024")
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
    # the column: ids are 0 .. n - 1 in a random order of keys, ~rows_per_key rows each (no tie to the clusters)
    g.create_attr("doc", "u32", fill=0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    ids = torch.arange(n, device=dev, dtype=torch.int32)
    vals = torch.randint(0, max(n // args.rows_per_key, 1), (n,), generator=gen, device=dev, dtype=torch.int32)
    absent = C.c_uint64()
    _, set_ms = timed(lambda: _lib.check(_lib.lib().rq_attr_set_device(g._h, b"doc", C.c_void_p(ids.data_ptr()), C.c_void_p(vals.data_ptr()), n,
                                                                      C.byref(absent))))
    assert absent.value == 0
    del ids, vals
    torch.cuda.empty_cache()
    out = {"vectors": n, "dim": d, "lists": k, "nprobe": args.nprobe, "rows_per_key": args.rows_per_key, "steps": args.steps,
           "build_ms": round(build_ms, 1), "column_set_ms": round(set_ms, 1), "runs": []}
    for B in (int(v) for v in args.batches.split(",")):
        q = synth.device_queries(centres, B, args.sigma, dev)
        for case in args.cases.split(","):
            topk, gs, fetch = (int(v) for v in case.split(":"))
            pd = torch.empty((B, fetch), device=dev, dtype=torch.float32)
            pi = torch.empty((B, fetch), device=dev, dtype=torch.int32)
            pn = torch.empty(B, device=dev, dtype=torch.int32)
            od = torch.empty((B, topk, gs), device=dev, dtype=torch.float32)
            oi = torch.empty((B, topk, gs), device=dev, dtype=torch.int32)
            ok = torch.empty((B, topk), device=dev, dtype=torch.int64)
            gn = torch.empty((B, topk), device=dev, dtype=torch.int32)
            on = torch.empty(B, device=dev, dtype=torch.int32)
            of = torch.empty(B, device=dev, dtype=torch.int32)
            plain = lambda: g.query_batch_device(q.data_ptr(), B, d, args.nprobe, fetch, pd.data_ptr(), pi.data_ptr(), pn.data_ptr())
            grouped = lambda: g.query_batch_grouped_device(q.data_ptr(), B, d, args.nprobe, topk, "doc", od.data_ptr(), oi.data_ptr(), ok.data_ptr(),
                                                           gn.data_ptr(), on.data_ptr(), of.data_ptr(), group_size=gs, fetch=fetch)
            for call in (plain, plain, grouped, grouped):   # warm-up: the first calls learn the survivor-buffer capacity
                timed(call)
            tp, tg, ms_g, ms_s = [], [], [], []
            for _ in range(args.steps):
                tp.append(timed(plain)[1])
                tg.append(timed(grouped)[1])
                st = ix.last_group_stats()
                ms_g.append(st["ms_group"])
                ms_s.append(st["ms_source"])
            assert bool((of == pn).all().item()) and int(on.sum().item()) == st["groups"]
            rec = {"batch": B, "topk": topk, "group_size": gs, "fetch": fetch, "plain_at_fetch": spread(tp), "grouped": spread(tg),
                   "ms_group": spread(ms_g), "ms_source": spread(ms_s), "candidates": st["candidates"], "kept": st["kept"], "groups": st["groups"],
                   "overhead_ms": round(float(np.median(tg) - np.median(tp)), 3),
                   "selection_share_of_grouped": round(float(np.median(ms_g) / np.median(tg)), 4)}
            out["runs"].append(rec)
            print(rec, file=sys.stderr, flush=True)
            del pd, pi, pn, od, oi, ok, gn, on, of
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
