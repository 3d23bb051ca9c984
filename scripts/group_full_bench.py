"""The complete exact grouped search at the headline shape (100M x 128 f32, 4096 lists, the synthetic mixture of tests/synth.py), in one
session on one index.  Two u32 columns: `doc` = id // --rows-per-doc (even groups; postings hold at most 2^22 values,
so 100M rows need at least 24 rows per value) and `tenant`, Zipf-sized groups.  Prints ONE JSON line (and writes it to --out).
Per column, batch and (topk, group_size), medians of --steps calls after 2 warm-ups:
  full      wall ms of rq_exact_search_grouped_full_device, the phases, records and hits per query of rq_last_group_full_stats
and per batch the two yardsticks of the same session:
  exact     wall ms of rq_exact_search_device at topk = 10
  grouped   wall ms of rq_exact_search_grouped_device at fetch = 2048, and how many queries got fewer groups than the complete form

  python scripts/group_full_bench.py [--vectors 100000000] [--out profiles/group_full_bench_100M.json]
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
    ap.add_argument("--rows-per-doc", type=int, default=32)
    ap.add_argument("--tenants", type=int, default=8192)
    ap.add_argument("--batches", default="64,4096")
    ap.add_argument("--shapes", default="10x1,10x3,100x1")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    n, d, k = args.vectors, args.dim, args.lists

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def med(v):
        return round(float(np.median(v)), 3)

    def walls(call, stats=None):
        timed(call), timed(call)
        w, st = [], []
        for _ in range(args.steps):
            w.append(timed(call)[1])
            st.append(stats() if stats else {})
        return w, st

    x, centres = synth.device_mixture(n, d, k, args.sigma, dev)
    g, build_ms = timed(lambda: rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=synth.random_orthogonal((d + 63) // 64 * 64, seed=99)))
    del x
    torch.cuda.empty_cache()
    w = 1.0 / np.arange(1, args.tenants + 1, dtype=np.float64)
    cdf = torch.from_numpy(np.cumsum(w) / w.sum()).to(dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    absent = C.c_uint64()
    for name in ("doc", "tenant"):
        g.create_attr(name, "u32", fill=0)
    for i0 in range(0, n, 1 << 24):
        m = min(1 << 24, n - i0)
        ids = torch.arange(i0, i0 + m, device=dev, dtype=torch.int64)
        doc = (ids // args.rows_per_doc).to(torch.int32)
        ten = torch.searchsorted(cdf, torch.rand(m, device=dev, dtype=torch.float64, generator=gen)).clamp_(max=args.tenants - 1).to(torch.int32)
        ids = ids.to(torch.int32)
        torch.cuda.synchronize()
        for name, v in (("doc", doc), ("tenant", ten)):
            _lib.check(_lib.lib().rq_attr_set_device(g._h, name.encode(), C.c_void_p(ids.data_ptr()), C.c_void_p(v.data_ptr()), m, C.byref(absent)))
    out = {"vectors": n, "dim": d, "lists": k, "rows_per_doc": args.rows_per_doc, "tenants": args.tenants, "steps": args.steps,
           "build_ms": round(build_ms, 1), "columns": {}, "runs": []}
    posts = {}
    for name in ("doc", "tenant"):
        posts[name], ms = timed(lambda: g.postings(name))
        out["columns"][name] = {"values": int(posts[name].values.size), "postings_ms": round(ms, 1), "largest_group_rows": int(posts[name].counts.max())}
    phases = ("ms_inverse", "ms_bound", "ms_scan", "ms_exact", "ms_scatter", "ms_select", "ms_rows")
    for B in (int(v) for v in args.batches.split(",")):
        q = synth.device_queries(centres, B, args.sigma, dev)
        ed, ei, en = torch.empty((B, 10), device=dev), torch.empty((B, 10), device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
        exact_w, _ = walls(lambda: g.exact_search_device(q.data_ptr(), B, d, 10, ed.data_ptr(), ei.data_ptr(), en.data_ptr()))
        for name, post in posts.items():
            for topk, gs in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
                bufs = lambda: (torch.empty((B, topk * gs), device=dev), torch.empty((B, topk * gs), device=dev, dtype=torch.int32),
                                torch.empty((B, topk), device=dev, dtype=torch.int64), torch.empty((B, topk), device=dev, dtype=torch.int32),
                                torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32))
                fo, go = bufs(), bufs()
                full_w, st = walls(lambda: g.exact_search_grouped_full_device(q.data_ptr(), B, d, topk, post, *(t.data_ptr() for t in fo), group_size=gs),
                                   g.last_group_full_stats)
                grp_w, _ = walls(lambda: g.exact_search_grouped_device(q.data_ptr(), B, d, topk, name, *(t.data_ptr() for t in go), group_size=gs, fetch=2048))
                run = {"column": name, "queries": B, "topk": topk, "group_size": gs, "full_wall_ms": med(full_w), "full_wall_ms_all": [round(v, 3) for v in full_w],
                       **{p: med([s[p] for s in st]) for p in phases}, "records_per_query": round(st[-1]["records"] / B, 1),
                       "hits_per_query": round(st[-1]["hits"] / B, 1), "scan_reruns": st[-1]["scan_reruns"], "plan_queries": st[-1]["plan_queries"],
                       "rows_listed": st[-1]["rows_listed"], "exact_top10_wall_ms": med(exact_w), "grouped_fetch2048_wall_ms": med(grp_w),
                       "queries_short_at_fetch2048": int((go[4] < fo[4]).sum()), "groups_equal_where_both_full": bool(torch.equal(go[2][go[4] == fo[4]], fo[2][go[4] == fo[4]]))}
                out["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
