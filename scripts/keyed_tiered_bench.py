"""Keyed exact search on wide and split-row indexes: n x 768 f32 (the synthetic mixture of tests/synth.py) with a u32
tenant column of Zipf-sized tenants, one index per layout in one session.  Prints ONE JSON line (and writes it to --out).
  plain   rq_exact_search_keyed_tiered_device (the dimension-sliced scan) against rq_exact_search_keyed_device on the same index and
          keys -- that entry runs its exact-only form at this dimension
  split   the same entry on a split-row index against the existing way there: per key, idx.where(col == key) and the filtered
          rq_exact_search_tiered_device of that key's query (--baseline-keys of them, summed)
Per batch of --batches (one query per DISTINCT tenant, drawn at random), medians of --steps calls after a warm-up: wall ms, the
phases of rq_last_keyed_stats, gathered row bytes per second (rows_gathered x the bytes the scan reads of a row), the pairs that
reached the exact path, and whether the two ways gave the same bits.

  python scripts/keyed_tiered_bench.py [--vectors 2000000] [--out profiles/keyed_tiered_bench_2M.json]
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
    ap.add_argument("--vectors", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--tenants", type=int, default=8192)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batches", default="16,256,4096")
    ap.add_argument("--baseline-keys", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib, col
    from rabitq_amd import index as ix
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    n, d, k, topk = args.vectors, args.dim, args.lists, args.topk

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def med(v):
        return round(float(np.median(v)), 3)

    def measure(g, call, row_bytes):
        timed(call), timed(call)
        wall, stats = [], []
        for _ in range(args.steps):
            wall.append(timed(call)[1])
            stats.append(g.last_keyed_stats())
        st = stats[-1]
        r = {"wall_ms": med(wall), **{p: med([s[p] for s in stats]) for p in ("ms_seed", "ms_scan", "ms_exact", "ms_select")},
             "prefilter": st["prefilter"], "reruns": st["reruns"], "rows_gathered": st["rows_gathered"], "rows_listed": st["rows_listed"],
             "pairs_exact": st["candidates"]}
        r["gather_TBps"] = round(st["rows_gathered"] * row_bytes / (r["ms_scan"] * 1e-3) / 1e12, 3) if st["prefilter"] and r["ms_scan"] else None
        return r

    x, centres = synth.device_mixture(n, d, k, args.sigma, dev)
    w = 1.0 / np.arange(1, args.tenants + 1, dtype=np.float64)
    cdf = torch.from_numpy(np.cumsum(w) / w.sum()).to(dev)
    out = {"vectors": n, "dim": d, "lists": k, "topk": topk, "steps": args.steps, "layouts": {}}
    for layout, split in (("plain", 0), ("split", 2)):
        ix.set_option("split_rows", split)
        try:
            g = rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=np.eye(d, dtype=np.float32))
        finally:
            ix.set_option("split_rows", 1)
        gen = torch.Generator(device=dev).manual_seed(5)
        t = torch.searchsorted(cdf, torch.rand(n, device=dev, dtype=torch.float64, generator=gen)).clamp_(max=args.tenants - 1).to(torch.int32)
        ids = torch.arange(n, device=dev, dtype=torch.int32)
        torch.cuda.synchronize()
        g.create_attr("tenant", "u32", fill=0)
        absent = C.c_uint64()
        _lib.check(_lib.lib().rq_attr_set_device(g._h, b"tenant", C.c_void_p(ids.data_ptr()), C.c_void_p(t.data_ptr()), n, C.byref(absent)))
        del t, ids
        post = g.postings("tenant")
        rng = np.random.default_rng(9)
        runs = []
        for B in (min(int(v), post.values.size) for v in args.batches.split(",")):
            keys = rng.choice(post.values, size=B, replace=False).astype(np.uint32)
            q = synth.device_queries(centres, B, args.sigma, dev)
            bufs = [(torch.empty((B, topk), device=dev, dtype=torch.float32), torch.empty((B, topk), device=dev, dtype=torch.int32),
                     torch.zeros(B, device=dev, dtype=torch.int32)) for _ in range(2)]
            new = lambda: g.exact_search_keyed_tiered_device(q.data_ptr(), B, d, keys, topk, post, *(b.data_ptr() for b in bufs[0]))
            run = {"queries": B, "key_rows": int(post.count_of(keys).sum()), "sliced": measure(g, new, 2 * d if split else 4 * d)}
            od, oi, on = bufs[0]
            if not split:   # the keyed entry as it stands: exact-only at this dimension
                old = lambda: g.exact_search_keyed_device(q.data_ptr(), B, d, keys, topk, post, *(b.data_ptr() for b in bufs[1]))
                run["keyed_entry"] = measure(g, old, 4 * d)
                nb = B
            else:           # per key: where + the filtered exact search of its query
                nb, ms = min(args.baseline_keys, B), []
                bd, bi, bn = bufs[1]
                for j in range(nb):
                    def one():
                        with g.where(col("tenant") == int(keys[j])) as f:
                            g.exact_search_tiered_device(q[j:j + 1].data_ptr(), 1, d, topk, bd[j:j + 1].data_ptr(), bi[j:j + 1].data_ptr(), bn[j:j + 1].data_ptr(), filter=f)
                    ms.append(timed(one)[1])
                run["where_filtered"] = {"keys": nb, "ms_per_key": med(ms), "ms_total": round(float(np.sum(ms)), 1)}
            (bd, bi, bn), live = bufs[1], torch.arange(topk, device=dev)[None, :] < on[:nb, None]
            run["bits_equal"] = bool(torch.equal(on[:nb], bn[:nb]) and torch.equal(oi[:nb][live], bi[:nb][live])
                                     and torch.equal(od[:nb].view(torch.int32)[live], bd[:nb].view(torch.int32)[live]))
            runs.append(run)
            print(layout, json.dumps(run), file=sys.stderr, flush=True)
        out["layouts"][layout] = {"tenants": int(post.values.size), "largest_tenant_rows": int(post.counts.max()), "runs": runs}
        post.close(), g.close()
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
