"""Keyed exact search at the headline shape (100M x 128 f32, 4096 lists, the synthetic mixture of tests/synth.py) with a u32 tenant
column of Zipf-sized tenants, in one session on one index.  Prints ONE JSON line (and writes it to --out).
  postings      wall ms of rq_postings_create and the bytes it holds
  keyed         per batch of --batches (one query per DISTINCT tenant, the tenants drawn at random), medians of --steps calls after
                a warm-up: wall ms of rq_exact_search_keyed_device, the phases of rq_last_keyed_stats, the rows of the keys asked
                for, gathered row bytes per second beside the by-id gather's measured 5.3 - 5.4 TB/s, the share of
                (query, row) pairs sent to the exact path
                -- gathered: the rows of the keys that take the matrix pass (rows_gathered), the only rows the scan itself reads
  baseline      the same answers the existing way on the same index: per distinct key, idx.where(col == key) and the filtered
                rq_exact_search_device of that key's query, for EVERY key of the batch (--baseline-keys 0) or its first N: the summed
                wall ms, and the bits compared with the keyed call's
  sweep         rq_keyed_tuning over --sweep-chunk x --sweep-small (postings per work item x the segment size below which a key
                takes neither bound nor matrix pass): median wall ms of 3 calls per batch -- the evidence behind the two defaults
  slabs         at a dimension where the double-buffered scan exists (64): one LDS slab per wave against two, alternated
What the table must show: the keyed call's time follows the rows of the keys asked for, the baseline's follows keys x n.

  python scripts/keyed_bench.py [--vectors 100000000] [--out profiles/keyed_bench_100M.json]
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
    ap.add_argument("--tenants", type=int, default=8192)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batches", default="16,256,4096")
    ap.add_argument("--baseline-keys", type=int, default=0, help="0 = every key of every batch")
    ap.add_argument("--sweep-chunk", default="1024,4096,16384,65536")
    ap.add_argument("--sweep-small", default="1024,4096,16384")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib, col
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

    x, centres = synth.device_mixture(n, d, k, args.sigma, dev)
    g, build_ms = timed(lambda: rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=synth.random_orthogonal((d + 63) // 64 * 64, seed=99)))
    del x
    torch.cuda.empty_cache()
    print("built in %.0f ms" % build_ms, file=sys.stderr, flush=True)
    # tenant of id i: Zipf(--zipf) over --tenants ranks by inverse CDF, drawn on the device in pieces
    w = 1.0 / np.arange(1, args.tenants + 1, dtype=np.float64) ** args.zipf
    cdf = torch.from_numpy(np.cumsum(w) / w.sum()).to(dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    g.create_attr("tenant", "u32", fill=0)
    absent = C.c_uint64()
    for i0 in range(0, n, 1 << 24):
        m = min(1 << 24, n - i0)
        t = torch.searchsorted(cdf, torch.rand(m, device=dev, dtype=torch.float64, generator=gen)).clamp_(max=args.tenants - 1).to(torch.int32)
        ids = torch.arange(i0, i0 + m, device=dev, dtype=torch.int64).to(torch.int32)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().rq_attr_set_device(g._h, b"tenant", C.c_void_p(ids.data_ptr()), C.c_void_p(t.data_ptr()), m, C.byref(absent)))
    del t, ids
    post, post_ms = timed(lambda: g.postings("tenant"))
    sizes = post.counts.astype(np.int64)
    print("postings in %.0f ms" % post_ms, file=sys.stderr, flush=True)
    out = {"vectors": n, "dim": d, "lists": k, "tenants": int(post.values.size), "zipf": args.zipf, "topk": topk, "steps": args.steps,
           "build_ms": round(build_ms, 1), "postings_ms": round(post_ms, 1), "postings_bytes": post.bytes,
           "largest_tenant_rows": int(sizes.max()), "smallest_tenant_rows": int(sizes.min()), "runs": []}
    rng = np.random.default_rng(9)
    row_bytes = d * 4
    tuning = _lib.lib().rq_keyed_tuning
    held = []   # per batch: (B, call) for the sweep and the slab comparison
    for B in (int(v) for v in args.batches.split(",")):
        B = min(B, post.values.size)
        keys = rng.choice(post.values, size=B, replace=False).astype(np.uint32)
        key_rows = int(post.count_of(keys).sum())
        q = synth.device_queries(centres, B, args.sigma, dev)
        od = torch.empty((B, topk), device=dev, dtype=torch.float32)
        oi = torch.empty((B, topk), device=dev, dtype=torch.int32)
        on = torch.empty(B, device=dev, dtype=torch.int32)
        call = lambda by=post, q=q, B=B, keys=keys, od=od, oi=oi, on=on: g.exact_search_keyed_device(q.data_ptr(), B, d, keys, topk, by, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        for _ in range(2):
            timed(call)
        wall, stats = [], []
        for _ in range(args.steps):
            wall.append(timed(call)[1])
            stats.append(g.last_keyed_stats())
        st = stats[-1]
        phase = {p: med([s[p] for s in stats]) for p in ("ms_plan", "ms_seed", "ms_scan", "ms_exact", "ms_select")}
        run = {"queries": B, "key_rows": key_rows, "keys_x_n": B * n, "wall_ms": med(wall), "wall_ms_all": [round(v, 3) for v in wall], **phase,
               "items": st["items"], "reruns": st["reruns"], "prefilter": st["prefilter"], "rows_gathered": st["rows_gathered"], "rows_listed": st["rows_listed"],
               "gather_TBps": round(st["rows_gathered"] * row_bytes / (phase["ms_scan"] * 1e-3) / 1e12, 3) if phase["ms_scan"] else None,
               "exact_share": round(st["candidates"] / max(st["rows_listed"], 1), 6)}
        # the existing way, key by key (each key's own query), on the first --baseline-keys keys
        nb = min(args.baseline_keys or B, B)
        bd = torch.empty((1, topk), device=dev, dtype=torch.float32)
        bi = torch.empty((1, topk), device=dev, dtype=torch.int32)
        bn = torch.empty(1, device=dev, dtype=torch.int32)
        base_ms, same = [], True
        for j in range(nb):
            def one():
                with g.where(col("tenant") == int(keys[j])) as f:
                    g.exact_search_device(q[j:j + 1].data_ptr(), 1, d, topk, bd.data_ptr(), bi.data_ptr(), bn.data_ptr(), filter=f)
            base_ms.append(timed(one)[1])
            c = int(bn[0])
            same = same and c == int(on[j]) and torch.equal(bi[0, :c], oi[j, :c]) and torch.equal(bd[0, :c].view(torch.int32), od[j, :c].view(torch.int32))
        run.update({"baseline_keys": nb, "baseline_ms_per_key": med(base_ms), "baseline_ms_total": round(float(np.sum(base_ms)), 1),
                    "baseline_bits_equal": bool(same)})
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        held.append((B, call, (q, od, oi, on, keys)))

    def walls(call, steps):
        timed(call), timed(call)
        w, scan = [], []
        for _ in range(steps):
            w.append(timed(call)[1])
            scan.append(g.last_keyed_stats()["ms_scan"])
        return med(w), med(scan)

    out["sweep"] = []
    for chunk in (int(v) for v in args.sweep_chunk.split(",") if v):
        for small in (int(v) for v in args.sweep_small.split(",") if v):
            _lib.check(tuning(chunk, small, 0))
            with g.postings("tenant") as fresh:   # (fresh postings: the candidate capacity another setting learnt does not carry over)
                out["sweep"].append({"chunk_rows": chunk, "small_rows": small,
                                     "wall_ms": {str(B): walls(lambda c=call: c(by=fresh), 3)[0] for B, call, _ in held}})
            print(json.dumps(out["sweep"][-1]), file=sys.stderr, flush=True)
    _lib.check(tuning(0, 0, 0))
    if d == 64:
        out["slabs"] = []
        for B, call, _ in held:
            rec = {"queries": B, "one": [], "two": []}
            for _ in range(3):
                for name, v in (("one", 1), ("two", 2)):
                    _lib.check(tuning(0, 0, v))
                    rec[name].append(walls(call, 3))
            rec = {"queries": B, "one_slab_wall_ms": med([w for w, _ in rec["one"]]), "one_slab_scan_ms": med([x for _, x in rec["one"]]),
                   "two_slabs_wall_ms": med([w for w, _ in rec["two"]]), "two_slabs_scan_ms": med([x for _, x in rec["two"]])}
            out["slabs"].append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
        _lib.check(tuning(0, 0, 0))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
