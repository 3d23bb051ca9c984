"""Restricted postings and the filtered exact multi-vector search at scripts/maxsim_keyed_bench.py's corpus (100M x 128, 4096 lists,
documents of 128 consecutive ids, T 32), under a filter that admits every second document.  In one session, after a
warm-up, alternated --steps times: p.restrict(f) (host clock around the call, which returns synchronised), the unfiltered
exact_search_maxsim, the filtered one (restrict inside the call) and the unfiltered one by a held p.restrict(f).  Prints ONE JSON
line (and appends it to --out): every run, the medians, and the restrict time as a share of the unfiltered call.  The filtered call
and the call by the held object must return the same bits.

  python scripts/postings_restrict_bench.py [--vectors 100000000] [--out profiles/postings_restrict_ab_runs.txt]
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
    ap.add_argument("--stride", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
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
    n, d, k, T, S, B = args.vectors, args.dim, args.lists, args.tokens, args.stride, args.batch

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    x, centres = synth.device_mixture(n, d, k, args.sigma, dev)
    g = rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=synth.random_orthogonal((d + 63) // 64 * 64, seed=99))
    del x
    torch.cuda.empty_cache()
    g.create_attr("doc", "u32", fill=0)
    ids = np.arange(n, dtype=np.uint32)
    g.set_attr("doc", ids, ids // np.uint32(S))
    p, post_ms = timed(lambda: g.postings("doc"))
    f = g.make_filter(mask=(ids // np.uint32(S)) % 2 == 0)
    print("index, postings and filter made", file=sys.stderr, flush=True)
    q = synth.device_queries(centres, B * T, args.sigma, dev)
    out = {name: (torch.empty((B, args.topk), device=dev, dtype=torch.float32), torch.zeros((B, args.topk), device=dev, dtype=torch.int64),
                  torch.empty(B, device=dev, dtype=torch.int32)) for name in ("unfiltered", "filtered", "held")}
    held = p.restrict(f)

    def search(name, by, filt):
        od, oi, on = out[name]
        g.exact_search_maxsim_device(q.data_ptr(), 0, B, T, d, args.topk, by, od.data_ptr(), oi.data_ptr(), on.data_ptr(), filter=filt)

    forms = {"restrict": lambda: p.restrict(f).close(), "unfiltered": lambda: search("unfiltered", p, None),
             "filtered": lambda: search("filtered", p, f), "held": lambda: search("held", held, None)}
    for _ in range(2):
        for fn in forms.values():
            timed(fn)
    runs, stats = {name: [] for name in forms}, {}
    for step in range(args.steps):
        for name, fn in forms.items():
            runs[name].append(round(timed(fn)[1], 3))
            if name != "restrict":
                stats[name] = ix.last_maxsim_exact_stats()
        print("step", step, {name: v[-1] for name, v in runs.items()}, file=sys.stderr, flush=True)
    same = all(bool((out["filtered"][i].view(torch.int32) == out["held"][i].view(torch.int32)).all().item()) for i in range(3))
    med = {name: round(float(np.median(v)), 3) for name, v in runs.items()}
    rec = {"vectors": n, "dim": d, "lists": k, "stride": S, "tokens": T, "topk": args.topk, "batch": B, "steps": args.steps,
           "postings": int(p.rows), "documents": len(p.values), "admitted_postings": int(held.rows), "admitted_documents": len(held.values),
           "postings_create_ms": round(post_ms, 1), "runs_ms": runs, "median_ms": med,
           "spread_ms": {name: round(max(v) - min(v), 3) for name, v in runs.items()},
           "restrict_share_of_unfiltered": round(med["restrict"] / med["unfiltered"], 4),
           "restrict_GBps_read_4B_per_posting": round(p.rows * 4 / med["restrict"] / 1e6, 1),
           "stats": {name: {s: stats[name][s] for s in ("documents", "survivors", "ms_bound", "ms_score", "ms_total")} for name in stats},
           "filtered_equals_held": same}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
