"""Adaptive probing at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, batches of 65 536, the synthetic mixture of
tests/synth.py as bench.py generates it; --distribution hard: bench.py's overlapping clusters, Zipf list sizes, trained centroids).
Truth comes from exact_search on the first --truth-queries queries of the batch; every recall below is recall@10 on that sample,
every time is one device call over the whole batch.  Prints ONE JSON line:
  fixed        nprobe 8 / 16 / 32 / 64 of the plain entry: recall, [median, min, max] ms per call
  adaptive     probe = --nprobe and a grid of ratios -- among them the ratios tune_probe_ratio returns for the recall of the plain
               call at --nprobe and for 0.95 -- : mean / max lists visited over the batch, recall, [median, min, max] ms per call
  no_cut       the adaptive entry with ratio = inf beside the plain entry, alternated: what the cut launch and the plan features a
               cut pass gives up cost when nothing is cut
  small_64     64 queries per call, adaptive (ratio = inf) beside plain: the price of leaving the few-launch path

  python scripts/adaptive_probe_bench.py [--vectors 100000000] [--distribution easy|hard] [--steps 5]
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
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--distribution", choices=["easy", "hard"], default="easy")
    ap.add_argument("--zipf", type=float, default=0.7)
    ap.add_argument("--truth-queries", type=int, default=1000)
    ap.add_argument("--ratios", default="1.05,1.1,1.2,1.35,1.5,2.0")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import numpy as np
    import torch
    import rabitq_amd
    from rabitq_amd import _lib, ops
    from tests import synth

    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda", 0)
    n, d, k, B, probe, topk = args.vectors, args.dim, args.lists, args.batch, args.nprobe, 10
    hard = args.distribution == "hard"
    t0 = time.time()
    centres = synth.device_centres(k, d, dev, args.sigma if hard else 1.0)
    weights = None
    if hard:
        wz = 1.0 / torch.arange(1, k + 1, device=dev, dtype=torch.float64) ** args.zipf
        weights = (wz / wz.sum()).float()[torch.randperm(k, device=dev, generator=torch.Generator(device=dev).manual_seed(5))]
    q = synth.device_queries(centres, B, args.sigma, dev, seed=7, weights=weights)
    P = synth.random_orthogonal(d, seed=99)
    chunk = 4_000_000
    chunks = [(ci, i0, min(chunk, n - i0)) for ci, i0 in enumerate(range(0, n, chunk))]

    def gen(ci, i0, m):
        return synth.device_mixture_chunk(centres, i0, m, args.sigma, ci, 42, 0, k, weights)[0].contiguous()

    centroids = centres
    if hard:
        ns = min(n, 256 * k)
        sample = synth.device_mixture_chunk(centres, 0, ns, args.sigma, 999_983, 42, 0, k, weights)[0].contiguous()
        centroids = torch.zeros((k, d), device=dev, dtype=torch.float32)
        ops.kmeans_device(sample.data_ptr(), ns, d, k, centroids.data_ptr(), iters=10, seed=3)
        del sample
    builder = rabitq_amd.RaBitQ.builder(n, d, centroids.data_ptr(), k, orthogonal=P)
    for ci, i0, m in chunks:
        xc = gen(ci, i0, m)
        torch.cuda.synchronize()
        builder.assign_chunk(xc.data_ptr(), i0, m)
        del xc
    builder.order()
    for ci, i0, m in chunks:
        xc = gen(ci, i0, m)
        torch.cuda.synchronize()
        builder.place_chunk(xc.data_ptr(), i0, m)
        del xc
    idx = builder.finish()
    torch.cuda.empty_cache()
    build_s = time.time() - t0

    od = torch.empty((B, topk), dtype=torch.float32, device=dev)
    oi = torch.empty((B, topk), dtype=torch.int32, device=dev)
    on = torch.empty(B, dtype=torch.int32, device=dev)
    onp = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    S = min(args.truth_queries, B)
    qs = q[:S].cpu().numpy()
    _, eids, ecnt = idx.exact_search(qs, topk)

    def plain(p=probe, m=B):
        idx.query_batch_device(q.data_ptr(), m, d, p, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())

    def adaptive(ratio, m=B, min_probe=1):
        idx.query_batch_adaptive_device(q.data_ptr(), m, d, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr(), onp.data_ptr(),
                                        ratio=ratio, min_probe=min_probe)

    def recall_now():
        torch.cuda.synchronize()
        return round(idx._recall_of(oi[:S].cpu().numpy().view(np.uint32), on[:S].cpu().numpy().view(np.uint32), eids, ecnt), 5)

    def timed(fn):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def stats(ts):
        return [round(float(np.median(ts)), 3), round(float(min(ts)), 3), round(float(max(ts)), 3)]

    def leg(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        return stats([timed(fn) for _ in range(args.steps)])

    out = {"vectors": n, "dim": d, "lists": k, "nprobe": probe, "batch": B, "distribution": args.distribution, "truth_queries": S,
           "build_s": round(build_s, 1), "version": _lib.lib().rq_version().decode(), "steps": args.steps, "fixed": {}, "adaptive": []}
    for p in (8, 16, 32, 64):
        ms = leg(lambda p=p: plain(p))
        out["fixed"][str(p)] = {"ms": ms, "recall": recall_now()}
    full = out["fixed"][str(probe)]["recall"] if str(probe) in out["fixed"] else None
    tuned = {}
    for name, target in (("recall_of_fixed", full), ("0.95", 0.95)):
        if target is None:
            continue
        r, rec, mean = idx.tune_probe_ratio(qs, probe, topk, target)
        tuned[name] = {"target": target, "ratio": r, "recall": round(rec, 5), "mean_nprobe": round(mean, 3)}
    out["tuned"] = tuned
    grid = sorted({float(x) for x in args.ratios.split(",") if x} | {t["ratio"] for t in tuned.values() if np.isfinite(t["ratio"])})
    for r in grid:
        ms = leg(lambda r=r: adaptive(r))
        rec = recall_now()
        npr = onp.cpu().numpy()
        out["adaptive"].append({"ratio": round(r, 5), "mean_nprobe": round(float(npr.mean()), 3), "max_nprobe": int(npr.max()),
                                "recall": rec, "ms": ms})
    # nothing cut: the adaptive entry beside the plain one, alternated
    inf = float("inf")
    for fn in (plain, lambda: adaptive(inf)):
        fn()
    tp, ta = [], []
    for _ in range(args.steps):
        tp.append(timed(plain))
        ta.append(timed(lambda: adaptive(inf)))
    out["no_cut"] = {"plain_ms": stats(tp), "adaptive_ms": stats(ta)}
    tp, ta = [], []
    for i in range(40):
        tp.append(timed(lambda: plain(probe, 64)))
        ta.append(timed(lambda: adaptive(inf, 64)))
    out["small_64"] = {"plain_ms": stats(tp[8:]), "adaptive_ms": stats(ta[8:])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
