"""Inner-product metric at the headline shapes (1M and 100M x 128, 4096 lists, nprobe 64, the synthetic mixture of tests/synth.py
with per-row lengths spread over 2^-o .. 2^o, --octaves).  One process measures ONE side and prints ONE JSON line:

  --side ip    an inner-product index of the rows (index dim = ceil64(d + 1): 192 for d = 128)
  --side l2    the L2 index of the same rows (dim 128), so that the price of the extra 64-wide word is visible

Each side records the build's engine time (the streamed builder's calls, as bench.py times its build; after a warm-up build; the
ip side includes the pass that finds the bound, rq_row_sqnorm_max_device), the median and the spread (min / max) of the step time
and the queries/s at batches of 64 and 65 536 over --steps calls, and recall@10 of --recall-queries queries against a float64
brute-force search by the side's own measure (largest inner product / smallest L2 distance).  Run the sides alternately and keep
every line:

  python scripts/ip_bench.py --side ip --vectors 1000000 --out profiles/ip_bench_1M.json
  python scripts/ip_bench.py --side l2 --vectors 1000000 --out profiles/ip_bench_1M.json
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
    ap.add_argument("--side", choices=["ip", "l2"], required=True)
    ap.add_argument("--vectors", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--octaves", type=float, default=1.0)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    n, d, k = args.vectors, args.dim, args.lists
    ip = args.side == "ip"
    dim = (d + 64) // 64 * 64 if ip else (d + 63) // 64 * 64
    x, cd = synth.device_mixture(n, d, k, args.sigma, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    for i0 in range(0, n, 4_000_000):   # per-row lengths
        m = min(4_000_000, n - i0)
        x[i0:i0 + m] *= torch.exp2((2.0 * torch.rand(m, 1, generator=g, device=dev) - 1.0) * args.octaves)
    queries = synth.device_queries(cd, 65536, args.sigma, dev)
    P = synth.random_orthogonal(dim, seed=99)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def engine_build(rows):
        ms = 0.0
        kw = {}
        if ip:   # the streamed builder has no automatic bound: one more pass over the rows
            bound, ms = timed(lambda: rq.ops.row_sqnorm_max_device(x.data_ptr(), rows, d))
            kw = {"metric": "ip", "max_sq_norm": bound}
        b = rq.RaBitQ.builder(rows, d, cd.data_ptr(), k, orthogonal=P, **kw)
        for call in (lambda: b.assign_chunk(x.data_ptr(), 0, rows), b.order, lambda: b.place_chunk(x.data_ptr(), 0, rows)):
            ms += timed(call)[1]
        idx, t = timed(b.finish)
        return idx, ms + t

    engine_build(min(n, 1 << 20))[0].close()   # warm-up: code objects, kernel attributes
    idx, build_ms = engine_build(n)
    out = {"side": args.side, "vectors": n, "d": d, "index_dim": idx.dim, "lists": k, "nprobe": args.nprobe, "topk": args.topk,
           "octaves": args.octaves, "build_engine_ms": round(build_ms, 1), "step_ms": {}}
    od = torch.empty((65536, args.topk), device=dev)
    oi = torch.zeros((65536, args.topk), device=dev, dtype=torch.int32)
    on = torch.zeros(65536, device=dev, dtype=torch.int32)
    for nq in (64, 65536):
        call = lambda: idx.query_batch_device(queries.data_ptr(), nq, d, args.nprobe, args.topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        timed(call), timed(call)
        ms = sorted(timed(call)[1] for _ in range(args.steps))
        med = ms[len(ms) // 2]
        out["step_ms"][str(nq)] = {"median": round(med, 4), "min": round(ms[0], 4), "max": round(ms[-1], 4),
                                   "queries_per_s": round(nq / med * 1e3, 1)}
    # recall@topk against float64 brute force (the last 65 536-query call left the first queries' results in oi)
    nr = min(args.recall_queries, 65536)
    q64 = queries[:nr].double()
    best_v = torch.full((nr, args.topk), float("-inf"), device=dev, dtype=torch.float64)
    best_i = torch.zeros((nr, args.topk), device=dev, dtype=torch.int64)
    for i0 in range(0, n, 2_000_000):
        xc = x[i0:i0 + 2_000_000].double()
        score = q64 @ xc.T                                    # the inner products
        if not ip:                                            # L2: smallest |x|^2 - 2<x, q> (|q|^2 is the same for every row)
            score = 2.0 * score - (xc * xc).sum(dim=1)[None, :]
        v, i = torch.topk(score, args.topk, dim=1)
        cat_v, cat_i = torch.cat([best_v, v], dim=1), torch.cat([best_i, i + i0], dim=1)
        best_v, sel = torch.topk(cat_v, args.topk, dim=1)
        best_i = torch.gather(cat_i, 1, sel)
        del xc, score
    got, truth = oi[:nr].cpu().numpy().view("uint32"), best_i.cpu().numpy()
    cnt = on[:nr].cpu().numpy()
    hits = sum(len(set(got[b, :cnt[b]].tolist()) & set(truth[b].tolist())) for b in range(nr))
    out["recall_at_%d" % args.topk] = round(hits / (nr * args.topk), 4)
    out["recall_queries"] = nr
    idx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
