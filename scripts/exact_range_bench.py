"""The exact range search (RaBitQ.exact_range_search_device) on the shape of profiles/exact_search_bench_1M.json (tests/synth.py
mixture, 1M x 128, 4096 lists), beside the exact top-k search of the same build at the matching topk, in one process on ONE index.
Prints ONE JSON line (and appends it to --out):

  python scripts/exact_range_bench.py --out profiles/exact_range_bench_1M.json

Per batch size (--batches, default 16 1000 65536) and neighbour rank kth (--ranks, default 10 100 1000):
  exact_search   [median, min, max] ms of exact_search_device at topk = kth over --steps calls after two warm-up calls, and its stats;
                 each query's radius is its own kth exact distance, so its range answer holds the rows strictly below it: kth - 1
                 of them unless the kth distance is tied
  exact_range    the same for exact_range_search_device at those radii: ms, rq_last_exact_stats of the last call (ms_scan / ms_exact /
                 ms_select, candidates, reruns, scan_launches, row_bytes_read), total results, bytes of the result, and
                 counts_match: every query's count equals the number of its top-kth distances below its radius
  range_recall   RaBitQ.range_recall of range_search at --probes (default 1 8 64) on the first --recall-queries queries of the batch
No figure is a pass condition; a wrong count is reported in the line and asserted once the line is written.
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
    ap.add_argument("--vectors", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 1000, 65536])
    ap.add_argument("--ranks", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4_000_000)
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
    dim = (d + 63) // 64 * 64
    centres = synth.device_centres(k, d, dev).contiguous()
    nq_max = max(args.batches)
    queries = synth.device_queries(centres, nq_max, args.sigma, dev).contiguous()
    P = synth.random_orthogonal(dim, seed=99)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def three(ms):
        ms = sorted(ms)
        return [round(ms[len(ms) // 2], 3), round(ms[0], 3), round(ms[-1], 3)]

    def rounded(st):
        return {key: (round(v, 3) if isinstance(v, float) else v) for key, v in st.items()}

    b = rq.RaBitQ.builder(n, d, centres.data_ptr(), k, orthogonal=P)
    for feed in (b.assign_chunk, b.place_chunk):
        for ci, i0 in enumerate(range(0, n, args.chunk)):
            m = min(args.chunk, n - i0)
            c = synth.device_mixture_chunk(centres, i0, m, args.sigma, ci)[0].contiguous()
            feed(c.data_ptr(), i0, m)
            del c
        if feed == b.assign_chunk:
            b.order()
    idx = b.finish()
    out = {"rows": "f32", "vectors": n, "dim": d, "lists": k, "n_hbm": idx.n_hbm, "row_bytes": dim * 4, "steps": args.steps,
           "version": _lib.lib().rq_version().decode(), "calls": {}}
    wrong = []
    for nq in args.batches:
        per_rank = {}
        for kth in args.ranks:
            od = torch.empty((nq, kth), device=dev)
            oi = torch.zeros((nq, kth), device=dev, dtype=torch.int32)
            on = torch.zeros(nq, device=dev, dtype=torch.int32)
            topk_call = lambda: idx.exact_search_device(queries.data_ptr(), nq, d, kth, od.data_ptr(), oi.data_ptr(), on.data_ptr())
            timed(topk_call)
            timed(topk_call)                                               # (the first call may have learnt its candidate capacity)
            t_topk = [timed(topk_call)[1] for _ in range(args.steps)]
            st_topk = rq.last_exact_stats()
            radii = od[:, kth - 1].contiguous()
            want = (od < radii[:, None]).sum(dim=1)

            def range_only():
                with idx.exact_range_search_device(queries.data_ptr(), nq, d, radii.data_ptr()) as res:
                    return res.total

            timed(range_only)
            timed(range_only)                                              # (the first call may have learnt its arena capacity)
            t_range, total = [], 0
            for _ in range(args.steps):
                total, ms = timed(range_only)
                t_range.append(ms)
            st_range = rq.last_exact_stats()
            with idx.exact_range_search_device(queries.data_ptr(), nq, d, radii.data_ptr()) as res:
                lims = res.to_host()[0]
            counts_match = bool(np.array_equal(np.diff(lims).astype(np.int64), want.cpu().numpy().astype(np.int64)))
            if not counts_match:
                wrong.append((nq, kth))
            m = min(nq, args.recall_queries)
            qh, rh = queries[:m].cpu().numpy(), radii[:m].cpu().numpy()
            recall = {str(p): round(idx.range_recall(qh, p, rh), 5) for p in args.probes}
            per_rank[str(kth)] = {
                "exact_search": {"ms": three(t_topk), **rounded(st_topk)},
                "exact_range": {"ms": three(t_range), **rounded(st_range), "total_results": int(total),
                                "results_per_query": round(total / nq, 2), "result_bytes": int(total) * 8 + (nq + 1) * 8,
                                "candidates_per_query": round(st_range["candidates"] / nq, 1), "counts_match": counts_match},
                "range_over_topk": round(sorted(t_range)[len(t_range) // 2] / sorted(t_topk)[len(t_topk) // 2], 3),
                "range_recall": {"queries": m, **recall}}
            del od, oi, on
        out["calls"][str(nq)] = per_rank
    idx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    assert not wrong, f"counts differ from the exact top-k's distances below the radius at (batch, rank) {wrong}"


if __name__ == "__main__":
    main()
