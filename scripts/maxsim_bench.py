"""Multi-vector search at the headline shape (100M x 128, 4096 lists, the synthetic mixture of tests/synth.py; documents of --stride
consecutive ids, whose rows the mixture scatters over the lists), in one session on one index.  Prints ONE JSON line
(and appends it to --out).  Per batch of --batches, medians of --steps calls after a warm-up, the forms alternated:
  maxsim        wall ms of rq_query_batch_maxsim_device (--tokens tokens a query, --fetch rows a token), ms_source / ms_score of
                rq_last_maxsim_stats (HIP events around the scoring launch), (token, row) pairs per second of the launch
  peak shares   the launch's matrix work, 2 x 32-token tiles x rows x dim flop, over ms_score against the 2.5 PFLOP/s dense bf16 peak,
                and its gathered bytes (rows_gathered x row bytes) per second beside the by-id gather's measured 5.3 - 5.4 TB/s
                 and the 8 TB/s HBM peak -- which of the two bounds it is the larger share
  no_prefilter  the same call with RQ_MAXSIM_NO_PREFILTER (every pair on the vector unit); its outputs must equal the first form's
  baseline      the same answer the way the entries before this one allow: query_batch per token, the candidate rows' distances_to
                in numpy-sized pieces on the host, min and sum in numpy (first --baseline-queries queries; the same documents)

  python scripts/maxsim_bench.py [--vectors 100000000] [--out profiles/maxsim_bench_100M.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF16_PEAK, HBM_PEAK = 2.5e15, 8.0e12


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
    ap.add_argument("--baseline-queries", type=int, default=4)
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
    n, d, k, T, S, F = args.vectors, args.dim, args.lists, args.tokens, args.stride, args.fetch

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
    out = {"vectors": n, "dim": d, "lists": k, "nprobe": args.nprobe, "stride": S, "tokens": T, "fetch": F, "topk": args.topk, "steps": args.steps,
           "build_ms": round(build_ms, 1), "runs": []}
    for B in (int(v) for v in args.batches.split(",")):
        q = synth.device_queries(centres, B * T, args.sigma, dev)
        od = [torch.empty((B, args.topk), device=dev, dtype=torch.float32) for _ in range(2)]
        oi = [torch.empty((B, args.topk), device=dev, dtype=torch.int32) for _ in range(2)]
        on = [torch.empty(B, device=dev, dtype=torch.int32) for _ in range(2)]
        oc = torch.empty(B, device=dev, dtype=torch.int32)
        call = lambda f: g.query_batch_maxsim_device(q.data_ptr(), 0, B, T, d, args.nprobe, args.topk, S, F, od[f].data_ptr(), oi[f].data_ptr(),
                                                     on[f].data_ptr(), oc.data_ptr(), prefilter=f == 0)
        for f in (0, 1, 0, 1):
            timed(lambda: call(f))
        wall, src, score, st = ([], []), ([], []), ([], []), [None, None]
        for _ in range(args.steps):
            for f in (0, 1):
                wall[f].append(timed(lambda: call(f))[1])
                st[f] = ix.last_maxsim_stats()
                src[f].append(st[f]["ms_source"]), score[f].append(st[f]["ms_score"])
        same = bool((od[0].view(torch.int32) == od[1].view(torch.int32)).all().item() and (oi[0] == oi[1]).all().item())
        ms = med(score[0]) * 1e-3
        flop = 2.0 * (-(-T // 32) * 32) * st[0]["rows_gathered"] * g.dim
        gbytes = st[0]["rows_gathered"] * g.dim * 4
        rec = {"batch": B, "maxsim_ms": med(wall[0]), "ms_source": med(src[0]), "ms_score": med(score[0]), "pairs": st[0]["pairs"],
               "pairs_per_s": round(st[0]["pairs"] / ms, 1), "exact_distances": st[0]["exact_distances"], "list_overflows": st[0]["list_overflows"],
               "candidates": st[0]["candidates"], "rows_gathered": st[0]["rows_gathered"], "lds_bytes": st[0]["lds_bytes"],
               "share_of_bf16_peak": round(flop / ms / BF16_PEAK, 5), "gather_TBps": round(gbytes / ms / 1e12, 3),
               "share_of_hbm_peak": round(gbytes / ms / HBM_PEAK, 4), "no_prefilter_ms": med(wall[1]), "no_prefilter_ms_score": med(score[1]),
               "no_prefilter_same_bits": same}
        nb = min(args.baseline_queries, B)
        if nb:   # the host way, on the first nb queries: the plain call, ids -> documents -> every id of them -> distances_to -> numpy
            qh = q[:nb * T].cpu().numpy()

            def host_way():
                _, ids, cnt = g.query_batch(qh, args.nprobe, F)
                best = []
                for b in range(nb):
                    docs = np.unique(np.concatenate([ids[b * T + t, :cnt[b * T + t]] for t in range(T)]) // S)
                    rows = (docs[:, None].astype(np.int64) * S + np.arange(S)[None, :]).reshape(1, -1)
                    rows = np.minimum(rows, 0xFFFFFFFF).astype(np.uint32)
                    dist = g.distances_to(qh[b * T:(b + 1) * T], np.repeat(rows, T, axis=0)).reshape(T, len(docs), S)
                    best.append(docs[np.argsort(dist.min(axis=2).sum(axis=0, dtype=np.float32), kind="stable")[:args.topk]])
                return best
            host_way()
            t_host = [timed(host_way)[1] for _ in range(max(args.steps // 2, 1))]
            rec["baseline_queries"] = nb
            rec["baseline_ms_per_query"] = round(float(np.median(t_host)) / nb, 3)
            rec["maxsim_ms_per_query"] = round(med(wall[0]) / B, 4)
        out["runs"].append(rec)
        print(rec, file=sys.stderr, flush=True)
        del q, od, oi, on, oc
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
