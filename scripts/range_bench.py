"""Range search at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, nprobe 64, batches of 65 536, the synthetic
mixture of tests/synth.py as bench.py generates it), beside the plain top-10 call of the same library in the same process, the
calls alternated.  Prints ONE JSON line:
  plain_ms_before    the plain top-10 device call (rq_query_batch_device) timed BEFORE the process has made any range call:
                     [median, min, max] ms over --steps calls, and its profile (matrix_additive_launches tells the scan gate)
  plain_ms           the same call alternated with the range legs ([median, min, max]; its profile must show the same gate)
  tight              radii = each query's own 10th plain distance, nudged up (nextafter * 1.0001): about 10 results per query --
                     [median, min, max] ms per call, total results, bytes of the result, one profiled call's per-kernel split beside the plain
                     call's (ms_scan / ms_rerank / ms_sort / ms_replay / ...; the range call's ms_sort is everything behind the hit
                     counts: offsets, emission, the segmented sort, the split)
  r100 / r1000       radii scaled (by bisection on a 2048-query sample) to give about 100 / about 1000 results per query: the same
  one_query          median ms of one query per call (host entry), tight radius, beside the plain one-query call
  tight_bf16_gate    the tight leg with option scan_gate = 1 (the bf16 threshold gate instead of the additive one)
--plain-only stops after plain_ms_before and touches no range entry: the script then also runs in a checkout of a commit
without range search (the parent's), which is how the plain column is compared with the parent's -- alternate the two.

  python scripts/range_bench.py [--vectors 100000000] [--steps 5]
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import rabitq_amd
    from rabitq_amd import _lib, index as ix
    from tests import synth

    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda", 0)
    n, d, k, B, probe, topk = args.vectors, args.dim, args.lists, args.batch, args.nprobe, 10
    t0 = time.time()
    centres = synth.device_centres(k, d, dev, 1.0)
    q = synth.device_queries(centres, B, args.sigma, dev, seed=7)
    P = synth.random_orthogonal(d, seed=99)
    chunk = 4_000_000
    chunks = [(ci, i0, min(chunk, n - i0)) for ci, i0 in enumerate(range(0, n, chunk))]

    def gen(ci, i0, m):
        return synth.device_mixture_chunk(centres, i0, m, args.sigma, ci, 42, 0, k, None)[0].contiguous()

    builder = rabitq_amd.RaBitQ.builder(n, d, centres.data_ptr(), k, orthogonal=P)
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
    torch.cuda.synchronize()

    def plain(m=B):
        idx.query_batch_device(q.data_ptr(), m, d, probe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())

    def ranged(r, m=B):
        with idx.range_search_device(q.data_ptr(), m, d, probe, r.data_ptr()) as res:
            return res.total

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def profiled(fn):
        ix.set_profiling(1)
        fn()
        pr = ix.last_profile()
        ix.set_profiling(0)
        return {key: round(v, 3) if isinstance(v, float) else v for key, v in pr.items()
                if key.startswith("ms_") or key in ("scan_candidates", "rerank_candidates", "rerank_shadow_rejects", "retries", "scan_launches",
                                                    "matrix_launches", "matrix_additive_launches")}

    def stats(ts):
        return [round(float(np.median(ts)), 3), round(float(min(ts)), 3), round(float(max(ts)), 3)]

    for _ in range(args.warmup + 1):
        plain()
    torch.cuda.synchronize()
    out = {"vectors": n, "dim": d, "lists": k, "nprobe": probe, "batch": B, "build_s": round(build_s, 1), "version": _lib.lib().rq_version().decode(),
           "steps": args.steps, "plain_ms_before": stats([timed(plain)[0] for _ in range(args.steps)]), "plain_profile_before": profiled(plain)}
    if args.plain_only:
        print(json.dumps(out))
        return
    kth = od.max(dim=1).values
    tight = torch.nextafter(kth, torch.full_like(kth, float("inf"))) * 1.0001

    def scale_for(target):  # radius = kth * s with about `target` results per query, by bisection on a sample
        lo, hi, m = 1.0, 4.0, min(B, 2048)
        for _ in range(12):
            mid = (lo + hi) / 2
            r = (kth * mid).contiguous()
            if ranged(r, m) / m < target:
                lo = mid
            else:
                hi = mid
        return hi

    legs = {"tight": tight.contiguous()}
    scales = {}
    for name, target in (("r100", 100), ("r1000", 1000)):
        scales[name] = scale_for(target)
        legs[name] = (kth * scales[name]).contiguous()
    out["radius_scales"] = {key: round(v, 4) for key, v in scales.items()}
    for _ in range(args.warmup):
        plain()
        for r in legs.values():
            ranged(r)
    torch.cuda.synchronize()
    t_plain, t_leg, totals = [], {name: [] for name in legs}, {}
    for _ in range(args.steps):   # alternated
        t_plain.append(timed(plain)[0])
        for name, r in legs.items():
            ms, total = timed(lambda r=r: ranged(r))
            t_leg[name].append(ms)
            totals[name] = total
    out["plain_ms"] = stats(t_plain)
    out["plain_profile"] = profiled(plain)
    for name, r in legs.items():
        out[name] = {"ms": stats(t_leg[name]), "total_results": int(totals[name]),
                     "results_per_query": round(totals[name] / B, 2), "result_bytes": int(totals[name]) * 8 + (B + 1) * 8,
                     "profile": profiled(lambda r=r: ranged(r))}
    ix.set_option("scan_gate", 1)
    ranged(legs["tight"])
    out["tight_bf16_gate"] = {"ms": stats([timed(lambda: ranged(legs["tight"]))[0] for _ in range(args.steps)]),
                              "profile": profiled(lambda: ranged(legs["tight"]))}
    ix.set_option("scan_gate", 0)
    # one query per call, host entry
    qh = q[:64].cpu().numpy()
    rh = tight[:64].cpu().numpy()
    t_one_plain, t_one_range = [], []
    for i in range(64):
        t = time.perf_counter()
        idx.query_batch(qh[i:i + 1], probe, topk)
        t_one_plain.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        idx.range_search(qh[i:i + 1], probe, rh[i:i + 1])
        t_one_range.append((time.perf_counter() - t) * 1e3)
    out["one_query"] = {"plain_ms": round(float(np.median(t_one_plain[8:])), 4), "range_ms": round(float(np.median(t_one_range[8:])), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
