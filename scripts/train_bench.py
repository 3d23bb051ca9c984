"""Centroid training at the build's headline shape: 4096 lists x dim 128 on a 2^20-row sample of the device mixture of
tests/synth.py (sigma 0.5, centre scale 0.5: overlapping clusters), the new trainer (rq_train_centroids_device) beside the old one
(rq_kmeans_device, the baseline: the parent's code) with the same sample size and iteration counts.  Writes ONE JSON file:
  per_iteration_ms   per trainer [median, min, max] over --repeats of (time(--iters) - time(--iters-short)) / (difference of the
                     iterations): whole calls timed with a host clock (each call ends in a device synchronise), alternated
  call_ms            the whole call at --iters, same form
  held_out_mse       mean squared distance of --held-out fresh rows of the mixture to their nearest centroid, per trainer
  lists              largest / mean list size of the index built on each trainer's centroids (the same base, the same rotation)
  new                iters_run, splits and the objective of the new trainer's run
  kernel_split       (after --fold-kernel-stats CSV) the new trainer's device time per iteration by stage -- assign, group,
                     reduce -- from a `rocprofv3 --kernel-trace --stats` run of `--profile-only`, which runs the new trainer alone

  python scripts/train_bench.py [--out profiles/train_centroids_bench.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/train_bench.py --profile-only
  python scripts/train_bench.py --fold-kernel-stats DIR/.../..._kernel_stats.csv --out profiles/train_centroids_bench.json   (no GPU)
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = {   # kernel name prefix -> stage of an iteration
    "assign": ("assign_", "to_bf16_kernel", "row_sqnorm_kernel", "transpose_kernel", "gather_rows_kernel"),
    "group": ("train_changed_kernel", "label_hist_kernel", "group_scan_kernel", "train_scatter_kernel", "list_sort_kernel"),
    "reduce": ("train_reduce_kernel", "train_split_kernel"),
}


def fold_kernel_stats(path, out_path, iters):
    rows = list(csv.DictReader(open(path)))
    split = {s: 0.0 for s in STAGES}
    split["other"] = 0.0
    names = {}
    for r in rows:
        name, ms = r["Name"], float(r["TotalDurationNs"]) / 1e6
        short = name.split("<")[0].split("(")[0].replace("void ", "").strip()
        stage = next((s for s, pre in STAGES.items() if any(short.startswith(p) for p in pre)), "other")
        split[stage] += ms
        names[short] = names.get(short, 0.0) + ms
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats of --profile-only (the new trainer alone, one call of %d iterations)" % iters,
                           "ms_per_iteration": {s: round(v / iters, 4) for s, v in split.items() if s != "other"},
                           "ms_other_kernels_whole_run": round(split["other"], 3),   # data generation, gather, transform, start, unpad
                           "kernels_ms_total": {k: round(v, 3) for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:12]}}
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res["kernel_split"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--iters-short", dest="iters_short", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--held-out", dest="held_out", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_centroids_bench.json"))
    ap.add_argument("--profile-only", dest="profile_only", action="store_true")
    ap.add_argument("--fold-kernel-stats", dest="fold", default=None)
    args = ap.parse_args()
    if args.fold:
        return fold_kernel_stats(args.fold, args.out, args.iters)

    import numpy as np
    import torch
    import rabitq_amd
    from rabitq_amd import _lib, ops
    from tests import synth

    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda", 0)
    n, d, k = args.rows, args.dim, args.lists
    ppc = max(1, n // k)          # both trainers sample min(n, ppc * k) = n rows
    x, centres = synth.device_mixture(n, d, k, args.sigma, dev, centre_scale=0.5)
    held, _ = synth.device_mixture_chunk(centres, 0, args.held_out, args.sigma, chunk_id=9999)
    out_new = torch.zeros((k, d), device=dev)
    out_old = torch.zeros((k, d), device=dev)

    def run_new(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = rabitq_amd.train_centroids_device(x.data_ptr(), n, d, k, out_new.data_ptr(), iters=iters, points_per_centroid=ppc, seed=3)
        return (time.perf_counter() - t0) * 1e3, st

    def run_old(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.kmeans_device(x.data_ptr(), n, d, k, out_old.data_ptr(), iters=iters, points_per_centroid=ppc, seed=3)
        return (time.perf_counter() - t0) * 1e3, None

    if args.profile_only:
        ms, st = run_new(args.iters)
        print(json.dumps({"profile_only": True, "iters_run": st.iters_run, "call_ms": round(ms, 2)}))
        return

    run_new(args.iters_short), run_old(args.iters_short)            # warm-up: code objects, allocations
    per_it = {"new": [], "old": []}
    call = {"new": [], "old": []}
    st_new = None
    for _ in range(args.repeats):                                    # alternated: other work shares the machine
        for name, fn in (("new", run_new), ("old", run_old)):
            short, _ = fn(args.iters_short)
            long_, st = fn(args.iters)
            if name == "new":
                st_new = st
                assert st.iters_run == args.iters, "the new trainer stopped early: time fewer iterations"
            per_it[name].append((long_ - short) / (args.iters - args.iters_short))
            call[name].append(long_)
    form = lambda v: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]

    def mse(c):
        best = torch.full((held.shape[0],), float("inf"), device=dev)
        for s in range(0, held.shape[0], 10_000):
            best[s:s + 10_000] = (torch.cdist(held[s:s + 10_000], c) ** 2).min(1).values
        return float(best.double().mean())

    def lists(c):
        idx = rabitq_amd.RaBitQ.build_device(x.data_ptr(), n, d, c.data_ptr(), k, orthogonal=synth.random_orthogonal(d, seed=99))
        sizes = np.diff(idx.offsets.astype(np.int64))
        idx.close()
        return {"largest": int(sizes.max()), "mean": float(sizes.mean()), "empty": int((sizes == 0).sum())}

    res = {"shape": {"sample_rows": n, "dim": d, "lists": k, "sigma": args.sigma, "iters": args.iters, "iters_short": args.iters_short,
                     "repeats": args.repeats, "device": torch.cuda.get_device_name(0)},
           "form": "[median, min, max]",
           "per_iteration_ms": {"new": form(per_it["new"]), "old": form(per_it["old"])},
           "call_ms": {"new": form(call["new"]), "old": form(call["old"])},
           "held_out_mse": {"new": mse(out_new), "old": mse(out_old), "generating_centres": mse(centres)},
           "lists": {"new": lists(out_new), "old": lists(out_old)},
           "new": {"iters_run": st_new.iters_run, "splits": st_new.splits, "sample_rows": st_new.sample_rows,
                   "objective": [float(v) for v in st_new.objective]}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
