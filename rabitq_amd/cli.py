"""Benchmark harness with the reference CLI's behaviour (crates/cli/src/main.rs:11-83):

    python -m rabitq_amd.cli -b base.fvecs -c centroids.fvecs -q query.fvecs -t truth.ivecs \
                             -s saved_dir [-p 100] [-k 10] [-h | --heuristic-rank] [--metric l2|cosine|ip] [--make-truth]

* the flags are the reference's, letter for letter: `-h` is the heuristic re-ranker there (`#[argh(switch, short = 'h')]`,
  main.rs:35-37), not help -- argh reserves only `--help` -- so a caller script written for the reference CLI runs unchanged;

* if `--saved` is an existing directory the index is loaded from it, otherwise it is built from
  base + centroids and dumped there (main.rs:52-61);
* every query is issued one at a time and timed individually, QPS = N / sum(elapsed)
  (main.rs:66-80) -- the faithful, latency-bound number; `--batch B` additionally reports the
  batched throughput the GPU engine is designed for;
* prints mean recall@k against the ground-truth ivecs (src/utils.rs:367-379) and the METRICS line
  (src/metrics.rs:30-41);
* `--make-truth`: when the `-t` file does not exist, the exact top-max(topk, 100) of the query file is computed on the GPU
  (RaBitQ.exact_search) and written there as .ivecs first; an existing file is never overwritten;
* `--train K [--train-iters I]`: when the `-c` file does not exist, K centroids are trained from the base file on the GPU
  (train_centroids, deterministic) and written there as .fvecs first; an existing file is used as it is.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np

from . import RaBitQ, _lib, calculate_recall, metrics_reset, metrics_str, train_centroids, vecs


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="RaBitQ CLI args", add_help=False)   # `-h` belongs to the reference's switch
    ap.add_argument("--help", action="help", help="display usage information")
    ap.add_argument("-b", "--base", required=True, help="base path")
    ap.add_argument("-c", "--centroids", required=True, help="centroids path")
    ap.add_argument("-q", "--query", required=True, help="query path")
    ap.add_argument("-t", "--truth", required=True, help="truth path")
    ap.add_argument("-p", "--probe", type=int, default=100)
    ap.add_argument("-k", "--topk", type=int, default=10)
    ap.add_argument("-s", "--saved", required=True, help="saved directory")
    ap.add_argument("-h", "--heuristic-rank", "--heuristic_rank", dest="heuristic_rank", action="store_true", help="heuristic re-rank (maybe faster when topk is large)")
    ap.add_argument("--batch", type=int, default=0, help="also time batches of this many queries")
    ap.add_argument("--seed", type=int, default=0, help="seed of the generated rotation when building")
    ap.add_argument("--metric", choices=["l2", "cosine", "ip"], default="l2",
                    help="metric of the index when building (a saved index keeps its own): cosine normalises rows and queries "
                         "on the GPU, distances are 2 - 2 cos; ip is maximum inner product search (rows get one more "
                         "coordinate, distances are S + |q|^2 - 2<x, q> with S the largest squared row norm)")
    ap.add_argument("--rows", choices=[t.name for t in _lib.ROW_TABLE if t.elem_bytes == 1], default=None,
                    help="build a byte-row index (L2 only): the base is a .bvecs file whose one-byte elements are stored as given, "
                         "dim bytes per vector; the centroids stay an fvecs file")
    ap.add_argument("--probe-ratio", dest="probe_ratio", type=float, default=None, metavar="R",
                    help="adaptive probing: every query visits only the lists whose centroid distance is within R times its nearest "
                         "one's, at most --probe of them (inf: no cut); also prints the mean and maximum number of lists visited")
    ap.add_argument("--min-probe", dest="min_probe", type=int, default=1, metavar="M", help="with --probe-ratio: never fewer than M lists")
    ap.add_argument("--make-truth", dest="make_truth", action="store_true",
                    help="when the truth path does not exist: compute the exact top-max(topk, 100) of the queries on the GPU "
                         "and write it there as .ivecs (an existing file is left alone)")
    ap.add_argument("--train", type=int, default=0, metavar="K",
                    help="when the centroids path does not exist: train K lists from the base file on the GPU (--metric / --rows "
                         "respected, --seed is the sample's seed too) and write them there as .fvecs (an existing file is used as it is)")
    ap.add_argument("--train-iters", dest="train_iters", type=int, default=20, metavar="I", help="with --train: the iteration cap")
    return ap


def train_missing_centroids(args) -> bool:
    """--train K: write the centroid file unless it exists -> whether it was written.  k x d records (--metric ip: k x (d + 1), the
    centroids of the augmented rows -- a record length the inner-product build takes)."""
    if not args.train or os.path.exists(args.centroids):
        return False
    base = vecs.read_bvecs(args.base, _lib.ROW_TYPE_BY_NAME[args.rows].returns) if args.rows else vecs.read_matrix(args.base)
    vecs.write_vecs(args.centroids, train_centroids(base, args.train, iters=args.train_iters, seed=args.seed, metric=args.metric, rows=args.rows))
    return True


def make_truth(index, queries, path, topk: int) -> bool:
    """Write the exact top-max(topk, 100) ids of `queries` to `path` as .ivecs unless the file exists -> whether it was written.
    A query with fewer stored rows than that gets a shorter record."""
    if os.path.exists(path):
        return False
    k = max(topk, 100)
    ids = np.zeros((0, k), np.uint32)
    cnt = np.zeros(0, np.uint32)
    for s in range(0, len(queries), 4096):
        _, i_, c_ = index.exact_search(np.stack(queries[s:s + 4096]), k)
        ids, cnt = np.concatenate([ids, i_]), np.concatenate([cnt, c_])
    if len(cnt) and int(cnt.min()) == k:
        vecs.write_ivecs(path, ids)
    else:
        vecs.write_vecs(path, [ids[j, :cnt[j]].astype("<i4") for j in range(len(cnt))])
    return True


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)

    if os.path.isdir(args.saved):
        print(f"loading from {args.saved!r}...")
        index = RaBitQ.load_from_dir(args.saved)
    else:
        if train_missing_centroids(args):
            print(f"{args.train} centroids trained and written to {args.centroids!r}")
        print("training...")
        if args.rows:
            base = vecs.read_bvecs(args.base, _lib.ROW_TYPE_BY_NAME[args.rows].returns)
            index = RaBitQ.build(base, vecs.read_matrix(args.centroids), seed=args.seed, metric=args.metric, rows=args.rows)
        else:
            index = RaBitQ.from_path(args.base, args.centroids, seed=args.seed, metric=args.metric)
        print(f"saving to local file: {args.saved!r}")
        index.dump_to_dir(args.saved)

    queries = vecs.read_vecs(args.query, np.float32)
    if args.make_truth and make_truth(index, queries, args.truth, args.topk):
        print(f"ground truth written to {args.truth!r} (exact search, top {max(args.topk, 100)})")
    truth = vecs.read_vecs(args.truth, np.int32)
    print("querying...")
    metrics_reset()
    total_time, recall = 0.0, 0.0
    for i, q in enumerate(queries):
        t0 = time.perf_counter()
        res = index.query(q, args.probe, args.topk, args.heuristic_rank)
        total_time += time.perf_counter() - t0
        ids = [i_ for _, i_ in res]
        ids += [-1] * (args.topk - len(ids))
        recall += calculate_recall(truth[i], ids, args.topk)
    n = len(queries)
    print(f"QPS: {n / total_time}, recall: {recall / n}")
    print(f"Metrics [{metrics_str()}]")
    if args.probe_ratio is not None:      # the same queries, each cut by its centroid distances (one query per call, timed alike)
        metrics_reset()
        total_time, recall, visited = 0.0, 0.0, []
        for i, q in enumerate(queries):
            t0 = time.perf_counter()
            _, ids, cnt, npr = index.query_batch_adaptive(np.asarray(q, np.float32)[None, :], args.probe, args.topk, args.probe_ratio,
                                                          args.min_probe, None, args.heuristic_rank)
            total_time += time.perf_counter() - t0
            got = ids[0, :cnt[0]].tolist()
            recall += calculate_recall(truth[i], got + [-1] * (args.topk - len(got)), args.topk)
            visited.append(int(npr[0]))
        print(f"adaptive (ratio {args.probe_ratio}, min {args.min_probe}): QPS: {n / total_time}, recall: {recall / n}, "
              f"lists visited: mean {np.mean(visited):.2f}, max {max(visited) if visited else 0}")
        print(f"Metrics [{metrics_str()}]")
    if args.batch > 0:
        q = np.stack(queries)
        t0 = time.perf_counter()
        hits = 0
        for s in range(0, n, args.batch):
            _, ids, cnt = index.query_batch(q[s:s + args.batch], args.probe, args.topk, args.heuristic_rank)
            for j in range(ids.shape[0]):
                hits += len(set(ids[j, :cnt[j]].tolist()) & set(truth[s + j][:args.topk].tolist()))
        dt = time.perf_counter() - t0
        print(f"batched ({args.batch}): QPS: {n / dt}, recall: {hits / (n * args.topk)}")
        if args.probe_ratio is not None:
            t0 = time.perf_counter()
            hits, visited = 0, []
            for s in range(0, n, args.batch):
                _, ids, cnt, npr = index.query_batch_adaptive(q[s:s + args.batch], args.probe, args.topk, args.probe_ratio, args.min_probe,
                                                              None, args.heuristic_rank)
                visited.append(npr)
                for j in range(ids.shape[0]):
                    hits += len(set(ids[j, :cnt[j]].tolist()) & set(truth[s + j][:args.topk].tolist()))
            dt = time.perf_counter() - t0
            visited = np.concatenate(visited)
            print(f"batched adaptive ({args.batch}, ratio {args.probe_ratio}, min {args.min_probe}): QPS: {n / dt}, "
                  f"recall: {hits / (n * args.topk)}, lists visited: mean {visited.mean():.2f}, max {int(visited.max())}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
