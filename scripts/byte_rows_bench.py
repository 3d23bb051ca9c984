"""Byte rows at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, nprobe 64, the synthetic mixture of tests/synth.py
scaled into the byte range) and at dim 768 with 40M rows: what the rerank of an index that stores u8 / i8 rows costs beside the f32
index's shadow-filtered one, and what the raw vectors take.  One process measures ONE index and prints ONE JSON line:

  --rows u8              the index of the mixture scaled by 32, moved to 128, rounded and clipped to 0 .. 255, built chunk by chunk
                         from uint8 chunks
  --rows i8              the mixture scaled by 32, rounded and clipped to -128 .. 127, from int8 chunks (other values than u8's:
                         its answers are its own; centroids and queries are moved likewise)
  --rows f32 --values T  the f32 index (8-bit shadow rows, the default pre-filter) of the same values the T index holds, widened: the
                         two answer identically

Every chunk of the base is generated on the device, rounded, fed to the streamed builder and dropped (each pass regenerates it), so
no side ever holds the n x d input.  Reported: the build's engine time, the raw-vector bytes of the index, and at batches of 64
and 65 536 queries the median / min / max wall time per call over --steps calls and, from one profiled call, ms_rerank and the
survivors the shadow rows rejected.  `--dump DIR` keeps the 65 536 results; `--compare A B` asserts two dumps identical.

  python scripts/byte_rows_bench.py --rows f32 --values u8 --dump out/f32 --out profiles/byte_rows_bench_100M.json
  python scripts/byte_rows_bench.py --rows u8 --dump out/u8 --out profiles/byte_rows_bench_100M.json
  python scripts/byte_rows_bench.py --rows i8 --out profiles/byte_rows_bench_100M.json
  python scripts/byte_rows_bench.py --compare out/f32 out/u8
  python scripts/byte_rows_bench.py --rows u8 --dim 768 --vectors 40000000 ...
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(a, b):
    import numpy as np
    for name in ("n", "ids", "dist"):
        x, y = np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{name} differs between {a} and {b}"
    print(json.dumps({"compare": [a, b], "identical": True}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=["f32", "u8", "i8"])
    ap.add_argument("--values", choices=["u8", "i8"], default="u8", help="with --rows f32: the byte type whose values the f32 index holds")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--vectors", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4_000_000)
    ap.add_argument("--dump", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib
    from rabitq_amd import index as ix
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    n, d, k = args.vectors, args.dim, args.lists
    dim = (d + 63) // 64 * 64
    values = args.values if args.rows == "f32" else args.rows
    lo, hi, off = (0.0, 255.0, 128.0) if values == "u8" else (-128.0, 127.0, 0.0)
    raw_centres = synth.device_centres(k, d, dev)
    centres = (raw_centres * 32.0 + off).contiguous()                                   # the mixture's centres in byte units (f32)
    queries = (synth.device_queries(raw_centres, 65536, args.sigma, dev) * 32.0 + off).contiguous()
    P = synth.random_orthogonal(dim, seed=99)

    def chunk_rows(ci, i0, m):   # the chunk as this side's builder takes it
        x, _ = synth.device_mixture_chunk(raw_centres, i0, m, args.sigma, ci)
        v = torch.clamp(torch.round(x * 32.0 + off), lo, hi)
        if args.rows == "f32":
            return v.contiguous()
        return v.to(torch.uint8 if values == "u8" else torch.int8).contiguous()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def engine_build(rows_n):
        b = rq.RaBitQ.builder(rows_n, d, centres.data_ptr(), k, orthogonal=P, rows=args.rows)
        ms = 0.0
        for feed in (b.assign_chunk, b.place_chunk):
            for ci, i0 in enumerate(range(0, rows_n, args.chunk)):
                m = min(args.chunk, rows_n - i0)
                c = chunk_rows(ci, i0, m)
                ms += timed(lambda: feed(c.data_ptr(), i0, m))[1]
                del c
            if feed == b.assign_chunk:
                ms += timed(b.order)[1]
        idx, t = timed(b.finish)
        return idx, ms + t

    engine_build(min(n, 1 << 20))[0].close()   # warm-up: code objects, kernel attributes
    idx, build_ms = engine_build(n)
    assert idx.row_type == args.rows
    free_b, total_b = torch.cuda.mem_get_info()
    out = {"rows": args.rows, "values": values, "vectors": n, "dim": d, "lists": k, "nprobe": args.nprobe, "n_hbm": idx.n_hbm,
           "split_rows": idx.split_rows, "raw_vector_bytes": n * dim * (4 if args.rows == "f32" else 1), "hbm_used_bytes": total_b - free_b,
           "build_engine_ms": round(build_ms, 1), "calls": {}}
    od = torch.empty((65536, args.topk), device=dev)
    oi = torch.zeros((65536, args.topk), device=dev, dtype=torch.int32)
    on = torch.zeros(65536, device=dev, dtype=torch.int32)
    for nq in (64, 65536):
        call = lambda: idx.query_batch_device(queries.data_ptr(), nq, d, args.nprobe, args.topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        timed(call), timed(call)
        ms = sorted(timed(call)[1] for _ in range(args.steps))
        ix.set_profiling(1)
        timed(call)
        prof = ix.last_profile()
        ix.set_profiling(0)
        out["calls"][str(nq)] = {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                                 "ms_rerank": round(prof["ms_rerank"], 4), "rerank_candidates": prof["rerank_candidates"],
                                 "rerank_shadow_rejects": prof["rerank_shadow_rejects"]}
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        np.save(os.path.join(args.dump, "dist.npy"), od.cpu().numpy())
        np.save(os.path.join(args.dump, "ids.npy"), oi.cpu().numpy())
        np.save(os.path.join(args.dump, "n.npy"), on.cpu().numpy())
    idx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
