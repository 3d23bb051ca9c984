"""The exact search (RaBitQ.exact_search_device) on the bench's synthetic index (tests/synth.py mixture, 4096 lists), beside the torch
brute force bench.py --full uses for its ground truth (f64, |q|^2 - 2 q.x + |x|^2, chunk by chunk), on the same queries and box.
One process builds ONE index and prints ONE JSON line:

  python scripts/exact_bench.py --vectors 1000000   --out profiles/exact_search_bench_1M.json
  python scripts/exact_bench.py --vectors 100000000 --out profiles/exact_search_bench_100M.json
  python scripts/exact_bench.py --vectors 100000000 --rows u8 --out profiles/exact_search_bench_100M_u8.json

Per batch size (--batches, default 16 1000 65536): the median / min / max wall time of a call over --steps calls after two warm-up
calls (a call that takes seconds: two warm-ups, one timed call), the stats of the last one (rq_last_exact_stats), and from them
  scan_GBps / hbm_frac     row_bytes_read / ms_scan, as a fraction of the 8 TB/s HBM peak -- what matters for a small batch;
  scan_TFLOPs / bf16_frac  pairs x 2 dim flop / ms_scan, as a fraction of the 2.5 PFLOP/s dense bf16 matrix peak -- a large batch;
  candidates / exact per query, the seed's share of the call.
It asserts that the (warmed) call read every row once per group of 4096 queries: reruns == 0 and row_bytes_read == n x row bytes x
ceil(nq / 4096).  The yardstick (batches up to --torch-max-queries; the base is regenerated chunk by chunk, only the f64
product and the top-k merge are timed) also gives the ids: on every query whose f64 gap at the cut is above 1e-4 relative the two
id sets must be equal.  Nothing is tuned for the comparison: where the exact search is slower, the line says so.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X HBM3E
BF16_PEAK_TFLOPS = 2500.0     # dense bf16 matrix peak
QGROUP = 4096                 # queries per scan launch (include/rabitq_hip.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--rows", choices=["f32", "u8"], default="f32")
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 1000, 65536])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4_000_000)
    ap.add_argument("--torch-max-queries", type=int, default=1000, help="largest batch the torch yardstick runs at (0: none)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    n, d, k, topk = args.vectors, args.dim, args.lists, args.topk
    dim = (d + 63) // 64 * 64
    byte = args.rows == "u8"
    raw_centres = synth.device_centres(k, d, dev)
    scale, off = (32.0, 128.0) if byte else (1.0, 0.0)
    centres = (raw_centres * scale + off).contiguous()
    nq_max = max(args.batches)
    queries = (synth.device_queries(raw_centres, nq_max, args.sigma, dev) * scale + off).contiguous()
    P = synth.random_orthogonal(dim, seed=99)

    def chunk_rows(ci, i0, m):
        x, _ = synth.device_mixture_chunk(raw_centres, i0, m, args.sigma, ci)
        if not byte:
            return x.contiguous()
        return torch.clamp(torch.round(x * scale + off), 0.0, 255.0).to(torch.uint8).contiguous()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    b = rq.RaBitQ.builder(n, d, centres.data_ptr(), k, orthogonal=P, rows=args.rows)
    for feed in (b.assign_chunk, b.place_chunk):
        for ci, i0 in enumerate(range(0, n, args.chunk)):
            m = min(args.chunk, n - i0)
            c = chunk_rows(ci, i0, m)
            feed(c.data_ptr(), i0, m)
            del c
        if feed == b.assign_chunk:
            b.order()
    idx = b.finish()
    row_bytes = dim * (1 if byte else 4)
    out = {"rows": args.rows, "vectors": n, "dim": d, "lists": k, "topk": topk, "n_hbm": idx.n_hbm, "row_bytes": row_bytes, "calls": {}}
    od = torch.empty((nq_max, topk), device=dev)
    oi = torch.zeros((nq_max, topk), device=dev, dtype=torch.int32)
    on = torch.zeros(nq_max, device=dev, dtype=torch.int32)

    def torch_truth(nq):
        """bench.py's ground truth (f64), topk + 1 deep; -> (ids, distances, ms of the products and merges alone)"""
        best_d = torch.full((nq, topk + 1), float("inf"), device=dev, dtype=torch.float64)
        best_i = torch.full((nq, topk + 1), -1, device=dev, dtype=torch.int64)
        ms = 0.0
        gchunk = max(65_536, min(1_000_000, (128 << 20) // d))
        for q0 in range(0, nq, 4096):
            q1 = min(q0 + 4096, nq)
            qg = queries[q0:q1].double()
            qn = (qg * qg).sum(1, keepdim=True)
            bd, bi = best_d[q0:q1], best_i[q0:q1]
            for ci, i0 in enumerate(range(0, n, args.chunk)):
                xc = chunk_rows(ci, i0, min(args.chunk, n - i0))

                def fold():
                    nonlocal bd, bi
                    for j0 in range(0, xc.shape[0], gchunk):
                        xb = xc[j0:j0 + gchunk].double()
                        d2 = qn - 2.0 * (qg @ xb.T) + (xb * xb).sum(1)[None, :]
                        cd, ci_ = torch.topk(d2, min(topk + 1, xb.shape[0]), dim=1, largest=False)
                        alld, alli = torch.cat([bd, cd], 1), torch.cat([bi, ci_ + i0 + j0], 1)
                        sel = torch.topk(alld, topk + 1, dim=1, largest=False).indices
                        bd, bi = torch.gather(alld, 1, sel), torch.gather(alli, 1, sel)
                ms += timed(fold)[1]
                del xc
            best_d[q0:q1], best_i[q0:q1] = bd, bi
        return best_i.cpu().numpy(), best_d.cpu().numpy(), ms

    failed = []
    for nq in args.batches:
        call = lambda: idx.exact_search_device(queries.data_ptr(), nq, d, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        first = timed(call)[1]                                         # warm-up (a call of seconds is timed once more, not --steps times)
        timed(call)                                                    # (the first call may have learnt its candidate capacity)
        ms = sorted(timed(call)[1] for _ in range(args.steps if first < 3000.0 else 1))
        st = rq.last_exact_stats()
        groups = (nq + QGROUP - 1) // QGROUP
        # the warmed call reads every row once per group of 4096 queries: no repeated launch, no launch cut short by the slot budget
        once = st["reruns"] == 0 and st["scan_launches"] == groups and st["row_bytes_read"] == n * row_bytes * groups
        if not once:
            failed.append((nq, st))                                    # (reported in the line, asserted once the line is written)
        pairs = nq * n
        rec = {"ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
               **{key: (round(v, 3) if isinstance(v, float) else v) for key, v in st.items()},
               "scan_GBps": round(st["row_bytes_read"] / st["ms_scan"] / 1e6, 1),
               "hbm_frac": round(st["row_bytes_read"] / st["ms_scan"] / 1e6 / HBM_PEAK_GBPS, 4),
               "scan_TFLOPs": round(pairs * 2 * dim / st["ms_scan"] / 1e9, 2),
               "bf16_frac": round(pairs * 2 * dim / st["ms_scan"] / 1e9 / BF16_PEAK_TFLOPS, 4),
               "reads_each_row_once": once, "candidates_per_query": round(st["candidates"] / nq, 1), "exact_per_query": round(st["exact"] / nq, 1),
               "seed_share": round(st["ms_seed"] / max(ms[len(ms) // 2], 1e-9), 3)}
        if args.torch_max_queries and nq <= args.torch_max_queries:
            ti, td, tms = torch_truth(nq)
            got = oi[:nq].cpu().numpy()
            firm = (td[:, topk] - td[:, topk - 1]) > 1e-4 * td[:, topk]
            same = [set(got[b_].tolist()) == set(ti[b_, :topk].tolist()) for b_ in range(nq) if firm[b_]]
            rec.update(torch_f64_ms=round(tms, 3), torch_over_exact=round(tms / ms[len(ms) // 2], 3), firm_queries=int(firm.sum()),
                       id_sets_equal=int(sum(same)), slower_than_torch=bool(ms[len(ms) // 2] > tms))
            assert all(same), f"{len(same) - sum(same)} of {len(same)} firm queries disagree with the f64 brute force"
        out["calls"][str(nq)] = rec
    idx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    assert not failed, f"row_bytes_read != n x row bytes x ceil(nq / 4096), or a launch was repeated: {failed}"


if __name__ == "__main__":
    main()
