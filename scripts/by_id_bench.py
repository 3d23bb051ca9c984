"""Rows by id at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, the synthetic mixture of tests/synth.py), in one
session on one index.  Prints ONE JSON line (and appends it to --out):
  directory   per form: what rq_last_by_id_stats reports of the call that made it (form, bytes, build ms, longest chain).  The
              hash form is reached by adding one row with id 2^32 - 1 at the end of the session (f32 rows only: a typed index is
              not mutated, so --rows u8 reports the dense form alone)
  locate      rq_locate_device at --locate-ids random ids: ms per call (median, min, max over --steps calls after a warm-up) and
              ids per second, per form
  fetch       rq_fetch_rows_device at each of --fetch-ids random ids: the stats' gather_bytes (every found row read once, every
              destination row written once, the positions) over its ms_gather (device events) = GB/s; wall ms of the whole call
              beside it (lookup included)
  extract     the yardstick, f32 rows only: rq_extract of the same ids on the same index, rq_last_mutate_stats' gather_bytes over
              ms_gather = GB/s of the project's existing gather, and ratio = fetch GB/s over it
  neighbours  rq_neighbours_of_device at --batch ids against rq_fetch_rows_device once + rq_query_batch_device at topk + 1 on the
              fetched rows by hand (the query alone is timed): the difference is the feature's overhead (lookup, gather, drop)

  python scripts/by_id_bench.py [--rows f32|u8] [--vectors 100000000] [--out profiles/by_id_bench_100M.json]
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
    ap.add_argument("--rows", choices=["f32", "u8"], default="f32")
    ap.add_argument("--vectors", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--locate-ids", type=int, default=1_000_000)
    ap.add_argument("--fetch-ids", default="1000000,16000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib, index as ix
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    n, d, k = args.vectors, args.dim, args.lists
    dim = (d + 63) // 64 * 64
    P = synth.random_orthogonal(dim, seed=99)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def spread(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}

    if args.rows == "f32":
        x, centres = synth.device_mixture(n, d, k, args.sigma, dev)
        g, build_ms = timed(lambda: rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=P))
        del x
    else:   # the mixture in byte units, built chunk by chunk from uint8 chunks (as scripts/byte_rows_bench.py builds it)
        raw = synth.device_centres(k, d, dev)
        centres = (raw * 32.0 + 128.0).contiguous()
        b = rq.RaBitQ.builder(n, d, centres.data_ptr(), k, orthogonal=P, rows="u8")
        build_ms = 0.0
        for feed in (b.assign_chunk, b.place_chunk):
            for ci, i0 in enumerate(range(0, n, args.chunk)):
                m = min(args.chunk, n - i0)
                c = torch.clamp(torch.round(synth.device_mixture_chunk(raw, i0, m, args.sigma, ci)[0] * 32.0 + 128.0), 0.0, 255.0).to(torch.uint8).contiguous()
                build_ms += timed(lambda: feed(c.data_ptr(), i0, m))[1]
                del c
            if feed == b.assign_chunk:
                build_ms += timed(b.order)[1]
        g, t = timed(b.finish)
        build_ms += t
    torch.cuda.empty_cache()
    assert g.row_type == args.rows and g.n == n
    out = {"rows": args.rows, "vectors": n, "dim": d, "lists": k, "nprobe": args.nprobe, "topk": args.topk, "steps": args.steps,
           "build_ms": round(build_ms, 1), "directory": [], "locate": [], "fetch": [], "extract": [], "neighbours": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    perm = torch.randperm(n, generator=gen, device=dev)     # random ids without repeats: a prefix of one permutation (ids are 0 .. n-1)

    def ids_of(m):
        return perm[:m].to(torch.int32).contiguous()

    def stats():
        return {kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in ix.last_by_id_stats().items()}

    def locate_run(form):
        m = args.locate_ids
        ids = ids_of(m)
        pos = torch.empty(m, device=dev, dtype=torch.int32)
        call = lambda: g.locate_device(ids.data_ptr(), m, pos.data_ptr())
        _, first = timed(call)                       # (the first by-id call of this layout: it makes the directory)
        st = stats()
        assert st["form"] == form and st["built"] == 1, st
        out["directory"].append({"form": st["form"], "bytes": st["directory_bytes"], "build_ms": st["ms_build"], "longest_chain": st["longest_chain"],
                                 "first_call_wall_ms": round(first, 3), "stored_rows": g.n})
        ts = [timed(call)[1] for _ in range(args.steps)]
        st = stats()
        assert st["built"] == 0 and st["found"] == m, st
        rec = {"form": form, "ids": m, **spread(ts), "lookup_device_ms": st["ms_lookup"]}
        rec["ids_per_s"] = round(m / (rec["median_ms"] * 1e-3))
        out["locate"].append(rec)
        print(rec, file=sys.stderr, flush=True)

    def fetch_run(form, m):
        ids = ids_of(m)
        rows = torch.empty((m, dim), device=dev, dtype=torch.float32)
        found = torch.empty(m, device=dev, dtype=torch.int32)
        call = lambda: g.fetch_device(ids.data_ptr(), m, rows.data_ptr(), found.data_ptr())
        timed(call)
        ts, gs, gb = [], [], 0
        for _ in range(args.steps):
            ts.append(timed(call)[1])
            st = stats()
            gs.append(st["ms_gather"])
            gb = st["gather_bytes"]
        assert int(found.sum().item()) == m
        rec = {"form": form, "ids": m, "gather_bytes": gb, "gather_ms": spread(gs), "call_wall_ms": spread(ts)}
        rec["gather_gb_per_s"] = round(gb / (rec["gather_ms"]["median_ms"] * 1e-3) / 1e9, 1)
        out["fetch"].append(rec)
        print(rec, file=sys.stderr, flush=True)
        return rec

    locate_run("dense")
    fetched = {m: fetch_run("dense", m) for m in (int(v) for v in args.fetch_ids.split(","))}

    # the yardstick: rq_extract of the same ids (its gather moves whole records: raw vector, codes, factors, id, key)
    if args.rows == "f32":
        for m, frec in fetched.items():
            ids = perm[:m].cpu().numpy().astype(np.uint32)
            sub, wall = timed(lambda: g.extract(ids=ids))
            ms = ix.last_mutate_stats()
            assert sub.n == m
            sub.close()
            rec = {"ids": m, "gather_bytes": ms["gather_bytes"], "gather_ms": round(ms["ms_gather"], 3), "call_wall_ms": round(wall, 1),
                   "gather_gb_per_s": round(ms["gather_bytes"] / (ms["ms_gather"] * 1e-3) / 1e9, 1)}
            rec["fetch_over_extract"] = round(frec["gather_gb_per_s"] / rec["gather_gb_per_s"], 3)
            out["extract"].append(rec)
            print(rec, file=sys.stderr, flush=True)
            torch.cuda.empty_cache()

    # neighbours_of against the same queries by hand
    m, w = args.batch, args.topk + 1
    ids = ids_of(m)
    rows = torch.empty((m, dim), device=dev, dtype=torch.float32)
    g.fetch_device(ids.data_ptr(), m, rows.data_ptr())
    od = torch.empty((m, w), device=dev, dtype=torch.float32)
    oi = torch.empty((m, w), device=dev, dtype=torch.int32)
    on = torch.empty(m, device=dev, dtype=torch.int32)
    plain = lambda: g.query_batch_device(rows.data_ptr(), m, dim, args.nprobe, w, od.data_ptr(), oi.data_ptr(), on.data_ptr())
    nd = torch.empty((m, args.topk), device=dev, dtype=torch.float32)
    ni = torch.empty((m, args.topk), device=dev, dtype=torch.int32)
    nf = torch.empty(m, device=dev, dtype=torch.int32)
    byid = lambda: g.neighbours_of_device(ids.data_ptr(), m, args.nprobe, args.topk, nd.data_ptr(), ni.data_ptr(), nf.data_ptr())
    for call in (plain, plain, byid, byid):   # warm-up: the first calls learn the survivor-buffer capacity
        timed(call)
    tp, tb = [], []
    for _ in range(args.steps):               # alternating, so that both see the same machine
        tp.append(timed(plain)[1])
        tb.append(timed(byid)[1])
    self_found = float((oi == ids[:, None]).any(1).float().mean().item())   # (the rest lost their last entry instead)
    out["neighbours"] = {"ids": m, "plain_at_topk_plus_1": spread(tp), "neighbours_of": spread(tb),
                         "overhead_ms": round(float(np.median(tb) - np.median(tp)), 3), "rows_in_their_own_plain_result": round(self_found, 4)}
    print(out["neighbours"], file=sys.stderr, flush=True)
    del rows, od, oi, on, nd, ni, nf
    torch.cuda.empty_cache()

    # the hash form: one row with id 2^32 - 1 puts the largest id far above 4 n + 65536
    if args.rows == "f32":
        one = torch.zeros((1, d), device=dev, dtype=torch.float32)
        top_id = torch.tensor([-1], device=dev, dtype=torch.int32)   # (the bits of 0xFFFFFFFF)
        g.add_device(one.data_ptr(), 1, d, ids_ptr=top_id.data_ptr())
        assert g.n == n + 1
        torch.cuda.synchronize()
        time.sleep(1.0)   # (the relayout has just freed the old layout's 65 GB: a 2 GB allocation right behind it waited 2.7 s for that memory once)
        locate_run("hash")
        fetch_run("hash", int(args.fetch_ids.split(",")[0]))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
