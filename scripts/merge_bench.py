"""rq_merge_from at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, the synthetic mixture of tests/synth.py), as
99M + 1M and as 50M + 50M.  Prints ONE JSON line (and writes it to --out).  Per split:
  add     (only where the second part has at most --add-limit rows) rq_add of the second part's raw rows to a build of the first:
          pass 1 of them, then the same merge and gather.  Wall ms, rq_last_mutate_stats' phases, the gather's GB/s
  rebuild_engine_ms  rq_build of all rows through the streamed builder, the calls timed as bench.py times its build (after a
          warm-up build); the index it leaves is the one the merged index is compared with
  merge   rq_merge_from(first, second, APPEND): wall ms, the phases, merge_gather_kernel's GB/s on the bytes it must move, the
          call over the rebuild's engine time and over the add
  equal   the merged index's arrays == the rebuilt index's, bit for bit (offsets / map_ids / codes / factors on the host, the raw
          vectors chunk by chunk on the device), and the 65 536 query results
Both routes derive the key cache of a fresh index on their first call (ms_keys); wall_ms_less_keys leaves that phase out.

  python scripts/merge_bench.py [--vectors 100000000] [--out profiles/merge_bench_100M.json]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--seconds", type=int, nargs="+", default=[1_000_000, 50_000_000], help="rows of the second part, per split")
    ap.add_argument("--add-limit", type=int, default=1_000_000, help="largest second part that is also added as raw rows")
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib, index as ix
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    hip = C.CDLL("libamdhip64.so")
    dev = torch.device("cuda")
    n, d, k = args.vectors, args.dim, args.lists
    P = synth.random_orthogonal(d, seed=99)
    out = {"vectors": n, "dim": d, "lists": k, "splits": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def engine_build(x, cd, rows):
        """the streamed builder's calls, timed as bench.py times its build"""
        b = rq.RaBitQ.builder(rows, d, cd.data_ptr(), k, orthogonal=P)
        ms = 0.0
        for call in (lambda: b.assign_chunk(x.data_ptr(), 0, rows), b.order, lambda: b.place_chunk(x.data_ptr(), 0, rows)):
            ms += timed(call)[1]
        idx, t = timed(b.finish)
        return idx, ms + t

    def phases(ms):
        st = ix.last_mutate_stats()
        st = {kk: (round(v, 2) if isinstance(v, float) else v) for kk, v in st.items()}
        st.update({"wall_ms": round(ms, 2), "wall_ms_less_keys": round(ms - st["ms_keys"], 2),
                   "gather_GBps": round(st["gather_bytes"] / (st["ms_gather"] * 1e-3) / 1e9, 1) if st["ms_gather"] else None})
        return st

    def same_index(g, c, q):
        eq = {"n": g.n == c.n and g.max_list_len == c.max_list_len}
        for name in ("offsets", "map_ids", "codes", "factors", "centroids", "orthogonal"):
            eq[name] = bool(np.array_equal(getattr(g, name).view(np.uint8), getattr(c, name).view(np.uint8)))
        pg, nb = g.device_ptr(ix.ARR_BASE)
        pc, nb2 = c.device_ptr(ix.ARR_BASE)
        same = nb == nb2
        chunk = 1 << 30
        a = torch.empty(chunk // 4, device=dev, dtype=torch.int32)
        b = torch.empty(chunk // 4, device=dev, dtype=torch.int32)
        for o in range(0, nb if same else 0, chunk):
            m = min(chunk, nb - o)
            assert hip.hipMemcpy(C.c_void_p(a.data_ptr()), C.c_void_p(pg + o), C.c_size_t(m), 3) == 0
            assert hip.hipMemcpy(C.c_void_p(b.data_ptr()), C.c_void_p(pc + o), C.c_size_t(m), 3) == 0
            same = same and bool(torch.equal(a[:m // 4], b[:m // 4]))
        eq["base"] = bool(same)
        res = []
        for idx in (g, c):
            od = torch.empty((args.batch, 10), device=dev, dtype=torch.float32)
            oi = torch.empty((args.batch, 10), device=dev, dtype=torch.int32)
            on = torch.empty((args.batch,), device=dev, dtype=torch.int32)
            idx.query_batch_device(q.data_ptr(), args.batch, d, args.nprobe, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr())
            torch.cuda.synchronize()
            res.append((od, oi, on))
        mask = torch.arange(10, device=dev)[None, :] < res[0][2][:, None]
        eq["queries"] = bool(torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][0][mask].view(torch.int32), res[1][0][mask].view(torch.int32))
                             and torch.equal(res[0][1][mask], res[1][1][mask]))
        return eq

    warm = True
    for second in args.seconds:
        first = n - second
        x, cd = synth.device_mixture(n, d, k, args.sigma, dev)
        if warm:   # code objects, kernel attributes: one small build, add and merge
            w, _ = engine_build(x, cd, 1 << 20)
            w2 = rq.RaBitQ.build_device(x[1 << 20:].data_ptr(), 1 << 18, d, cd.data_ptr(), k, orthogonal=P)
            w.merge_from(w2)
            w.add_device(x.data_ptr(), 1 << 18, d)
            w.close()
            w2.close()
            warm = False
        row = {"first": first, "second": second}
        if second <= args.add_limit:
            a = rq.RaBitQ.build_device(x.data_ptr(), first, d, cd.data_ptr(), k, orthogonal=P)
            _, t = timed(lambda: a.add_device(x[first:].data_ptr(), second, d))
            row["add"] = phases(t)
            assert a.n == n
            a.close()
        whole, row["rebuild_engine_ms"] = engine_build(x, cd, n)
        row["rebuild_engine_ms"] = round(row["rebuild_engine_ms"], 2)
        a = rq.RaBitQ.build_device(x.data_ptr(), first, d, cd.data_ptr(), k, orthogonal=P)
        b = rq.RaBitQ.build_device(x[first:].data_ptr(), second, d, cd.data_ptr(), k, orthogonal=P)
        q = synth.device_queries(cd, args.batch, args.sigma, dev)
        del x
        torch.cuda.empty_cache()
        shift, t = timed(lambda: a.merge_from(b, "append"))
        assert shift == first and a.n == n
        row["merge"] = phases(t)
        row["merge"]["x_rebuild_engine"] = round(t / row["rebuild_engine_ms"], 3)
        if "add" in row:
            row["merge"]["x_add"] = round(t / row["add"]["wall_ms"], 3)
            row["merge"]["x_add_less_keys"] = round(row["merge"]["wall_ms_less_keys"] / row["add"]["wall_ms_less_keys"], 3)
            row["merge"]["gather_x_add_gather"] = round(row["merge"]["gather_GBps"] / row["add"]["gather_GBps"], 3)
        b.close()
        row["equal"] = same_index(a, whole, q)
        a.close()
        whole.close()
        del q, cd
        torch.cuda.empty_cache()
        out["splits"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
