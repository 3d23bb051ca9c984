"""In-place mutation at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, the synthetic mixture of tests/synth.py).
Prints ONE JSON line (and writes it to --out):
  rebuild_engine_ms  rq_build of 101M rows through the streamed builder, the calls timed as bench.py times its build ("engine
                     time": assign + order + place + finish, input generation excluded; after a warm-up build)
  steps              per call, wall ms and rq_last_mutate_stats' phases (keys / assign / alloc / merge / gather / derive / free),
                     the gather's GB/s on the bytes it must move, and the call over the rebuild's engine time:
                     --samples adds of 1M rows (the first derives the key cache), --samples removes of 1M random ids, and one
                     remove of a whole list (the longest)
  equal              the mutated index's arrays == canonical(S) (the build of its live rows in id order, map_ids translated), bit
                     for bit: offsets / map_ids / codes / factors on the host, the raw vectors chunk by chunk on the device; and the
                     65 536 query results
  query_ms           median ms per call, 65 536 queries, nprobe 64, top 10 (device entry), on the mutated and on the rebuilt index

  python scripts/mutate_bench.py [--vectors 100000000] [--samples 3] [--steps 5] [--out profiles/mutate_bench_100M.json]
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
    ap.add_argument("--delta", type=int, default=1_000_000, help="rows per add / random remove")
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=3)
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
    n, d, k, dm, S = args.vectors, args.dim, args.lists, args.delta, args.samples
    x, cd = synth.device_mixture(n + S * dm, d, k, args.sigma, dev)
    P = synth.random_orthogonal(d, seed=99)
    out = {"vectors": n, "dim": d, "lists": k, "delta": dm, "samples": S}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def engine_build(rows):
        """the streamed builder's calls, timed as bench.py times its build"""
        b = rq.RaBitQ.builder(rows, d, cd.data_ptr(), k, orthogonal=P)
        ms = 0.0
        for call in (lambda: b.assign_chunk(x.data_ptr(), 0, rows), b.order, lambda: b.place_chunk(x.data_ptr(), 0, rows)):
            ms += timed(call)[1]
        idx, t = timed(b.finish)
        return idx, ms + t

    engine_build(1 << 20)[0].close()   # warm-up: code objects, kernel attributes
    c0, out["rebuild_engine_ms"] = engine_build(n + dm)
    c0.close()
    base_ms = out["rebuild_engine_ms"]
    g = rq.RaBitQ.build_device(x.data_ptr(), n, d, cd.data_ptr(), k, orthogonal=P)
    steps = []

    def record(kind, ms):
        st = ix.last_mutate_stats()
        st = {kk: (round(v, 2) if isinstance(v, float) else v) for kk, v in st.items()}
        st.update({"step": kind, "wall_ms": round(ms, 2), "x_rebuild_engine": round(ms / base_ms, 3),
                   "gather_GBps": round(st["gather_bytes"] / (st["ms_gather"] * 1e-3) / 1e9, 1) if st["ms_gather"] else None})
        steps.append(st)

    for s_ in range(S):
        _, t = timed(lambda: g.add_device(x[n + s_ * dm:].data_ptr(), dm, d))
        record("add 1M" + (" (keys derived)" if s_ == 0 else ""), t)
    rng = np.random.default_rng(5)
    alive = np.ones(n + S * dm, dtype=bool)
    for s_ in range(S):
        gone = rng.choice(np.nonzero(alive)[0], dm, replace=False)
        removed, t = timed(lambda: g.remove(ids=gone))
        assert removed == dm
        alive[gone] = False
        record("remove 1M random", t)
    offs = g.offsets.astype(np.int64)
    big = int(np.argmax(np.diff(offs)))
    lst = g.map_ids[offs[big]:offs[big + 1]].copy()
    removed, t = timed(lambda: g.remove(ids=lst))
    alive[lst] = False
    record(f"remove one list ({removed} rows)", t)
    out["steps"] = steps

    q = synth.device_queries(cd, args.batch, args.sigma, dev)
    od = torch.empty((args.batch, 10), device=dev, dtype=torch.float32)
    oi = torch.empty((args.batch, 10), device=dev, dtype=torch.int32)
    on = torch.empty((args.batch,), device=dev, dtype=torch.int32)

    def qms(idx):
        ts = []
        for s in range(args.steps + 1):
            _, t = timed(lambda: idx.query_batch_device(q.data_ptr(), args.batch, d, args.nprobe, 10, od.data_ptr(), oi.data_ptr(),
                                                        on.data_ptr()))
            if s:
                ts.append(t)
        return float(np.median(ts)), (od.clone(), oi.clone(), on.clone())

    out["query_ms_mutated"], res_g = qms(g)
    keep = np.nonzero(alive)[0]
    xs = x[torch.from_numpy(keep).to(dev)].contiguous()
    del x
    torch.cuda.empty_cache()
    c = rq.RaBitQ.build_device(xs.data_ptr(), xs.shape[0], d, cd.data_ptr(), k, orthogonal=P)
    del xs
    torch.cuda.empty_cache()
    out["query_ms_rebuilt"], res_c = qms(c)
    ids = keep.astype(np.uint32)
    eq = {"n": g.n == c.n and g.max_list_len == c.max_list_len}
    for name in ("offsets", "codes", "factors", "centroids", "orthogonal"):
        eq[name] = bool(np.array_equal(getattr(g, name).view(np.uint8), getattr(c, name).view(np.uint8)))
    eq["map_ids"] = bool(np.array_equal(g.map_ids, ids[c.map_ids]))
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
    n_ok = torch.equal(res_g[2], res_c[2])
    idm = torch.from_numpy(ids.view(np.int32)).to(dev)
    mask = torch.arange(10, device=dev)[None, :] < res_g[2][:, None]
    eq["queries"] = bool(n_ok and torch.equal(res_g[0][mask].view(torch.int32), res_c[0][mask].view(torch.int32))
                         and torch.equal(res_g[1][mask], idm[res_c[1][mask].long()]))
    out["equal"] = eq
    out["n_final"] = int(g.n)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
