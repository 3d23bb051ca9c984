"""Attribute columns and predicate filters at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, the synthetic mixture
of tests/synth.py), in one session on one index.  Prints ONE JSON line (and appends it to --out):
  where      per case, rq_filter_create_where --steps times after a warm-up: the predicate kernel's device ms (rq_last_where_stats'
             ms_eval, HIP events) and its GB/s on the column bytes it reads, ms_finish, and the wall ms of the whole call.  Cases:
             one u32 column with EQ at 0.1 %, 10 % and 50 % selectivity, a three-column AND, one u64 BETWEEN
  memcpy     the yardstick of the kernel: hipMemcpyAsync, device to device, of the same number of bytes (it reads AND writes them)
  routes     the whole rq_filter_create_where against what a caller did before for the same admitted set: rq_filter_create from
             an id bitmap already on the device, and from a host id bitmap (its upload included; the host-side evaluation of the
             predicate and the packing of the bitmap, which that route also needs, are NOT counted)
  mutations  add --delta rows, remove them, mark --delta rows dead and compact, --samples times each, with 0, 1 and 4 columns on
             the index: wall ms and rq_last_mutate_stats' phases.  --mutations-only --columns 0 is the part that also runs on a
             checkout without this feature: `--tree PATH` imports the package from there (the parent commit's, same session)

  python scripts/attr_filter_bench.py [--vectors 100000000] [--out profiles/attr_filter_bench_100M.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--delta", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--columns", default="0,1,4", help="column counts of the mutation part")
    ap.add_argument("--mutations-only", action="store_true")
    ap.add_argument("--tree", default="", help="import rabitq_amd from this checkout instead of the script's own")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib, index as ix
    from tests import synth
    assert os.path.dirname(os.path.dirname(os.path.abspath(rq.__file__))) == root, rq.__file__
    L = _lib.lib()
    _lib.check(L.rq_init(0))
    dev = torch.device("cuda")
    n, d, k = args.vectors, args.dim, args.lists
    P = synth.random_orthogonal((d + 63) // 64 * 64, seed=99)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def spread(ts):
        return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}

    x, centres = synth.device_mixture(n, d, k, args.sigma, dev)
    g, build_ms = timed(lambda: rq.RaBitQ.build_device(x.data_ptr(), n, d, centres.data_ptr(), k, orthogonal=P))
    del x
    torch.cuda.empty_cache()
    out = {"label": args.label, "tree": root if args.tree else "", "version": L.rq_version().decode(), "vectors": n, "dim": d, "lists": k,
           "steps": args.steps, "build_ms": round(build_ms, 1)}
    ids_all = torch.arange(n, device=dev, dtype=torch.int32)

    def set_column(name, values):          # values: a device tensor of n elements, value of id j at j
        absent = C.c_uint64()
        torch.cuda.synchronize()
        _lib.check(L.rq_attr_set_device(g._h, name.encode(), C.c_void_p(ids_all.data_ptr()), C.c_void_p(values.data_ptr()), n, C.byref(absent)))
        assert absent.value == 0

    if not args.mutations_only:
        from rabitq_amd import col
        # sel: 0 for half of the ids, 1 for a tenth, 2 for a thousandth, 3 .. 1002 otherwise (a hash of the id picks the class)
        h = (ids_all.to(torch.int64) * 2654435761) % 1000003 % 1000
        sel = h + 3
        sel[h < 500] = 0
        sel[(h >= 500) & (h < 600)] = 1
        sel[h == 600] = 2
        sel = sel.to(torch.int32).contiguous()
        tenant = ((ids_all.to(torch.int64) * 40503) % 97).to(torch.int32).contiguous()
        score = ((ids_all.to(torch.int64) * 69069) % 10007).to(torch.float32).div_(10007.0).contiguous()
        ts = (ids_all.to(torch.int64) * 1000 + (1 << 40)).contiguous()
        for name, dtype, vals in (("sel", "u32", sel), ("tenant", "u32", tenant), ("score", "f32", score), ("ts", "u64", ts)):
            _, ms = timed(lambda: g.create_attr(name, dtype))
            _, ms_set = timed(lambda: set_column(name, vals))
            out.setdefault("columns", []).append({"name": name, "dtype": dtype, "create_ms": round(ms, 3), "set_all_ms": round(ms_set, 3)})
        lo, hi = (1 << 40) + 1000 * (n // 4), (1 << 40) + 1000 * (n // 2)
        cases = [("u32 EQ 0.1%", col("sel") == 2), ("u32 EQ 10%", col("sel") == 1), ("u32 EQ 50%", col("sel") == 0),
                 ("three-column AND", (col("sel") == 0) & (col("tenant") < 48) & (col("score") >= 0.25)),
                 ("u64 BETWEEN", col("ts").between(lo, hi))]
        out["where"] = []
        for label, expr in cases:
            g.where(expr).close()
            ev, fin, wall, st = [], [], [], None
            for _ in range(args.steps):
                f, ms = timed(lambda: g.where(expr))
                st = ix.last_where_stats()
                ev.append(st["ms_eval"]), fin.append(st["ms_finish"]), wall.append(ms)
                f.close()
            rec = {"case": label, "columns": st["columns"], "bytes_read": st["bytes_read"], "admitted": st["admitted"],
                   "selectivity": round(st["admitted"] / n, 5), "eval_ms": spread(ev), "finish_ms": spread(fin), "call_wall_ms": spread(wall)}
            rec["eval_gb_per_s"] = round(st["bytes_read"] / (rec["eval_ms"]["median_ms"] * 1e-3) / 1e9, 1)
            out["where"].append(rec)
            print(rec, file=sys.stderr, flush=True)
        # the yardstick: hipMemcpyAsync device to device of the same bytes, on the null stream, between two events
        hip_path = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0]
        hip = C.CDLL(hip_path)
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        out["memcpy"] = []
        for nbytes in sorted({r["bytes_read"] for r in out["where"]}):
            src = torch.empty(nbytes, device=dev, dtype=torch.uint8).fill_(1)
            dst = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            ms = []
            for it in range(args.steps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None) == 0      # 3 = hipMemcpyDeviceToDevice
                e1.record()
                torch.cuda.synchronize()
                if it:
                    ms.append(e0.elapsed_time(e1))
            rec = {"bytes": nbytes, **spread(ms)}
            rec["copied_gb_per_s"] = round(nbytes / (rec["median_ms"] * 1e-3) / 1e9, 1)
            out["memcpy"].append(rec)
            print(rec, file=sys.stderr, flush=True)
            del src, dst
        by_bytes = {r["bytes"]: r["median_ms"] for r in out["memcpy"]}
        for r in out["where"]:
            r["eval_over_memcpy"] = round(r["eval_ms"]["median_ms"] / by_bytes[r["bytes_read"]], 3)
        # the whole call against the id-bitmap routes, for the same admitted set
        out["routes"] = []
        words = (n + 31) // 32
        for label, expr in (cases[1], cases[3]):
            with g.where(expr) as f:
                d_bits = torch.zeros(words, device=dev, dtype=torch.int32)
                torch.cuda.synchronize()
                _lib.check(L.rq_filter_id_bits(f._h, C.c_void_p(d_bits.data_ptr()), n, 1))
                rows = f.rows
            h_bits = d_bits.cpu().numpy().view(np.uint32)
            t_where, t_dev, t_host = [], [], []
            for it in range(args.steps + 1):
                a, ms_a = timed(lambda: g.where(expr))
                b, ms_b = timed(lambda: g.make_filter_device(d_bits.data_ptr(), n))
                hnd = C.c_void_p()
                _, ms_c = timed(lambda: _lib.check(L.rq_filter_create(g._h, C.c_void_p(h_bits.ctypes.data), n, 0, C.byref(hnd))))
                c = rq.Filter(g, hnd)
                assert a.rows == b.rows == c.rows == rows
                for flt in (a, b, c):
                    flt.close()
                if it:
                    t_where.append(ms_a), t_dev.append(ms_b), t_host.append(ms_c)
            rec = {"case": label, "admitted": rows, "where_ms": spread(t_where), "from_device_bitmap_ms": spread(t_dev),
                   "from_host_bitmap_ms": spread(t_host)}
            rec["device_bitmap_over_where"] = round(rec["from_device_bitmap_ms"]["median_ms"] / rec["where_ms"]["median_ms"], 2)
            rec["host_bitmap_over_where"] = round(rec["from_host_bitmap_ms"]["median_ms"] / rec["where_ms"]["median_ms"], 2)
            out["routes"].append(rec)
            print(rec, file=sys.stderr, flush=True)
            del d_bits
        for name in ("sel", "tenant", "score", "ts"):
            g.drop_attr(name)
        torch.cuda.empty_cache()

    # mutations with 0, 1 and 4 columns
    out["mutations"] = []
    centres_raw = synth.device_centres(k, d, dev)
    made = 0
    rng = np.random.default_rng(17)
    for ncols in [int(v) for v in args.columns.split(",") if v != ""]:
        want = [("c0", "u32"), ("c1", "u32"), ("c2", "u64"), ("c3", "u64")][:ncols]
        while made < len(want):
            g.create_attr(*want[made])
            made += 1
        steps = []

        def record(step, fn):
            _, wall = timed(fn)
            st = ix.last_mutate_stats()
            rec = {"step": step, "wall_ms": round(wall, 2), **{kk: (round(v, 3) if isinstance(v, float) else v) for kk, v in st.items()}}
            steps.append(rec)
            print(ncols, rec, file=sys.stderr, flush=True)

        for s in range(args.samples):
            rows, _ = synth.device_mixture_chunk(centres_raw, 0, args.delta, args.sigma, 1000 + s)
            rows = rows.contiguous()
            first = []
            record("add", lambda: first.append(g.add_device(rows.data_ptr(), args.delta, d)))
            new_ids = np.arange(first[0], first[0] + args.delta, dtype=np.uint32)
            record("remove", lambda: g.remove(ids=new_ids))
            del rows
        for s in range(args.samples):
            dead = np.unique(rng.integers(0, g.n, size=args.delta))            # positions (a few less than --delta: repeats drop out)
            live_ids = g.map_ids[dead]                     # (ids of stored rows: the index has lost ids by now)
            _, ms_mark = timed(lambda: g.remove(ids=live_ids, lazy=True))
            record("compact", lambda: g.compact())
            steps[-1]["mark_wall_ms"] = round(ms_mark, 2)
        out["mutations"].append({"columns": ncols, "column_bytes_per_row": sum(4 if t == "u32" else 8 for _, t in want), "rows": g.n, "steps": steps})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
