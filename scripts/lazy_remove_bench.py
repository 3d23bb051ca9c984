"""Lazy removal at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, the synthetic mixture of tests/synth.py), in one
session on one index.  Prints ONE JSON line (and writes it to --out):
  removal   per call: the entry (rq_remove_lazy / rq_remove / rq_compact), what it took, whether it was the first lazy call since
            a relayout (it makes the live filter) or a later one (it updates it), rows affected, wall ms of the C call alone (the id
            bitmap is packed and uploaded before the clock starts) and, for the relayouts, rq_last_mutate_stats' phases
  query     per state of the index (untouched; 1 permille, 1 %, 10 % of its rows pending; after each compact): ms per call of a
            --batch-query call and of a 64-query call (device entry, nprobe 64, top 10): median, min, max over --steps calls after
            one warm-up call, and the profile's filtered / small-batch pass counts of the last call
  equal     after each compact: the 65 536-query answer equals the answer the pending index gave just before it, bit for bit

  python scripts/lazy_remove_bench.py [--vectors 100000000] [--samples 3] [--steps 5] [--out profiles/lazy_remove_bench_100M.json]
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
    ap.add_argument("--delta", type=int, default=1_000_000, help="rows per random removal")
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
    L = _lib.lib()
    _lib.check(L.rq_init(0))
    dev = torch.device("cuda")
    n, d, k, dm, S = args.vectors, args.dim, args.lists, args.delta, args.samples
    x, cd = synth.device_mixture(n, d, k, args.sigma, dev)
    P = synth.random_orthogonal(d, seed=99)
    g = rq.RaBitQ.build_device(x.data_ptr(), n, d, cd.data_ptr(), k, orthogonal=P)
    del x
    torch.cuda.empty_cache()
    out = {"vectors": n, "dim": d, "lists": k, "delta": dm, "samples": S, "steps": args.steps, "batch": args.batch, "nprobe": args.nprobe}
    rng = np.random.default_rng(5)
    alive = np.ones(n, dtype=bool)
    removal, query, equal = [], [], {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def remove(ids, lazy, what):
        """one C call on a device-resident bitmap; the packing and the upload are not timed"""
        words, nbits = rq.pack_filter_bits(ids=ids, nbits=n)
        dw = torch.from_numpy(words.view(np.int32)).to(dev)
        cnt = C.c_uint64()
        first = g.pending_removals == 0
        entry = L.rq_remove_lazy if lazy else L.rq_remove
        st, ms = timed(lambda: entry(g._h, C.c_void_p(dw.data_ptr()), nbits, 1, C.byref(cnt)))
        _lib.check(st)
        g._refresh()
        alive[ids] = False
        rec = {"entry": "rq_remove_lazy" if lazy else "rq_remove", "what": what, "rows": int(cnt.value), "wall_ms": round(ms, 3),
               "pending_after": g.pending_removals}
        if lazy:
            rec["call"] = "first" if first else "later"
        else:
            rec.update({kk: (round(v, 2) if isinstance(v, float) else v) for kk, v in ix.last_mutate_stats().items()})
        removal.append(rec)
        print(rec, file=sys.stderr, flush=True)   # progress

    def pick(m):
        return rng.choice(np.nonzero(alive)[0], m, replace=False)

    def compact(what):
        cnt = C.c_uint64()
        st, ms = timed(lambda: L.rq_compact(g._h, C.byref(cnt)))
        _lib.check(st)
        g._refresh()
        rec = {"entry": "rq_compact", "what": what, "rows": int(cnt.value), "wall_ms": round(ms, 3), "pending_after": g.pending_removals}
        rec.update({kk: (round(v, 2) if isinstance(v, float) else v) for kk, v in ix.last_mutate_stats().items()})
        removal.append(rec)
        print(rec, file=sys.stderr, flush=True)   # progress

    q = synth.device_queries(cd, args.batch, args.sigma, dev)
    od = torch.empty((args.batch, 10), device=dev, dtype=torch.float32)
    oi = torch.empty((args.batch, 10), device=dev, dtype=torch.int32)
    on = torch.empty((args.batch,), device=dev, dtype=torch.int32)

    def qms(state):
        rec = {"state": state, "stored_rows": g.n, "pending": g.pending_removals}
        for nq in (args.batch, 64):
            ts = []
            for s in range(args.steps + 1):
                _, t = timed(lambda: g.query_batch_device(q.data_ptr(), nq, d, args.nprobe, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr()))
                if s:
                    ts.append(t)
            pr = ix.last_profile()
            rec[f"nq{nq}"] = {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                              "small_batch_passes": pr["small_batch_passes"], "scan_launches": pr["scan_launches"],
                              "matrix_launches": pr["matrix_launches"]}
        query.append(rec)
        print(rec, file=sys.stderr, flush=True)
        g.query_batch_device(q.data_ptr(), args.batch, d, args.nprobe, 10, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        torch.cuda.synchronize()
        return od.clone(), oi.clone(), on.clone()

    def same(a, b):
        mask = torch.arange(10, device=dev)[None, :] < a[2][:, None]
        return bool(torch.equal(a[2], b[2]) and torch.equal(a[0][mask].view(torch.int32), b[0][mask].view(torch.int32))
                    and torch.equal(a[1][mask], b[1][mask]))

    qms("untouched")
    remove(pick(1), True, "1 id")
    for _ in range(S):
        remove(pick(1), True, "1 id")
    remove(pick(n // 1000 - g.pending_removals), True, "random ids up to 1 permille pending")
    qms("1 permille pending")
    remove(pick(n // 100 - g.pending_removals), True, "random ids up to 1 % pending")
    before = qms("1 % pending")
    compact("after 1 % (1M rows) pending")
    equal["compact_1pct"] = same(before, qms("compacted after 1 % pending"))
    for s_ in range(S):
        remove(pick(dm), True, "1M random ids")
    offs = g.offsets.astype(np.int64)
    mids = g.map_ids
    big = int(np.argmax(np.bincount(np.repeat(np.arange(k), np.diff(offs))[alive[mids]], minlength=k)))   # the list with most live rows
    lst = mids[offs[big]:offs[big + 1]]
    lst = lst[alive[lst]].copy()
    remove(lst, True, f"one whole list ({lst.size} live rows)")
    remove(pick(g.n // 10 - g.pending_removals), True, "random ids up to 10 % pending")
    before = qms("10 % pending")
    compact("after 10 % pending")
    equal["compact_10pct"] = same(before, qms("compacted after 10 % pending"))
    # the comparison point, in the same session: the eager remove of the same kinds of sets
    remove(pick(1), False, "1 id")
    for s_ in range(S):
        remove(pick(dm), False, "1M random ids")
    offs = g.offsets.astype(np.int64)
    big = int(np.argmax(np.diff(offs)))
    remove(g.map_ids[offs[big]:offs[big + 1]].copy(), False, "one whole list")
    # a first lazy call of 1M ids and of a whole list (no live filter yet: it is made)
    remove(pick(dm), True, "1M random ids")
    compact("after 1M pending")
    offs = g.offsets.astype(np.int64)
    big = int(np.argmax(np.diff(offs)))
    remove(g.map_ids[offs[big]:offs[big + 1]].copy(), True, "one whole list")
    out.update({"removal": removal, "query": query, "equal": equal, "n_final": int(g.n), "pending_final": g.pending_removals})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
