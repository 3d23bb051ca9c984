"""Filtered queries at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, nprobe 64, batches of 65 536, the
synthetic mixture of tests/synth.py as bench.py generates it).  Prints ONE JSON line:
  filter_ms          time to make a filter (rq_filter_create from a device bitmap: one pass over map_ids), per admitted fraction
  qps                queries/s of the unfiltered call and of filtered calls admitting 100 %, 50 %, 10 %, 1 % of the ids at random,
                     and 10 % as whole lists (every tenth list: correlated with the clustering); median call over --steps calls,
                     the timed calls rotate over four query batches
  profile            per leg, one profiled call (rq_set_profiling(1)): scan / rerank device time, candidates scanned and re-ranked
  legs beyond the filters: the unfiltered call on the bf16 threshold gate (the form filtered stages run), and "tenant" queries
                     drawn from the admitted lists' own centres, unfiltered and with the by-list filter
  sub_index_...      the by-list filter's sub-index built on its own: its unfiltered call timed, and whether its results (ids mapped
                     back) equal the filtered call's bit for bit
  small_calls        median ms per call of one query per call (host entry) and of 64 queries per call (device entry):
                     unfiltered, random 10 % and 1 %, 10 % by lists
  recall10_filtered  recall@10 of --gt-queries queries with the random 10 % filter against brute force over the admitted rows

  python scripts/filtered_bench.py [--vectors 100000000] [--steps 5]
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
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gt-queries", type=int, default=200)
    args = ap.parse_args()

    import numpy as np
    import torch
    import rabitq_amd
    from rabitq_amd import _lib
    from tests import synth

    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda", 0)
    n, d, k, B, topk = args.vectors, args.dim, args.lists, args.batch, args.topk
    assert n % 32 == 0
    t0 = time.time()
    centres = synth.device_centres(k, d, dev, 1.0)
    qsets = [synth.device_queries(centres, B, args.sigma, dev, seed=7 + 1000 * i) for i in range(4)]
    P = synth.random_orthogonal(d, seed=99)
    chunk = 4_000_000
    chunks = [(ci, i0, min(chunk, n - i0)) for ci, i0 in enumerate(range(0, n, chunk))]

    def gen(ci, i0, m):
        return synth.device_mixture_chunk(centres, i0, m, args.sigma, ci, 42, 0, k, None)[0]

    g = torch.Generator(device=dev)
    g.manual_seed(2024)
    rand = torch.rand(n, generator=g, device=dev)   # ids are generation order: row i has id i
    masks = {"100": torch.ones(n, dtype=torch.bool, device=dev), "50": rand < 0.5, "10": rand < 0.1, "1": rand < 0.01}
    del rand

    # pass 1 + brute-force ground truth of the random 10 % filter over its admitted rows (f64, as bench.py)
    ngt = min(args.gt_queries, B)
    qg = qsets[0][:ngt].double()
    qn = (qg * qg).sum(1, keepdim=True)
    best_d = torch.full((ngt, topk), float("inf"), device=dev, dtype=torch.float64)
    best_i = torch.full((ngt, topk), -1, device=dev, dtype=torch.int64)
    builder = rabitq_amd.RaBitQ.builder(n, d, centres.data_ptr(), k, orthogonal=P)
    for ci, i0, m in chunks:
        xc = gen(ci, i0, m)
        for j0 in range(0, m, 1_000_000):
            xb = xc[j0:j0 + 1_000_000].double()
            d2 = qn - 2.0 * (qg @ xb.T) + (xb * xb).sum(1)[None, :]
            d2[:, ~masks["10"][i0 + j0:i0 + j0 + xb.shape[0]]] = float("inf")
            cd, cidx = torch.topk(d2, min(topk, xb.shape[0]), dim=1, largest=False)
            alld, alli = torch.cat([best_d, cd], 1), torch.cat([best_i, cidx + i0 + j0], 1)
            sel = torch.topk(alld, topk, dim=1, largest=False).indices
            best_d, best_i = torch.gather(alld, 1, sel), torch.gather(alli, 1, sel)
            del d2, xb
        builder.assign_chunk(xc.data_ptr(), i0, m)
        del xc
    gt = best_i.cpu().numpy()
    del best_d, best_i, qg, qn
    torch.cuda.synchronize()
    builder.order()
    for ci, i0, m in chunks:
        xc = gen(ci, i0, m).contiguous()
        torch.cuda.synchronize()
        builder.place_chunk(xc.data_ptr(), i0, m)
        del xc
    idx = builder.finish()
    torch.cuda.empty_cache()
    build_s = time.time() - t0

    # whole lists: every tenth list admitted (ids of its members)
    offs = idx.offsets.astype(np.int64)
    mids = idx.map_ids
    lists_of_pos = np.repeat(np.arange(k), np.diff(offs))
    sel_ids = mids[(lists_of_pos % 10) == 0]
    m_lists = torch.zeros(n, dtype=torch.bool, device=dev)
    m_lists[torch.from_numpy(sel_ids.astype(np.int64)).to(dev)] = True
    masks["10_lists"] = m_lists
    del offs, mids, lists_of_pos, sel_ids

    shifts = torch.arange(32, device=dev, dtype=torch.int64)

    def device_words(mask):  # bit (id & 31) of u32 word id >> 5, as int32 words
        w = (mask.view(-1, 32).to(torch.int64) << shifts).sum(1)
        return (w - ((w >> 31) << 32)).to(torch.int32)

    filters, filter_ms, rows = {}, {}, {}
    for name, mask in masks.items():
        words = device_words(mask)
        torch.cuda.synchronize()
        tf = time.perf_counter()
        f = idx.make_filter_device(words.data_ptr(), n)
        filter_ms[name] = round((time.perf_counter() - tf) * 1e3, 2)
        rows[name] = f.rows
        assert f.rows == int(mask.sum().item()), name
        filters[name] = f
        del words

    od = torch.empty((B, topk), dtype=torch.float32, device=dev)
    oi = torch.empty((B, topk), dtype=torch.int32, device=dev)
    on = torch.empty(B, dtype=torch.int32, device=dev)

    def run(filt, q, index=None):
        (index or idx).query_batch_device(q.data_ptr(), B, d, args.nprobe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr(), filter=filt)

    # the sub-index of the by-list filter, built on its own from the admitted rows (same centroids and rotation, rows in id
    # order: every list holds its admitted rows in stored order, ids renumbered 0 .. m-1 in id order): what the filtered call
    # must equal, timed unfiltered
    sub_mask = masks["10_lists"]
    n_sub = int(sub_mask.sum().item())
    sub_ids = torch.nonzero(sub_mask).flatten()

    def sub_chunks():
        o = 0
        for ci, i0, m in chunks:
            xc = gen(ci, i0, m)[sub_mask[i0:i0 + m]].contiguous()
            torch.cuda.synchronize()
            if xc.shape[0]:
                yield o, xc
            o += xc.shape[0]

    sb = rabitq_amd.RaBitQ.builder(n_sub, d, centres.data_ptr(), k, orthogonal=P)
    for o, xc in sub_chunks():
        sb.assign_chunk(xc.data_ptr(), o, xc.shape[0])
    sb.order()
    for o, xc in sub_chunks():
        sb.place_chunk(xc.data_ptr(), o, xc.shape[0])
    sidx = sb.finish()
    torch.cuda.empty_cache()
    run(filters["10_lists"], qsets[0])
    torch.cuda.synchronize()
    fa = (od.clone(), oi.clone(), on.clone())
    run(None, qsets[0], sidx)
    torch.cuda.synchronize()
    sub_same = bool(torch.equal(fa[2], on))
    if sub_same:
        valid = torch.arange(topk, device=dev)[None, :] < on[:, None].long()
        gid = sub_ids[oi.long().clamp(min=0, max=n_sub - 1)]
        sub_same = bool(torch.equal(fa[0].view(torch.int32)[valid], od.view(torch.int32)[valid]) and
                        torch.equal(fa[1].long()[valid], gid[valid]))

    # "tenant" queries: drawn from the centres of the admitted lists only (every tenth list), for the by-list filter
    own = [synth.device_queries(centres[::10].contiguous(), B, args.sigma, dev, seed=77 + 1000 * i) for i in range(4)]

    from rabitq_amd import index as rqi
    qps, ms_call, prof = {}, {}, {}
    legs = [("unfiltered", None, qsets, 0), ("unfiltered_bf16_gate", None, qsets, 1)] + \
        [(name, filters[name], qsets, 0) for name in ("100", "50", "10", "1", "10_lists")] + \
        [("sub_index_of_10_lists_unfiltered", None, qsets, 0)] + \
        [("unfiltered_tenant_queries", None, own, 0), ("10_lists_tenant_queries", filters["10_lists"], own, 0)]
    for name, filt, qs, gate in legs:
        index = sidx if name.startswith("sub_index") else idx
        rqi.set_option("scan_gate", gate)   # (1: the bf16 threshold form, which filtered stages always run)
        for w in range(args.warmup):
            run(filt, qs[w % 4], index)
        torch.cuda.synchronize()
        times = []
        for s in range(args.steps):
            q = qs[s % 4]
            torch.cuda.synchronize()
            ts = time.perf_counter()
            run(filt, q, index)
            times.append(time.perf_counter() - ts)
        med = float(np.median(times))
        ms_call[name] = round(med * 1e3, 2)
        qps[name] = round(B / med)
        # one more call with the per-kernel profile (level 1: every kernel group bracketed; not part of the timing above)
        rqi.set_profiling(1)
        run(filt, qs[0], index)
        p = rqi.last_profile()
        rqi.set_profiling(0)
        prof[name] = {key: (round(p[key], 2) if isinstance(p[key], float) else p[key]) for key in
                      ("ms_scan", "ms_scan_matrix", "ms_rerank", "ms_total", "scan_candidates", "rerank_candidates")}
        rqi.set_option("scan_gate", 0)
    # small calls: one query per call through the host entry (the reference's own loop) and 64 queries per device call, on the
    # small-batch path with or without a filter (option small_batch_filtered); median wall time per call
    small = {}
    qhost = qsets[0][:200].cpu().numpy()
    for name, filt in (("unfiltered", None), ("10", filters["10"]), ("1", filters["1"]), ("10_lists", filters["10_lists"])):
        t1 = []
        for i in range(qhost.shape[0]):
            ts = time.perf_counter()
            idx.query(qhost[i], args.nprobe, topk, filter=filt)
            t1.append(time.perf_counter() - ts)
        t64 = []
        for i in range(20):
            q = qsets[1][64 * i:64 * (i + 1)]
            torch.cuda.synchronize()
            ts = time.perf_counter()
            idx.query_batch_device(q.data_ptr(), 64, d, args.nprobe, topk, od.data_ptr(), oi.data_ptr(), on.data_ptr(), filter=filt)
            t64.append(time.perf_counter() - ts)
        small[name] = {"ms_batch1": round(float(np.median(t1[10:])) * 1e3, 3), "ms_batch64": round(float(np.median(t64[2:])) * 1e3, 3)}
    # recall@10 of the random 10 % filter
    run(filters["10"], qsets[0])
    torch.cuda.synchronize()
    got = oi[:ngt].cpu().numpy().view(np.uint32).astype(np.int64)
    cnt = on[:ngt].cpu().numpy()
    hits = sum(len(set(got[i, :cnt[i]].tolist()) & set(gt[i].tolist())) for i in range(ngt))
    recall = hits / float(ngt * topk)
    for f in filters.values():
        f.close()
    line = {"metric": "filtered_queries_per_s", "vectors": n, "dim": d, "lists": k, "nprobe": args.nprobe, "topk": topk, "batch": B,
            "steps": args.steps, "qps": qps, "ms_per_call": ms_call, "profile": prof, "small_calls": small, "sub_index_10_lists_rows": n_sub,
            "sub_index_10_lists_same_results": sub_same, "filter_ms": filter_ms, "admitted_rows": rows,
            "recall10_filtered_10pct": round(recall, 4), "gt_queries": ngt, "build_s": round(build_s, 1),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
