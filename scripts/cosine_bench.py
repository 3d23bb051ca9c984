"""Cosine metric at the headline shape (BASELINE configs[2]: 100M x 128, 4096 lists, nprobe 64, the synthetic mixture of
tests/synth.py with per-row lengths spread over 2^-10 .. 2^10).  One process measures ONE side and prints ONE JSON line:

  --side cosine     this commit's cosine index on the raw rows and raw queries
  --side baseline   the parent commit (--package-root: a checkout of it with its library built, or RABITQ_HIP_SO; it knows no
                    metric) as an L2 index on rows and queries normalised BEFOREHAND -- by this commit's rq_normalize_device,
                    loaded from --normalize-so next to the baseline library, so both sides see the same bits; the normalisation
                    is outside the timed regions, which is the point: the difference between the sides is what the index now
                    does itself

Each side records the build's engine time (the streamed builder's calls, as bench.py times its build; after a warm-up build),
the median and the spread (min / max) of the step time at batches of 1, 64 and 65 536 over --steps calls, and writes its
65 536 results to --dump DIR (dist / ids / n as .npy).  `--compare A B` asserts that two dumps are identical, byte for byte.
Run the sides alternately (A B A B) and keep every line, as profiles/prep_placement_ab_runs.txt does:

  python scripts/cosine_bench.py --side baseline --package-root ../parent --normalize-so rabitq_amd/librabitq_hip.so --dump out/base
  python scripts/cosine_bench.py --side cosine --dump out/cos
  python scripts/cosine_bench.py --compare out/base out/cos
"""
import argparse
import ctypes as C
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
    ap.add_argument("--side", choices=["cosine", "baseline"])
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--normalize-so", default="", help="baseline: the library whose rq_normalize_device prepares rows and queries")
    ap.add_argument("--package-root", default="", help="baseline: the tree whose rabitq_amd package (and library) is measured")
    ap.add_argument("--vectors", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--dump", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    import numpy as np
    import torch
    import rabitq_amd as rq
    from rabitq_amd import _lib
    from tests import synth
    _lib.check(_lib.lib().rq_init(0))
    dev = torch.device("cuda")
    n, d, k = args.vectors, args.dim, args.lists
    dim = (d + 63) // 64 * 64
    x, cd = synth.device_mixture(n, d, k, args.sigma, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    for i0 in range(0, n, 4_000_000):   # per-row lengths: powers of two times [0.5, 2)
        m = min(4_000_000, n - i0)
        x[i0:i0 + m] *= torch.exp2(torch.randint(-10, 11, (m, 1), generator=g, device=dev).float()) * (0.5 + 1.5 * torch.rand(m, 1, generator=g, device=dev))
    queries = synth.device_queries(cd, 65536, args.sigma, dev) * 37.0
    P = synth.random_orthogonal(dim, seed=99)
    cosine = args.side == "cosine"

    if cosine:
        norm = _lib.lib()
    else:
        assert args.normalize_so, "--side baseline needs --normalize-so"
        norm = C.CDLL(args.normalize_so)
        norm.rq_normalize_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    # centroids of the normalised data on both sides: the mixture's centres, normalised
    cn = torch.empty((k, dim), device=dev)
    torch.cuda.synchronize()
    assert norm.rq_normalize_device(C.c_void_p(cd.data_ptr()), k, d, C.c_void_p(cn.data_ptr())) == 0
    if not cosine:   # normalised beforehand, in place where the shape allows it (d == dim), outside every timed region
        assert d == dim, "the baseline side normalises in place: use a dimension that is a multiple of 64"
        for buf in (x, queries):
            for i0 in range(0, buf.shape[0], 1 << 20):   # chunks: the kernel reads a row group before it writes it
                m = min(1 << 20, buf.shape[0] - i0)
                tmp = torch.empty((m, dim), device=dev)
                torch.cuda.synchronize()
                assert norm.rq_normalize_device(C.c_void_p(buf[i0:].data_ptr()), m, d, C.c_void_p(tmp.data_ptr())) == 0
                buf[i0:i0 + m] = tmp
    kw = {"metric": "cosine"} if cosine else {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def engine_build(rows):
        b = rq.RaBitQ.builder(rows, d, cn.data_ptr(), k, orthogonal=P, **kw)
        ms = 0.0
        for call in (lambda: b.assign_chunk(x.data_ptr(), 0, rows), b.order, lambda: b.place_chunk(x.data_ptr(), 0, rows)):
            ms += timed(call)[1]
        idx, t = timed(b.finish)
        return idx, ms + t

    engine_build(min(n, 1 << 20))[0].close()   # warm-up: code objects, kernel attributes
    idx, build_ms = engine_build(n)
    out = {"side": args.side, "library": _lib.SO_PATH, "vectors": n, "dim": d, "lists": k, "nprobe": args.nprobe,
           "build_engine_ms": round(build_ms, 1), "step_ms": {}}
    od = torch.empty((65536, args.topk), device=dev)
    oi = torch.zeros((65536, args.topk), device=dev, dtype=torch.int32)
    on = torch.zeros(65536, device=dev, dtype=torch.int32)
    for nq in (1, 64, 65536):
        call = lambda: idx.query_batch_device(queries.data_ptr(), nq, d, args.nprobe, args.topk, od.data_ptr(), oi.data_ptr(), on.data_ptr())
        timed(call), timed(call)
        ms = sorted(timed(call)[1] for _ in range(args.steps))
        out["step_ms"][str(nq)] = {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}
        out["step_ms"][str(nq)]["normalise_bytes"] = nq * dim * 8 if cosine else 0
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
