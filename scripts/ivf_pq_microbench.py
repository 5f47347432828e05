"""IVF over PQ residual codes (cx_search_pq_window_topk + cx_topk_merge_lists) next to its neighbours, by
scripts/ivf_int8_microbench.py's method and on its corpus: same box, ONE process in which all paths ALTERNATE run by run, device
events, one warm-up round of all, medians of --reps runs with p10 - p90.

  legs   : FlatIPIndex.search, PQFlatIndex.search, search_pq_rescored at R = --factor, and per nprobe in --nprobe:
           IVFFlatIndex.search, IVFInt8Index.search, IVFPQIndex.search with and without residuals, search_ivf_pq_rescored of both
           at R = --factor with the bf16 rows on the device
  recall : recall@k of every leg against the exact result
  index  : bytes held per format, list sizes (min / median / max), build times (ONE run each)
All IVF indexes share one centroid table; the flat and the raw-row IVF PQ codes share one set of codebooks.

usage: python scripts/ivf_pq_microbench.py [--m 8192] [--n 2000000] [--d 768] [--dsub 8] [--k 100] [--nlist 1024]
                                           [--nprobe 1 8 32] [--factor 4] [--reps 7] [--out profiles/ivf_pq_microbench.json]
The JSON record on stdout and, in a list, in --out.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from ivf_int8_microbench import DEV, alternate, mixture, recall_of, summary  # noqa: E402


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench(args):
    import torch

    from contrastors_amd.search import (FlatIPIndex, IVFFlatIndex, IVFInt8Index, IVFPQIndex, PQFlatIndex, search_ivf_pq_rescored,
                                        search_pq_rescored)

    M, N, d, k, R = args.m, args.n, args.d, args.k, args.factor
    g = torch.Generator(device=DEV).manual_seed(0)
    D = mixture(N, d, args.centres, g)
    Q = mixture(M, d, args.centres, g)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    ivf = IVFFlatIndex(d, args.nlist, device=DEV)
    ivf.train(D, max_iter=args.train_iters, sample=args.train_sample)
    ivf.add(D)
    ivf8 = IVFInt8Index(d, args.nlist, device=DEV)
    ivf8.train(centroids=ivf.centroids)
    ivf8.add(D)
    build = {}
    pq = PQFlatIndex(d, args.dsub, device=DEV)
    build["pq_flat_train_s"] = timed(lambda: pq.train(D))
    build["pq_flat_add_s"] = timed(lambda: pq.add(D))
    res = IVFPQIndex(d, args.nlist, args.dsub, device=DEV)
    build["ivf_pq_residual_train_s"] = timed(lambda: res.train(D, centroids=ivf.centroids))
    build["ivf_pq_residual_add_s"] = timed(lambda: res.add(D))
    raw = IVFPQIndex(d, args.nlist, args.dsub, by_residual=False, device=DEV)
    raw.train(centroids=ivf.centroids, codebooks=pq.masters)
    build["ivf_pq_raw_add_s"] = timed(lambda: raw.add(D))
    sizes = res.list_sizes                                   # (sorts the indexes before anything is timed)
    assert torch.equal(sizes, ivf.list_sizes) and torch.equal(sizes, raw.list_sizes) and torch.equal(sizes, ivf8.list_sizes)
    fns = {"exact": lambda: flat.search(Q, k), "pq_flat": lambda: pq.search(Q, k),
           f"pq_flat_rescored_R{R}": lambda: search_pq_rescored(pq, flat.vectors, Q, k, R)}
    for p in args.nprobe:
        fns[f"ivf_bf16_nprobe{p}"] = (lambda p=p: ivf.search(Q, k, p))
        fns[f"ivf_int8_nprobe{p}"] = (lambda p=p: ivf8.search(Q, k, p))
        fns[f"ivf_pq_residual_nprobe{p}"] = (lambda p=p: res.search(Q, k, p))
        fns[f"ivf_pq_raw_nprobe{p}"] = (lambda p=p: raw.search(Q, k, p))
        fns[f"ivf_pq_residual_rescored_R{R}_nprobe{p}"] = (lambda p=p: search_ivf_pq_rescored(res, flat.vectors, Q, k, p, R))
        fns[f"ivf_pq_raw_rescored_R{R}_nprobe{p}"] = (lambda p=p: search_ivf_pq_rescored(raw, flat.vectors, Q, k, p, R))
    runs = alternate(fns, args.reps)
    exact = flat.search(Q, k)[1]
    m = d // args.dsub
    rec = {"what": "IVF-PQ index vs exact bf16, flat PQ, IVF bf16 and IVF int8 search", "shape": [M, N, d], "dsub": args.dsub, "k": k,
           "reps": args.reps, "centres": args.centres, "nlist": args.nlist,
           "train": {"sample": args.train_sample, "iters": args.train_iters, "pq_sample": 65536, "pq_iters": 25},
           "list_sizes": {"min": int(sizes.min()), "median": int(sizes.median()), "max": int(sizes.max())},
           "index_bytes": {"bf16": N * d * 2, "int8": N * d + 4 * N, "pq_flat": N * m + 512 * d,
                           "ivf_pq": N * m + 512 * d + 2 * args.nlist * d, "ivf_bookkeeping_per_row": 20},
           "build_single_runs": build, "paths": {n: summary(v) for n, v in runs.items()},
           f"recall@{k}": {n: recall_of(f()[1], exact) for n, f in fns.items() if n != "exact"}}
    e = rec["paths"]["exact"]["median_s"]
    rec["over_exact"] = {n: v["median_s"] / e for n, v in rec["paths"].items()}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--dsub", type=int, default=8)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--train_sample", type=int, default=262_144)
    ap.add_argument("--train_iters", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ivf_pq_microbench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    Path(args.out).write_text(json.dumps([bench(args)], indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
