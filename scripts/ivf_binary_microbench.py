"""IVF over sign codes (cx_search_hamming_window_topk + cx_hamming_merge_lists) next to its neighbours, by
scripts/ivf_pq_microbench.py's method and on its corpus: same box, ONE process in which all paths ALTERNATE run by run, device
events, one warm-up round of all, medians of --reps runs with p10 - p90.

  legs   : FlatIPIndex.search (the exact result), BinaryFlatIndex.search, and per nprobe in --nprobe: IVFBinaryIndex.search,
           search_ivf_binary_rescored at R = --factor with the bf16 rows on the device, IVFPQIndex.search (dsub 8: the same
           bytes per row)
  recall : recall@k of every leg against the exact result
  index  : list sizes after training (min / median / max), train and add times (ONE run each)

usage: python scripts/ivf_binary_microbench.py [--m 8192] [--n 2000000] [--d 768] [--k 100] [--nlist 1024] [--nprobe 1 8 32]
                                               [--factor 4] [--reps 7] [--out profiles/ivf_binary_microbench.json]
The JSON record on stdout and, in a list, in --out.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from ivf_int8_microbench import DEV, alternate, mixture, recall_of, summary  # noqa: E402
from ivf_pq_microbench import timed  # noqa: E402


def bench(args):
    import torch

    from contrastors_amd.search import (BinaryFlatIndex, FlatIPIndex, IVFBinaryIndex, IVFPQIndex, pack_sign_bits,
                                        search_ivf_binary_rescored)

    M, N, d, k, R = args.m, args.n, args.d, args.k, args.factor
    g = torch.Generator(device=DEV).manual_seed(0)
    D = mixture(N, d, args.centres, g)
    Q = mixture(M, d, args.centres, g)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    codes, qc = pack_sign_bits(D), pack_sign_bits(Q)
    bflat = BinaryFlatIndex(d, device=DEV)
    bflat.add(codes)
    build = {}
    ivfb = IVFBinaryIndex(d, args.nlist, device=DEV)
    build["ivf_binary_train_s"] = timed(lambda: ivfb.train(codes, max_iter=args.train_iters, sample=args.train_sample))
    build["ivf_binary_add_s"] = timed(lambda: ivfb.add(codes))
    sizes = ivfb.list_sizes                                  # (sorts the index before anything is timed)
    ivfpq = IVFPQIndex(d, args.nlist, 8, device=DEV)
    ivfpq.train(D, max_iter=args.train_iters, sample=args.train_sample)
    ivfpq.add(D)
    ivfpq.list_sizes
    fns = {"exact": lambda: flat.search(Q, k), "binary_flat": lambda: bflat.search(qc, k)}
    for p in args.nprobe:
        fns[f"ivf_binary_nprobe{p}"] = (lambda p=p: ivfb.search(qc, k, p))
        fns[f"ivf_binary_rescored_R{R}_nprobe{p}"] = (lambda p=p: search_ivf_binary_rescored(ivfb, flat.vectors, Q, k, p, R))
        fns[f"ivf_pq_residual_nprobe{p}"] = (lambda p=p: ivfpq.search(Q, k, p))
    runs = alternate(fns, args.reps)
    exact = flat.search(Q, k)[1]
    rec = {"what": "IVF binary index vs exact bf16, flat binary and IVF-PQ search", "shape": [M, N, d], "k": k, "reps": args.reps,
           "centres": args.centres, "nlist": args.nlist, "train": {"sample": args.train_sample, "iters": args.train_iters},
           "list_sizes": {"min": int(sizes.min()), "median": int(sizes.median()), "max": int(sizes.max())},
           "build_single_runs": build, "paths": {n: summary(v) for n, v in runs.items()},
           f"recall@{k}": {n: recall_of(f()[1], exact) for n, f in fns.items() if n != "exact"}}
    e = rec["paths"]["binary_flat"]["median_s"]
    rec["over_binary_flat"] = {n: v["median_s"] / e for n, v in rec["paths"].items()}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--train_sample", type=int, default=262_144)
    ap.add_argument("--train_iters", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ivf_binary_microbench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    Path(args.out).write_text(json.dumps([bench(args)], indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
