"""IVF over int8 codes (cx_search_int8_window_topk + cx_topk_merge_lists) next to its three neighbours: the exact bf16 search,
the flat int8 search and the bf16 IVF index.  scripts/search_int8_microbench.py's method: same box, ONE process per width in
which all paths ALTERNATE run by run, device events, one warm-up round of all, medians of --reps runs with p10 - p90.

  legs   : FlatIPIndex.search, Int8FlatIndex.search, and per nprobe in --nprobe: IVFFlatIndex.search, IVFInt8Index.search,
           search_ivf_int8_rescored at R = --factor with the bf16 rows on the device
  recall : recall@k of every leg against the exact result
  index  : bytes held per format, list sizes (min / median / max)
Corpus: a planted mixture of --centres unit-norm directions, rows = centre + noise, normalised; queries from the same mixture.
Both IVF indexes share one centroid table (spherical k-means on a seeded sample of --train_sample rows, --train_iters updates).

Every width runs in a child process of its own under --limit seconds; after a child that fails or runs out of time nothing more
is started, and the records so far are written.

usage: python scripts/ivf_int8_microbench.py [--m 8192] [--n 2000000] [--d 768 64] [--k 100] [--nlist 1024] [--nprobe 1 8 32]
                                             [--factor 2] [--reps 7] [--limit 400] [--out profiles/ivf_int8_microbench.json]
One JSON record per line on stdout; all of them as a list in --out.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
DEV = "cuda:0"


def once(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def alternate(fns, reps):
    """fns: name -> callable.  One warm-up round, then each run of one is followed by a run of the next."""
    import torch

    for f in fns.values():
        f()
    torch.cuda.synchronize()
    runs = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            runs[n].append(once(f))
    return runs


def summary(v):
    s = sorted(v)
    return {"median_s": statistics.median(s), "p10_s": s[max(0, round(0.1 * (len(s) - 1)))],
            "p90_s": s[min(len(s) - 1, round(0.9 * (len(s) - 1)))], "runs_s": v}


def mixture(n, d, centres, g):
    import torch

    c = torch.nn.functional.normalize(torch.randn(centres, d, device=DEV, generator=g), dim=1)
    out = torch.empty(n, d, dtype=torch.bfloat16, device=DEV)
    for r0 in range(0, n, 1 << 18):
        m = min(1 << 18, n - r0)
        pick = torch.randint(0, centres, (m,), device=DEV, generator=g)
        x = c[pick] + torch.randn(m, d, device=DEV, generator=g) / d ** 0.5
        out[r0: r0 + m] = torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)
    return out


def recall_of(got, exact):
    hits = 0.0
    for r0 in range(0, got.shape[0], 1024):
        g, e = got[r0: r0 + 1024], exact[r0: r0 + 1024]
        hits += float((g[:, :, None] == e[:, None, :]).any(2).float().sum())
    return hits / exact.numel()


def bench(args, d):
    import torch

    from contrastors_amd.search import (FlatIPIndex, Int8FlatIndex, IVFFlatIndex, IVFInt8Index, quantize_rows_int8,
                                        search_ivf_int8_rescored)

    M, N, k, R = args.m, args.n, args.k, args.factor
    g = torch.Generator(device=DEV).manual_seed(0)
    D = mixture(N, d, args.centres, g)
    Q = mixture(M, d, args.centres, g)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    flat8 = Int8FlatIndex(d, device=DEV)
    flat8.add(D)
    ivf = IVFFlatIndex(d, args.nlist, device=DEV)
    ivf.train(D, max_iter=args.train_iters, sample=args.train_sample)
    ivf.add(D)
    ivf8 = IVFInt8Index(d, args.nlist, device=DEV)
    ivf8.train(centroids=ivf.centroids)
    ivf8.add(D)
    sizes = ivf8.list_sizes                                  # (sorts both indexes before anything is timed)
    assert torch.equal(sizes, ivf.list_sizes)
    qpair = quantize_rows_int8(Q)
    fns = {"exact": lambda: flat.search(Q, k), "int8_flat": lambda: flat8.search(qpair, k)}
    for p in args.nprobe:
        fns[f"ivf_bf16_nprobe{p}"] = (lambda p=p: ivf.search(Q, k, p))
        fns[f"ivf_int8_nprobe{p}"] = (lambda p=p: ivf8.search(Q, k, p))
        fns[f"ivf_int8_rescored_R{R}_nprobe{p}"] = (lambda p=p: search_ivf_int8_rescored(ivf8, flat.vectors, Q, k, p, R))
    runs = alternate(fns, args.reps)
    exact = flat.search(Q, k)[1]
    rec = {"what": "IVF int8 index vs exact bf16, flat int8 and IVF bf16 search", "shape": [M, N, d], "k": k, "reps": args.reps,
           "centres": args.centres, "nlist": args.nlist, "train": {"sample": args.train_sample, "iters": args.train_iters},
           "list_sizes": {"min": int(sizes.min()), "median": int(sizes.median()), "max": int(sizes.max())},
           "index_bytes": {"bf16": N * d * 2, "int8": N * d + 4 * N},
           "paths": {n: summary(v) for n, v in runs.items()},
           f"recall@{k}": {n: recall_of(f()[1], exact) for n, f in fns.items() if n != "exact"}}
    e = rec["paths"]["exact"]["median_s"]
    rec["over_exact"] = {n: v["median_s"] / e for n, v in rec["paths"].items()}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, nargs="+", default=[768, 64])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--train_sample", type=int, default=262_144)
    ap.add_argument("--train_iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=400, help="seconds one width's process may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ivf_int8_microbench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    if args.child:
        bench(args, args.d[0])
        return 0
    records, status = [], 0
    passed = [a for a in sys.argv[1:]]
    for d in args.d:
        cmd = [sys.executable, str(Path(__file__).resolve()), *passed, "--d", str(d), "--child"]      # (the last --d wins)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"d": d, "error": f"no result within {args.limit} s"}), flush=True)
            status = 1
            break
        if r.returncode != 0:
            print(json.dumps({"d": d, "error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}), flush=True)
            status = 1
            break
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        records.append(json.loads(line))
    if records:
        Path(args.out).write_text(json.dumps(records, indent=1) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
