"""Int8 scalar-quantised index (cx_search_int8_topk + cx_rescore_topk) against the exact bf16 search (cx_search_topk): same
box, same process, the paths ALTERNATED run by run, device events, one warm-up round of all, medians of --reps runs.

  paths    : FlatIPIndex.search, Int8FlatIndex.search (queries quantised beforehand), search_int8_rescored at R in --factors
             with the rows on the device (query quantisation and, past 1024 candidates, the paging included)
  quantiser: cx_quantize_rows_int8 over the corpus, GB/s read + written, next to the box's copy rate (cx_calib_copy, the
             measurement scripts/box_calibration.py reports as hbm_copy_tbs)
  recall   : recall@k of every path against the exact result
Corpus: a planted mixture of --centres unit-norm directions, rows = centre + noise, normalised; queries from the same mixture.

usage: python scripts/search_int8_microbench.py [--m 8192] [--n 2000000] [--d 768 64] [--k 100] [--reps 7] [--factors 1 2 4]
                                                [--out profiles/search_int8_microbench.json]
One JSON record per line on stdout; all of them as a list in --out.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from contrastors_amd import _C  # noqa: E402
from contrastors_amd.search import FlatIPIndex, Int8FlatIndex, quantize_rows_int8, search_int8_rescored  # noqa: E402

DEV = "cuda:0"


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def alternate(fns, reps):
    """fns: name -> callable.  One warm-up round, then each run of one is followed by a run of the next."""
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


def copy_rate(nbytes=1 << 30):
    lib = _C.lib()
    src = torch.empty(nbytes, dtype=torch.uint8, device=DEV).random_(0, 255)
    dst = torch.empty_like(src)
    with torch.cuda.device(DEV):
        runs = alternate({"copy": lambda: _C.check(lib.cx_calib_copy(src.data_ptr(), dst.data_ptr(), nbytes, _C.cur_stream()),
                                                   "cx_calib_copy")}, 7)["copy"]
    return 2.0 * nbytes / statistics.median(runs) / 1e9


def bench(M, N, d, k, reps, factors, centres):
    g = torch.Generator(device=DEV).manual_seed(0)
    D = mixture(N, d, centres, g)
    Q = mixture(M, d, centres, g)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    ix = Int8FlatIndex(d, device=DEV)
    ix.add(D)
    qpair = quantize_rows_int8(Q)
    fns = {"exact": lambda: flat.search(Q, k), "int8": lambda: ix.search(qpair, k)}
    for R in factors:
        fns[f"int8_rescored_R{R}"] = (lambda R=R: search_int8_rescored(ix, flat.vectors, Q, k, R))
    runs = alternate(fns, reps)
    exact = flat.search(Q, k)[1]
    rec = {"what": "int8 index vs exact bf16 search", "shape": [M, N, d], "k": k, "reps": reps, "centres": centres,
           "index_bytes": {"bf16": N * d * 2, "int8": N * d + 4 * N},
           "paths": {n: summary(v) for n, v in runs.items()},
           f"recall@{k}": {"int8": recall_of(ix.search(qpair, k)[1], exact)}}
    for R in factors:
        rec[f"recall@{k}"][f"int8_rescored_R{R}"] = recall_of(search_int8_rescored(ix, flat.vectors, Q, k, R)[1], exact)
    e, i8 = rec["paths"]["exact"], rec["paths"]["int8"]
    rec["int8_over_exact"] = i8["median_s"] / e["median_s"]
    rec["int8_slower_than_exact_beyond_spread"] = bool(i8["median_s"] - e["median_s"] > max(e["p90_s"] - e["p10_s"],
                                                                                          i8["p90_s"] - i8["p10_s"]))
    q = summary(alternate({"quantize": lambda: quantize_rows_int8(D)}, reps)["quantize"])
    rec["quantiser"] = {"rows": N, "dtype": "bf16", **q, "GBps_read_plus_written": (N * d * 3 + 4 * N) / q["median_s"] / 1e9}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, nargs="+", default=[768, 64])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--factors", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "search_int8_microbench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    records = [{"what": "HBM copy rate (cx_calib_copy, 1 GiB read + 1 GiB written)", "GBps": copy_rate()}]
    print(json.dumps(records[0]), flush=True)
    for d in args.d:
        records.append(bench(args.m, args.n, d, args.k, args.reps, args.factors, args.centres))
    Path(args.out).write_text(json.dumps(records, indent=1) + "\n")


if __name__ == "__main__":
    main()
