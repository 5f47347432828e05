"""Product-quantised index (cx_pq_assign / cx_pq_update / cx_search_pq_topk) against the exact bf16 search (cx_search_topk),
the int8 index and the sign-code index: same box, same process, the paths ALTERNATED run by run, device events, one warm-up
round of all, medians of --reps runs.

  paths  : FlatIPIndex.search, Int8FlatIndex.search (queries quantised beforehand), BinaryFlatIndex.search (queries packed
           beforehand), PQFlatIndex.search
  build  : PQFlatIndex.train (a seeded sample of --sample rows, --iters Lloyd steps) and the encoding of the corpus, one run each
  recall : recall@k against the exact result of PQ alone and re-scored at R in --factors, next to the sign index's
Corpus: a planted mixture of --centres unit-norm directions, rows = centre + noise, normalised; queries from the same mixture
(scripts/search_int8_microbench.py's).

usage: python scripts/pq_search_microbench.py [--m 8192] [--n 2000000] [--shapes 768:8 768:16 64:8] [--k 100] [--reps 7]
                                              [--factors 2 4 8] [--out profiles/pq_search_microbench.json]
One JSON record per line on stdout; all of them as a list in --out.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from search_int8_microbench import DEV, alternate, mixture, once, recall_of, summary  # noqa: E402

from contrastors_amd.search import (BinaryFlatIndex, FlatIPIndex, Int8FlatIndex, PQFlatIndex, pack_sign_bits,  # noqa: E402
                                    quantize_rows_int8, search_binary_rescored, search_pq_rescored)


def bench(M, N, d, dsub, k, reps, factors, centres, sample, iters):
    g = torch.Generator(device=DEV).manual_seed(0)
    D = mixture(N, d, centres, g)
    Q = mixture(M, d, centres, g)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    i8 = Int8FlatIndex(d, device=DEV)
    i8.add(D)
    sign = BinaryFlatIndex(d, device=DEV)
    sign.add(D)
    pq = PQFlatIndex(d, dsub, device=DEV)
    train_s = once(lambda: pq.train(D, max_iter=iters, sample=sample))
    pq.reserve(N)
    encode_s = once(lambda: pq.add(D))
    qpair, qbits = quantize_rows_int8(Q), pack_sign_bits(Q)
    fns = {"exact": lambda: flat.search(Q, k), "int8": lambda: i8.search(qpair, k), "sign": lambda: sign.search(qbits, k),
           "pq": lambda: pq.search(Q, k)}
    runs = alternate(fns, reps)
    exact = flat.search(Q, k)[1]
    rec = {"what": "PQ index vs exact bf16, int8 and sign-code search", "shape": [M, N, d], "dsub": dsub, "k": k, "reps": reps,
           "centres": centres,
           "index_bytes": {"bf16": N * d * 2, "int8": N * d + 4 * N, "sign": N * d // 8,
                           "pq": N * (d // dsub) + 256 * d * 2},
           "pq_train": {"sample": min(N, sample), "iters": iters, "seconds": train_s},
           "pq_encode": {"rows": N, "seconds": encode_s, "rows_per_s": N / encode_s},
           "paths": {n: summary(v) for n, v in runs.items()},
           f"recall@{k}": {"pq": recall_of(pq.search(Q, k)[1], exact), "sign": recall_of(sign.search(qbits, k)[1], exact),
                           "int8": recall_of(i8.search(qpair, k)[1], exact)}}
    for R in factors:
        rec[f"recall@{k}"][f"pq_rescored_R{R}"] = recall_of(search_pq_rescored(pq, flat.vectors, Q, k, R)[1], exact)
        rec[f"recall@{k}"][f"sign_rescored_R{R}"] = recall_of(search_binary_rescored(sign, flat.vectors, Q, k, R)[1], exact)
    e, p = rec["paths"]["exact"], rec["paths"]["pq"]
    rec["pq_over_exact"] = p["median_s"] / e["median_s"]
    rec["pq_slower_than_exact_beyond_spread"] = bool(p["median_s"] - e["median_s"] > max(e["p90_s"] - e["p10_s"],
                                                                                        p["p90_s"] - p["p10_s"]))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--shapes", nargs="+", default=["768:8", "768:16", "64:8"], help="d:dsub pairs")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--factors", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--sample", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "pq_search_microbench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    records = []
    for shape in args.shapes:
        d, dsub = (int(v) for v in shape.split(":"))
        records.append(bench(args.m, args.n, d, dsub, args.k, args.reps, args.factors, args.centres, args.sample, args.iters))
        torch.cuda.empty_cache()
        Path(args.out).write_text(json.dumps(records, indent=1) + "\n")


if __name__ == "__main__":
    main()
