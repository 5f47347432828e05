"""Binary index (cx_search_hamming_topk + cx_rescore_topk) against the exact bf16 search (cx_search_topk): same box, same
process, the two searches ALTERNATED run by run, median of --reps runs each after a warm-up of both.

  timing : Hamming top-k over sign codes vs FlatIPIndex.search at (M, N, d, k); then the re-scoring stage at k * R candidates
  recall : recall@k of binary + re-scoring (R in --factors) against the exact search on embeddings of synthetic text from a
           tiny random-init BiEncoder with `hamming: true` (reported, says little about a trained model)

usage: python scripts/search_binary_microbench.py [--m 8192] [--n 2000000] [--d 768 64] [--k 100] [--reps 7]
                                                  [--factors 4 10 16] [--recall_docs 50000] [--recall_queries 512]
One JSON record per line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from contrastors_amd.search import (BinaryFlatIndex, FlatIPIndex, encode, pack_sign_bits, rescore,  # noqa: E402
                                    search_binary_rescored)

DEV = "cuda:0"


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def alternate(fns, reps):
    """fns: name -> callable.  Each run of one is followed by a run of the next; -> name -> (median, all runs)."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    runs = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            runs[n].append(once(f))
    return {n: (statistics.median(v), v) for n, v in runs.items()}


def timing(M, N, d, k, reps, factors):
    g = torch.Generator(device=DEV).manual_seed(0)
    Q = torch.nn.functional.normalize(torch.randn(M, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
    D = torch.nn.functional.normalize(torch.randn(N, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    binary = BinaryFlatIndex(d, device=DEV)
    binary.add(D)
    qc = pack_sign_bits(Q)
    res = alternate({"exact": lambda: flat.search(Q, k), "hamming": lambda: binary.search(qc, k)}, reps)
    ops = 2.0 * M * N * d
    rec = {"what": "coarse stage vs exact search", "shape": [M, N, d], "k": k, "reps": reps,
           "exact_s": res["exact"][0], "hamming_s": res["hamming"][0], "hamming_over_exact": res["hamming"][0] / res["exact"][0],
           "exact_tflops": ops / res["exact"][0] / 1e12, "hamming_tops": ops / res["hamming"][0] / 1e12,
           "exact_runs_s": res["exact"][1], "hamming_runs_s": res["hamming"][1],
           "index_bytes": {"bf16": N * d * 2, "codes": N * d // 8}}
    print(json.dumps(rec), flush=True)
    pack_s = alternate({"pack": lambda: pack_sign_bits(D)}, reps)["pack"][0]
    print(json.dumps({"what": "pack_sign_bits of the corpus", "rows": N, "d": d, "s": pack_s,
                      "read_GBps": N * d * 2 / pack_s / 1e9}), flush=True)
    for R in factors:
        c = min(k * R, 4096)
        if c > 1024:   # the coarse stage then runs in pages of 1024 (search_binary_rescored): not a kernel timing
            continue
        n = max(3, reps // 2)
        hs = alternate({"hamming": lambda: binary.search(qc, c)}, n)["hamming"][0]
        cand = binary.search(qc, c)[1]
        rs = alternate({"rescore": lambda: rescore(Q, cand, D, k)}, n)["rescore"][0]
        print(json.dumps({"what": "two-stage search", "factor": R, "candidates": c, "hamming_s": hs, "rescore_s": rs,
                          "total_over_exact": (hs + rs) / res["exact"][0]}), flush=True)


def recall(n_docs, n_queries, k, factors):
    from contrastors_amd.biencoder import BiEncoder, BiEncoderConfig
    from contrastors_amd.nomic_bert import NomicBertConfig
    from oracle import encoder_ref
    from oracle.data_fixture import WORDS, ToyTokenizer
    from oracle.make_golden import TINY_NOMIC

    cfg = NomicBertConfig(**{a: b for a, b in TINY_NOMIC.items() if a in NomicBertConfig.__dataclass_fields__})
    model = BiEncoder(BiEncoderConfig(pooling="mean", hamming=True, trunk_config=cfg), device=DEV)
    model.trunk.load_reference_state_dict(encoder_ref.random_state_dict(SimpleNamespace(**TINY_NOMIC), 3))
    rng = np.random.default_rng(0)
    docs = [" ".join(rng.choice(WORDS, int(rng.integers(4, 24)))) for _ in range(n_docs)]
    # a query is a document with a third of its words replaced
    queries = []
    for i in rng.choice(n_docs, n_queries, replace=False):
        w = docs[i].split()
        for j in rng.choice(len(w), max(1, len(w) // 3), replace=False):
            w[j] = str(rng.choice(WORDS))
        queries.append(" ".join(w))
    tok = ToyTokenizer()
    D = encode(model, docs, tok, batch_size=512, max_length=32)
    Q = encode(model, queries, tok, batch_size=512, max_length=32)
    d = D.shape[1]
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    binary = BinaryFlatIndex(d, device=DEV)
    binary.add(D)
    _, exact = flat.search(Q, k)
    out = {"what": "recall of binary + re-scoring vs exact search", "model": "tiny random-init NomicBert BiEncoder, hamming=true",
           "docs": n_docs, "queries": n_queries, "d": d, "k": k}
    for R in factors:
        _, got = search_binary_rescored(binary, flat.vectors, Q, k, R)
        hits = (got[:, :, None] == exact[:, None, :]).any(2).float().sum(1)
        out[f"recall@{k}_R{R}"] = float((hits / k).mean())
    _, got = binary.search(Q, k)
    out[f"recall@{k}_hamming_only"] = float(((got[:, :, None] == exact[:, None, :]).any(2).float().sum(1) / k).mean())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, nargs="+", default=[768, 64])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--factors", type=int, nargs="+", default=[4, 10, 16])
    ap.add_argument("--recall_docs", type=int, default=50_000)
    ap.add_argument("--recall_queries", type=int, default=512)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    for d in args.d:
        timing(args.m, args.n, d, args.k, args.reps, args.factors)
    if args.recall_docs:
        recall(args.recall_docs, args.recall_queries, args.k, args.factors)


if __name__ == "__main__":
    main()
