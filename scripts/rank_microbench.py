"""Time cx_rank_targets (csrc/rank.hip) against the dense torch form and, for scale, against cx_search_topk.

    python scripts/rank_microbench.py [--reps 20] [--warmup 3] [--out FILE.json]

Shapes (M queries x N corpus x d, targets per row): ImageNet zero-shot 50 000 x 1000 x 768 (1), Flickr text retrieval
1000 x 5000 x 768 (5), a retrieval set 8192 x 1 000 000 x 768 (1).  Dense form: bf16 matmul of a row chunk, then
`(S > t) | ((S == t) & (col < id))` summed -- it writes the (chunk x N) scores and is run where they fit (the third shape
is timed for the kernel alone).  Times are medians of device-event timings after warm-up, alternating the two forms in
one process; the dense form's ranks are compared with the kernel's on the way (a bf16 matmul rounds its scores, so they
differ on near-ties: the share is printed, not asserted).  One JSON line per shape."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"
SHAPES = [("imagenet", 50_000, 1000, 768, 1, True), ("flickr_t2i", 1000, 5000, 768, 5, True),
          ("retrieval", 8192, 1_000_000, 768, 1, False)]
DENSE_CHUNK_ELEMS = 1 << 28   # (rows x N) scores per chunk of the dense form


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def dense_ranks(Q, D, ids, per):
    """Per-entry ranks by the dense form, chunked over rows; ids (M, per)."""
    M, N = Q.shape[0], D.shape[0]
    col = torch.arange(N, device=DEV)
    out = torch.empty(M, per, dtype=torch.int64, device=DEV)
    ch = max(1, DENSE_CHUNK_ELEMS // N)
    for r0 in range(0, M, ch):
        S = Q[r0: r0 + ch] @ D.T                                   # bf16 in, bf16 out: what autocast gives the reference
        for j in range(per):
            t_id = ids[r0: r0 + ch, j]
            t = S.gather(1, t_id[:, None])
            out[r0: r0 + ch, j] = ((S > t) | ((S == t) & (col[None, :] < t_id[:, None]))).sum(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--only", help="comma-separated shape names")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rank_microbench needs the GPU")
    from contrastors_amd.search import FlatIPIndex

    rows = []
    for name, M, N, d, per, dense in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        g = torch.Generator(device=DEV).manual_seed(1)
        Q = torch.nn.functional.normalize(torch.randn(M, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
        D = torch.nn.functional.normalize(torch.randn(N, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
        ids = torch.randint(0, N, (M, per), device=DEV, generator=g)
        ix = FlatIPIndex(d, device=DEV)
        ix.add(D)
        ptr = torch.arange(M + 1, dtype=torch.int64) * per
        targets = (ptr.numpy(), ids.reshape(-1).cpu().numpy())
        reps = args.reps if N < 1_000_000 else max(3, args.reps // 4)
        runs = {"rank": lambda: ix.rank(Q, targets)}               # the whole call: CSR upload, three launches, int64 widening
        if dense:
            runs["dense"] = lambda: dense_ranks(Q, D, ids, per)
        if name == "imagenet":
            runs["search_k1024"] = lambda: ix.search(Q, 1000)      # k = min(N, 1024)
        times = {k: [] for k in runs}
        for k, fn in runs.items():
            timed(fn, 0, args.warmup)
        for _ in range(reps):                                        # alternate the forms
            for k, fn in runs.items():
                times[k] += timed(fn, 1, 0)
        row = {"shape": name, "M": M, "N": N, "d": d, "targets_per_row": per, "reps": reps,
               "tflops_rank": None, **{f"{k}_ms_median": round(statistics.median(v), 3) for k, v in times.items()},
               **{f"{k}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}}
        row["tflops_rank"] = round(2.0 * M * N * d / (row["rank_ms_median"] * 1e-3) / 1e12, 1)   # count walk only: the useful work
        if dense:
            row["rank_over_dense"] = round(row["rank_ms_median"] / row["dense_ms_median"], 3)
            kr = ix.rank(Q, targets)[0].view(M, per)
            row["share_of_ranks_differing_from_dense_bf16"] = round(float((kr != dense_ranks(Q, D, ids, per)).double().mean()), 5)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del Q, D, ix
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
