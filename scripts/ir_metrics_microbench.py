"""Time a whole contrastors_amd.retrieval_eval.ir_metrics call (cx_ir_metrics, csrc/ir_metrics.hip) against the same metrics
written in host numpy and in batched torch on the device.

    python scripts/ir_metrics_microbench.py [--reps 50] [--warmup 5] [--out FILE.json]

Shapes (M query rows x targets per row): a NanoBEIR task 50 x ~50, an MS MARCO-dev-like set 6980 x 1, deep judgement pools
50 x 1000.  The inputs (ranks, gains) start on the device, as FlatIPIndex.rank leaves them; every form ends with the
per-query metrics at ks = (1, 3, 5, 10, 100) where the caller reads them: `ir_metrics` on the device (its validation reads
three scalars back), `torch` = rows padded to a (M, L) rectangle on the device and the counts as (M, L, L) comparisons, `numpy`
= download + a per-row sort-and-walk on the host.  Times are medians of host-clock timings around a device synchronise after
warm-up, alternating the forms in one process.  Asserts nothing about speed; the three forms' values are compared on the way
and the largest difference is printed.  One JSON line per shape."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"
KS = (1, 3, 5, 10, 100)
SHAPES = [("nanobeir", 50, 50, True), ("msmarco_dev", 6980, 1, False), ("deep_pools", 50, 1000, True)]


def make(M, per, ragged, seed=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(max(1, per // 2), per + per // 2 + 1, size=M) if ragged else np.full(M, per)
    row_ptr = np.zeros(M + 1, np.int64)
    row_ptr[1:] = np.cumsum(lens)
    ranks = np.concatenate([rng.choice(20 * n + 1000, size=n, replace=False) for n in lens]).astype(np.int64)
    gains = rng.integers(1, 4, size=ranks.size).astype(np.float32)
    gains[row_ptr[:-1][lens > 2]] = 0.0          # one excluded entry in the longer rows
    return row_ptr, ranks, gains


def numpy_form(row_ptr, ranks_dev, gains_dev):
    ranks, gains = ranks_dev.cpu().numpy(), gains_dev.cpu().numpy()
    M = row_ptr.size - 1
    out = np.zeros((M, len(KS), 6))
    for m in range(M):
        r, g = ranks[row_ptr[m]: row_ptr[m + 1]], gains[row_ptr[m]: row_ptr[m + 1]].astype(np.float64)
        o = np.argsort(r, kind="stable")
        r, g = r[o], g[o]
        rel = g > 0
        a = (r - np.cumsum(~rel) )[rel]
        g = g[rel]
        R = g.size
        if R == 0:
            continue
        ideal = np.sort(g)[::-1]
        disc, idisc = g / np.log2(a + 2.0), ideal / np.log2(np.arange(R) + 2.0)
        prec = (np.arange(R) + 1.0) / (a + 1.0)
        for j, k in enumerate(KS):
            h = int(np.searchsorted(a, k))
            out[m, j] = (disc[:h].sum() / idisc[:k].sum(), prec[:h].sum() / R, h / R, h / k, 1.0 / (a[0] + 1.0) if h else 0.0, float(h > 0))
    return out


def torch_form(row_ptr_dev, lens_dev, ranks, gains, L):
    """Batched on the device: pad to (M, L), sort by rank, cumulative sums."""
    M = lens_dev.numel()
    col = torch.arange(L, device=DEV)
    valid = col[None, :] < lens_dev[:, None]
    idx = (row_ptr_dev[:-1, None] + col[None, :]).clamp(max=ranks.numel() - 1)
    r = torch.where(valid, ranks[idx], torch.iinfo(torch.int64).max)
    g = torch.where(valid, gains[idx].double(), torch.tensor(-1.0, dtype=torch.float64, device=DEV))
    r, o = torch.sort(r, dim=1, stable=True)
    g = g.gather(1, o)
    rel, exc = g > 0, g == 0
    a = (r - torch.cumsum(exc, 1)).double()
    R = rel.sum(1).clamp(min=1).double()
    nth = torch.cumsum(rel, 1).double()                                  # relevant documents down to this entry
    ideal = torch.sort(torch.where(rel, g, torch.zeros_like(g)), dim=1, descending=True).values
    idisc = torch.cumsum(ideal / torch.log2(col.double() + 2.0)[None, :], 1)
    out = torch.zeros(M, len(KS), 6, dtype=torch.float64, device=DEV)
    first = torch.where(rel, a, torch.full_like(a, float("inf"))).min(1).values
    for j, k in enumerate(KS):
        inside = rel & (a < k)
        h = inside.sum(1).double()
        dcg = torch.where(inside, g / torch.log2(a + 2.0), torch.zeros_like(g)).sum(1)
        idcg = idisc[:, min(k, L) - 1].clamp(min=1e-300)
        ap = torch.where(inside, nth / (a + 1.0), torch.zeros_like(g)).sum(1)
        out[:, j] = torch.stack([dcg / idcg, ap / R, h / R, h / k, torch.where(first < k, 1.0 / (first + 1.0), torch.zeros_like(first)),
                                 (h > 0).double()], 1)
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ir_metrics_microbench needs the GPU")
    from contrastors_amd.retrieval_eval import METRICS, ir_metrics

    rows = []
    for name, M, per, ragged in SHAPES:
        row_ptr, ranks_h, gains_h = make(M, per, ragged)
        ranks, gains = torch.from_numpy(ranks_h).to(DEV), torch.from_numpy(gains_h).to(DEV)
        rp_dev = torch.from_numpy(row_ptr).to(DEV)
        lens_dev = rp_dev[1:] - rp_dev[:-1]
        L = int(np.diff(row_ptr).max())
        runs = {"ir_metrics": lambda: ir_metrics(ranks, gains, row_ptr, KS),
                "torch": lambda: torch_form(rp_dev, lens_dev, ranks, gains, L),
                "numpy": lambda: numpy_form(row_ptr, ranks, gains)}
        for fn in runs.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in runs}
        for _ in range(args.reps):                                       # alternate the forms
            for k, fn in runs.items():
                times[k].append(clock(fn))
        m = ir_metrics(ranks, gains, row_ptr, KS)
        got = torch.stack([m[n] for n in METRICS], -1)
        row = {"shape": name, "M": M, "nnz": int(ranks.numel()), "longest_row": L, "reps": args.reps,
               **{f"{k}_ms_median": round(statistics.median(v), 4) for k, v in times.items()},
               **{f"{k}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
               "max_abs_diff_vs_numpy": float((got.cpu() - torch.from_numpy(runs["numpy"]())).abs().max()),
               "max_abs_diff_vs_torch": float((got - runs["torch"]()).abs().max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
