"""Time the range search (csrc/range.hip) and, in the same process on the same operands, the kernels it is measured against.

    python scripts/range_search_microbench.py [--reps 7] [--warmup 2] [--out FILE.json] [--M 8192] [--N 2000000] [--dims 768,64]

Operands: unit-norm random embeddings, M queries x N corpus x d (the other microbenches' shape).  Per d and per hit rate
(0, ~1e-6, ~1e-3 of the M x N pairs; the radius is the matching quantile of a sample of scores, the achieved rate is reported):
  count        cx_range_count (count walk + sum), the C call on device-resident arguments
  emit         cx_range_emit alone, after that count
  search       FlatIPIndex.range_search, the whole call: count, the host's read of the total, allocation, emit
  selfjoin_*   cx_range_count of M consecutive corpus rows with min_id = their own ids, at the start, the middle and the end of
               the corpus (all, half, none of the corpus tiles lie above the rows); their mean over `count` of the same rows
               without min_id is the cost of a whole self-join relative to the full join
and per d, with one random target per row: cx_rank_targets (gather + count walk + sum), the same call against a 128-row
corpus (the gather and the launches without the walk; subtracted, it leaves the count walk), cx_search_topk at k = 1.
Times are device-event timings after warm-up, the forms alternating; median, p10 and p90 are reported.  On the way the counts
are checked against the top-1 scores at this scale (a row has a result iff its best score is above the radius).  One JSON line
per d."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"
RATES = (0.0, 1e-6, 1e-3)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, max(0, round(p * (len(v) - 1))))]
    return {"median": round(statistics.median(v), 3), "p10": round(q(0.1), 3), "p90": round(q(0.9), 3), "n": len(v)}


def radius_for(Q, D, rate):
    """The score above which `rate` of a (512 x 65536) sample of pairs lie (rate 0: above every possible score)."""
    if rate == 0.0:
        return 2.0
    S = (Q[:512].float() @ D[:65536].float().T).reshape(-1)
    k = max(1, round(rate * S.numel()))
    return float(torch.topk(S, k).values[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--M", type=int, default=8192)
    ap.add_argument("--N", type=int, default=2_000_000)
    ap.add_argument("--dims", default="768,64")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("range_search_microbench needs the GPU")
    from contrastors_amd import _C
    from contrastors_amd.search import FlatIPIndex

    h = _C.lib()
    M, N = args.M, args.N
    rows = []
    for d in (int(x) for x in args.dims.split(",")):
        g = torch.Generator(device=DEV).manual_seed(1)
        Q = torch.nn.functional.normalize(torch.randn(M, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
        D = torch.nn.functional.normalize(torch.randn(N, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
        ix = FlatIPIndex(d, device=DEV, workspace_bytes=1 << 34)     # one query batch
        ix.add(D)
        del D
        D = ix.vectors
        stream = _C.cur_stream()
        ws = torch.empty(h.cx_range_ws_bytes(M, N, 0), dtype=torch.uint8, device=DEV)
        counts = torch.empty(M, dtype=torch.int64, device=DEV)
        runs, after = {}, {}
        radii = {rate: radius_for(Q, D, rate) for rate in RATES}
        keep = []                                                       # tensors the closures point into

        def range_args(q, rad, mid):
            return (q.data_ptr(), D.data_ptr(), M, N, d, d, d, rad.data_ptr(), None if mid is None else mid.data_ptr(), 0,
                    ws.data_ptr())

        achieved = {}
        for rate in RATES:
            rad = torch.full((M,), radii[rate], dtype=torch.float32, device=DEV)
            keep.append(rad)
            a = range_args(Q, rad, None)
            tag = f"rate{rate:g}"
            runs[f"count_{tag}"] = lambda a=a: _C.check(h.cx_range_count(*a, counts.data_ptr(), stream))
            runs[f"search_{tag}"] = lambda rad=rad: ix.range_search(Q, rad, max_results=1 << 30)
            # emit alone: the workspace must be this rate's, so every timing re-runs the count first, outside the events
            _C.check(h.cx_range_count(*a, counts.data_ptr(), stream))
            lims = torch.zeros(M + 1, dtype=torch.int64, device=DEV)
            torch.cumsum(counts, 0, out=lims[1:])
            nnz = int(lims[-1])
            achieved[tag] = nnz / (M * N)
            if nnz:
                out_s = torch.empty(nnz, dtype=torch.float32, device=DEV)
                out_i = torch.empty(nnz, dtype=torch.int64, device=DEV)
                keep += [lims, out_s, out_i]
                runs[f"emit_{tag}"] = lambda a=a, lims=lims, s=out_s, i=out_i: \
                    _C.check(h.cx_range_emit(*a, lims.data_ptr(), s.data_ptr(), i.data_ptr(), stream))
                after[f"emit_{tag}"] = f"count_{tag}"
        # self-join batches: M consecutive corpus rows, with and without min_id
        rad = torch.full((M,), radii[1e-6], dtype=torch.float32, device=DEV)
        keep.append(rad)
        for name, b0 in (("start", 0), ("middle", (N - M) // 2 // 128 * 128), ("end", N - M)):
            mid = torch.arange(b0, b0 + M, dtype=torch.int64, device=DEV)
            keep.append(mid)
            runs[f"selfjoin_{name}"] = lambda a=range_args(D[b0:], rad, mid): _C.check(h.cx_range_count(*a, counts.data_ptr(), stream))
            runs[f"fulljoin_{name}"] = lambda a=range_args(D[b0:], rad, None): _C.check(h.cx_range_count(*a, counts.data_ptr(), stream))
        # the kernels it is measured against: one target per row
        tptr = torch.arange(M + 1, dtype=torch.int64, device=DEV)
        tids = torch.randint(0, N, (M,), device=DEV, generator=g)
        rws = torch.empty(h.cx_rank_ws_bytes(M, N, M, 0), dtype=torch.uint8, device=DEV)
        ranks = torch.empty(M, dtype=torch.int32, device=DEV)
        rscores = torch.empty(M, dtype=torch.float32, device=DEV)
        tids_small = tids % 128

        def rank_call(n, ids):
            return lambda: _C.check(h.cx_rank_targets(Q.data_ptr(), D.data_ptr(), M, n, d, d, d, tptr.data_ptr(), ids.data_ptr(), 0,
                                                      rws.data_ptr(), ranks.data_ptr(), rscores.data_ptr(), stream))

        runs["rank_targets"] = rank_call(N, tids)
        runs["rank_targets_128_row_corpus"] = rank_call(128, tids_small)
        sws = torch.empty(h.cx_search_ws_bytes(M, N, 1, 0), dtype=torch.uint8, device=DEV)
        top_s = torch.empty(M, 1, dtype=torch.float32, device=DEV)
        top_i = torch.empty(M, 1, dtype=torch.int64, device=DEV)
        runs["search_topk_k1"] = lambda: _C.check(h.cx_search_topk(Q.data_ptr(), D.data_ptr(), M, N, d, d, d, 1, None, None, None, 0,
                                                                   sws.data_ptr(), top_s.data_ptr(), top_i.data_ptr(), stream))
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):                      # alternate the forms
            for k, fn in runs.items():
                if k in after:
                    runs[after[k]]()
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
        row = {"M": M, "N": N, "d": d, "reps": args.reps, "radius": {f"rate{r:g}": radii[r] for r in RATES},
               "achieved_hit_rate": achieved, "ms": {k: stats(v) for k, v in times.items()}}
        ms = {k: v["median"] for k, v in row["ms"].items()}
        row["rank_count_walk_ms"] = round(ms["rank_targets"] - ms["rank_targets_128_row_corpus"], 3)
        row["rank_spread_p10_p90_ms"] = round(row["ms"]["rank_targets"]["p90"] - row["ms"]["rank_targets"]["p10"], 3)
        row["count_minus_rank_walk_ms"] = {k[6:]: round(ms[k] - row["rank_count_walk_ms"], 3) for k in ms if k.startswith("count_")}
        row["tflops_count"] = {k[6:]: round(2.0 * M * N * d / (ms[k] * 1e-3) / 1e12, 1) for k in ms if k.startswith("count_")}
        row["selfjoin_over_fulljoin"] = round(sum(ms[f"selfjoin_{n}"] for n in ("start", "middle", "end"))
                                              / sum(ms[f"fulljoin_{n}"] for n in ("start", "middle", "end")), 3)
        # a check at this scale on the way: a row has a result above the radius iff its top-1 score is above it (same bits)
        runs["count_rate1e-06"]()
        runs["search_topk_k1"]()
        torch.cuda.synchronize()
        row["rows_where_count_disagrees_with_top1"] = int(((counts > 0) != (top_s[:, 0] > radii[1e-6])).sum())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del Q, D, ix, ws, rws, sws, keep, runs
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
