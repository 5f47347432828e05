"""Time IVFFlatIndex.search against the exact search, in one process on the same rows, and count the tiles it walks.

    python scripts/ivf_search_microbench.py [--reps 5] [--warmup 1] [--out FILE.json] [--N 4000000] [--dims 768,64] [--M 8192]
                                            [--k 100] [--nlists 1024,4096] [--nprobes 1,8,32,128]

Rows: a planted mixture -- `--centres` unit-norm centres, a row is normalise(centre + noise * g), g standard normal scaled to
unit expected norm -- because random rows have no list structure.  Queries are fresh draws from the same
mixture.  Per (d, nlist): one spherical k-means fit on a sample (its time, the add and the sort are reported apart), then per
nprobe, alternating in every round after the warm-up and timed with device events (medians, p10 / p90):
  exact    FlatIPIndex.search of all rows (the parent's path)
  ivf      IVFFlatIndex.search, the whole host call
  and the parts of ivf, each run on what the part before it produced: coarse (the centroid search), plan (ivf_pair_plan and the
  gather of the pair rows' queries), window (cx_search_window_topk alone), merge (cx_topk_merge_lists alone).
Tiles: `tiles` enumerates the corpus tiles every 128-pair tile walks by the kernel's own rule (search.window_band);
`tiles_model` is the closed form  pair_tiles * (1 + lists_per_pair_tile * mean_list_tiles)  with lists_per_pair_tile =
1 + 127 * nlist / P (P = M * nprobe pair rows spread evenly over the lists) and mean_list_tiles = N / nlist / 128;
`tiles_useful` = the scores needed / 128^2 (sum over pair rows of their list's rows), so `waste` = tiles / tiles_useful is
what tile granularity costs -- large when a list is probed by fewer than 128 queries (`pairs_per_list` < 128).
`tiles_exact` = ceil(M / 128) * ceil(N / 128).  recall@k is against the exact result of the same run.  One JSON line per
(d, nlist, nprobe)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"
T = 128


def stats(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, max(0, round(p * (len(v) - 1))))]
    return {"median": round(statistics.median(v), 3), "p10": round(q(0.1), 3), "p90": round(q(0.9), 3), "n": len(v)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def mixture(n, d, centres, noise, g):
    """n rows of the planted mixture, (n, d) fp32 unit norm, in chunks."""
    out = torch.empty(n, d, device=DEV)
    for b0 in range(0, n, 1 << 18):
        m = min(1 << 18, n - b0)
        which = torch.randint(0, centres.shape[0], (m,), device=DEV, generator=g)
        x = centres[which] + noise / d ** 0.5 * torch.randn(m, d, device=DEV, generator=g)
        out[b0: b0 + m] = torch.nn.functional.normalize(x, dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--N", type=int, default=4_000_000)
    ap.add_argument("--M", type=int, default=8192)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--dims", default="768,64")
    ap.add_argument("--nlists", default="1024,4096")
    ap.add_argument("--nprobes", default="1,8,32,128")
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--fit_sample", type=int, default=262144)
    ap.add_argument("--fit_iters", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ivf_search_microbench needs the GPU")
    from contrastors_amd import _C
    from contrastors_amd.search import FlatIPIndex, IVFFlatIndex, ivf_pair_plan, window_band

    h = _C.lib()
    N, M, k = args.N, args.M, args.k
    rows = []
    for d in (int(x) for x in args.dims.split(",")):
        g = torch.Generator(device=DEV).manual_seed(1)
        centres = torch.nn.functional.normalize(torch.randn(args.centres, d, device=DEV, generator=g), dim=1)
        D = mixture(N, d, centres, args.noise, g).to(torch.bfloat16)
        Q = mixture(M, d, centres, args.noise, g).to(torch.bfloat16)
        flat = FlatIPIndex(d, device=DEV)
        flat.add(D)
        for nlist in (int(x) for x in args.nlists.split(",")):
            ivf = IVFFlatIndex(d, nlist, device=DEV, workspace_bytes=8 << 30)
            fit_ms, _ = event_timed(lambda: ivf.train(D, max_iter=args.fit_iters, sample=args.fit_sample))
            add_ms, _ = event_timed(lambda: ivf.add(D))
            sort_ms, sizes = event_timed(lambda: ivf.list_sizes)
            sizes = sizes.double()
            stream = _C.cur_stream()
            for nprobe in (int(x) for x in args.nprobes.split(",")):
                if nprobe > min(nlist, 256):
                    continue
                P = M * nprobe
                assert ivf.batch_queries(M, k, nprobe) == M, "the parts are timed on one batch"
                ws = torch.empty(h.cx_search_window_ws_bytes(P, k), dtype=torch.uint8, device=DEV)
                ls = torch.empty(P, k, dtype=torch.float32, device=DEV)
                li = torch.empty(P, k, dtype=torch.int64, device=DEV)
                out_s = torch.empty(M, k, dtype=torch.float32, device=DEV)
                out_i = torch.empty(M, k, dtype=torch.int64, device=DEV)
                state = {}

                def coarse():
                    state["probes"] = ivf._coarse.search(Q, nprobe)[1]

                def plan():
                    pair_q, mid, end, src = ivf_pair_plan(state["probes"], ivf._list_ptr)
                    state.update(mid=mid, end=end, src=src, qg=Q[pair_q])

                def window():
                    _C.check(h.cx_search_window_topk(state["qg"].data_ptr(), ivf._rows.data_ptr(), P, N, d, d, d, k,
                                                     state["mid"].data_ptr(), state["end"].data_ptr(), None, None, None,
                                                     ws.data_ptr(), ls.data_ptr(), li.data_ptr(), stream), "cx_search_window_topk")

                def merge():
                    _C.check(h.cx_topk_merge_lists(ls.data_ptr(), li.data_ptr(), P, k, state["src"].data_ptr(), M, nprobe,
                                                   ivf._order.data_ptr(), N, out_s.data_ptr(), out_i.data_ptr(), stream),
                             "cx_topk_merge_lists")

                paths = {"exact": lambda: flat.search(Q, k), "ivf": lambda: ivf.search(Q, k, nprobe), "coarse": coarse,
                         "plan": plan, "window": window, "merge": merge}
                times = {name: [] for name in paths}
                res = {}
                for rep in range(args.warmup + args.reps):                      # alternate the paths
                    for name, fn in paths.items():
                        t, res[name] = event_timed(fn)
                        if rep >= args.warmup:
                            times[name].append(t)
                parts_equal = torch.equal(out_s, res["ivf"][0]) and torch.equal(out_i, res["ivf"][1])
                ei, ii = res["exact"][1], res["ivf"][1]
                hits = (ii[:, :, None] == ei[:, None, :]).any(2) & (ii >= 0)
                recall = float(hits.sum()) / float((ei >= 0).sum())
                tiles = int(window_band(state["mid"], state["end"], P, N).sum())
                useful = float((state["end"] - state["mid"] - 1).clamp(min=0).sum()) / (T * T)
                pair_tiles = -(-P // T)
                model = pair_tiles * (1 + (1 + 127.0 * nlist / P) * (N / nlist / T))
                ms = {name: stats(v) for name, v in times.items()}
                spread = max(ms["exact"]["p90"] - ms["exact"]["p10"], ms["ivf"]["p90"] - ms["ivf"]["p10"])
                row = {"N": N, "d": d, "M": M, "k": k, "nlist": nlist, "nprobe": nprobe, "reps": args.reps,
                       "centres": args.centres, "noise": args.noise, "fit_ms": round(fit_ms, 1), "add_ms": round(add_ms, 1),
                       "sort_ms": round(sort_ms, 1), "fit_sample": args.fit_sample, "fit_iters": args.fit_iters,
                       "list_rows": {"min": int(sizes.min()), "mean": float(sizes.mean()), "max": int(sizes.max()),
                                     "size_biased_mean": float((sizes ** 2).sum() / sizes.sum())},
                       "ms": ms, "exact_over_ivf": round(ms["exact"]["median"] / ms["ivf"]["median"], 2),
                       "faster_by_more_than_the_spread": bool(ms["exact"]["median"] - ms["ivf"]["median"] > spread),
                       "spread_p10_p90_ms": round(spread, 3), "parts_equal_search": bool(parts_equal),
                       "recall_at_k": round(recall, 4), "pairs_per_list": round(P / nlist, 2),
                       "tiles": tiles, "tiles_model": round(model), "tiles_useful": round(useful, 1),
                       "waste": round(tiles / max(useful, 1e-9), 2), "tiles_exact": -(-M // T) * -(-N // T),
                       "window_tflops": round(tiles * 2.0 * T * T * d / (ms["window"]["median"] * 1e-3) / 1e12, 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not parts_equal:
                    sys.exit("the timed parts and IVFFlatIndex.search returned different results")
                del ws, ls, li, state
            del ivf
            torch.cuda.empty_cache()
        del D, Q, flat
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
