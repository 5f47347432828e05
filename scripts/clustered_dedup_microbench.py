"""Time the cluster-scoped near-duplicate search against the exact self-join, in one process on the same rows.

    python scripts/clustered_dedup_microbench.py [--reps 5] [--warmup 1] [--out FILE.json] [--N 2000000] [--dims 768,64] [--K 2048]

Rows: N unit-norm random embeddings of width d; labels from ONE spherical k-means fit with K clusters (its time is reported
apart and is in none of the paths); threshold: the score above which ~1e-6 of a sample of pairs lie.  Three paths to the
duplicate pairs, each a whole host call ending in a device synchronise (host clock), alternated, medians after warm-up:
  a  dedup.duplicate_edges: the exact self-join in 8192-row batches (every pair; the yardstick)
  b  the same kernel on the label-sorted rows, in 8192-row batches against the corpus slice [batch start, end of the batch's
     last cluster), pairs with different labels dropped on the host
  c  dedup.clustered_duplicate_edges: one windowed self-join over the sorted rows
b and c both start from the labels (cluster_plan and the gather of the sorted rows are inside the timing) and must return
identical edges (checked; the run fails otherwise); a returns the pairs of all clusters.  Parts of c, timed apart in the same
rounds: c_plan (cluster_plan on the host), c_search (the windowed range_search over the already sorted rows: band description,
count, host read of the total, emit) and cx_range_window_count alone (device events), with TFLOP/s over the band's tiles.
Tiles (128 x 128 score tiles computed by the count pass), per path: `tiles` enumerates the walk of every query tile by the
kernels' own rule; `tiles_model` is the closed form of DESIGN.md 7k from N and the cluster sizes.  One JSON line per d."""
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
BATCH = 8192
T = 128


def stats(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, max(0, round(p * (len(v) - 1))))]
    return {"median": round(statistics.median(v), 3), "p10": round(q(0.1), 3), "p90": round(q(0.9), 3), "n": len(v)}


def host_timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def threshold_for(D, rate):
    S = (D[:2048].float() @ D[2048:2048 + 65536].float().T).reshape(-1)
    return float(torch.topk(S, max(1, round(rate * S.numel()))).values[-1])


def ceil_div(a, b):
    return -(-a // b)


def tiles_a(n):
    """Query tile i of the self-join walks corpus tiles i .. tiles_n - 1."""
    t = ceil_div(n, T)
    return t * (t + 1) // 2


def tiles_b(n, end):
    """Per 8192-row batch of sorted rows: the slice ends where the batch's last cluster ends; query tile j walks j .. its end."""
    total = 0
    for b0 in range(0, n, BATCH):
        b1 = min(n, b0 + BATCH)
        tn, tm = ceil_div(int(end[b1 - 1]) - b0, T), ceil_div(b1 - b0, T)
        total += tm * tn - tm * (tm - 1) // 2
    return total


def tiles_model(n, sizes):
    """a query tile's band reaches from its own tile to the end of the cluster of its last row, whose residual
    length is E[s^2] / (2 E[s]) rows on average; + 1 for its own tile, + 1/2 for the rounding up to a tile edge."""
    t = ceil_div(n, T)
    residual = float((sizes.astype(np.float64) ** 2).sum() / (2.0 * sizes.sum())) / T
    per_batch_tm = BATCH // T
    c = t * (1.5 + residual)
    b = t * (1.5 + residual + per_batch_tm - (per_batch_tm - 1) / 2.0 - 1.0)
    return {"a": tiles_a(n), "b": round(b), "c": round(c)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--N", type=int, default=2_000_000)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--dims", default="768,64")
    ap.add_argument("--fit_sample", type=int, default=262144)
    ap.add_argument("--fit_iters", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clustered_dedup_microbench needs the GPU")
    from contrastors_amd import _C
    from contrastors_amd.cluster import KMeans
    from contrastors_amd.dedup import cluster_plan, clustered_duplicate_edges, duplicate_edges
    from contrastors_amd.search import FlatIPIndex, window_band

    h = _C.lib()
    n = args.N
    rows = []
    for d in (int(x) for x in args.dims.split(",")):
        g = torch.Generator(device=DEV).manual_seed(1)
        ix = FlatIPIndex(d, device=DEV)
        ix.reserve(n)
        for b0 in range(0, n, 1 << 18):
            ix.add(torch.nn.functional.normalize(torch.randn(min(1 << 18, n - b0), d, device=DEV, generator=g), dim=1))
        D = ix.vectors
        thr = threshold_for(D, 1e-6)
        km = KMeans(args.K, d, spherical=True, device=DEV, seed=0)
        fit_ms, _ = host_timed(lambda: km.fit(D, max_iter=args.fit_iters, sample=args.fit_sample))
        labels = km.labels_.cpu().numpy().astype(np.int64)
        sizes = np.bincount(labels, minlength=args.K)
        order, end, chunks = cluster_plan(labels, 1 << 22)
        assert len(chunks) == 1, "the parts of c are timed on one chunk: N <= 2^22"
        # the sorted rows, for the timings of c's parts (b and c gather their own copies: that is part of their cost)
        sorted_ix = FlatIPIndex(d, device=DEV)
        sorted_ix.add(D[torch.from_numpy(order).to(DEV)])
        Ds = sorted_ix.vectors
        view = FlatIPIndex(d, device=DEV)      # a window onto rows b0 : e of b's sorted copy: no further copy

        def path_a():
            return duplicate_edges(ix, thr, BATCH, 1 << 30)

        def path_b():
            order, end, _ = cluster_plan(labels, 1 << 22)
            Ds = D[torch.from_numpy(order).to(DEV)]
            lab_sorted = labels[order]
            src, dst, score = [], [], []
            for b0 in range(0, n, BATCH):
                b1 = min(n, b0 + BATCH)
                e = int(end[b1 - 1])
                view._store, view.ntotal = Ds[b0:e], e - b0
                pos = torch.arange(b1 - b0, dtype=torch.int64, device=DEV)
                lims, s, ids = view.range_search(Ds[b0:b1], thr, min_id=pos, max_results=1 << 30)
                if ids.numel():
                    a = b0 + torch.repeat_interleave(pos, lims[1:] - lims[:-1]).cpu().numpy()
                    b = b0 + ids.cpu().numpy()
                    keep = lab_sorted[a] == lab_sorted[b]                      # the host filter by label
                    src.append(order[a[keep]])
                    dst.append(order[b[keep]])
                    score.append(s.cpu().numpy()[keep])
            if not src:
                return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
            src, dst, score = np.concatenate(src), np.concatenate(dst), np.concatenate(score)
            by = np.lexsort((dst, src))
            return src[by], dst[by], score[by]

        def path_c():
            return clustered_duplicate_edges(D, labels, thr, 1 << 22, 1 << 30, DEV)

        # cx_range_window_count alone over the first chunk of sorted rows
        c0, c1 = chunks[0]
        m = c1 - c0
        pos = torch.arange(m, dtype=torch.int64, device=DEV)
        end_dev = torch.from_numpy(end[c0:c1] - c0).to(DEV)
        band = window_band(pos, end_dev, m, m)
        ptr = torch.zeros(band.numel() + 1, dtype=torch.int64, device=DEV)
        ptr[1:] = torch.cumsum(band, 0)
        band_tiles = int(ptr[-1])
        ws = torch.empty(h.cx_range_window_ws_bytes(m, m, band_tiles, 0), dtype=torch.uint8, device=DEV)
        rad = torch.full((m,), thr, dtype=torch.float32, device=DEV)
        counts = torch.empty(m, dtype=torch.int64, device=DEV)
        stream = _C.cur_stream()

        def count_alone():
            _C.check(h.cx_range_window_count(Ds[c0].data_ptr(), Ds[c0].data_ptr(), m, m, d, d, d, rad.data_ptr(), pos.data_ptr(),
                                             end_dev.data_ptr(), ptr.data_ptr(), band_tiles, 0, ws.data_ptr(), counts.data_ptr(),
                                             stream), "cx_range_window_count")

        def c_search():
            return sorted_ix.range_search(Ds, thr, min_id=pos, end_id=end_dev, max_results=1 << 30)

        paths = {"a": path_a, "b": path_b, "c": path_c, "c_plan": lambda: cluster_plan(labels, 1 << 22), "c_search": c_search}
        times = {k: [] for k in (*paths, "window_count")}
        edges = {}
        for rep in range(args.warmup + args.reps):                      # alternate the paths
            for k, fn in paths.items():
                t, out = host_timed(fn)
                edges[k] = out
                if rep >= args.warmup:
                    times[k].append(t)
            t = event_timed(count_alone)
            if rep >= args.warmup:
                times["window_count"].append(t)
        identical = all(np.array_equal(x, y) for x, y in zip(edges["b"], edges["c"])) and \
            np.array_equal(edges["b"][2].view(np.int32), edges["c"][2].view(np.int32))
        same_label = labels[edges["a"][0]] == labels[edges["a"][1]]
        a_within = tuple(x[same_label] for x in edges["a"])
        identical_a = all(np.array_equal(x, y) for x, y in zip(a_within, edges["c"]))
        ms = {k: stats(v) for k, v in times.items()}
        tiles = {"a": tiles_a(n), "b": tiles_b(n, end),
                 "c": int(sum(int(window_band(torch.arange(b1 - b0), torch.from_numpy(end[b0:b1] - b0), b1 - b0, b1 - b0).sum())
                              for b0, b1 in chunks))}
        row = {"N": n, "d": d, "K": args.K, "reps": args.reps, "threshold": thr, "kmeans_fit_ms": round(fit_ms, 1),
               "fit_sample": args.fit_sample, "fit_iters": args.fit_iters,
               "cluster_rows": {"min": int(sizes.min()), "mean": float(sizes.mean()), "max": int(sizes.max()),
                                "size_biased_mean": float((sizes.astype(np.float64) ** 2).sum() / sizes.sum())},
               "ms": ms, "tiles": tiles, "tiles_model": tiles_model(n, sizes),
               "edges": {k: int(edges[k][0].size) for k in "abc"}, "edges_a_within_clusters": int(same_label.sum()),
               "b_and_c_identical": bool(identical), "c_equals_a_within_clusters": bool(identical_a),
               "edge_recall_of_c": round(edges["c"][0].size / max(1, edges["a"][0].size), 4),
               "a_over_c": round(ms["a"]["median"] / ms["c"]["median"], 2),
               "b_over_c": round(ms["b"]["median"] / ms["c"]["median"], 3),
               "a_spread_p10_p90_ms": round(ms["a"]["p90"] - ms["a"]["p10"], 3),
               "window_count_band_tiles": band_tiles,
               "window_count_tflops": round(band_tiles * 2.0 * T * T * d / (ms["window_count"]["median"] * 1e-3) / 1e12, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not identical:
            sys.exit("paths b and c returned different edges")
        del D, Ds, ix, sorted_ix, view, ws, km, edges
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
