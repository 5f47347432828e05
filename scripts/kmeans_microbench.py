"""Time the k-means kernels (csrc/kmeans.hip) at curation shapes and, in the same process on the same operands, what a user
would write without them.

    python scripts/kmeans_microbench.py [--reps 5] [--warmup 1] [--out FILE.json] [--N 4000000] [--shapes 4096x256,4096x768,65536x256,65536x768]

Operands: N unit-norm random points of width d (bf16), K centroids = K of the points.  Per (K, d), device-event timings after
warm-up, the forms alternating; median, p10 and p90 are reported:
  assign_ip         cx_kmeans_assign without a bias (spherical mode), the C call on device-resident arguments
  assign_l2         cx_kmeans_assign with half norms (Euclidean mode)
  search_k1         FlatIPIndex.search(points, 1) over the centroid table: the spherical assignment without the feature
  matmul_argmax     the Euclidean assignment in torch: bf16 matmul in row chunks of at most 2 GiB of fp32 scores, minus the half
                    norms, max + argmax
  update            _update_plan (torch: stable sort, searchsorted) + cx_kmeans_partial + cx_kmeans_finish, on the labels of
                    assign_l2; update_kernels is the two C calls alone on a prepared plan
  index_add         the update in torch: zeros(K, d).index_add_(0, labels, points.float()) in row chunks + bincount + a division
On the way the two assignments are compared with their torch forms (labels that differ are rows whose best two values lie within
fp32 rounding, or ties) and the two updates with each other.  One JSON line per shape."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"
CHUNK_BYTES = 2 << 30


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--N", type=int, default=4_000_000)
    ap.add_argument("--shapes", default="4096x256,4096x768,65536x256,65536x768")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kmeans_microbench needs the GPU")
    from contrastors_amd import _C
    from contrastors_amd.cluster import KMeans, _update_plan
    from contrastors_amd.search import FlatIPIndex

    h = _C.lib()
    N = args.N
    rows = []
    for K, d in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
        g = torch.Generator(device=DEV).manual_seed(1)
        X = torch.empty(N, d, dtype=torch.bfloat16, device=DEV)
        for r0 in range(0, N, 1 << 20):
            n = min(1 << 20, N - r0)
            X[r0: r0 + n] = torch.nn.functional.normalize(torch.randn(n, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
        pick = torch.randperm(N, device=DEV, generator=g)[:K]
        km_l2, km_ip = KMeans(K, d, device=DEV), KMeans(K, d, spherical=True, device=DEV)
        km_l2.set_centroids(X[pick].float())
        km_ip.set_centroids(X[pick].float())
        C, hn = km_l2._shadow, km_l2._half_norm
        ix = FlatIPIndex(d, device=DEV)
        ix.add(km_ip._shadow)
        stream = _C.cur_stream()
        labels = torch.empty(N, dtype=torch.int32, device=DEV)
        best = torch.empty(N, dtype=torch.float32, device=DEV)
        second = torch.empty(N, dtype=torch.float32, device=DEV)
        chunk = max(128, CHUNK_BYTES // (4 * K))
        t_lab = torch.empty(N, dtype=torch.int64, device=DEV)
        t_best = torch.empty(N, dtype=torch.float32, device=DEV)

        def assign(Cm, bias):
            return lambda: _C.check(h.cx_kmeans_assign(X.data_ptr(), Cm.data_ptr(), _C.ptr(bias), N, K, d, d, d, labels.data_ptr(),
                                                       best.data_ptr(), second.data_ptr(), stream))

        def matmul_argmax():
            for r0 in range(0, N, chunk):
                v = (X[r0: r0 + chunk] @ C.T).float() - hn[None, :]
                torch.max(v, 1, out=(t_best[r0: r0 + chunk], t_lab[r0: r0 + chunk]))

        # the update, on the Euclidean labels
        assign(C, hn)()
        torch.cuda.synchronize()
        lab_l2 = labels.clone()
        plan = _update_plan(lab_l2, K)
        mp = plan[1].numel()
        partial = torch.empty(mp, d, dtype=torch.float32, device=DEV)
        counts = torch.empty(K, dtype=torch.int32, device=DEV)
        cent, shadow, hn_out = km_l2.centroids.clone(), C.clone(), hn.clone()

        def update_kernels(p=plan):
            order, ps, pe, _, pp, npc = p
            _C.check(h.cx_kmeans_partial(X.data_ptr(), N, d, d, order.data_ptr(), ps.data_ptr(), pe.data_ptr(), npc.data_ptr(), mp,
                                         partial.data_ptr(), stream))
            _C.check(h.cx_kmeans_finish(partial.data_ptr(), ps.data_ptr(), pe.data_ptr(), pp.data_ptr(), K, d, mp, 0,
                                        counts.data_ptr(), cent.data_ptr(), shadow.data_ptr(), d, hn_out.data_ptr(), stream))

        t_cent = torch.empty(K, d, dtype=torch.float32, device=DEV)
        lab64 = lab_l2.long()

        def index_add():
            t_cent.zero_()
            for r0 in range(0, N, 1 << 20):
                t_cent.index_add_(0, lab64[r0: r0 + (1 << 20)], X[r0: r0 + (1 << 20)].float())
            t_cent.div_(torch.bincount(lab64, minlength=K).clamp_min(1)[:, None])

        runs = {
            "assign_ip": assign(km_ip._shadow, None),
            "assign_l2": assign(C, hn),
            "search_k1": lambda: ix.search(X, 1),
            "matmul_argmax": matmul_argmax,
            "update": lambda: update_kernels(_update_plan(lab_l2, K)),
            "update_kernels": update_kernels,
            "index_add": index_add,
        }
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):                      # alternate the forms
            for k, fn in runs.items():
                t = timed(fn)
                if rep >= args.warmup:
                    times[k].append(t)
        row = {"N": N, "K": K, "d": d, "reps": args.reps, "ms": {k: stats(v) for k, v in times.items()}}
        ms = {k: v["median"] for k, v in row["ms"].items()}
        row["tflops"] = {k: round(2.0 * N * K * d / (ms[k] * 1e-3) / 1e12, 1) for k in ("assign_ip", "assign_l2", "search_k1",
                                                                                       "matmul_argmax")}
        row["update_gather_TBps"] = round(N * d * 2 / (ms["update_kernels"] * 1e-3) / 1e12, 2)
        row["speedup"] = {"assign_ip_vs_search_k1": round(ms["search_k1"] / ms["assign_ip"], 2),
                          "assign_l2_vs_matmul_argmax": round(ms["matmul_argmax"] / ms["assign_l2"], 2),
                          "update_vs_index_add": round(ms["index_add"] / ms["update"], 2)}
        # checks at this scale on the way
        runs["assign_l2"]()
        matmul_argmax()
        differ = labels.long() != t_lab
        row["l2_labels_differing_from_torch"] = int(differ.sum())
        row["l2_differing_rows_outside_1e-3_gap"] = int((differ & ((best - second) > 1e-3)).sum())
        runs["assign_ip"]()
        s, i = ix.search(X, 1)
        row["ip_rows_differing_from_search_k1"] = int(((labels.long() != i[:, 0]) | (best != s[:, 0])).sum())
        update_kernels()
        index_add()
        live = counts > 0
        row["update_max_abs_diff_vs_index_add"] = float((cent - t_cent)[live].abs().max())
        row["clusters_nonempty"] = int(live.sum())
        row["largest_cluster"] = int(counts.max())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del X, ix, partial, runs, km_l2, km_ip, plan, t_cent, lab64, lab_l2
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
