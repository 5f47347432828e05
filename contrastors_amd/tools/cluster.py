"""k-means over an embedding file (contrastors_amd.cluster): labels for every row, optionally the centroids and an evaluation.

--embeddings X.npy (n, d) is memory-mapped; the centroids are fitted on all rows, or on --sample of them (a seeded subsample),
and every row is then labelled in streamed batches, so the file may be larger than the device.  --spherical clusters by cosine
(the fitted rows are L2-normalised; the arg-max of a row does not depend on its norm).  Written: --out labels.npy (n,) int32
and, with --centroids_out, the (k, d) float32 centroids.  One JSON line reports n, k, the objective, iterations and convergence;
with --labels Y.npy (n,) true classes a second line holds the clustering evaluation of these labels: v_measure, homogeneity,
completeness, k, n.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

from ._common import load_npy


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m contrastors_amd.tools.cluster", description=__doc__.split("\n\n")[0],
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--embeddings", required=True, help=".npy, (n, d)")
    ap.add_argument("--k", type=int, required=True, help="number of clusters")
    ap.add_argument("--out", required=True, help="labels .npy, (n,) int32")
    ap.add_argument("--centroids_out", help="centroids .npy, (k, d) float32")
    ap.add_argument("--spherical", action="store_true", help="cosine k-means with unit-norm centroids")
    ap.add_argument("--sample", type=int, default=None, help="fit on this many rows (seeded subsample); all rows are labelled")
    ap.add_argument("--n_init", type=int, default=1, help="restarts; the best objective is kept")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--labels", help="true classes .npy (n,): print the clustering evaluation of the labels as JSON")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.k < 1 or args.n_init < 1:
        ap.error("--k and --n_init must be positive")
    if args.sample is not None and args.sample < 1:
        ap.error("--sample must be positive")
    for name in ("embeddings", "labels"):
        if getattr(args, name) and not Path(getattr(args, name)).exists():
            ap.error(f"--{name} {getattr(args, name)} does not exist")
    x = load_npy(args.embeddings, None, "input", mmap=True)
    n, d = x.shape
    if args.k > (n if args.sample is None else min(n, args.sample)):
        ap.error(f"--k {args.k} exceeds the {n if args.sample is None else min(n, args.sample)} rows that are fitted")
    y = None
    if args.labels:
        y = np.load(args.labels)
        if y.ndim != 1 or y.shape[0] != n:
            ap.error(f"--labels {args.labels} has shape {y.shape}, expected ({n},)")
    import torch

    from ..cluster import KMeans, v_measure

    km = KMeans(args.k, d, spherical=args.spherical, device=args.device, seed=args.seed)   # (refuses a CPU device, a bad width)
    if args.sample is not None and args.sample < n:
        g = torch.Generator().manual_seed(args.seed)
        rows = np.sort(torch.randperm(n, generator=g)[: args.sample].numpy())
        xs = np.asarray(x[rows], dtype=np.float32)
    else:
        xs = np.array(x, dtype=np.float32)          # (a copy: the map is read-only)
    if args.spherical:
        xs = xs / np.maximum(np.linalg.norm(xs, axis=1, keepdims=True), 1e-12)
    km.fit(torch.from_numpy(xs), n_init=args.n_init)
    labels = km.assign(x)[0]
    np.save(args.out, labels)
    if args.centroids_out:
        np.save(args.centroids_out, km.centroids.cpu().numpy())
    print(json.dumps({"n": int(n), "k": args.k, "objective": km.objective_, "n_iter": km.n_iter_, "converged": km.converged_}))
    if y is not None:
        hom, com, v = v_measure(y, labels)
        print(json.dumps({"v_measure": v, "homogeneity": hom, "completeness": com, "k": args.k, "n": int(n)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
