"""Near-duplicate removal and decontamination of a corpus on the exact range search (contrastors_amd.dedup).

Every pair of rows with cosine above --threshold is found (all of them: a duplicate cluster of any size comes back whole),
grouped, and one row per group is kept: --rule components keeps the lowest row id of every connected component, --rule
greedy scans the rows in order and drops a row iff an already kept earlier row is its neighbour.  With --against EVAL.npy,
rows that score above --against_threshold with any evaluation row are dropped as well (decontamination).
Embeddings: --embeddings X.npy (row i = record i), or --dataset records (.jsonl / .jsonl.gz / a shard directory) whose
--key field is encoded with --model and --tokenizer (local); both may be given: the .npy then stands for the encoder.
Embeddings are L2-normalised before indexing unless --no_normalize is given.
Cluster-scoped search, for corpora past what the all-pairs join can serve: with --clusters K (k-means fitted on the indexed
rows, spherical unless --no_normalize) or --cluster_labels L.npy (any partition: source, language, shard) only pairs inside a
part are sought, --chunk_rows sorted rows per windowed self-join; --recall_sample R measures on R rows which share of the exact
pairs that kept.  Written to --output_dir:
  kept.npy         bool mask over the rows
  duplicates.json  {component label (its lowest row id): [member row ids]} for components larger than 1
  report.json      n, edges, components, kept, contaminated, threshold(s), rule; cluster-scoped runs add clusters,
                   largest_cluster, edge_recall (null without --recall_sample), edge_recall_rows
  cluster_labels.npy  the fitted labels (--clusters)
and, with --dataset, the kept records as shard-%05d.jsonl.gz with counts.json / offsets.json.gz.
"""
from __future__ import annotations

import argparse
import gzip
import json
import sys
from pathlib import Path

import numpy as np

from ._common import encode_texts, load_npy, write_shards


def _records(path):
    path = Path(path)
    files = sorted(path.glob("shard-*.jsonl.gz")) if path.is_dir() else [path]
    for file in files:
        with (gzip.open if file.suffix == ".gz" else open)(file, "rt") as f:
            for line in f:
                yield json.loads(line)


def _normalized(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m contrastors_amd.tools.dedup", description=__doc__.split("\n\n")[0],
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--embeddings", help=".npy, one row per record")
    ap.add_argument("--dataset", help="records: a shard directory or a .jsonl(.gz) file; the kept ones are written out")
    ap.add_argument("--key", default="document", help="record field that is embedded")
    ap.add_argument("--model", help="local BiEncoder checkpoint directory (when no .npy is given)")
    ap.add_argument("--tokenizer", help="local tokenizer directory")
    ap.add_argument("--prefix", default="")
    ap.add_argument("--threshold", type=float, required=True, help="pairs with cosine strictly above it are duplicates")
    ap.add_argument("--rule", choices=("components", "greedy"), default="components")
    ap.add_argument("--against", help=".npy of evaluation embeddings to decontaminate against")
    ap.add_argument("--against_threshold", type=float, default=None, help="default: --threshold")
    ap.add_argument("--no_normalize", action="store_true", help="index the embeddings as they are (inner product)")
    ap.add_argument("--max_edges", type=int, default=1 << 27, help="refuse more duplicate pairs than this")
    ap.add_argument("--batch_rows", type=int, default=8192, help="query rows per range search")
    ap.add_argument("--clusters", type=int, default=None, help="fit k-means with this many clusters; search inside them only")
    ap.add_argument("--cluster_sample", type=int, default=None, help="fit on this many rows (a seeded subsample)")
    ap.add_argument("--cluster_iters", type=int, default=25)
    ap.add_argument("--cluster_seed", type=int, default=0)
    ap.add_argument("--cluster_labels", help=".npy of one integer label per row: a given partition instead of --clusters")
    ap.add_argument("--chunk_rows", type=int, default=1 << 22, help="sorted rows per windowed self-join (whole clusters)")
    ap.add_argument("--recall_sample", type=int, default=None, help="rows on which the recall of the exact pairs is measured")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--max_length", type=int, default=512)
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.embeddings is None and args.dataset is None:
        ap.error("give --embeddings, --dataset, or both")
    if args.embeddings is None and not (args.model and args.tokenizer):
        ap.error("without --embeddings, --model and --tokenizer are required")
    if args.max_edges < 1 or args.batch_rows < 1:
        ap.error("--max_edges and --batch_rows must be positive")
    if args.against_threshold is not None and args.against is None:
        ap.error("--against_threshold goes with --against")
    if args.clusters is not None and args.cluster_labels is not None:
        ap.error("--clusters and --cluster_labels are mutually exclusive")
    if args.clusters is not None and args.clusters < 1:
        ap.error("--clusters must be at least 1")
    if args.chunk_rows < 1 or args.cluster_iters < 1 or (args.cluster_sample is not None and args.cluster_sample < 1):
        ap.error("--chunk_rows, --cluster_iters and --cluster_sample must be positive")
    scoped = args.clusters is not None or args.cluster_labels is not None
    if args.recall_sample is not None and (not scoped or args.recall_sample < 1):
        ap.error("--recall_sample takes a positive number and goes with --clusters or --cluster_labels")
    for name in ("embeddings", "dataset", "against", "cluster_labels"):
        if getattr(args, name) and not Path(getattr(args, name)).exists():
            ap.error(f"--{name} {getattr(args, name)} does not exist")
    import torch

    from ..dedup import clustered_duplicate_edges, components, contaminated, duplicate_edges, edge_recall, select_kept
    from ..search import FlatIPIndex

    recs = list(_records(args.dataset)) if args.dataset else None
    if args.embeddings:
        x = np.load(args.embeddings) if recs is None else load_npy(args.embeddings, len(recs), args.key)
        if x.ndim != 2:
            ap.error(f"--embeddings {args.embeddings} has shape {x.shape}, expected (n, d)")
    else:
        x = encode_texts([r[args.key] for r in recs], args.model, args.tokenizer, args.batch_size, args.max_length,
                         args.device, args.prefix).cpu().numpy()
    x = np.asarray(x, dtype=np.float32) if args.no_normalize else _normalized(x)
    n, d = x.shape
    part, fitted = None, False
    if args.cluster_labels:                          # (checked before anything touches the GPU)
        part = np.load(args.cluster_labels)
        if part.shape != (n,) or part.dtype.kind not in "iu":
            ap.error(f"--cluster_labels {args.cluster_labels} has shape {part.shape} and dtype {part.dtype}, expected {n} integers")
    elif args.clusters is not None and args.clusters > n:
        ap.error(f"--clusters {args.clusters} for {n} rows")
    index = FlatIPIndex(d, device=args.device)       # (refuses a CPU device and an unsupported width)
    index.add(torch.from_numpy(x))
    out = Path(args.output_dir)
    if args.clusters is not None:
        from ..cluster import KMeans

        km = KMeans(args.clusters, d, spherical=not args.no_normalize, device=args.device, seed=args.cluster_seed)
        km.fit(index.vectors, max_iter=args.cluster_iters, sample=args.cluster_sample)
        part, fitted = km.labels_.cpu().numpy().astype(np.int64), True      # (fit labels every row, sampled or not)
    if part is None:
        src, dst, _ = duplicate_edges(index, args.threshold, args.batch_rows, args.max_edges)
    else:
        src, dst, _ = clustered_duplicate_edges(index.vectors, part, args.threshold, args.chunk_rows, args.max_edges,
                                                args.device)
    labels = components(n, src, dst)
    kept = select_kept(n, src, dst, args.rule)
    n_dup_dropped = int(n - kept.sum())
    leak = np.zeros(n, dtype=bool)
    t2 = None
    if args.against:
        t2 = args.threshold if args.against_threshold is None else args.against_threshold
        e = np.load(args.against)
        if e.ndim != 2 or e.shape[1] != d:
            ap.error(f"--against {args.against} has shape {e.shape}, expected (m, {d})")
        ev = FlatIPIndex(d, device=args.device)
        ev.add(torch.from_numpy(np.asarray(e, dtype=np.float32) if args.no_normalize else _normalized(e)))
        leak = contaminated(x, ev, t2)
        kept &= ~leak
    members = {}
    order = np.argsort(labels, kind="stable")
    sizes = np.bincount(labels, minlength=n)
    for i in order[sizes[labels[order]] > 1].tolist():
        members.setdefault(str(int(labels[i])), []).append(i)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "kept.npy", kept)
    (out / "duplicates.json").write_text(json.dumps(members))
    report = {"n": int(n), "edges": int(src.size), "components": int(np.unique(labels).size), "kept": int(kept.sum()),
              "duplicates_dropped": n_dup_dropped, "contaminated": int(leak.sum()), "threshold": args.threshold,
              "against_threshold": t2, "rule": args.rule}
    if part is not None:
        if fitted:
            np.save(out / "cluster_labels.npy", part)
        recall, recall_rows = None, 0
        if args.recall_sample is not None:
            recall_rows = min(n, args.recall_sample)
            recall = edge_recall(index, src, dst, args.threshold, args.recall_sample, args.cluster_seed)[2]
        report.update(clusters=int(np.unique(part).size), largest_cluster=int(np.unique(part, return_counts=True)[1].max()),
                      edge_recall=recall, edge_recall_rows=recall_rows)
    (out / "report.json").write_text(json.dumps(report, indent=1))
    if recs is not None:
        from ..data import build_index

        paths = write_shards([r for r, k in zip(recs, kept.tolist()) if k], out, None)
        if paths:
            build_index([str(p) for p in paths])
    print(f"keeping {report['kept']} out of {n} ({report['edges']} duplicate pairs, {report['contaminated']} contaminated)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
