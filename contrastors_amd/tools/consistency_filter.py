"""Consistency filtering of (query, document) pairs on the exact inner-product search (contrastors_amd.search).

The rule of scripts/text/index_filtering.py:363-391 (filter_points): index the documents in ascending id order, search
every query for its top-2, keep pair i if its own document is among them.  Output as the reference writes it:
<output_dir>/ids_to_keep_<n>.json (n = the number of such files already there), a JSON list of the kept ids.
Embeddings: --query_embeddings / --document_embeddings .npy (row i = pair i) with optional --ids (a JSON list, default
0 .. n-1), or --dataset records (.jsonl / .jsonl.gz / a shard directory) encoded with --model and --tokenizer (local).
Ties at the second place go to the lower document id (faiss leaves them unspecified).
"""
from __future__ import annotations

import argparse
import gzip
import json
import sys
from pathlib import Path
from typing import List

import numpy as np

from ._common import add_search_arguments, check_search_arguments, encode_texts, host_documents, load_npy, search


def keep_ids(ids: List, top_k_indices) -> List:
    """filter_points' decision (index_filtering.py:372-391) given the search result of the queries in ascending id order:
    row j of top_k_indices are the document positions found for the j-th smallest id."""
    order = sorted(ids)
    top = np.asarray(top_k_indices)
    valid = np.equal(top, np.arange(len(order))[:, None]).sum(axis=1)
    return [order[j] for j in range(len(order)) if valid[j]]


def filter_pairs(ids: List, q_emb, d_emb, device: str = "cuda", k: int = 2, coarse: str = "exact",
                 rescore_factor: int = 4, storage: str = "bf16", **ivf) -> List:
    """ids[i] names pair i; -> the kept ids, in ascending id order.  ivf: the ivf_* arguments of _common.search."""
    pos = sorted(range(len(ids)), key=lambda i: ids[i])
    _, top = search(np.asarray(d_emb)[pos], np.asarray(q_emb)[pos], k, device, coarse=coarse, rescore_factor=rescore_factor,
                    storage=storage, **ivf)
    return keep_ids(ids, top)


def _records(path):
    path = Path(path)
    files = sorted(path.glob("shard-*.jsonl.gz")) if path.is_dir() else [path]
    for file in files:
        with (gzip.open if file.suffix == ".gz" else open)(file, "rt") as f:
            for line in f:
                yield json.loads(line)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m contrastors_amd.tools.consistency_filter",
                                 description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter,
                                 epilog="deviation: ties at the k-th place go to the lower document id")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--query_embeddings")
    ap.add_argument("--document_embeddings")
    ap.add_argument("--ids", help="JSON list naming the pairs (default: their row numbers)")
    ap.add_argument("--dataset", help="records to encode when no .npy is given")
    ap.add_argument("--query_key", default="query")
    ap.add_argument("--document_key", default="document")
    ap.add_argument("--id_key", default=None, help="record field holding the id (default: the record's position)")
    ap.add_argument("--model")
    ap.add_argument("--tokenizer")
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--max_length", type=int, default=512)
    ap.add_argument("--device", default="cuda")
    add_search_arguments(ap)
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 1 <= args.k <= 1024:
        ap.error("--k must be in [1, 1024]")
    ivf = check_search_arguments(ap, args)
    if (args.query_embeddings is None) != (args.document_embeddings is None):
        ap.error("give both --query_embeddings and --document_embeddings, or neither")
    if args.query_embeddings:
        q = np.load(args.query_embeddings)
        n = q.shape[0]
        d = load_npy(args.document_embeddings, n, "document", mmap=host_documents(args))
        ids = json.loads(Path(args.ids).read_text()) if args.ids else list(range(n))
        if len(ids) != n:
            ap.error(f"--ids has {len(ids)} entries for {n} pairs")
    else:
        if not (args.dataset and args.model and args.tokenizer):
            ap.error("without .npy embeddings, --dataset, --model and --tokenizer are required")
        recs = list(_records(args.dataset))
        ids = [r[args.id_key] if args.id_key else i for i, r in enumerate(recs)]
        q = encode_texts([r[args.query_key] for r in recs], args.model, args.tokenizer, args.batch_size,
                         args.max_length, args.device).cpu().numpy()
        d = encode_texts([r[args.document_key] for r in recs], args.model, args.tokenizer, args.batch_size,
                         args.max_length, args.device).cpu().numpy()
    if len(set(ids)) != len(ids):
        ap.error("pair ids must be unique")
    kept = filter_pairs(ids, q, d, args.device, args.k, args.coarse, args.rescore_factor, storage=args.storage, **ivf)
    out = Path(args.output_dir)
    out.mkdir(parents=True, exist_ok=True)
    n_existing = len(list(out.glob("ids_to_keep_*.json")))
    (out / f"ids_to_keep_{n_existing}.json").write_text(json.dumps(kept))
    print(f"keeping {len(kept)} out of {len(ids)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
