"""Hard-negative mining on the exact inner-product search (contrastors_amd.search).

Two selection rules, restated from the reference scripts (their rules sit under `__main__` and cannot be imported):

* `--rule topk` (scripts/text/get_negatives.py): the k nearest documents of each record's query, minus its positive and
  the query text itself, filled up to k with random documents (:170-194); documents are the records' positives in
  first-seen order (load_dataset, :32-79).
* `--rule margin` (scripts/text/mine_beir_negatives_full.py): per (query, positive) pair of a BEIR train split, the
  documents scoring below margin * s(query, positive), the query's positives excluded, in descending score order, the
  first --max_negatives; a pair with fewer than --k of them is dropped (:98-136; the script reads --min_negatives but
  compares with --k).  The search asks the kernel for k = --max_negatives with the bound and the exclusions, not for a
  full sort of every row.

Output: shard-%05d.jsonl.gz of 100 000 records, each with the triplet `metadata.objective` entry (readable by
contrastors_amd.data.StreamingShardDataset after contrastors_amd.data.build_index).
Embeddings: --query_embeddings / --document_embeddings .npy (rows in query / document order), or --model (a local
BiEncoder checkpoint) with --tokenizer (a local tokenizer).

Deviations from the reference (also in --help):
* the random fill of --rule topk is seeded (--seed); so is the record shuffle of --rule margin;
* --rule topk writes the fill's document TEXTS under --negatives_key; the reference appends whole records to
  data["negatives"] (get_negatives.py:187-194);
* --rule topk compares document texts with the positive and the query; the reference compares the document record (a
  dict) with the text (:181), which is never equal, so it drops nothing;
* a --rule topk fill that cannot be completed (too few admissible documents) is an error; the reference loops forever.
"""
from __future__ import annotations

import argparse
import csv
import gzip
import json
import random
import sys
from pathlib import Path
from typing import Dict, List

import numpy as np

from ._common import (add_search_arguments, check_search_arguments, encode_texts, host_documents, load_npy, search,
                      triplet_metadata, write_shards)

DEVIATIONS = """deviations from the reference scripts:
  the random fill (topk) and the record shuffle (margin) are seeded by --seed;
  topk appends the fill's document texts under --negatives_key (the reference appends whole records to data["negatives"]);
  topk compares document texts with the positive and the query (the reference compares a record with a text: never equal);
  a topk fill that cannot be completed is an error (the reference loops forever)."""


# ---- --rule topk (scripts/text/get_negatives.py) ----------------------------------------------------------------------
def load_records(path, query_key: str, document_key: str, negatives_key: str):
    """get_negatives.py:32-79 load_dataset: -> (query texts, document texts, records).  Note the reference's order of
    operations: a record's negatives are added to `seen` BEFORE the extend, so they never become documents."""
    path = Path(path)
    files = sorted(path.glob("shard-*.jsonl.gz")) if path.is_dir() else [path]
    queries, documents, records, seen = [], [], [], set()
    for file in files:
        opener = gzip.open if file.suffix == ".gz" else open
        with opener(file, "rt") as f:
            for line in f:
                data = json.loads(line)
                queries.append(data[query_key])
                docs = data[document_key]
                if not isinstance(docs, str):
                    raise SystemExit(f"error: {document_key} must be a string per record (the reference's list form "
                                     "is unhashable at get_negatives.py:52)")
                if docs not in seen:
                    documents.append(docs)
                if negatives_key in data:
                    negs = data[negatives_key]
                    negs = [negs] if isinstance(negs, str) else list(negs)
                    seen.update(negs)
                seen.add(docs)
                records.append(data)
    return queries, documents, records


def select_topk(records: List[dict], documents: List[str], indices, k: int, query_key: str, document_key: str,
                negatives_key: str, rng: np.random.RandomState) -> List[dict]:
    """get_negatives.py:170-194: keep the searched ids that are neither the positive nor the query text (stop at -1),
    then draw random documents (np.random.randint, size = what is missing) until one draw is entirely admissible."""
    for i, data in enumerate(records):
        query, pos = data[query_key], data[document_key]
        kept = []
        for inx in indices[i]:
            if inx == -1:
                break
            if documents[inx] != pos and documents[inx] != query:
                kept.append(documents[inx])
        data[negatives_key] = kept
        if len(kept) < k:
            remaining = k - len(kept)
            if not any(doc != pos and doc != query for doc in documents):
                raise SystemExit(f"error: record {i}: no admissible document to fill its negatives with")
            while True:
                draw = rng.randint(0, len(documents), size=remaining).tolist()
                fill = [documents[j] for j in draw if documents[j] != pos and documents[j] != query]
                if len(fill) == remaining:
                    break
            data[negatives_key].extend(fill)
    return records


# ---- --rule margin (scripts/text/mine_beir_negatives_full.py) ---------------------------------------------------------
def load_beir(beir_dir, split: str = "train"):
    """beir GenericDataLoader(...).load(split) as load_beir (:31-45) uses it: corpus.jsonl ({_id, title, text}),
    queries.jsonl ({_id, text}), qrels/<split>.tsv (header; query-id, corpus-id, score); queries are those of the qrels,
    in qrels order.  -> (corpus, queries, qrels, qid2index, docid2index, documents)."""
    beir_dir = Path(beir_dir)
    corpus: Dict[str, dict] = {}
    with open(beir_dir / "corpus.jsonl") as f:
        for line in f:
            d = json.loads(line)
            corpus[d.get("_id")] = {"text": d.get("text"), "title": d.get("title")}
    all_queries: Dict[str, str] = {}
    with open(beir_dir / "queries.jsonl") as f:
        for line in f:
            d = json.loads(line)
            all_queries[d.get("_id")] = d.get("text")
    qrels: Dict[str, Dict[str, int]] = {}
    with open(beir_dir / "qrels" / f"{split}.tsv") as f:
        reader = csv.reader(f, delimiter="\t", quoting=csv.QUOTE_MINIMAL)
        next(reader)
        for row in reader:
            qrels.setdefault(row[0], {})[row[1]] = int(row[2])
    queries = {qid: all_queries[qid] for qid in qrels}
    qid2index = {qid: i for i, qid in enumerate(queries)}
    docid2index, documents = {}, []
    for doc_id, doc in corpus.items():
        docid2index[doc_id] = len(documents)
        documents.append((doc.get("title") + " " + doc.get("text")).strip())
    return corpus, queries, qrels, qid2index, docid2index, documents


def margin_pairs(qrels, qid2index, docid2index, q_emb, d_emb, margin: float):
    """One search row per (query, positive): (query row, exclusions = the query's positives, bound = margin * s(q, pos))
    with s the fp32 dot product of the bf16-rounded embeddings the kernel scores.  Only the positives' rows of the
    corpus are converted."""
    import torch

    pairs, rows, excl, pos_rows = [], [], [], []
    for qid in qrels:
        pos_ids = list(qrels[qid])
        pos_idx = [docid2index[p] for p in pos_ids]
        for p, pi in zip(pos_ids, pos_idx):
            pairs.append((qid, p))
            rows.append(qid2index[qid])
            excl.append(pos_idx)
            pos_rows.append(pi)
    if not pairs:
        return pairs, rows, excl, np.zeros(0, np.float32)
    qb = torch.as_tensor(np.asarray(np.asarray(q_emb)[rows], dtype=np.float32)).to(torch.bfloat16).float()
    pb = torch.as_tensor(np.asarray(np.asarray(d_emb)[pos_rows], dtype=np.float32)).to(torch.bfloat16).float()
    s = (qb * pb).sum(1).numpy().astype(np.float32)
    below = (s * np.float32(margin)).astype(np.float32)
    return pairs, rows, excl, below


def select_margin(pairs, indices, corpus, queries, documents, k: int, query_key: str, document_key: str,
                  negatives_key: str):
    """:111-136 per pair: the searched ids (already below the bound, positives excluded, descending) -> a row if at least
    k of them exist.  -> (rows, number of pairs dropped)."""
    rows, dropped = [], 0
    for (qid, pid), ids in zip(pairs, indices):
        neg = [int(j) for j in ids if j >= 0]
        if len(neg) < k:
            dropped += 1
            continue
        doc = corpus[pid]
        rows.append({query_key: queries[qid], document_key: (doc.get("title") + " " + doc.get("text")).strip(),
                     negatives_key: [documents[j] for j in neg]})
    return rows, dropped


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m contrastors_amd.tools.mine_negatives", description=__doc__.split("\n\n")[0],
                                 epilog=DEVIATIONS, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rule", choices=("topk", "margin"), required=True)
    ap.add_argument("--dataset", required=True, help="topk: a shard directory or .jsonl(.gz) file; margin: a BEIR directory")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--split", default="train", help="margin: the qrels split")
    ap.add_argument("--k", type=int, default=None, help="topk: negatives per record (20); margin: fewest kept (75)")
    ap.add_argument("--min_negatives", type=int, default=10, help="margin: read but unused, as in the reference")
    ap.add_argument("--max_negatives", type=int, default=100)
    ap.add_argument("--margin", type=float, default=0.95)
    ap.add_argument("--query_key", default=None)
    ap.add_argument("--document_key", default=None)
    ap.add_argument("--negatives_key", default=None)
    ap.add_argument("--query_embeddings", help=".npy, one row per query: topk, per record in file order; margin, per query "
                    "of the qrels split in the order its ids first appear in qrels/<split>.tsv (or see --query_ids)")
    ap.add_argument("--query_ids", help="margin: JSON list of the query ids of the --query_embeddings rows, in row order "
                    "(the rows are then matched by id)")
    ap.add_argument("--document_embeddings", help=".npy, one row per document: topk, the positives in first-seen order; "
                    "margin, corpus.jsonl order")
    ap.add_argument("--model", help="local BiEncoder checkpoint directory (when no .npy is given)")
    ap.add_argument("--tokenizer", help="local tokenizer directory")
    ap.add_argument("--query_prefix", default="")
    ap.add_argument("--document_prefix", default="")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--max_length", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    add_search_arguments(ap)
    return ap


def _embeddings(args, q_texts, d_texts):
    if (args.query_embeddings is None) != (args.document_embeddings is None):
        raise SystemExit("error: give both --query_embeddings and --document_embeddings, or neither")
    if args.query_embeddings:
        return (load_npy(args.query_embeddings, len(q_texts), "query"),
                load_npy(args.document_embeddings, len(d_texts), "document", mmap=host_documents(args)))
    q = encode_texts(q_texts, args.model, args.tokenizer, args.batch_size, args.max_length, args.device, args.query_prefix)
    d = encode_texts(d_texts, args.model, args.tokenizer, args.batch_size, args.max_length, args.device,
                     args.document_prefix)
    return q.cpu().numpy(), d.cpu().numpy()


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    topk = args.rule == "topk"
    args.k = args.k if args.k is not None else (20 if topk else 75)
    args.query_key = args.query_key or ("question" if topk else "query")
    args.document_key = args.document_key or ("positive_ctxs" if topk else "pos")
    args.negatives_key = args.negatives_key or ("hard_negative_ctxs" if topk else "neg")
    if args.k < 1 or args.max_negatives < 1:
        ap.error("--k and --max_negatives must be positive")
    if topk and args.k > 1024:
        ap.error("--k is at most 1024")
    if not topk and args.max_negatives > 1024:
        ap.error("--max_negatives is at most 1024")
    if not Path(args.dataset).exists():
        ap.error(f"--dataset {args.dataset} does not exist")
    ivf = check_search_arguments(ap, args)
    if (args.query_embeddings is None) != (args.document_embeddings is None):
        ap.error("give both --query_embeddings and --document_embeddings, or neither")
    if args.query_ids and (topk or args.query_embeddings is None):
        ap.error("--query_ids goes with --rule margin and --query_embeddings")
    if args.query_embeddings is None and not (args.model and args.tokenizer):
        ap.error("without .npy embeddings, --model and --tokenizer are required")
    meta = triplet_metadata(args.query_key, args.document_key, args.negatives_key)
    if topk:
        queries, documents, records = load_records(args.dataset, args.query_key, args.document_key, args.negatives_key)
        q_emb, d_emb = _embeddings(args, queries, documents)
        _, indices = search(d_emb, q_emb, args.k, args.device, coarse=args.coarse, rescore_factor=args.rescore_factor,
                            storage=args.storage, **ivf)
        records = select_topk(records, documents, indices, args.k, args.query_key, args.document_key,
                              args.negatives_key, np.random.RandomState(args.seed))
        write_shards(records, args.output_dir, meta)
        print(f"mined {len(records)} records into {args.output_dir}")
        return 0
    corpus, queries, qrels, qid2index, docid2index, documents = load_beir(args.dataset, args.split)
    if args.query_ids:
        row_ids = json.loads(Path(args.query_ids).read_text())
        q_all = np.load(args.query_embeddings)
        if len(row_ids) != q_all.shape[0]:
            ap.error(f"--query_ids has {len(row_ids)} ids for {q_all.shape[0]} rows")
        where = {qid: i for i, qid in enumerate(row_ids)}
        missing = [qid for qid in queries if qid not in where]
        if missing:
            ap.error(f"--query_ids lacks {len(missing)} queries of the qrels split, e.g. {missing[0]!r}")
        q_emb = q_all[[where[qid] for qid in queries]]
        d_emb = load_npy(args.document_embeddings, len(documents), "document", mmap=host_documents(args))
    else:
        q_emb, d_emb = _embeddings(args, list(queries.values()), documents)
    pairs, rows, excl, below = margin_pairs(qrels, qid2index, docid2index, q_emb, d_emb, args.margin)
    _, indices = search(d_emb, np.asarray(q_emb)[rows], args.max_negatives, args.device, exclude=excl, below=below,
                        coarse=args.coarse, rescore_factor=args.rescore_factor, storage=args.storage, **ivf)
    mined, dropped = select_margin(pairs, indices, corpus, queries, documents, args.k, args.query_key,
                                   args.document_key, args.negatives_key)
    random.Random(args.seed).shuffle(mined)
    write_shards(mined, args.output_dir, meta)
    print(f"lt_negatives={dropped} len(mined_dataset)={len(mined)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
