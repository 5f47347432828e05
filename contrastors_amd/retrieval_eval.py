"""Text retrieval evaluation: nDCG@k, MAP@k, recall@k, precision@k, MRR@k and hit rate of a bi-encoder over local copies of
BEIR-layout evaluation sets (the numbers the reference takes from NanoBEIR in training, sc/trainers/text_text.py:243, 453-471,
and from BEIR / pytrec_eval in its offline scripts, sc/eval/eval_beir.py).  Neither library is used: every cut-off metric of a
query is a function of the ranks of that query's judged-relevant documents, which `FlatIPIndex.rank` (csrc/rank.hip) gives
without a top-k list or the score matrix; `ir_metrics` (csrc/ir_metrics.hip, cx_ir_metrics) turns them into per-query metrics
in one launch.

    task = load_beir_task("nano/NanoNFCorpus")
    evaluate_task(model, tokenizer, task, query_prefix="search_query: ", document_prefix="search_document: ")["ndcg@10"]

Definitions (trec_eval's ndcg_cut, map_cut, recall, P; BEIR's MRR): linear gains, the ideal ranking over the JUDGED documents
of a query, AP divided by the number of relevant documents, queries without a relevant document left out of the means.
Differences from pytrec_eval are listed in INTEGRATION.md.  Nothing is ever downloaded.
"""
from __future__ import annotations

import json
import logging
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _C

MAX_ROW = 4096     # CX_IR_MAX_ROW: entries (relevant + excluded) per query
MAX_KS = 8         # CX_IR_MAX_K
DEFAULT_KS = (1, 3, 5, 10, 100)
METRICS = ("ndcg", "map", "recall", "precision", "mrr", "hit")    # the order of cx_ir_metrics' last axis

log = logging.getLogger(__name__)

LAYOUT = ("expected the BEIR on-disk layout: corpus.jsonl ({\"_id\", \"title\"?, \"text\"} per line), queries.jsonl "
          "({\"_id\", \"text\"} per line) and qrels/<split>.tsv (query-id <tab> corpus-id <tab> score, after a header line)")


def _check_ks(ks) -> List[int]:
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= MAX_KS:
        raise ValueError(f"ks must hold 1 to {MAX_KS} cut-offs, got {len(ks)}")
    if any(k < 1 for k in ks):
        raise ValueError(f"every cut-off must be at least 1, got {ks}")
    return ks


def ir_metrics(ranks, gains, row_ptr, ks: Sequence[int] = DEFAULT_KS) -> dict:
    """Per-query metrics from the CSR rows `FlatIPIndex.rank` returns (cx_ir_metrics; the definitions are in
    include/contrastors_hip.h).

    ranks (nnz) integer, gains (nnz) float, row_ptr (M + 1): torch tensors (ranks / gains on the GPU or not) or numpy arrays.
    gain > 0: a relevant document of that graded gain; gain == 0: an excluded document, taken out of the ranking.  Ranks
    within a row must be distinct (the caller that holds the ids refuses duplicates: evaluate_embeddings does).
    -> {"ndcg", "map", "recall", "precision", "mrr", "hit": (M, K) float64, "nrel": (M,) int32, "ks": [..]} on the GPU (numpy
    when `ranks` was numpy).  Rows with nrel == 0 hold zeros: leave them out of means."""
    ks = _check_ks(ks)
    as_numpy = not isinstance(ranks, torch.Tensor)
    dev = ranks.device if not as_numpy and ranks.is_cuda else torch.device("cuda", torch.cuda.current_device())
    rp = torch.as_tensor(row_ptr).detach().to("cpu", torch.int64).reshape(-1)
    r = torch.as_tensor(ranks).detach().reshape(-1)
    g = torch.as_tensor(gains).detach().reshape(-1)
    if r.dtype.is_floating_point or r.dtype == torch.bool:
        raise ValueError(f"ranks must be integers, got {r.dtype}")
    M = rp.numel() - 1
    if M < 0 or int(rp[0]) != 0 or bool((rp[1:] < rp[:-1]).any()) or int(rp[-1]) != r.numel() or g.numel() != r.numel():
        raise ValueError("malformed CSR: row_ptr must be M + 1 non-decreasing offsets from 0 to len(ranks) == len(gains)")
    if M and int((rp[1:] - rp[:-1]).max()) > MAX_ROW:
        raise ValueError(f"a query row holds {int((rp[1:] - rp[:-1]).max())} entries; cx_ir_metrics stages at most {MAX_ROW}")
    g = g.to(dev, torch.float32).contiguous()
    r = r.to(dev, torch.int64).contiguous()
    if g.numel():
        if not bool(torch.isfinite(g).all()) or float(g.min()) < 0:
            raise ValueError("gains must be finite and >= 0 (0 marks an excluded document)")
        if int(r.min()) < 0:
            raise ValueError("ranks must be >= 0")
    else:   # valid pointers; no row reads them
        g, r = torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    K = len(ks)
    out = torch.zeros(M, K, 6, dtype=torch.float64, device=dev)
    nrel = torch.zeros(M, dtype=torch.int32, device=dev)
    if M:
        import ctypes

        with torch.cuda.device(dev):
            drp = rp.to(dev)
            _C.check(_C.lib().cx_ir_metrics(drp.data_ptr(), r.data_ptr(), g.data_ptr(), M, (ctypes.c_int * K)(*ks), K,
                                            out.data_ptr(), nrel.data_ptr(), _C.cur_stream()), "cx_ir_metrics")
    res = {name: out[:, :, i] for i, name in enumerate(METRICS)}
    res["nrel"] = nrel
    if as_numpy:
        res = {k: v.cpu().numpy() for k, v in res.items()}
    res["ks"] = ks
    return res


@dataclass
class RetrievalTask:
    """One evaluation set in memory.  qrels[i] maps corpus INDEX -> graded relevance (> 0) for query i."""
    name: str
    corpus_ids: List[str]
    corpus_texts: List[str]
    query_ids: List[str]
    query_texts: List[str]
    qrels: List[Dict[int, float]]
    n_qrels_dropped: int = 0          # qrel lines that name a document the corpus does not hold
    _doc_index: Dict[str, int] = field(default_factory=dict, repr=False)

    def __post_init__(self):
        if not self._doc_index:
            self._doc_index = {d: i for i, d in enumerate(self.corpus_ids)}
        if len(self._doc_index) != len(self.corpus_ids):
            raise ValueError(f"{self.name}: the corpus repeats a document id")

    def doc_index(self, doc_id: str) -> Optional[int]:
        return self._doc_index.get(doc_id)


def _read_jsonl(path: Path):
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            try:
                yield json.loads(line)
            except json.JSONDecodeError as e:
                raise ValueError(f"{path}:{n}: not a JSON object ({e.msg})") from None


def is_task_dir(path) -> bool:
    p = Path(path)
    return (p / "corpus.jsonl").is_file() and (p / "queries.jsonl").is_file() and (p / "qrels").is_dir()


def load_beir_task(path, split: str = "test") -> RetrievalTask:
    """Read a task from a LOCAL directory in the BEIR layout.  A document's text is `title + " " + text` when it has a
    non-empty title (BEIR's own join).  Kept: queries with at least one qrel line of the split; qrels with a score > 0 whose
    document is in the corpus.  Qrels naming a missing document are dropped and counted (one warning) -- trec_eval would count
    them in R."""
    p = Path(path)
    qrel_path = p / "qrels" / f"{split}.tsv"
    missing = [str(x) for x in (p / "corpus.jsonl", p / "queries.jsonl", qrel_path) if not x.is_file()]
    if missing:
        raise FileNotFoundError(f"{p}: missing {', '.join(missing)}; {LAYOUT}.  Nothing is downloaded: copy the set here.")
    corpus_ids, corpus_texts = [], []
    for rec in _read_jsonl(p / "corpus.jsonl"):
        title, text = (rec.get("title") or "").strip(), rec.get("text") or ""
        corpus_ids.append(str(rec["_id"]))
        corpus_texts.append(f"{title} {text}".strip() if title else text.strip())
    doc_index = {d: i for i, d in enumerate(corpus_ids)}
    if len(doc_index) != len(corpus_ids):
        raise ValueError(f"{p / 'corpus.jsonl'} repeats a document id")
    queries = {str(rec["_id"]): rec.get("text") or "" for rec in _read_jsonl(p / "queries.jsonl")}
    judged: Dict[str, Dict[int, float]] = {}     # in the order of the qrels file
    dropped = 0
    with open(qrel_path, encoding="utf-8") as f:
        next(f, None)                             # the header line
        for n, line in enumerate(f, 2):
            line = line.rstrip("\n")
            if not line.strip():
                continue
            cols = line.split("\t")
            if len(cols) != 3:
                raise ValueError(f"{qrel_path}:{n}: expected query-id <tab> corpus-id <tab> score")
            qid, did, score = cols[0], cols[1], float(cols[2])
            row = judged.setdefault(qid, {})
            if score <= 0:
                continue
            if did not in doc_index:
                dropped += 1
                continue
            row[doc_index[did]] = score
    unknown = [q for q in judged if q not in queries]
    if unknown:
        raise ValueError(f"{qrel_path}: {len(unknown)} query ids are not in queries.jsonl (first: {unknown[0]!r})")
    if dropped:
        log.warning("%s: %d qrels name documents that are not in corpus.jsonl; dropped (trec_eval would count them as relevant "
                    "documents that were never retrieved)", p, dropped)
    qids = list(judged)
    return RetrievalTask(name=p.name, corpus_ids=corpus_ids, corpus_texts=corpus_texts, query_ids=qids,
                         query_texts=[queries[q] for q in qids], qrels=[judged[q] for q in qids], n_qrels_dropped=dropped,
                         _doc_index=doc_index)


def task_targets(task: RetrievalTask, exclude_identical: bool = True):
    """-> (row_ptr int64 (M + 1), ids int64 (nnz), gains float32 (nnz)) numpy: per query its relevant documents (corpus index
    ascending) and, with exclude_identical, the document whose id equals the query's (gain 0) when the corpus holds one.  A
    same-id document that is also judged relevant is excluded, as BEIR's ignore_identical_ids removes it before scoring."""
    row_ptr, ids, gains = [0], [], []
    for qid, rel in zip(task.query_ids, task.qrels):
        same = task.doc_index(qid) if exclude_identical else None
        for d in sorted(rel):
            if d != same:
                ids.append(d)
                gains.append(rel[d])
        if same is not None:
            ids.append(same)
            gains.append(0.0)
        row_ptr.append(len(ids))
    return np.asarray(row_ptr, np.int64), np.asarray(ids, np.int64), np.asarray(gains, np.float32)


def evaluate_embeddings(query_emb, corpus_emb, task: RetrievalTask, ks: Sequence[int] = DEFAULT_KS,
                        exclude_identical: bool = True, per_query: bool = False, device="cuda") -> dict:
    """Score a task from embeddings: one FlatIPIndex over the corpus, one rank() call over every query's relevant (and
    excluded) documents, one ir_metrics launch, means over the queries with a relevant document.
    -> {"ndcg@10": ..., "map@100": ..., ..., "n_queries", "n_skipped"}; per_query adds "per_query" = ir_metrics' arrays (numpy)
    and "query_ids"."""
    from .search import FlatIPIndex

    ks = _check_ks(ks)
    q = query_emb if isinstance(query_emb, torch.Tensor) else torch.as_tensor(np.asarray(query_emb))
    c = corpus_emb if isinstance(corpus_emb, torch.Tensor) else torch.as_tensor(np.asarray(corpus_emb))
    if q.dim() != 2 or c.dim() != 2 or q.shape[1] != c.shape[1]:
        raise ValueError(f"expected (M, d) query and (N, d) corpus embeddings, got {tuple(q.shape)} and {tuple(c.shape)}")
    if q.shape[0] != len(task.query_ids) or c.shape[0] != len(task.corpus_ids):
        raise ValueError(f"{q.shape[0]} query / {c.shape[0]} corpus embeddings for a task of {len(task.query_ids)} queries and "
                         f"{len(task.corpus_ids)} documents")
    dev = torch.device(device) if not (isinstance(c, torch.Tensor) and c.is_cuda) else c.device
    index = FlatIPIndex(int(c.shape[1]), device=dev)    # (refuses widths that are no multiple of 64 in [64, 1024])
    row_ptr, ids, gains = task_targets(task, exclude_identical)
    lens = np.diff(row_ptr)
    if lens.size and int(lens.max()) > MAX_ROW:
        raise ValueError(f"query {task.query_ids[int(lens.argmax())]!r} has {int(lens.max())} judged documents; at most {MAX_ROW}")
    index.add(c)
    ranks, _, _ = index.rank(q.to(dev), (row_ptr, ids))
    m = ir_metrics(ranks, torch.from_numpy(gains), row_ptr, ks)
    host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in m.items()}
    keep = host["nrel"] > 0
    n = int(keep.sum())
    out = {}
    for name in METRICS:
        for j, k in enumerate(ks):   # the mean of M fp64 values on the host, correctly rounded sum
            out[f"{name}@{k}"] = math.fsum(host[name][keep, j].tolist()) / n if n else 0.0
    out["n_queries"] = n
    out["n_skipped"] = len(task.query_ids) - n
    if per_query:
        out["per_query"] = host
        out["query_ids"] = list(task.query_ids)
    return out


def _truncate(emb: torch.Tensor, dim: int) -> torch.Tensor:
    """The first `dim` coordinates, re-normalised (how a Matryoshka model is used at a smaller width)."""
    if not 1 <= dim <= emb.shape[1]:
        raise ValueError(f"dims: {dim} is not a prefix width of {emb.shape[1]}-dimensional embeddings")
    return torch.nn.functional.normalize(emb[:, :dim], dim=-1)


def evaluate_task(model, tokenizer, task: RetrievalTask, ks: Sequence[int] = DEFAULT_KS, query_prefix: str = "",
                  document_prefix: str = "", max_length: int = 512, batch_size: int = 256, dims: Optional[Sequence[int]] = None,
                  exclude_identical: bool = True, per_query: bool = False) -> dict:
    """Embed the task's queries and documents with search.encode (the prefixes prepended as the reference passes
    query_prompts / corpus_prompts to its evaluator) and evaluate.  dims: Matryoshka widths, each evaluated on the
    re-normalised truncation; their keys carry the suffix `_matryoshka_<dim>`.  The model's training mode is restored."""
    from .search import encode

    qe = encode(model, [query_prefix + t for t in task.query_texts], tokenizer, batch_size=batch_size, max_length=max_length)
    ce = encode(model, [document_prefix + t for t in task.corpus_texts], tokenizer, batch_size=batch_size, max_length=max_length)
    out = evaluate_embeddings(qe, ce, task, ks, exclude_identical=exclude_identical, per_query=per_query)
    for d in dims or ():
        sub = evaluate_embeddings(_truncate(qe, int(d)), _truncate(ce, int(d)), task, ks, exclude_identical=exclude_identical)
        out.update({f"{k}_matryoshka_{int(d)}": v for k, v in sub.items() if k not in ("n_queries", "n_skipped")})
    return out


def find_tasks(path, tasks: Optional[Sequence[str]] = None) -> List[Path]:
    """The task directories under `path`: `path` itself when it is one, else its sub-directories that are (sorted by name),
    narrowed to `tasks` (directory names, case-insensitive) when given."""
    p = Path(path)
    if not p.is_dir():
        raise FileNotFoundError(f"{p} is not a directory; {LAYOUT}, or one such directory per task.  Nothing is downloaded.")
    found = [p] if is_task_dir(p) else sorted((s for s in p.iterdir() if s.is_dir() and is_task_dir(s)), key=lambda s: s.name)
    if not found:
        raise FileNotFoundError(f"{p} holds no evaluation task; {LAYOUT}, or one such directory per task")
    if tasks:
        by_name = {s.name.lower(): s for s in found}
        missing = [t for t in tasks if t.lower() not in by_name]
        if missing:
            raise FileNotFoundError(f"{p}: no task named {missing}; found {[s.name for s in found]}")
        found = [by_name[t.lower()] for t in tasks]
    return found


def evaluate_path(model, tokenizer, path, tasks: Optional[Sequence[str]] = None, split: str = "test", **kwargs) -> dict:
    """{task directory name: evaluate_task(...)} over a directory of tasks or a single task directory."""
    return {p.name: evaluate_task(model, tokenizer, load_beir_task(p, split), **kwargs) for p in find_tasks(path, tasks)}


def beir_log_name(task_name: str) -> str:
    """sc/trainers/text_text.py:463: `beir/<task>` with "Nano" removed and lower-cased (a leading `nano` here)."""
    n = task_name.lower()
    return "beir/" + (n[4:] if n.startswith("nano") and len(n) > 4 else n)


def beir_log_metrics(results: dict, key: str = "ndcg@10") -> dict:
    """What the trainer logs for evaluate_path's results: beir/<task> = nDCG@10 per task, and their mean as beir/mean."""
    out = {beir_log_name(name): float(r[key]) for name, r in results.items()}
    if out:
        out["beir/mean"] = float(sum(out.values()) / len(out))
    return out
