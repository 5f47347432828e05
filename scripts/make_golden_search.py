"""Write tests/golden/search_curation.json: small fixtures of the data-curation rules behind contrastors_amd.tools.

* consistency: filter_points (scripts/text/index_filtering.py:363-391) is run as the reference's OWN code, read from the
  reference tree, with faiss replaced by an exact numpy IndexFlatIP stand-in (float64 scores, stable sort: ties to the
  lower id) and torch.distributed / tqdm stubbed.
* topk and margin: both mining rules sit under the scripts' `__main__` and cannot be imported, so they are RESTATED here
  (get_negatives.py:170-194 and mine_beir_negatives_full.py:98-136, cited inline) over a full stable sort of exact
  scores.  The expected outputs are that restatement, with the tool's stated deviations (seeded draws, texts under
  negatives_key, text comparisons).
Inputs are tiny embeddings whose entries are multiples of 1/8 (exact in bf16; every score is exact in fp32), with tied
scores, exclusions, a corpus shorter than k (search padding), a query equal to a document, margin pairs that are
dropped and a kept pair with exactly k negatives.

usage: python scripts/make_golden_search.py [reference_root]
"""
from __future__ import annotations

import ast
import json
import random
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "search_curation.json"
D = 64


def emb(rng, n):
    return rng.integers(-4, 5, size=(n, D)).astype(np.float32) / 8.0


class NumpyFlatIP:
    """faiss.IndexFlatIP stand-in: exact scores, descending, ties to the lower id."""

    def __init__(self, d):
        self.x = np.zeros((0, d), np.float64)

    def add(self, x):
        self.x = np.concatenate([self.x, np.asarray(x, np.float64)])

    def search(self, q, k):
        s = np.asarray(q, np.float64) @ self.x.T
        order = np.argsort(-s, axis=1, kind="stable")[:, :k]
        return np.take_along_axis(s, order, 1).astype(np.float32), order.astype(np.int64)


def reference_filter_points(ref_root: Path):
    src = (ref_root / "scripts" / "text" / "index_filtering.py").read_text()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "filter_points")
    faiss = types.SimpleNamespace(IndexFlatIP=NumpyFlatIP, GpuMultipleClonerOptions=lambda: types.SimpleNamespace(),
                                  index_cpu_to_all_gpus=lambda index, co=None: index)
    ns = {"np": np, "faiss": faiss, "dist": types.SimpleNamespace(get_rank=lambda: 0),
          "tqdm": lambda it, **kw: it, "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "index_filtering.py", "exec"), ns)
    return ns["filter_points"]


def full_sort(q, d):
    s = np.asarray(q, np.float64) @ np.asarray(d, np.float64).T
    return s, np.argsort(-s, axis=1, kind="stable")


def make_consistency(rng, ref_root):
    n = 40
    q, d = emb(rng, n), emb(rng, n)
    d[7] = d[3]                       # duplicate documents: a tie at the top
    q[10] = d[10]                     # a query equal to its document
    q[11] = d[12]                     # ... and one equal to another pair's document
    ids = [int(v) for v in rng.permutation(1000)[:n]]
    id2emb = {i: (q[j], d[j]) for j, i in enumerate(ids)}
    kept = reference_filter_points(ref_root)(id2emb, batch_size=16)
    return {"ids": ids, "q": q.tolist(), "d": d.tolist(), "kept": kept}


WORDS = "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau".split()


def make_topk(rng):
    n_rec, k = 12, 10                                                   # k > the 9 documents: -1 padding in the search
    records = []
    for i in range(n_rec):
        pos = " ".join(rng.choice(WORDS, 3)) + f" p{i % 9}"          # some positives repeat: fewer documents
        records.append({"question": f"q{i} " + " ".join(rng.choice(WORDS, 2)), "positive_ctxs": pos})
    records[4]["question"] = records[2]["positive_ctxs"]                # a query text equal to a document
    for j in (7, 8, 9):
        records[j]["positive_ctxs"] = records[1]["positive_ctxs"]       # repeated positives: 9 documents
    # get_negatives.py:32-79 load_dataset (string form): documents = positives, first seen
    documents, seen = [], set()
    for r in records:
        if r["positive_ctxs"] not in seen:
            documents.append(r["positive_ctxs"])
        seen.add(r["positive_ctxs"])
    q, d = emb(rng, n_rec), emb(rng, len(documents))
    d[1] = d[0]
    q[4] = d[2]
    _, order = full_sort(q, d)
    indices = [row[:k].tolist() + [-1] * (k - min(k, len(documents))) for row in order]
    # get_negatives.py:170-194, with the deviations: texts compared, texts appended under negatives_key, seeded draws
    rs = np.random.RandomState(7)
    out = []
    for i, data in enumerate(records):
        data = dict(data)
        query, pos = data["question"], data["positive_ctxs"]
        kept = []
        for inx in indices[i]:                                          # :174-185
            if inx == -1:
                break
            if documents[inx] != pos and documents[inx] != query:
                kept.append(documents[inx])
        data["hard_negative_ctxs"] = kept                               # :187
        if len(kept) < k:                                               # :188-196
            remaining = k - len(kept)
            while True:
                draw = rs.randint(0, len(documents), size=remaining).tolist()
                fill = [documents[j] for j in draw if documents[j] != pos and documents[j] != query]
                if len(fill) == remaining:
                    break
            data["hard_negative_ctxs"].extend(fill)
        out.append(data)
    return {"records": records, "documents": documents, "q": q.tolist(), "d": d.tolist(), "k": k, "seed": 7,
            "expected": out}


def make_margin(rng):
    n_doc, n_q, margin, k_min, max_neg = 30, 8, 0.5, 4, 6
    corpus = [{"_id": f"d{j}", "title": f"T{j}" if j % 3 else "", "text": " ".join(rng.choice(WORDS, 4))}
              for j in range(n_doc)]
    queries = [{"_id": f"q{i}", "text": " ".join(rng.choice(WORDS, 3))} for i in range(n_q + 2)]   # two without qrels
    qrels = []
    for i in range(n_q):
        for p in sorted(rng.choice(n_doc, size=1 + i % 3, replace=False).tolist()):
            qrels.append([f"q{i}", f"d{p}", 1])
    qd = emb(rng, n_q)                  # rows in qrels order (q0 .. q7)
    dd = emb(rng, n_doc)
    dd[5] = dd[6]                       # tied documents
    qd[2] = dd[int(qrels[0][1][1:])]    # a query equal to a document
    qd[3] = np.abs(qd[3])               # strong positive scores: bounds that bite
    dd[: n_doc // 2] = np.abs(dd[: n_doc // 2])
    qd[6] = 0.0                         # every score 0: no document below its bound, its pairs are dropped
    # mine_beir_negatives_full.py:98-136 (torch topk over the full row -> stable sort here: ties to the lower id)
    by_q = {}
    for qid, did, _ in qrels:
        by_q.setdefault(qid, []).append(did)
    scores, order = full_sort(qd, dd)

    def text(c):
        return (c["title"] + " " + c["text"]).strip()

    rows, dropped = [], 0
    for qi, qid in enumerate(by_q):
        pos_idx = [int(p[1:]) for p in by_q[qid]]
        for p in pos_idx:
            thr = np.float32(np.float32(scores[qi, p]) * np.float32(margin))                   # :117-118
            neg = [j for j in order[qi] if scores[qi, j] < thr and j not in pos_idx][:max_neg]   # :122-125
            if len(neg) < k_min:                                                                # :127-129 (min = args.k)
                dropped += 1
                continue
            rows.append({"query": queries[qi]["text"], "pos": text(corpus[p]), "neg": [text(corpus[j]) for j in neg]})
    random.Random(0).shuffle(rows)                                                              # :140 (seeded here)
    return {"corpus": corpus, "queries": queries, "qrels": qrels, "q": qd.tolist(), "d": dd.tolist(),
            "margin": margin, "k": k_min, "max_negatives": max_neg, "seed": 0, "dropped": dropped, "expected": rows}


def main():
    ref_root = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("/root/reference")
    rng = np.random.default_rng(20261016)
    fx = {"d": D, "consistency": make_consistency(rng, ref_root), "topk": make_topk(rng), "margin": make_margin(rng)}
    OUT.write_text(json.dumps(fx, separators=(",", ":")))
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
