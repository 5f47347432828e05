"""Near-duplicate removal and decontamination on the exact range search (FlatIPIndex.range_search / range_count).

The standard recipe: take ALL pairs of corpus rows with cosine above a threshold (`duplicate_edges`, a self-join of the index
in query batches -- a duplicate cluster of any size comes back whole, which a top-k search cannot promise), group them
(`components`) and keep one row per group (`select_kept`); and drop training rows that sit within a threshold of any
evaluation row (`contaminated`).  The GPU work goes through the index; the graph logic is host numpy.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

RULES = ("components", "greedy")
DEFAULT_BATCH_ROWS = 8192
DEFAULT_MAX_EDGES = 1 << 27


def duplicate_edges(index, threshold: float, batch_rows: int = DEFAULT_BATCH_ROWS,
                    max_edges: int = DEFAULT_MAX_EDGES) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (src int64, dst int64, score float32): every pair of stored rows with score > threshold, once, with src < dst and
    no self-match, in (src, dst) order.  The stored rows are searched against the index `batch_rows` at a time with
    min_id = their own row id, so corpus tiles below a batch are never computed (half the all-pairs work).  More than
    max_edges pairs raise ValueError before they are allocated."""
    n = index.ntotal
    batch_rows = max(1, int(batch_rows))
    src, dst, score = [], [], []
    total = 0
    D = index.vectors
    for b0 in range(0, n, batch_rows):
        b1 = min(n, b0 + batch_rows)
        rows = torch.arange(b0, b1, dtype=torch.int64, device=index.device)
        try:
            lims, s, ids = index.range_search(D[b0:b1], float(threshold), min_id=rows, max_results=max_edges - total)
        except ValueError as e:
            raise ValueError(f"duplicate_edges: more than max_edges = {max_edges} pairs above {threshold} "
                             f"({total} before rows {b0}:{b1}; {e})") from None
        total += int(ids.numel())
        if ids.numel():
            src.append(torch.repeat_interleave(rows, lims[1:] - lims[:-1]).cpu().numpy())
            dst.append(ids.cpu().numpy())
            score.append(s.cpu().numpy())
    if not src:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(src), np.concatenate(dst), np.concatenate(score)


def _edges(n: int, src, dst) -> Tuple[np.ndarray, np.ndarray]:
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    if src.shape != dst.shape:
        raise ValueError(f"{src.size} sources for {dst.size} destinations")
    if src.size and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= n):
        raise ValueError(f"edge endpoints must lie in [0, {n})")
    return src, dst


def components(n: int, src, dst) -> np.ndarray:
    """-> labels (n,) int64: connected components of the undirected graph on n rows; a component's label is its lowest row id.
    Union-find on whole arrays: every round hooks the root of each edge's higher-labelled end under the lower label, then
    compresses all paths by pointer jumping; labels only ever decrease, and a round without a change ends it."""
    src, dst = _edges(n, src, dst)
    parent = np.arange(n, dtype=np.int64)
    while src.size:
        ls, ld = parent[src], parent[dst]
        differ = ls != ld
        if not differ.any():
            break
        src, dst, ls, ld = src[differ], dst[differ], ls[differ], ld[differ]   # settled edges never differ again
        np.minimum.at(parent, np.maximum(ls, ld), np.minimum(ls, ld))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    return parent


def select_kept(n: int, src, dst, rule: str = "components") -> np.ndarray:
    """-> keep (n,) bool.  rule="components": the lowest id of every connected component (transitive: a chain a~b~c keeps a
    only).  rule="greedy": rows in ascending order, row i is dropped iff an already KEPT row j < i is its neighbour (a chain
    a~b~c with a !~ c keeps a and c)."""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
    src, dst = _edges(n, src, dst)
    if rule == "components":
        return components(n, src, dst) == np.arange(n)
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    real = lo != hi
    lo, hi = lo[real], hi[real]
    order = np.argsort(hi, kind="stable")
    lo, hi = lo[order], hi[order]
    keep = np.ones(n, dtype=bool)
    rows, starts = np.unique(hi, return_index=True)      # ascending: a row's lower neighbours are decided before it
    ends = np.append(starts[1:], hi.size)
    for i, a, b in zip(rows.tolist(), starts.tolist(), ends.tolist()):
        keep[i] = not keep[lo[a:b]].any()
    return keep


def contaminated(train_vectors, eval_index, threshold: float, batch_rows: int = 1 << 16) -> np.ndarray:
    """-> (n,) bool: training row i scores above `threshold` with at least one vector of eval_index (range_count > 0)."""
    n = int(np.shape(train_vectors)[0])
    batch_rows = max(1, int(batch_rows))
    out = np.zeros(n, dtype=bool)
    for b0 in range(0, n, batch_rows):
        x = train_vectors[b0: b0 + batch_rows]
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x, dtype=np.float32))
        out[b0: b0 + batch_rows] = (eval_index.range_count(x.to(eval_index.device), float(threshold)) > 0).cpu().numpy()
    return out
