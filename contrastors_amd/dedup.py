"""Near-duplicate removal and decontamination on the exact range search (FlatIPIndex.range_search / range_count).

The standard recipe: take ALL pairs of corpus rows with cosine above a threshold (`duplicate_edges`, a self-join of the index
in query batches -- a duplicate cluster of any size comes back whole, which a top-k search cannot promise), group them
(`components`) and keep one row per group (`select_kept`); and drop training rows that sit within a threshold of any
evaluation row (`contaminated`).  The GPU work goes through the index; the graph logic is host numpy.

Past the sizes an O(N^2 d) self-join can serve, the pairs are sought inside the parts of a partition -- k-means labels
(SemDeDup), or any partition a curator already has: `cluster_plan` sorts the rows by label, `clustered_duplicate_edges` runs
one windowed self-join per chunk of whole clusters (min_id = own position, end_id = the cluster's end: only the block-diagonal
band of the sorted corpus is computed), and `edge_recall` estimates on a sample of rows what the partition lost.
"""
from __future__ import annotations

from typing import List, Tuple

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


def label_order(labels: np.ndarray) -> np.ndarray:
    """-> (n,) int64: the stable argsort of a 1-d integer host array, so equal labels keep ascending row ids (the sort of
    cluster_plan and of IVFFlatIndex's lists)."""
    key = labels
    if labels.size and int(labels.max()) - int(labels.min()) < 1 << 16:
        key = (labels - labels.min()).astype(np.uint16)      # numpy sorts 16-bit keys by radix: 6 x faster at 2 M rows
    return np.argsort(key, kind="stable").astype(np.int64, copy=False)


def cluster_plan(labels, chunk_rows: int) -> Tuple[np.ndarray, np.ndarray, List[Tuple[int, int]]]:
    """-> (order, end, chunks) for a cluster-scoped self-join.  order (n,) int64: the stable argsort of the labels, so a
    cluster is a run of sorted positions holding ASCENDING row ids; end (n,) int64: the exclusive end, in sorted positions, of
    the run that holds position i; chunks: [b0, b1) position ranges of whole runs with at most chunk_rows rows each (a longer
    run is a chunk of its own), covering [0, n) in order.  labels: any integers (negative, not dense); host arrays."""
    labels = np.asarray(labels).reshape(-1)
    if labels.dtype.kind not in "iu":
        raise ValueError(f"labels: expected integers, got {labels.dtype}")
    chunk_rows = max(1, int(chunk_rows))
    n = labels.size
    order = label_order(labels)
    sl = labels[order]
    starts = np.flatnonzero(np.concatenate([[True], sl[1:] != sl[:-1]])) if n else np.zeros(0, np.int64)
    ends = np.append(starts[1:], n)[: starts.size]
    end = np.repeat(ends, ends - starts).astype(np.int64, copy=False)
    chunks, b0 = [], 0
    for a, b in zip(starts.tolist(), ends.tolist()):
        if b - b0 > chunk_rows and a > b0:      # this run no longer fits: close the chunk before it
            chunks.append((b0, a))
            b0 = a
    if n:
        chunks.append((b0, n))
    return order, end, chunks


def _gather_rows(vectors, rows: np.ndarray, device) -> torch.Tensor:
    """vectors[rows] on the device: a device tensor is indexed there; a host tensor, array or memmap on the host."""
    if isinstance(vectors, torch.Tensor):
        return vectors[torch.from_numpy(rows).to(vectors.device)].to(device)
    return torch.from_numpy(np.ascontiguousarray(vectors[rows])).to(device)


def clustered_duplicate_edges(vectors, labels, threshold: float, chunk_rows: int = 1 << 22,
                              max_edges: int = DEFAULT_MAX_EDGES, device="cuda") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (src int64, dst int64, score float32): `duplicate_edges` restricted to pairs with equal labels -- the same order
    (src < dst, sorted by (src, dst)) and the same score bits.  vectors (n, d): a device tensor, a host array or a memmap
    (rounded to bf16 as FlatIPIndex.add rounds); labels (n,): any integers.

    Per chunk of cluster_plan(labels, chunk_rows) the rows are gathered in label order into an index of their own and ONE
    windowed self-join (min_id = own position, end_id = the cluster's end) walks the block-diagonal band of the chunk; ids map
    back through `order`.  Rows of a cluster keep ascending ids under the stable sort, so src < dst needs no swap.  More than
    max_edges pairs raise ValueError before they are allocated."""
    from .search import FlatIPIndex

    n, d = int(np.shape(vectors)[0]), int(np.shape(vectors)[1])
    if np.shape(labels) != (n,):
        raise ValueError(f"labels has shape {tuple(np.shape(labels))} for {n} rows")
    lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    order, end, chunks = cluster_plan(lab, chunk_rows)
    src, dst, score = [], [], []
    total = 0
    for b0, b1 in chunks:
        index = FlatIPIndex(d, device=device)
        index.add(_gather_rows(vectors, order[b0:b1], index.device))
        pos = torch.arange(b1 - b0, dtype=torch.int64, device=index.device)
        try:
            lims, s, ids = index.range_search(index.vectors, float(threshold), min_id=pos,
                                              end_id=torch.from_numpy(end[b0:b1] - b0), max_results=max_edges - total)
        except ValueError as e:
            raise ValueError(f"clustered_duplicate_edges: more than max_edges = {max_edges} pairs above {threshold} "
                             f"({total} before sorted rows {b0}:{b1}; {e})") from None
        total += int(ids.numel())
        if ids.numel():
            src.append(order[b0 + torch.repeat_interleave(pos, lims[1:] - lims[:-1]).cpu().numpy()])
            dst.append(order[b0 + ids.cpu().numpy()])
            score.append(s.cpu().numpy())
    if not src:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    src, dst, score = np.concatenate(src), np.concatenate(dst), np.concatenate(score)
    by = np.lexsort((dst, src))
    return src[by], dst[by], score[by]


def edge_recall(index, src, dst, threshold: float, sample: int = 4096, seed: int = 0) -> Tuple[int, int, float]:
    """-> (found, exact, recall) of an edge list against the exact answer, on a seeded sample S of the stored rows (sample >= n:
    all rows).  exact = sum over r in S of the number of rows n != r with s(r, n) > threshold -- two range_count calls,
    min_id = r (the rows after r) and end_id = r (the rows before it); found = sum over r in S of r's degree in (src, dst);
    recall = found / exact, 1.0 when exact == 0."""
    n = index.ntotal
    src, dst = _edges(n, src, dst)
    rows = np.arange(n) if int(sample) >= n else np.sort(np.random.default_rng(seed).choice(n, int(sample), replace=False))
    exact = 0
    if rows.size:
        r = torch.from_numpy(rows).to(index.device)
        q = index.vectors[r]
        exact = int(index.range_count(q, float(threshold), min_id=r).sum()) + \
            int(index.range_count(q, float(threshold), end_id=r).sum())
    degree = np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)
    found = int(degree[rows].sum())
    return found, exact, (found / exact if exact else 1.0)


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
