"""k-means over an embedding set on one GPU, and clustering evaluation on top of it.

`KMeans` is Lloyd's algorithm on bf16 points with fp32 master centroids -- the contract the indexes of contrastors_amd.search
have: points are rounded to bf16 once, every score has the bits `FlatIPIndex.search` gives the pair.  Euclidean mode assigns by
arg-max of x.c - |c|^2 / 2 (the same arg-min as |x - c|^2), spherical mode by arg-max of x.c with unit-norm centroids.  The
assignment is one fused kernel that never writes the (points x centroids) scores (cx_kmeans_assign); the update sums rows by
label without float atomics (cx_kmeans_partial / cx_kmeans_finish over the plan of `_update_plan`), so two runs with the same
seed give the same bits -- curation outputs are diffed between runs.  What it is for: cluster-scoped curation (SemDeDup,
cluster-balanced sampling: "k-means, then work inside clusters"), coarse quantisers, and MTEB-style clustering evaluation:
`evaluate_clustering` reports the V-measure of the k-means labels against true labels (`v_measure`, host numpy, float64).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _C

PIECE_ROWS = 256                 # CX_KMEANS_PIECE_ROWS: rows summed by one workgroup of the update
MAX_ROWS = 2 ** 31 - 129         # cx_kmeans_assign's bound on points and centroids (int ids of the last tile)
ASSIGN_BATCH_ROWS = 1 << 18      # rows cast and uploaded per step when assign() streams


def _check_dim(d: int) -> None:
    if d % 64 or not 64 <= d <= 1024:
        raise ValueError(f"d must be a multiple of 64 in [64, 1024], got {d}")


def _update_plan(labels: torch.Tensor, k: int, piece_rows: int = PIECE_ROWS):
    """The work list of the centroid update, from torch ops on the labels' device (CPU tensors too) without a device-to-host
    synchronisation: -> (order, piece_start, piece_end, piece_cluster, piece_ptr, n_pieces), all int32.

    order (N): the point ids sorted by label, stable -- cluster c is the run order[run_start[c] : run_start[c] + count[c]] in
    ascending id order.  Every run is cut into pieces of at most piece_rows entries; piece p covers
    order[piece_start[p] : piece_end[p]] and belongs to cluster piece_cluster[p]; cluster c owns the pieces
    piece_ptr[c] : piece_ptr[c + 1] (k + 1 entries), in run order.  n_pieces (1,) = piece_ptr[k] stays on the device; the piece
    arrays have the host-known length ceil(N / piece_rows) + k >= n_pieces, entries past n_pieces are (0, 0, -1)."""
    if labels.dim() != 1:
        raise ValueError(f"labels must be 1-d, got shape {tuple(labels.shape)}")
    if k < 1 or piece_rows < 1:
        raise ValueError("k and piece_rows must be positive")
    N, dev = labels.numel(), labels.device
    lab = labels.to(torch.int64)
    order = torch.sort(lab, stable=True).indices
    ids = torch.arange(k, device=dev)
    sorted_lab = lab[order]
    run_start = torch.searchsorted(sorted_lab, ids)
    counts = torch.searchsorted(sorted_lab, ids, right=True) - run_start
    piece_ptr = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    piece_ptr[1:] = torch.cumsum((counts + piece_rows - 1) // piece_rows, 0)
    max_pieces = (N + piece_rows - 1) // piece_rows + k
    p = torch.arange(max_pieces, device=dev)
    live = p < piece_ptr[k]
    cl = torch.searchsorted(piece_ptr[1:], p, right=True).clamp_(max=k - 1)
    start = run_start[cl] + (p - piece_ptr[cl]) * piece_rows
    end = torch.minimum(start + piece_rows, run_start[cl] + counts[cl])
    zero = torch.zeros_like(p)
    i32 = torch.int32
    return (order.to(i32), torch.where(live, start, zero).to(i32), torch.where(live, end, zero).to(i32),
            torch.where(live, cl, zero - 1).to(i32), piece_ptr.to(i32), piece_ptr[k:].to(i32))


def _as_bf16_rows(x, d: int, device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() != 2 or t.shape[1] != d:
        raise ValueError(f"expected a (n, {d}) array, got shape {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.bfloat16).contiguous()


class KMeans:
    """Lloyd's k-means with k centroids of width d on one GPU.  spherical: centroids are kept at unit L2 norm and points go to
    the largest inner product (cosine k-means for normalised embeddings); otherwise Euclidean."""

    def __init__(self, k: int, d: int, spherical: bool = False, device="cuda", seed: int = 0):
        _check_dim(d)
        if not 1 <= int(k) <= MAX_ROWS:
            raise ValueError(f"k must be in [1, {MAX_ROWS}], got {k}")
        self.k, self.d = int(k), int(d)
        self.spherical = bool(spherical)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("KMeans runs on the GPU (cx_kmeans_assign); there is no CPU path")
        self.seed = int(seed)
        self.centroids: Optional[torch.Tensor] = None     # (k, d) fp32 master copy
        self._shadow: Optional[torch.Tensor] = None       # (k, d) bf16: the operand of the assignment
        self._half_norm: Optional[torch.Tensor] = None    # (k,) fp32: |shadow|^2 / 2 (zeros in spherical mode)
        self.labels_: Optional[torch.Tensor] = None
        self.counts_: Optional[torch.Tensor] = None
        self.objective_: Optional[float] = None
        self.n_iter_ = 0
        self.converged_ = False

    # ---- centroids ---------------------------------------------------------------------------------------------------------
    def set_centroids(self, c) -> None:
        """Take (k, d) centroids (copied to fp32 on the device; spherical mode scales them to unit norm)."""
        c = torch.as_tensor(c).to(device=self.device, dtype=torch.float32)
        if tuple(c.shape) != (self.k, self.d):
            raise ValueError(f"expected ({self.k}, {self.d}) centroids, got shape {tuple(c.shape)}")
        c = c.clone()
        if self.spherical:
            c = c / c.norm(dim=1, keepdim=True).clamp_min(1e-30)
        self.centroids = c
        self._shadow = c.to(torch.bfloat16)
        self._half_norm = torch.zeros(self.k, dtype=torch.float32, device=self.device) if self.spherical else \
            0.5 * self._shadow.float().square().sum(1)

    def _require_centroids(self) -> None:
        if self.centroids is None:
            raise RuntimeError("KMeans has no centroids yet: call fit() or set_centroids()")

    # ---- the two device steps ------------------------------------------------------------------------------------------------
    def _assign_dev(self, xb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        n = xb.shape[0]
        labels = torch.empty(n, dtype=torch.int32, device=self.device)
        best = torch.empty(n, dtype=torch.float32, device=self.device)
        second = torch.empty(n, dtype=torch.float32, device=self.device)
        if n:
            with torch.cuda.device(self.device):
                _C.check(_C.lib().cx_kmeans_assign(xb.data_ptr(), self._shadow.data_ptr(),
                                                   None if self.spherical else self._half_norm.data_ptr(), n, self.k, self.d,
                                                   xb.stride(0), self.d, labels.data_ptr(), best.data_ptr(), second.data_ptr(),
                                                   _C.cur_stream()), "cx_kmeans_assign")
        return labels, best, second

    def _update_dev(self, xb: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """Centroids, shadow and half norms of the non-empty clusters from the labelled points -> counts (k,) int32."""
        n = xb.shape[0]
        order, p_start, p_end, _, p_ptr, n_pieces = _update_plan(labels, self.k)
        max_pieces = p_start.numel()
        partial = torch.empty(max_pieces, self.d, dtype=torch.float32, device=self.device)
        counts = torch.empty(self.k, dtype=torch.int32, device=self.device)
        h = _C.lib()
        with torch.cuda.device(self.device):
            stream = _C.cur_stream()
            _C.check(h.cx_kmeans_partial(xb.data_ptr(), n, self.d, xb.stride(0), order.data_ptr(), p_start.data_ptr(),
                                         p_end.data_ptr(), n_pieces.data_ptr(), max_pieces, partial.data_ptr(), stream),
                     "cx_kmeans_partial")
            _C.check(h.cx_kmeans_finish(partial.data_ptr(), p_start.data_ptr(), p_end.data_ptr(), p_ptr.data_ptr(), self.k,
                                        self.d, max_pieces, int(self.spherical), counts.data_ptr(), self.centroids.data_ptr(),
                                        self._shadow.data_ptr(), self.d, self._half_norm.data_ptr(), stream), "cx_kmeans_finish")
        return counts

    def _reseed_empty(self, xb: torch.Tensor, best: torch.Tensor, counts: torch.Tensor) -> int:
        """Empty clusters, in ascending id, take the not-yet-used point with the smallest `best` (ties to the lower point id:
        a stable sort) as their centroid.  -> the number of clusters re-seeded."""
        empty = torch.nonzero(counts == 0).flatten()
        m = min(int(empty.numel()), xb.shape[0])
        if m == 0:
            return 0
        src = torch.sort(best, stable=True).indices[:m]
        rows = xb[src].float()
        if self.spherical:
            rows = rows / rows.norm(dim=1, keepdim=True).clamp_min(1e-30)
        shadow = rows.to(torch.bfloat16)
        self.centroids[empty[:m]] = rows
        self._shadow[empty[:m]] = shadow
        if not self.spherical:
            self._half_norm[empty[:m]] = 0.5 * shadow.float().square().sum(1)
        return m

    def _objective(self, best: torch.Tensor, x_sq: float) -> float:
        """float64, from `best`: the inertia sum |x|^2 - 2 best (Euclidean, minimised) or sum best (spherical, maximised)."""
        s = float(best.double().sum())
        return s if self.spherical else x_sq - 2.0 * s

    def step(self, x):
        """One Lloyd iteration on the points x (n, d): assign to the current centroids, then move every non-empty cluster's
        centroid and re-seed the empty ones.  -> (labels (n,) int32, best (n,) fp32, counts (k,) int32), the assignment the
        new centroids were computed from."""
        self._require_centroids()
        xb = _as_bf16_rows(x, self.d, self.device)
        labels, best, _ = self._assign_dev(xb)
        counts = self._update_dev(xb, labels)
        self._reseed_empty(xb, best, counts)
        self.counts_ = counts
        return labels, best, counts

    # ---- fit ---------------------------------------------------------------------------------------------------------------
    def _initial(self, xb: torch.Tensor, init, run: int) -> torch.Tensor:
        if isinstance(init, str):
            if init != "random":
                raise ValueError(f"init must be 'random' or a ({self.k}, {self.d}) tensor, got {init!r}")
            n = xb.shape[0]
            if n < self.k:
                raise ValueError(f"{n} points for k = {self.k} centroids")
            g = torch.Generator().manual_seed(self.seed + run)
            return xb[torch.randperm(n, generator=g)[: self.k].to(self.device)].float()
        return torch.as_tensor(init)

    def _lloyd(self, xb: torch.Tensor, max_iter: int, tol: float):
        x_sq = 0.0 if self.spherical else float(xb.double().square().sum())
        prev_labels, prev_obj = None, None
        n_iter, converged = 0, False
        while True:
            labels, best, _ = self._assign_dev(xb)
            obj = self._objective(best, x_sq)
            if prev_labels is not None:
                if not bool((labels != prev_labels).any()):
                    converged = True
                else:
                    gain = obj - prev_obj if self.spherical else prev_obj - obj
                    converged = gain <= tol * abs(prev_obj)
            if converged or n_iter == max_iter:
                return labels, obj, n_iter, converged
            n_iter += 1
            counts = self._update_dev(xb, labels)
            self._reseed_empty(xb, best, counts)
            prev_labels, prev_obj = labels, obj

    def fit(self, x, max_iter: int = 25, tol: float = 0.0, n_init: int = 1, init=None, sample: Optional[int] = None):
        """Fit the centroids to x (n, d) -- a tensor or array, rounded to bf16 once.  init: "random" (default: k distinct rows
        through a CPU generator seeded with seed + run) or a (k, d) tensor.  sample: fit on that many rows, a seeded subsample,
        then label all of x.  The loop is assign -> plan -> update; it stops when no label changes, when the relative gain of
        the objective is <= tol, or after max_iter updates.  n_init > 1 keeps the run with the best objective.  Afterwards
        `labels_` (n,) int32, `counts_`, `objective_`, `n_iter_`, `converged_` describe the kept run: labels and objective
        are the assignment to the final centroids."""
        init = "random" if init is None else init
        if max_iter < 1 or n_init < 1:
            raise ValueError("max_iter and n_init must be positive")
        if not isinstance(init, str) and n_init != 1:
            raise ValueError("n_init > 1 needs init='random': given centroids start every run alike")
        xb = _as_bf16_rows(x, self.d, self.device)
        n = xb.shape[0]
        if n == 0:
            raise ValueError("fit: no points")
        xs = xb
        if sample is not None and int(sample) < n:
            if int(sample) < 1:
                raise ValueError(f"sample must be positive, got {sample}")
            g = torch.Generator().manual_seed(self.seed)
            xs = xb[torch.randperm(n, generator=g)[: int(sample)].sort().values.to(self.device)]
        kept = None
        for run in range(n_init):
            self.set_centroids(self._initial(xs, init, run))
            labels, obj, n_iter, converged = self._lloyd(xs, int(max_iter), float(tol))
            better = kept is None or (obj > kept[0] if self.spherical else obj < kept[0])
            if better:
                kept = (obj, labels, n_iter, converged, self.centroids.clone(), self._shadow.clone(), self._half_norm.clone())
        obj, labels, self.n_iter_, self.converged_, self.centroids, self._shadow, self._half_norm = kept
        if xs is not xb:
            labels, best, _ = self._assign_dev(xb)
            obj = self._objective(best, 0.0 if self.spherical else float(xb.double().square().sum()))
        self.labels_ = labels
        self.objective_ = obj
        self.counts_ = torch.bincount(labels.long(), minlength=self.k).to(torch.int32)
        return self

    # ---- streaming assignment ------------------------------------------------------------------------------------------------
    def assign(self, x, batch_rows: Optional[int] = None):
        """-> (labels (n,) int32, best (n,) fp32, second (n,) fp32) of the rows of x against the current centroids: the
        arg-max, its value and the runner-up value (x.c - |c|^2 / 2, or x.c in spherical mode).  x: a tensor on the device or
        the host, a numpy array or a numpy memmap; rows are cast and uploaded batch_rows at a time (default: a device bf16
        tensor in one call, anything else 2^18 rows per step).  numpy in -> numpy out, torch in -> torch out on the device."""
        self._require_centroids()
        as_numpy = not isinstance(x, torch.Tensor)
        if len(np.shape(x)) != 2 or np.shape(x)[1] != self.d:
            raise ValueError(f"expected a (n, {self.d}) array, got shape {tuple(np.shape(x))}")
        n = int(np.shape(x)[0])
        if batch_rows is None:
            on_dev = not as_numpy and x.device == self.device and x.dtype == torch.bfloat16
            batch_rows = max(n, 1) if on_dev else ASSIGN_BATCH_ROWS
        if int(batch_rows) < 1:
            raise ValueError(f"batch_rows must be positive, got {batch_rows}")
        out = [torch.empty(n, dtype=dt, device=self.device) for dt in (torch.int32, torch.float32, torch.float32)]
        for b0 in range(0, n, int(batch_rows)):
            rows = x[b0: b0 + int(batch_rows)]
            rows = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.array(rows))   # (a copy: memmaps are read-only)
            for o, r in zip(out, self._assign_dev(_as_bf16_rows(rows, self.d, self.device))):
                o[b0: b0 + r.numel()] = r
        if as_numpy:
            return tuple(o.cpu().numpy() for o in out)
        return tuple(out)


def v_measure(labels_true, labels_pred) -> Tuple[float, float, float]:
    """-> (homogeneity, completeness, v) of a clustering against true classes (Rosenberg & Hirschberg 2007, beta = 1), in
    float64 from the contingency table: h = 1 - H(C|K) / H(C) = I(C; K) / H(C), c = I(C; K) / H(K), v = 2 h c / (h + c).
    A zero entropy makes its ratio 1 (a single class is homogeneous in any clustering), h + c == 0 makes v 0."""
    t = np.asarray(labels_true).reshape(-1)
    p = np.asarray(labels_pred).reshape(-1)
    if t.size != p.size:
        raise ValueError(f"{t.size} true labels for {p.size} predicted labels")
    if t.size == 0:
        return 1.0, 1.0, 1.0
    _, ti = np.unique(t, return_inverse=True)
    _, pi = np.unique(p, return_inverse=True)
    nt, npred = int(ti.max()) + 1, int(pi.max()) + 1
    table = np.bincount(ti.astype(np.int64) * npred + pi, minlength=nt * npred).reshape(nt, npred).astype(np.float64)
    n = float(t.size)
    a, b = table.sum(1), table.sum(0)

    def entropy(m):
        m = m[m > 0]
        return float(-np.sum(m / n * (np.log(m) - math.log(n))))

    r, c = np.nonzero(table)
    nij = table[r, c]
    mi = max(0.0, float(np.sum(nij / n * ((np.log(nij) - np.log(a[r])) + (math.log(n) - np.log(b[c]))))))
    h_true, h_pred = entropy(a), entropy(b)
    hom = mi / h_true if h_true > 0 else 1.0
    com = mi / h_pred if h_pred > 0 else 1.0
    v = 2.0 * hom * com / (hom + com) if hom + com > 0 else 0.0
    return hom, com, v


def evaluate_clustering(embeddings, labels_true, spherical: bool = True, seed: int = 0, n_init: int = 1, device="cuda") -> dict:
    """The MTEB clustering protocol: k-means with k = the number of distinct true labels, scored by the V-measure of its
    labels.  spherical: the embeddings are L2-normalised and clustered by cosine.  -> {"v_measure", "homogeneity",
    "completeness", "k", "n"}."""
    y = np.asarray(labels_true.cpu() if isinstance(labels_true, torch.Tensor) else labels_true).reshape(-1)
    x = embeddings if isinstance(embeddings, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(embeddings))
    if x.dim() != 2 or x.shape[0] != y.size:
        raise ValueError(f"embeddings of shape {tuple(x.shape)} for {y.size} labels")
    x = x.to(device=device, dtype=torch.float32)
    if spherical:
        x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)
    k = int(np.unique(y).size)
    km = KMeans(k, x.shape[1], spherical=spherical, device=device, seed=seed).fit(x, n_init=n_init)
    hom, com, v = v_measure(y, km.labels_.cpu().numpy())
    return {"v_measure": v, "homogeneity": hom, "completeness": com, "k": k, "n": int(y.size)}
