"""Exact inner-product search for the data-curation stage (hard-negative mining, consistency filtering).

`FlatIPIndex` stands where the reference scripts build a faiss `IndexFlatIP` cloned to the GPUs with fp16 storage
(scripts/text/index_filtering.py:364-377, scripts/text/get_negatives.py:163-168): same method names (`add`, `search`,
`ntotal`, `reset`), bf16 storage, one fused HIP kernel per query batch (csrc/search.hip, cx_search_topk) that never writes
the (queries x corpus) scores.  `search` adds what the margin miner needs on top of faiss: per-row excluded ids (the
positives) and a per-row exclusive score bound (margin * s(q, pos)).  `rank` gives the position of given ids in that order
(csrc/rank.hip); `range_count` / `range_search` answer "which rows score above a threshold", however many there are -- faiss's
`range_search`, which faiss has on the CPU only (csrc/range.hip; near-duplicate removal and decontamination on top of it are
in contrastors_amd/dedup.py).

`IVFFlatIndex` searches inside k-means lists instead of the whole corpus (faiss `IndexIVFFlat`): rows sorted by list, one
windowed top-k launch over the (query, probed list) pairs sorted by list, one merge per query (csrc/search.hip,
cx_search_window_topk / cx_topk_merge_lists); with every list probed it is `FlatIPIndex.search` bit for bit.

`BinaryFlatIndex` is the same surface over sign codes (faiss `IndexBinaryFlat`, d / 8 bytes per vector) for the recipes
trained with `hamming: true`; `rescore` / `search_binary_rescored` re-score its candidates exactly against the bf16 rows,
which may stay on the host or in a memory-mapped file (csrc/search_binary.hip).

`Int8FlatIndex` is the format in between (faiss SQ8, sentence-transformers "int8"): d int8 codes + one fp32 scale per row
(`quantize_rows_int8`, csrc/quantize_int8.hip), searched with an exact integer dot product on the matrix cores
(cx_search_int8_topk, csrc/search.hip); `search_int8_rescored` re-scores its candidates exactly like the binary pipeline.

`IVFInt8Index` is both at once (faiss `IndexIVFScalarQuantizer`, QT_8bit): IVFFlatIndex's lists over Int8FlatIndex's codes,
scanned by the windowed int8 kernel (cx_search_int8_window_topk); `search_ivf_int8_rescored` is its two-stage form.

`PQFlatIndex` is the format at the small end (faiss `IndexPQ`, 8 bits per sub-quantiser): d / dsub bytes per row, each the
index of the nearest of 256 trained centroids of a dsub-wide sub-vector (`pq_encode`, csrc/pq.hip), searched with bf16 queries
by the bf16 tile kernel with its document panel gathered from the codebook (cx_search_pq_topk, csrc/search.hip): bit for bit
`FlatIPIndex.search` over the decoded rows; `search_pq_rescored` re-scores its candidates exactly.

`encode` is the embedding side: this project's BiEncoder under no_grad, length-sorted batches, results in input order.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _C

MAX_K = 1024
MAX_NTOTAL = 2 ** 31 - 129        # cx_search_topk's corpus bound (int column indices of the last tile)
DEFAULT_WORKSPACE_BYTES = 1 << 30   # per-batch scratch bound of the kernel's candidate lists; picks the query batch


def _to_device_2d(x, d: int, device) -> torch.Tensor:
    t = torch.as_tensor(x)
    if t.dim() != 2 or t.shape[1] != d:
        raise ValueError(f"expected a (n, {d}) array, got shape {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.bfloat16).contiguous()


def _exclusion_csr_host(exclude, M: int) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """exclude: None, a length-M sequence of id lists, or a (row_ptr (M+1), ids) pair -> int64 host CSR (validated)."""
    if exclude is None:
        return None, None
    if isinstance(exclude, tuple) and len(exclude) == 2 and not isinstance(exclude[0], (list, tuple)):
        row_ptr = torch.as_tensor(np.asarray(exclude[0]), dtype=torch.int64)
        ids = torch.as_tensor(np.asarray(exclude[1]), dtype=torch.int64)
    else:
        if len(exclude) != M:
            raise ValueError(f"exclude has {len(exclude)} rows for {M} queries")
        lens = [len(e) for e in exclude]
        row_ptr = torch.zeros(M + 1, dtype=torch.int64)
        row_ptr[1:] = torch.as_tensor(np.cumsum(lens, dtype=np.int64))
        ids = torch.as_tensor(np.asarray([i for e in exclude for i in e], dtype=np.int64))
    if row_ptr.numel() != M + 1 or int(row_ptr[0]) != 0 or bool((row_ptr[1:] < row_ptr[:-1]).any()) \
            or int(row_ptr[-1]) != ids.numel():
        raise ValueError("exclude: malformed CSR (row_ptr must be M+1 non-decreasing offsets from 0 to len(ids))")
    return row_ptr, ids


def _exclusion_csr(exclude, M: int, device) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """exclude: None, a length-M sequence of id lists, or a (row_ptr (M+1), ids) pair -> int64 device CSR."""
    row_ptr, ids = _exclusion_csr_host(exclude, M)
    if row_ptr is None:
        return None, None
    if ids.numel() == 0:
        ids = torch.zeros(1, dtype=torch.int64)   # a valid pointer; no row reads it
    return row_ptr.to(device), ids.to(device)


TILE = 128                         # rows per query tile and ids per corpus tile of the search kernels


def window_band(min_id, end_id, M: int, N: int) -> torch.Tensor:
    """-> (ceil(M / 128),) int64, on the inputs' device: the corpus tiles t1 - t0 that each 128-row query tile of a windowed
    range search walks (cx_range_window_count).  Over the tile's rows whose window min_id < n < end_id is not empty after
    clamping min_id to [-1, N] and end_id to [0, N]:  t0 = (min min_id + 1) // 128,  t1 = ceil(max end_id / 128);  a tile
    without such a row walks nothing.  min_id / end_id: (M,) int64 tensors or None (-1 / N everywhere).  Its prefix sum is the
    kernel's band_ptr and its sum sizes the workspace."""
    dev = (min_id if min_id is not None else end_id).device if (min_id is not None or end_id is not None) else "cpu"
    mid = torch.full((M,), -1, dtype=torch.int64, device=dev) if min_id is None else min_id.clamp(-1, N)
    end = torch.full((M,), N, dtype=torch.int64, device=dev) if end_id is None else end_id.clamp(0, N)
    tiles_m = (M + TILE - 1) // TILE
    live = end > mid + 1
    pad = tiles_m * TILE - M
    lo = torch.nn.functional.pad(torch.where(live, mid, N), (0, pad), value=N).view(tiles_m, TILE).amin(1)
    hi = torch.nn.functional.pad(torch.where(live, end, 0), (0, pad), value=0).view(tiles_m, TILE).amax(1)
    return torch.where(hi > 0, (hi + TILE - 1) // TILE - (lo + 1) // TILE, 0)


def _window_ws_bytes(M: int, N: int, band_ptr: np.ndarray, mb: int, nsplit: int):
    """cx_range_window_ws_bytes of every query batch of mb rows (mb == M or a multiple of 128)."""
    h = _C.lib()
    out = []
    for b0 in range(0, M, mb):
        m = min(mb, M - b0)
        tiles = int(band_ptr[(b0 + m + TILE - 1) // TILE] - band_ptr[b0 // TILE])
        out.append(h.cx_range_window_ws_bytes(m, N, tiles, nsplit))
    return out


class FlatIPIndex:
    """Exact maximum-inner-product index over bf16 vectors on one GPU (faiss IndexFlatIP with useFloat16)."""

    def __init__(self, d: int, device="cuda", workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        if d % 64 or not 64 <= d <= 1024:
            raise ValueError(f"d must be a multiple of 64 in [64, 1024], got {d}")
        self.d = int(d)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FlatIPIndex runs on the GPU (cx_search_topk); there is no CPU path")
        self.workspace_bytes = int(workspace_bytes)
        self._store: Optional[torch.Tensor] = None   # (capacity, d) bf16; rows [0, ntotal) are the corpus
        self.ntotal = 0

    def reset(self) -> None:
        self._store = None
        self.ntotal = 0

    @property
    def vectors(self) -> torch.Tensor:
        """The stored corpus, (ntotal, d) bf16 (a view)."""
        if self._store is None:
            return torch.empty(0, self.d, dtype=torch.bfloat16, device=self.device)
        return self._store[: self.ntotal]

    def reserve(self, n: int) -> None:
        """Allocate room for n vectors in total, so that adding a corpus in chunks never copies it."""
        if n > MAX_NTOTAL:
            raise ValueError(f"FlatIPIndex holds at most {MAX_NTOTAL} vectors")
        cap = 0 if self._store is None else self._store.shape[0]
        if n > cap:
            grown = torch.empty(n, self.d, dtype=torch.bfloat16, device=self.device)
            if self.ntotal:
                grown[: self.ntotal].copy_(self._store[: self.ntotal])
            self._store = grown

    def add(self, x) -> None:
        """Append rows; fp32 / fp16 inputs are rounded to bf16 (round-to-nearest-even) as faiss rounds to fp16.
        Without a reserve() covering them, the store grows to exactly the new size (one copy of the old rows)."""
        x = _to_device_2d(x, self.d, self.device)
        n = x.shape[0]
        self.reserve(self.ntotal + n)
        self._store[self.ntotal: self.ntotal + n].copy_(x)
        self.ntotal += n

    def batch_rows(self, M: int, k: int) -> int:
        """The largest query batch (all of M, else halved down to a multiple of 128) whose workspace fits the bound."""
        h = _C.lib()
        m = M
        while m > 128 and h.cx_search_ws_bytes(m, max(self.ntotal, 1), k, 0) > self.workspace_bytes:
            m = max(128, (m // 2) // 128 * 128)
        return m

    def search(self, queries, k: int, exclude=None, below=None, nsplit: int = 0):
        """-> (scores (M, k) float32, ids (M, k) int64): per query the k largest inner products with the stored vectors,
        descending, ties to the lower id; missing entries are (-inf, -1).  exclude: per-row ids never returned (a list of
        id lists or a CSR (row_ptr, ids) pair); below: per-row exclusive upper bound on the score.  numpy in -> numpy
        out, torch in -> torch out on the index's device.  nsplit: corpus ranges per launch (0 = chosen; no effect on the
        result)."""
        as_numpy = not isinstance(queries, torch.Tensor)
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        q = _to_device_2d(queries, self.d, self.device)
        M = q.shape[0]
        xptr, xids = _exclusion_csr(exclude, M, self.device)
        bel = None
        if below is not None:
            bel = torch.as_tensor(np.asarray(below) if not isinstance(below, torch.Tensor) else below)
            bel = bel.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
            if bel.numel() != M:
                raise ValueError(f"below has {bel.numel()} entries for {M} queries")
        scores = torch.empty(M, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(M, k, dtype=torch.int64, device=self.device)
        if M:
            h = _C.lib()
            with torch.cuda.device(self.device):
                stream = _C.cur_stream()
                mb = self.batch_rows(M, k)
                ws = None
                if self.ntotal:
                    # the split count (and so the scratch) follows the batch's rows: size it for both batch sizes used
                    last = M - (M - 1) // mb * mb
                    nbytes = max(h.cx_search_ws_bytes(mb, self.ntotal, k, nsplit),
                                 h.cx_search_ws_bytes(last, self.ntotal, k, nsplit))
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                D = self.vectors
                for b0 in range(0, M, mb):
                    m = min(mb, M - b0)
                    _C.check(h.cx_search_topk(q[b0].data_ptr(), D.data_ptr() if self.ntotal else None, m, self.ntotal,
                                              self.d, self.d, self.d, k,
                                              None if xptr is None else xptr[b0:].data_ptr(), _C.ptr(xids),
                                              None if bel is None else bel[b0:].data_ptr(), int(nsplit), _C.ptr(ws),
                                              scores[b0].data_ptr(), ids[b0].data_ptr(), stream), "cx_search_topk")
        if as_numpy:
            return scores.cpu().numpy(), ids.cpu().numpy()
        return scores, ids

    def rank_batch_rows(self, row_ptr: torch.Tensor, nsplit: int = 0) -> int:
        """The largest query batch (all rows, else halved down to a multiple of 128) whose cx_rank_ws_bytes -- for the batch
        with the most targets -- fits the workspace bound.  row_ptr: the host CSR offsets (M + 1)."""
        h = _C.lib()
        M = row_ptr.numel() - 1
        m = M
        while m > 128:
            starts = torch.arange(0, M, m)
            nnz = int((row_ptr[torch.clamp(starts + m, max=M)] - row_ptr[starts]).max())
            if h.cx_rank_ws_bytes(m, max(self.ntotal, 1), nnz, nsplit) <= self.workspace_bytes:
                break
            m = max(128, (m // 2) // 128 * 128)
        return m

    def rank(self, queries, targets, nsplit: int = 0):
        """-> (ranks int64, scores float32, row_ptr int64): for every (query row, target id) entry the number of stored
        vectors that come before the target in search()'s order (descending score, ties to the lower id) -- its 0-based
        position, `search(...)[1][m, rank] == target` wherever rank < k -- and the target's score, with the bits search()
        gives it (cx_rank_targets, csrc/rank.hip; the (M, ntotal) scores are never written).

        targets: a length-M sequence of id lists (rows may be empty or repeat an id), a CSR pair (row_ptr (M + 1), ids), or a
        1-D length-M integer tensor / array (one target per row: ranks and scores come back with shape (M,)).  Entries keep
        the caller's order; row_ptr delimits the rows.  Ids outside [0, ntotal) raise before anything is launched.  numpy
        queries -> numpy out, torch in -> torch out on the index's device.  nsplit has no effect on the result."""
        as_numpy = not isinstance(queries, torch.Tensor)
        q = _to_device_2d(queries, self.d, self.device)
        M = q.shape[0]
        if isinstance(targets, (torch.Tensor, np.ndarray)):
            t = torch.as_tensor(targets).detach().cpu()
            if t.dim() != 1 or t.numel() != M or t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"targets: expected {M} integer ids (one per query), got {tuple(t.shape)} {t.dtype}")
            row_ptr, ids = torch.arange(M + 1, dtype=torch.int64), t.to(torch.int64)
        else:
            try:
                row_ptr, ids = _exclusion_csr_host(targets, M)
            except ValueError as e:
                raise ValueError(str(e).replace("exclude", "targets")) from None
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.ntotal):
            raise ValueError(f"targets: ids must lie in [0, {self.ntotal})")
        nnz = ids.numel()
        ranks = torch.zeros(nnz, dtype=torch.int32, device=self.device)
        scores = torch.zeros(nnz, dtype=torch.float32, device=self.device)
        if nnz and M:
            h = _C.lib()
            with torch.cuda.device(self.device):
                stream = _C.cur_stream()
                mb = self.rank_batch_rows(row_ptr, nsplit)
                dptr, dids = row_ptr.to(self.device), ids.to(self.device)
                D = self.vectors
                ws = None
                for b0 in range(0, M, mb):
                    m = min(mb, M - b0)
                    e0, e1 = int(row_ptr[b0]), int(row_ptr[b0 + m])
                    if e1 == e0:
                        continue
                    nbytes = h.cx_rank_ws_bytes(m, self.ntotal, e1 - e0, nsplit)
                    if ws is None or ws.numel() < nbytes:
                        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                    bptr = dptr[b0: b0 + m + 1] - e0 if b0 else dptr   # offsets from 0 within the batch
                    _C.check(h.cx_rank_targets(q[b0].data_ptr(), D.data_ptr(), m, self.ntotal, self.d, self.d, self.d,
                                               bptr.data_ptr(), dids[e0:].data_ptr(), int(nsplit), ws.data_ptr(),
                                               ranks[e0:].data_ptr(), scores[e0:].data_ptr(), stream), "cx_rank_targets")
        ranks = ranks.to(torch.int64)
        if as_numpy:
            return ranks.cpu().numpy(), scores.cpu().numpy(), row_ptr.numpy()
        return ranks, scores, row_ptr.to(self.device)

    def range_batch_rows(self, M: int, nsplit: int = 0) -> int:
        """The largest query batch (all of M, else halved down to a multiple of 128) whose cx_range_ws_bytes fits the bound."""
        h = _C.lib()
        m = M
        while m > 128 and h.cx_range_ws_bytes(m, max(self.ntotal, 1), nsplit) > self.workspace_bytes:
            m = max(128, (m // 2) // 128 * 128)
        return m

    def _range_bounds(self, radius, min_id, M: int, end_id=None):
        """radius (a scalar or M values), min_id and end_id (None or M ids) -> device tensors (M,) float32 and (M,) int64 / None."""
        if isinstance(radius, (int, float)):
            rad = torch.full((M,), float(radius), dtype=torch.float32, device=self.device)
        else:
            rad = torch.as_tensor(np.asarray(radius) if not isinstance(radius, torch.Tensor) else radius)
            rad = rad.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
            if rad.numel() == 1 and M != 1:
                rad = rad.expand(M).contiguous()
            if rad.numel() != M:
                raise ValueError(f"radius has {rad.numel()} entries for {M} queries")
        ids = []
        for name, v in (("min_id", min_id), ("end_id", end_id)):
            if v is not None:
                v = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v)
                if v.dtype.is_floating_point or v.dtype == torch.bool:
                    raise ValueError(f"{name}: expected integer ids, got {v.dtype}")
                v = v.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
                if v.numel() != M:
                    raise ValueError(f"{name} has {v.numel()} entries for {M} queries")
            ids.append(v)
        return rad, ids[0], ids[1]

    def range_window_batch_rows(self, M: int, band_ptr: np.ndarray, nsplit: int = 0) -> int:
        """The largest query batch (all of M, else halved down to a multiple of 128) whose cx_range_window_ws_bytes fits the
        bound in every batch.  band_ptr: the host prefix sum (tiles_m + 1) of window_band over all M rows."""
        m = M
        while m > 128 and max(_window_ws_bytes(M, self.ntotal, band_ptr, m, nsplit)) > self.workspace_bytes:
            m = max(128, (m // 2) // 128 * 128)
        return m

    def _range_batches(self, q, rad, mid, nsplit: int, end=None):
        """Per query batch, after its count pass: (b0, m, the emit entry point, the C-ABI arguments it shares with the count
        pass (Q .. ws), counts (m,) int64).  One workspace serves all batches: a batch's emit must be launched before the next
        batch is drawn.  end is None: cx_range_count / cx_range_emit; otherwise the windowed pair, whose band description and
        workspace size both come from window_band(mid, end)."""
        h = _C.lib()
        M = q.shape[0]
        D = self.vectors
        stream = _C.cur_stream()
        if end is None:
            mb = self.range_batch_rows(M, nsplit)
            last = M - (M - 1) // mb * mb
            nbytes = max(h.cx_range_ws_bytes(mb, self.ntotal, nsplit), h.cx_range_ws_bytes(last, self.ntotal, nsplit))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            for b0 in range(0, M, mb):
                m = min(mb, M - b0)
                args = (q[b0].data_ptr(), D.data_ptr(), m, self.ntotal, self.d, self.d, self.d, rad[b0:].data_ptr(),
                        None if mid is None else mid[b0:].data_ptr(), int(nsplit), ws.data_ptr())
                counts = torch.empty(m, dtype=torch.int64, device=self.device)
                _C.check(h.cx_range_count(*args, counts.data_ptr(), stream), "cx_range_count")
                yield b0, m, h.cx_range_emit, args, counts
            return
        band_ptr = np.zeros((M + TILE - 1) // TILE + 1, dtype=np.int64)
        np.cumsum(window_band(mid, end, M, self.ntotal).cpu().numpy(), out=band_ptr[1:])   # (the host waits for the band here)
        mb = self.range_window_batch_rows(M, band_ptr, nsplit)
        ws = torch.empty(max(_window_ws_bytes(M, self.ntotal, band_ptr, mb, nsplit)), dtype=torch.uint8, device=self.device)
        for b0 in range(0, M, mb):
            m = min(mb, M - b0)
            t0, t1 = b0 // TILE, (b0 + m + TILE - 1) // TILE
            bp = torch.from_numpy(band_ptr[t0: t1 + 1] - band_ptr[t0]).to(self.device)
            args = (q[b0].data_ptr(), D.data_ptr(), m, self.ntotal, self.d, self.d, self.d, rad[b0:].data_ptr(),
                    None if mid is None else mid[b0:].data_ptr(), end[b0:].data_ptr(), bp.data_ptr(),
                    int(band_ptr[t1] - band_ptr[t0]), int(nsplit), ws.data_ptr())
            counts = torch.empty(m, dtype=torch.int64, device=self.device)
            _C.check(h.cx_range_window_count(*args, counts.data_ptr(), stream), "cx_range_window_count")
            yield b0, m, h.cx_range_window_emit, args, counts   # (bp lives in this frame until the batch's emit is launched)

    def range_count(self, queries, radius, min_id=None, end_id=None, nsplit: int = 0):
        """-> counts (M,) int64: per query the number of stored vectors n with score > radius (strict) and min_id < n < end_id
        (cx_range_count, or cx_range_window_count when end_id is given; csrc/range.hip; the (M, ntotal) scores are never
        written).  radius: a scalar or M values (NaN admits nothing, -inf every finite score); min_id: None (= -1) or M ids;
        end_id: None (= ntotal) or M ids.  numpy in -> numpy out, torch in -> torch out on the index's device.  nsplit has no
        effect on the result."""
        as_numpy = not isinstance(queries, torch.Tensor)
        q = _to_device_2d(queries, self.d, self.device)
        M = q.shape[0]
        rad, mid, end = self._range_bounds(radius, min_id, M, end_id)
        counts = torch.zeros(M, dtype=torch.int64, device=self.device)
        if M and self.ntotal:
            with torch.cuda.device(self.device):
                for b0, m, _, _, c in self._range_batches(q, rad, mid, nsplit, end):
                    counts[b0: b0 + m] = c
        return counts.cpu().numpy() if as_numpy else counts

    def range_search(self, queries, radius, min_id=None, end_id=None, max_results: int = 1 << 27, nsplit: int = 0):
        """-> (lims (M + 1) int64, scores (nnz) float32, ids (nnz) int64), faiss's range_search layout: the stored vectors
        with score > radius[m] (strict) and min_id[m] < id < end_id[m] of query m are entries lims[m] : lims[m + 1], in
        ascending id order, with the score bits search() gives the pair.  However many there are: nothing is cut at a k.

        Per query batch the kernel counts first (cx_range_count); the total is read on the host and a running total above
        max_results raises ValueError BEFORE the batch's results are allocated; only then cx_range_emit writes them (not
        launched for a batch without results).  radius, min_id, end_id, nsplit: as range_count.  min_id = the queries' own
        corpus ids turns a self-join into every unordered pair once; with end_id (the windowed kernels) only the corpus tiles
        between a query tile's smallest min_id and largest end_id are computed, so rows sorted by a partition with
        end_id = the end of the row's part join every part with itself in one call (contrastors_amd.dedup).  numpy in ->
        numpy out, torch in -> torch out."""
        as_numpy = not isinstance(queries, torch.Tensor)
        q = _to_device_2d(queries, self.d, self.device)
        M = q.shape[0]
        rad, mid, end = self._range_bounds(radius, min_id, M, end_id)
        max_results = int(max_results)
        lims = torch.zeros(M + 1, dtype=torch.int64, device=self.device)
        out_s, out_i = [], []
        total = 0
        if M and self.ntotal:
            with torch.cuda.device(self.device):
                stream = _C.cur_stream()
                for b0, m, emit, args, counts in self._range_batches(q, rad, mid, nsplit, end):
                    blims = torch.zeros(m + 1, dtype=torch.int64, device=self.device)
                    torch.cumsum(counts, 0, out=blims[1:])
                    n = int(blims[-1])   # (the host waits for the count pass here)
                    if total + n > max_results:
                        raise ValueError(f"range_search: {total + n} results after {b0 + m} of {M} queries exceed "
                                         f"max_results = {max_results}; raise the radius or max_results")
                    lims[b0 + 1: b0 + m + 1] = blims[1:] + total
                    total += n
                    if n == 0:
                        continue
                    s = torch.empty(n, dtype=torch.float32, device=self.device)
                    i = torch.empty(n, dtype=torch.int64, device=self.device)
                    _C.check(emit(*args, blims.data_ptr(), s.data_ptr(), i.data_ptr(), stream), "cx_range_emit")
                    out_s.append(s)
                    out_i.append(i)
        if len(out_s) == 1:
            scores, ids = out_s[0], out_i[0]
        elif out_s:
            scores, ids = torch.cat(out_s), torch.cat(out_i)
        else:
            scores = torch.empty(0, dtype=torch.float32, device=self.device)
            ids = torch.empty(0, dtype=torch.int64, device=self.device)
        if as_numpy:
            return lims.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()
        return lims, scores, ids


MAX_NPROBE = 256                 # cx_topk_merge_lists' bound on the lists merged into one row


def ivf_pair_plan(probes: torch.Tensor, list_ptr: torch.Tensor):
    """The work list of an IVF search, from torch ops on the inputs' device (CPU tensors too), no host synchronisation.

    probes (M, L) int64: the lists each query probes (in any order; an entry outside [0, nlist) probes nothing);
    list_ptr (nlist + 1) int64: list l holds the sorted-corpus positions list_ptr[l] : list_ptr[l + 1].  The M * L
    (query, list) pairs are stable-sorted by list, so pair rows that share a list are adjacent (in ascending query order) and a
    128-row tile of them spans a short run of consecutive lists.  -> (pair_query (P,), min_id (P,), end_id (P,), src (M, L)),
    int64: pair row r searches query pair_query[r] inside the window min_id[r] < n < end_id[r] = its list, and src[m, j] is
    the pair row of (query m, its j-th probe) -- the lists cx_topk_merge_lists merges into output row m."""
    if probes.dim() != 2 or list_ptr.dim() != 1 or list_ptr.numel() < 1:
        raise ValueError(f"expected probes (M, L) and list_ptr (nlist + 1), got {tuple(probes.shape)} and {tuple(list_ptr.shape)}")
    M, L = probes.shape
    nlist = list_ptr.numel() - 1
    lists = probes.reshape(-1).to(torch.int64)
    lp = list_ptr.to(torch.int64)
    perm = torch.sort(lists, stable=True).indices
    sl = lists[perm]
    ok = (sl >= 0) & (sl < nlist)
    sl = sl.clamp(0, max(nlist - 1, 0))
    zero = torch.zeros_like(sl)
    min_id = torch.where(ok, lp[sl] - 1, zero) if nlist else zero      # (0, 0): an empty window
    end_id = torch.where(ok, lp[sl + 1], zero) if nlist else zero
    src = torch.empty(M * L, dtype=torch.int64, device=probes.device)
    src[perm] = torch.arange(M * L, dtype=torch.int64, device=probes.device)
    return torch.div(perm, max(L, 1), rounding_mode="floor"), min_id, end_id, src.view(M, L)


def ivf_pair_exclusions(row_ptr: torch.Tensor, ids: torch.Tensor, pair_query: torch.Tensor, inv_order: torch.Tensor,
                        nprobe: int):
    """The exclusion lists of the queries (CSR row_ptr (M + 1) from 0, ids: ORIGINAL corpus ids) as a CSR over the pair rows of
    ivf_pair_plan, in sorted-corpus POSITIONS: pair row r gets the list of query pair_query[r], every id through inv_order
    (inv_order[order[p]] = p); ids outside [0, N) become -1, which no position equals.  Every query has nprobe pair rows, so
    the result has nprobe * len(ids) entries -- known on the host, nothing is read back.  -> (pair_ptr (P + 1), pair_ids)."""
    P, N = pair_query.numel(), inv_order.numel()
    dev = pair_query.device
    total = int(nprobe) * ids.numel()
    plen = (row_ptr[1:] - row_ptr[:-1])[pair_query]
    pair_ptr = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    torch.cumsum(plen, 0, out=pair_ptr[1:])
    row = torch.repeat_interleave(torch.arange(P, dtype=torch.int64, device=dev), plen, output_size=total)
    e = row_ptr[pair_query[row]] + (torch.arange(total, dtype=torch.int64, device=dev) - pair_ptr[row])
    x = ids[e]
    ok = (x >= 0) & (x < N)
    pos = inv_order[x.clamp(0, max(N - 1, 0))] if N else x
    return pair_ptr, torch.where(ok, pos, torch.full_like(x, -1))


class _IVFLists:
    """The list bookkeeping of the inverted-file indexes: the coarse quantiser, labelling, the pending chunks, the stable sort
    by label, the pair plan of a search and the merge.  A subclass supplies what is stored per row (a tuple of tensors per chunk,
    kept in self._cols in list order), how many bytes a gathered pair row takes (_pair_row_bytes), how queries are taken
    (_check_queries / _prepare_queries) and which kernel entry scans the pair rows (_ENTRY, _scan)."""

    _ENTRY = ""                      # the windowed top-k entry point of the list scan

    def __init__(self, d: int, nlist: int, device="cuda", workspace_bytes: int = DEFAULT_WORKSPACE_BYTES, seed: int = 0):
        name = type(self).__name__
        if d % 64 or not 64 <= d <= 1024:
            raise ValueError(f"d must be a multiple of 64 in [64, 1024], got {d}")
        if not 1 <= int(nlist) <= MAX_NTOTAL:
            raise ValueError(f"nlist must be in [1, {MAX_NTOTAL}], got {nlist}")
        self.d, self.nlist = int(d), int(nlist)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{name} runs on the GPU ({self._ENTRY}); there is no CPU path")
        self.workspace_bytes = int(workspace_bytes)
        self.seed = int(seed)
        self._centroids: Optional[torch.Tensor] = None    # (nlist, d) fp32
        self._coarse: Optional[FlatIPIndex] = None         # over the centroids' bf16 shadows
        self.reset()

    def reset(self) -> None:
        """Drop the stored rows; the centroids stay."""
        self._cols: Optional[tuple] = None                # what is stored per row, (n sorted, ...) tensors in list order
        self._order: Optional[torch.Tensor] = None        # (n sorted) int64: original id of every sorted position
        self._inv: Optional[torch.Tensor] = None          # (n sorted) int64: its inverse
        self._labels: Optional[torch.Tensor] = None       # (n sorted) int32, ascending
        self._list_ptr: Optional[torch.Tensor] = None     # (nlist + 1) int64
        self._pending = []                                # (per-row tensors, labels) chunks added since the last sort
        self.ntotal = 0

    @property
    def is_trained(self) -> bool:
        return self._centroids is not None

    @property
    def centroids(self) -> torch.Tensor:
        """(nlist, d) fp32; the quantiser compares against their bf16 roundings."""
        self._require_trained()
        return self._centroids

    def _require_trained(self) -> None:
        if self._centroids is None:
            raise RuntimeError(f"{type(self).__name__} has no centroids yet: call train() first")

    def train(self, x=None, max_iter: int = 25, sample: Optional[int] = None, centroids=None) -> None:
        """Fit the nlist centroids to x (n >= nlist rows) with spherical k-means (contrastors_amd.cluster.KMeans, seeded: the
        same x and seed give the same bits; sample: fit on a seeded subsample), or take a given (nlist, d) table as it is."""
        if (x is None) == (centroids is None):
            raise ValueError("train: give either the training rows or centroids=")
        if self.ntotal:
            raise RuntimeError("train: the index holds rows labelled by the current centroids; reset() first")
        if centroids is not None:
            if tuple(np.shape(centroids)) != (self.nlist, self.d):
                raise ValueError(f"expected ({self.nlist}, {self.d}) centroids, got shape {tuple(np.shape(centroids))}")
            c = torch.as_tensor(centroids).to(device=self.device, dtype=torch.float32).clone()
        else:
            from .cluster import KMeans

            km = KMeans(self.nlist, self.d, spherical=True, device=self.device, seed=self.seed)
            c = km.fit(x, max_iter=int(max_iter), sample=sample).centroids
        self._centroids = c
        self._coarse = FlatIPIndex(self.d, device=self.device, workspace_bytes=self.workspace_bytes)
        self._coarse.add(c)

    def _append(self, cols: tuple, xb: torch.Tensor) -> None:
        """One chunk of rows: cols is what the index keeps of them, xb (n, d) their bf16 roundings on the device.  Every row is
        labelled with the list of its largest inner product over the centroids' bf16 roundings, ties to the lower list
        (cx_kmeans_assign without a bias): the first probe the coarse search returns for the same vector."""
        n = xb.shape[0]
        labels = torch.empty(n, dtype=torch.int32, device=self.device)
        best = torch.empty(n, dtype=torch.float32, device=self.device)
        C = self._coarse.vectors
        with torch.cuda.device(self.device):
            _C.check(_C.lib().cx_kmeans_assign(xb.data_ptr(), C.data_ptr(), None, n, self.nlist, self.d, self.d, self.d,
                                               labels.data_ptr(), best.data_ptr(), None, _C.cur_stream()), "cx_kmeans_assign")
        self._pending.append((cols, labels))
        self.ntotal += n

    def _finalise(self) -> None:
        """Sort what was added since the last search into the lists.  The sorted rows and the new chunks are concatenated
        (sorted rows keep ascending ids per list and new ids are larger, so one stable sort by label restores the invariant),
        the sources are released, and the rows are gathered into list order: twice the stored corpus at the peak."""
        if not self._pending:
            return
        from .dedup import label_order

        n_old = 0 if self._cols is None else self._cols[0].shape[0]
        ncol = len(self._pending[0][0])
        cols = [([self._cols[c]] if n_old else []) + [r[c] for r, _ in self._pending] for c in range(ncol)]
        labs = ([self._labels] if n_old else []) + [l for _, l in self._pending]
        ids = ([self._order] if n_old else []) + [torch.arange(n_old, self.ntotal, dtype=torch.int64, device=self.device)]
        self._cols, self._pending = None, []
        lab = labs[0] if len(labs) == 1 else torch.cat(labs)
        ids = ids[0] if len(ids) == 1 else torch.cat(ids)
        perm = torch.from_numpy(label_order(lab.cpu().numpy())).to(self.device)
        out = []
        for c in range(ncol):
            parts, cols[c] = cols[c], None
            x = parts[0] if len(parts) == 1 else torch.cat(parts)
            del parts
            out.append(x[perm])
            del x
        self._cols = tuple(out)
        self._labels = lab[perm]
        self._order = ids[perm]
        self._inv = torch.empty_like(self._order)
        self._inv[self._order] = torch.arange(self.ntotal, dtype=torch.int64, device=self.device)
        self._list_ptr = torch.searchsorted(self._labels, torch.arange(self.nlist + 1, dtype=torch.int32, device=self.device)
                                            ).to(torch.int64)

    @property
    def list_sizes(self) -> torch.Tensor:
        """(nlist,) int64: rows per list."""
        self._require_trained()
        if not self.ntotal:
            return torch.zeros(self.nlist, dtype=torch.int64, device=self.device)
        self._finalise()
        return self._list_ptr[1:] - self._list_ptr[:-1]

    def _pair_row_bytes(self) -> int:
        """Bytes of one gathered query as the scan takes it."""
        raise NotImplementedError

    def batch_queries(self, M: int, k: int, nprobe: int) -> int:
        """Queries per launch: their nprobe pair rows each hold a gathered query, a (k) list in the kernel's workspace and one
        in the merge's input; as many (all of M, else a multiple of 128, at least one) as fit workspace_bytes."""
        per_pair = k * 12 + k * 8 + 4 + self._pair_row_bytes() + 32
        m = self.workspace_bytes // (nprobe * per_pair)
        if m >= 128:
            m = m // 128 * 128
        return max(1, min(M, m))

    def _check_queries(self, queries) -> int:
        """-> M; a wrong shape raises (host only)."""
        if len(np.shape(queries)) != 2 or np.shape(queries)[1] != self.d:
            raise ValueError(f"expected a (n, {self.d}) array, got shape {tuple(np.shape(queries))}")
        return int(np.shape(queries)[0])

    def _prepare_queries(self, queries):
        """-> (the queries rounded to bf16 on the device, for the coarse probe; what _scan gathers its pair rows from)."""
        raise NotImplementedError

    def _scan(self, h, prepared, b0: int, m: int, pair_q, k: int, mid, end, pptr, pids, bg, ws, ls, li, stream) -> None:
        """One windowed top-k launch over the pair rows of queries [b0, b0 + m): lists into (ls, li)."""
        raise NotImplementedError

    def search(self, queries, k: int, nprobe: int, exclude=None, below=None):
        as_numpy = not isinstance(queries, torch.Tensor)
        k, nprobe = int(k), int(nprobe)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        if not 1 <= nprobe <= min(self.nlist, MAX_NPROBE):
            raise ValueError(f"nprobe must be in [1, min(nlist, {MAX_NPROBE})] = [1, {min(self.nlist, MAX_NPROBE)}], got {nprobe}")
        self._require_trained()
        M = self._check_queries(queries)
        row_ptr, xhost = _exclusion_csr_host(exclude, M)
        bel = None
        if below is not None:
            bel = torch.as_tensor(np.asarray(below) if not isinstance(below, torch.Tensor) else below)
            if bel.numel() != M:
                raise ValueError(f"below has {bel.numel()} entries for {M} queries")
            bel = bel.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        q, prepared = self._prepare_queries(queries)
        scores = torch.full((M, k), -float("inf"), dtype=torch.float32, device=self.device)
        ids = torch.full((M, k), -1, dtype=torch.int64, device=self.device)
        if M and self.ntotal:
            self._finalise()
            h = _C.lib()
            with torch.cuda.device(self.device):
                stream = _C.cur_stream()
                probes = self._coarse.search(q, nprobe)[1]
                dptr = xids = None
                if row_ptr is not None and xhost.numel():
                    dptr, xids = row_ptr.to(self.device), xhost.to(self.device)
                mq = self.batch_queries(M, k, nprobe)
                for b0 in range(0, M, mq):
                    m = min(mq, M - b0)
                    P = m * nprobe
                    pair_q, mid, end, src = ivf_pair_plan(probes[b0: b0 + m], self._list_ptr)
                    bg = None if bel is None else bel[b0: b0 + m][pair_q]
                    pptr = pids = None
                    if dptr is not None:
                        e0, e1 = int(row_ptr[b0]), int(row_ptr[b0 + m])      # (host copies)
                        if e1 > e0:
                            pptr, pids = ivf_pair_exclusions(dptr[b0: b0 + m + 1] - e0, xids[e0: e1], pair_q, self._inv, nprobe)
                    ws = torch.empty(h.cx_search_window_ws_bytes(P, k), dtype=torch.uint8, device=self.device)
                    ls = torch.empty(P, k, dtype=torch.float32, device=self.device)
                    li = torch.empty(P, k, dtype=torch.int64, device=self.device)
                    self._scan(h, prepared, b0, m, pair_q, k, mid, end, pptr, pids, bg, ws, ls, li, stream)
                    _C.check(h.cx_topk_merge_lists(ls.data_ptr(), li.data_ptr(), P, k, src.data_ptr(), m, nprobe,
                                                   self._order.data_ptr(), self.ntotal, scores[b0].data_ptr(),
                                                   ids[b0].data_ptr(), stream), "cx_topk_merge_lists")
        if as_numpy:
            return scores.cpu().numpy(), ids.cpu().numpy()
        return scores, ids


class IVFFlatIndex(_IVFLists):
    """Inverted-file index with uncompressed bf16 rows on one GPU (faiss IndexIVFFlat, inner product): a coarse quantiser of
    nlist centroids, every stored row in the list of its best centroid, and a search that scores only the rows of the nprobe
    lists whose centroids are nearest to the query.  Scores have the bits FlatIPIndex.search gives the pair, so probing every
    list returns exactly its result.

    The rows are kept sorted by list (a stable sort: a list is a run of ascending original ids); a search sorts its
    (query, probed list) pairs by list too and ONE windowed top-k launch per batch (cx_search_window_topk) walks, for every
    128-pair tile, only the corpus tiles of the lists that tile probes; cx_topk_merge_lists merges each query's nprobe lists
    and maps positions back to original ids.  No per-list launches; nothing but sizes is read back.

    The sort happens at the first search after an add and needs, at its peak, twice the corpus in device memory (the old
    rows and their gathered copy).  Not here: L2, residual / PQ codes (int8 codes with one scale per row: IVFInt8Index), host
    rows, save / load (centroids go in and out as arrays), incremental adds without a re-sort."""

    _ENTRY = "cx_search_window_topk"

    @property
    def _rows(self) -> Optional[torch.Tensor]:
        """(n sorted, d) bf16 in list order."""
        return None if self._cols is None else self._cols[0]

    def add(self, x) -> None:
        """Append rows (rounded to bf16 as FlatIPIndex.add rounds); row i of the n-th add gets id ntotal + i.  Every row is
        labelled with the list of its largest inner product over the centroids' bf16 roundings, ties to the lower list
        (cx_kmeans_assign without a bias): the first probe the coarse search returns for the same vector."""
        self._require_trained()
        xb = _to_device_2d(x, self.d, self.device)
        if isinstance(x, torch.Tensor) and xb.data_ptr() == x.data_ptr():
            xb = xb.clone()
        n = xb.shape[0]
        if self.ntotal + n > MAX_NTOTAL:
            raise ValueError(f"IVFFlatIndex holds at most {MAX_NTOTAL} vectors")
        if n == 0:
            return
        self._append((xb,), xb)

    def _pair_row_bytes(self) -> int:
        return 2 * self.d

    def _prepare_queries(self, queries):
        q = _to_device_2d(queries, self.d, self.device)
        return q, q

    def _scan(self, h, q, b0, m, pair_q, k, mid, end, pptr, pids, bg, ws, ls, li, stream) -> None:
        qg = q[b0: b0 + m][pair_q]
        _C.check(h.cx_search_window_topk(qg.data_ptr(), self._rows.data_ptr(), pair_q.numel(), self.ntotal, self.d,
                                         self.d, self.d, k, mid.data_ptr(), end.data_ptr(), _C.ptr(pptr), _C.ptr(pids),
                                         _C.ptr(bg), ws.data_ptr(), ls.data_ptr(), li.data_ptr(), stream),
                 "cx_search_window_topk")

    def search(self, queries, k: int, nprobe: int, exclude=None, below=None):
        """-> (scores (M, k) float32, ids (M, k) int64), the conventions of FlatIPIndex.search (descending score, ties to the
        lower id, (-inf, -1) where the probed lists hold fewer than k admissible rows; numpy in -> numpy out) over the rows of
        the nprobe lists nearest to each query, 1 <= nprobe <= min(nlist, 256).  ids, and the ids of exclude, are the ids
        add() gave.  nprobe == nlist is the exact search, bit for bit."""
        return super().search(queries, k, nprobe, exclude=exclude, below=below)


MAX_CANDIDATES = 4096            # cx_rescore_topk's candidate-list bound


def _check_code_dim(d: int) -> None:
    if d % 64 or not 64 <= d <= 1024:
        raise ValueError(f"d must be a multiple of 64 in [64, 1024], got {d}")


def pack_sign_bits(x):
    """Sign codes of the rows of x (n, d): uint8 (n, d / 8) in the layout of numpy.packbits(x > 0, axis=1) -- dimension 0 is
    bit 7 of byte 0; +-0 and NaN give bit 0 -- which is what faiss binary indexes and sentence-transformers "ubinary" take.
    A tensor on the GPU goes through cx_pack_sign_bits (fp32 and bf16 as they are, other dtypes as fp32; a row stride is
    honoured); a CPU tensor or a numpy array through numpy.  Same bytes either way; torch in -> torch out."""
    is_torch = isinstance(x, torch.Tensor)
    if not is_torch:
        x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"expected a (n, d) array, got shape {tuple(x.shape)}")
    n, d = int(x.shape[0]), int(x.shape[1])
    _check_code_dim(d)
    if not is_torch or x.device.type != "cuda":
        a = x.float().numpy() if is_torch else x
        out = np.packbits(a > 0, axis=1)
        return torch.from_numpy(out) if is_torch else out
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    if x.stride(1) != 1 or (n > 1 and x.stride(0) < d):
        x = x.contiguous()
    out = torch.empty(n, d // 8, dtype=torch.uint8, device=x.device)
    if n:
        with torch.cuda.device(x.device):
            _C.check(_C.lib().cx_pack_sign_bits(x.data_ptr(), 0 if x.dtype == torch.float32 else 1, n, d,
                                                x.stride(0) if n > 1 else d, out.data_ptr(), d // 8, _C.cur_stream()),
                     "cx_pack_sign_bits")
    return out


class BinaryFlatIndex:
    """Exact Hamming index over sign codes on one GPU (faiss IndexBinaryFlat; d counts BITS): d / 8 bytes per vector where
    FlatIPIndex keeps 2 d.  Same surface as FlatIPIndex; distances come from cx_search_hamming_topk (csrc/search_binary.hip)."""

    def __init__(self, d: int, device="cuda", workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        _check_code_dim(d)
        self.d = int(d)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BinaryFlatIndex runs on the GPU (cx_search_hamming_topk); there is no CPU path")
        self.workspace_bytes = int(workspace_bytes)
        self._store: Optional[torch.Tensor] = None   # (capacity, d / 8) uint8; rows [0, ntotal) are the corpus
        self.ntotal = 0

    def reset(self) -> None:
        self._store = None
        self.ntotal = 0

    @property
    def codes(self) -> torch.Tensor:
        """The stored codes, (ntotal, d / 8) uint8 (a view)."""
        if self._store is None:
            return torch.empty(0, self.d // 8, dtype=torch.uint8, device=self.device)
        return self._store[: self.ntotal]

    def reserve(self, n: int) -> None:
        """Allocate room for n codes in total, so that adding a corpus in chunks never copies it."""
        if n > MAX_NTOTAL:
            raise ValueError(f"BinaryFlatIndex holds at most {MAX_NTOTAL} vectors")
        cap = 0 if self._store is None else self._store.shape[0]
        if n > cap:
            grown = torch.empty(n, self.d // 8, dtype=torch.uint8, device=self.device)
            if self.ntotal:
                grown[: self.ntotal].copy_(self._store[: self.ntotal])
            self._store = grown

    def _codes_of(self, x) -> torch.Tensor:
        """(n, d) float rows (binarised by sign) or (n, d / 8) uint8 codes -> codes on the index's device."""
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        if t.dim() != 2:
            raise ValueError(f"expected a 2-d array, got shape {tuple(t.shape)}")
        if t.dtype == torch.uint8:
            if t.shape[1] != self.d // 8:
                raise ValueError(f"expected (n, {self.d // 8}) uint8 codes, got shape {tuple(t.shape)}")
            return t.to(self.device).contiguous()
        if t.shape[1] != self.d:
            raise ValueError(f"expected a (n, {self.d}) array, got shape {tuple(t.shape)}")
        return pack_sign_bits(t.to(self.device))

    def add(self, x) -> None:
        """Append rows: float vectors are binarised by sign (x > 0), uint8 (n, d / 8) arrays are taken as codes."""
        c = self._codes_of(x)
        n = c.shape[0]
        self.reserve(self.ntotal + n)
        self._store[self.ntotal: self.ntotal + n].copy_(c)
        self.ntotal += n

    def batch_rows(self, M: int, k: int) -> int:
        h = _C.lib()
        m = M
        while m > 128 and h.cx_search_hamming_ws_bytes(m, max(self.ntotal, 1), k, 0) > self.workspace_bytes:
            m = max(128, (m // 2) // 128 * 128)
        return m

    def search(self, queries, k: int, exclude=None, max_dist=None, nsplit: int = 0):
        """-> (dist (M, k) int32, ids (M, k) int64): per query the k nearest stored codes by Hamming distance, ascending, ties
        to the lower id; missing entries are (INT32_MAX, -1).  queries: float rows or uint8 codes, as for add.  exclude: as
        FlatIPIndex.search; max_dist: per-row INCLUSIVE upper bound on the distance.  numpy in -> numpy out, torch in -> torch
        out on the index's device.  nsplit has no effect on the result."""
        as_numpy = not isinstance(queries, torch.Tensor)
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        M = int(np.shape(queries)[0])
        xptr, xids = _exclusion_csr_host(exclude, M)
        q = self._codes_of(queries)
        if xptr is not None:
            xptr = xptr.to(self.device)
            xids = (xids if xids.numel() else torch.zeros(1, dtype=torch.int64)).to(self.device)
        md = None
        if max_dist is not None:
            md = torch.as_tensor(np.asarray(max_dist) if not isinstance(max_dist, torch.Tensor) else max_dist)
            md = md.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            if md.numel() != M:
                raise ValueError(f"max_dist has {md.numel()} entries for {M} queries")
        dist = torch.empty(M, k, dtype=torch.int32, device=self.device)
        ids = torch.empty(M, k, dtype=torch.int64, device=self.device)
        if M:
            h = _C.lib()
            nb = self.d // 8
            with torch.cuda.device(self.device):
                stream = _C.cur_stream()
                mb = self.batch_rows(M, k)
                ws = None
                if self.ntotal:
                    last = M - (M - 1) // mb * mb
                    nbytes = max(h.cx_search_hamming_ws_bytes(mb, self.ntotal, k, nsplit),
                                 h.cx_search_hamming_ws_bytes(last, self.ntotal, k, nsplit))
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                D = self.codes
                for b0 in range(0, M, mb):
                    m = min(mb, M - b0)
                    _C.check(h.cx_search_hamming_topk(q[b0].data_ptr(), D.data_ptr() if self.ntotal else None, m,
                                                      self.ntotal, self.d, nb, nb, k,
                                                      None if xptr is None else xptr[b0:].data_ptr(), _C.ptr(xids),
                                                      None if md is None else md[b0:].data_ptr(), int(nsplit), _C.ptr(ws),
                                                      dist[b0].data_ptr(), ids[b0].data_ptr(), stream),
                             "cx_search_hamming_topk")
        if as_numpy:
            return dist.cpu().numpy(), ids.cpu().numpy()
        return dist, ids


RESCORE_UPLOAD_BYTES = 1 << 30   # host sources: bf16 bytes of gathered rows uploaded per query batch, at most


def _rescore_call(q, D, cand, ids, k, bel, scores, out_ids):
    M, c = cand.shape
    _C.check(_C.lib().cx_rescore_topk(q.data_ptr(), D.data_ptr() if D.shape[0] else None, cand.data_ptr(), _C.ptr(ids), M,
                                      D.shape[0], q.shape[1], q.stride(0), D.stride(0) if D.shape[0] else q.shape[1], c, k,
                                      _C.ptr(bel), scores.data_ptr(), out_ids.data_ptr(), _C.cur_stream()), "cx_rescore_topk")


def rescore(queries, cand_ids, vectors, k: int, below=None, device=None):
    """Exact re-scoring of per-query candidate lists (the second stage of a binary search).

    queries (M, d); cand_ids (M, c) int64 corpus ids, -1 = no candidate, distinct within a row, c <= 4096; vectors: the
    full-precision corpus, (R, d) -- a bf16 tensor on the GPU, or a CPU tensor / numpy array / numpy memmap (rounded to bf16
    as FlatIPIndex.add rounds).  For a host source the distinct candidate rows of a query batch are gathered on the host,
    uploaded once and the ids remapped, so only candidates ever cross the bus.  -> (scores (M, k) float32, ids (M, k) int64):
    the k best candidates by (score descending, id ascending) with CORPUS ids, (-inf, -1) where there are fewer; below: per-row
    exclusive upper bound on the score.  A pair's score has the bits FlatIPIndex.search gives it.  numpy queries -> numpy
    out.  device: the GPU that scores host rows (default: the queries' GPU, else the current one)."""
    as_numpy = not isinstance(queries, torch.Tensor)
    k = int(k)
    on_device = isinstance(vectors, torch.Tensor) and vectors.device.type == "cuda"
    if on_device:
        dev = vectors.device
    elif device is not None:
        dev = torch.device(device)
    else:   # host rows: score where the queries are, else on the current GPU
        dev = queries.device if not as_numpy and queries.is_cuda else torch.device("cuda")
    if len(np.shape(vectors)) != 2:
        raise ValueError(f"vectors must be (R, d), got shape {tuple(np.shape(vectors))}")
    R, d = int(np.shape(vectors)[0]), int(np.shape(vectors)[1])
    _check_code_dim(d)
    cand = torch.as_tensor(cand_ids if isinstance(cand_ids, torch.Tensor) else np.asarray(cand_ids)).to(torch.int64)
    if cand.dim() != 2:
        raise ValueError(f"cand_ids must be (M, c), got shape {tuple(cand.shape)}")
    M, c = cand.shape
    if not 1 <= c <= MAX_CANDIDATES:
        raise ValueError(f"the candidate lists must hold 1 to {MAX_CANDIDATES} ids, got {c}")
    if not 1 <= k <= min(c, MAX_K):
        raise ValueError(f"k must be in [1, min(c, {MAX_K})] = [1, {min(c, MAX_K)}], got {k}")
    if np.shape(queries)[0] != M:
        raise ValueError(f"{np.shape(queries)[0]} queries for {M} candidate lists")
    q = _to_device_2d(queries, d, dev)
    bel = None
    if below is not None:
        bel = torch.as_tensor(np.asarray(below) if not isinstance(below, torch.Tensor) else below)
        bel = bel.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if bel.numel() != M:
            raise ValueError(f"below has {bel.numel()} entries for {M} queries")
    scores = torch.empty(M, k, dtype=torch.float32, device=dev)
    ids = torch.empty(M, k, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        if on_device:
            D = vectors if vectors.dtype == torch.bfloat16 else vectors.to(torch.bfloat16)
            if D.stride(1) != 1 or D.stride(0) % 8 or D.data_ptr() % 16:
                D = D.contiguous()
            if M:
                _rescore_call(q, D, cand.to(dev).contiguous(), None, k, bel, scores, ids)
        else:
            host = cand.cpu().numpy()
            mb = max(1, RESCORE_UPLOAD_BYTES // (c * d * 2))
            for b0 in range(0, M, mb):
                hb = host[b0: b0 + mb]
                uniq = np.unique(hb[(hb >= 0) & (hb < R)])
                rows = vectors[torch.from_numpy(uniq)] if isinstance(vectors, torch.Tensor) else \
                    torch.from_numpy(np.ascontiguousarray(vectors[uniq]))
                D = rows.to(device=dev, dtype=torch.bfloat16).contiguous()
                local = np.searchsorted(uniq, hb) if uniq.size else np.zeros_like(hb)
                local = np.where((hb >= 0) & (hb < R), local, -1).astype(np.int64)
                _rescore_call(q[b0: b0 + mb], D, torch.from_numpy(local).to(dev), torch.from_numpy(hb).to(dev).contiguous(),
                              k, None if bel is None else bel[b0: b0 + mb], scores[b0: b0 + mb], ids[b0: b0 + mb])
    if as_numpy:
        return scores.cpu().numpy(), ids.cpu().numpy()
    return scores, ids


def _paged_candidates(search_page, M: int, c: int, ntotal: int, exclude) -> torch.Tensor:
    """-> (M, <= c) int64 ids: the first c entries of a coarse ranking whose kernel returns at most 1024 per call.
    search_page(kp, exclude) -> the (M, kp) ids of the top kp under `exclude`.  Lists longer than 1024 are fetched in pages of
    1024, each page excluding the ones before it (the order is strict, so the pages are the consecutive runs of one ranking);
    the loop stops once the pages cover the index."""
    xptr, xids = _exclusion_csr_host(exclude, M)
    pages = []
    for p0 in range(0, c, MAX_K):
        kp = min(MAX_K, c - p0)
        ex = None if xptr is None else (xptr, xids)
        if pages:
            # CSR of (the caller's exclusions + the pages so far) per row
            prev = torch.cat(pages, 1).cpu()
            base = [xids[int(xptr[r]): int(xptr[r + 1])] for r in range(M)] if xptr is not None else [prev[:0, 0]] * M
            rows = [torch.cat([base[r], prev[r][prev[r] >= 0]]) for r in range(M)]
            ptr = torch.zeros(M + 1, dtype=torch.int64)
            ptr[1:] = torch.cumsum(torch.as_tensor([len(r) for r in rows], dtype=torch.int64), 0)
            ex = (ptr.numpy(), (torch.cat(rows) if rows else prev[:0, 0]).numpy())
        pages.append(search_page(kp, ex))
        if ntotal <= p0 + kp:
            break
    return torch.cat(pages, 1) if len(pages) > 1 else pages[0]


def _rescore_candidates(qd, cand, vectors, k: int, below, device, as_numpy: bool):
    """The exact stage of a two-stage search: rescore() of the candidate lists, padded to k columns."""
    M = cand.shape[0]
    s, i = rescore(qd, cand, vectors, min(k, cand.shape[1]), below=below, device=device)
    if s.shape[1] < k:    # fewer candidates than k: an index smaller than k
        s = torch.cat([s, torch.full((M, k - s.shape[1]), -float("inf"), dtype=s.dtype, device=s.device)], 1)
        i = torch.cat([i, torch.full((M, k - i.shape[1]), -1, dtype=i.dtype, device=i.device)], 1)
    if as_numpy:
        return s.cpu().numpy(), i.cpu().numpy()
    return s, i


def _check_rescored_arguments(index, vectors, k: int, rescore_factor: int) -> int:
    """-> the candidate count c of a two-stage search (refusals first)."""
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    if int(rescore_factor) < 1:
        raise ValueError(f"rescore_factor must be at least 1, got {rescore_factor}")
    if np.shape(vectors)[0] != index.ntotal:
        raise ValueError(f"{np.shape(vectors)[0]} vectors for an index of {index.ntotal} codes")
    return max(k, min(k * int(rescore_factor), MAX_CANDIDATES))


def search_binary_rescored(index: BinaryFlatIndex, vectors, queries, k: int, rescore_factor: int = 4, exclude=None,
                           below=None):
    """Coarse Hamming search + exact re-scoring: the min(k * rescore_factor, 4096) nearest codes of `index` per query, then
    the k best of those by exact inner product with `vectors` (the corpus the codes were made from: see rescore).  exclude
    applies to the coarse stage, below to the exact score.  -> (scores, ids) as FlatIPIndex.search; equal to it when the
    candidate lists cover the corpus.  Lists longer than the Hamming kernel's k bound (1024) are fetched in pages
    (_paged_candidates)."""
    k = int(k)
    c = _check_rescored_arguments(index, vectors, k, rescore_factor)
    as_numpy = not isinstance(queries, torch.Tensor)
    M = int(np.shape(queries)[0])
    qd = _to_device_2d(queries, index.d, index.device)
    qc = pack_sign_bits(qd)
    cand = _paged_candidates(lambda kp, ex: index.search(qc, kp, exclude=ex)[1], M, c, index.ntotal, exclude)
    return _rescore_candidates(qd, cand, vectors, k, below, index.device, as_numpy)


INT8_ZERO_AMAX = 2.0 ** -100     # rows whose largest magnitude is below this quantise to zero codes and a zero scale
QUANTIZE_ROWS = 1 << 16          # Int8FlatIndex.add: float rows uploaded and quantised per step


def _quantize_rows_numpy(a: np.ndarray):
    """The contract of cx_quantize_rows_int8 in numpy: every step one IEEE fp32 operation."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    amax = np.abs(a).max(axis=1) if a.shape[0] else np.zeros(0, dtype=np.float32)
    zero = ~(amax >= np.float32(INT8_ZERO_AMAX))
    safe = np.where(zero, np.float32(1), amax).astype(np.float32)
    with np.errstate(all="ignore"):
        inv = np.where(zero, np.float32(0), np.float32(127) / safe).astype(np.float32)
        scale = np.where(zero, np.float32(0), safe / np.float32(127)).astype(np.float32)
        codes = np.clip(np.rint(a * inv[:, None]), np.float32(-127), np.float32(127))
        codes = np.where(np.isnan(codes), np.float32(-127), codes).astype(np.int8)
    return codes, scale


def _quantize_rows_device(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> None:
    """x (n, d) fp32 / bf16 on the GPU (unit column stride) -> codes (n, d) int8 and scales (n) fp32 views, in place."""
    n, d = x.shape
    if n:
        with torch.cuda.device(x.device):
            _C.check(_C.lib().cx_quantize_rows_int8(x.data_ptr(), 0 if x.dtype == torch.float32 else 1, n, d,
                                                    x.stride(0) if n > 1 else d, codes.data_ptr(), codes.stride(0) if n > 1 else d,
                                                    scales.data_ptr(), _C.cur_stream()), "cx_quantize_rows_int8")


def _quantizable(x: torch.Tensor) -> torch.Tensor:
    """A GPU tensor as the kernel takes it: fp32 or bf16 (other dtypes as fp32), unit column stride, rows not overlapping."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def _float_chunks(x, n: int, device):
    """The n float rows of x (a tensor anywhere, an array or a memmap) as the quantiser takes them, QUANTIZE_ROWS rows at a time:
    yields (r0, r1, rows r0 : r1 on the device, fp32 or bf16).  A host source is never on the device as a whole."""
    for r0 in range(0, n, QUANTIZE_ROWS):
        r1 = min(n, r0 + QUANTIZE_ROWS)
        part = x[r0:r1]
        if not isinstance(part, torch.Tensor):
            part = np.asarray(part)
            part = np.ascontiguousarray(part if part.dtype == np.float32 else part.astype(np.float32))
            part = torch.from_numpy(part if part.flags.writeable else part.copy())   # (a read-only memmap slice)
        yield r0, r1, _quantizable(part.to(device))


def quantize_rows_int8(x):
    """Per-row symmetric int8 codes of the rows of x (n, d) -> (codes int8 (n, d), scales float32 (n,)), x ~ codes * scale:
    sentence-transformers' "int8" precision / faiss SQ8 with one range per row.  amax = max |x_j| in fp32; a row with
    amax < 2^-100 gets zero codes and scale 0; otherwise scale = amax / 127 and code_j = clamp(rint(x_j * (127 / amax)), -127,
    127), every step one IEEE fp32 operation with round-half-to-even (-128 never occurs).  A tensor on the GPU goes through
    cx_quantize_rows_int8 (fp32 and bf16 as they are, other dtypes as fp32; a row stride is honoured); a CPU tensor or a numpy
    array through numpy.  Same bytes either way for finite input; torch in -> torch out.  Non-finite input never faults and is
    otherwise unspecified: the kernel skips NaN in the maximum and gives a NaN product the code -127, numpy turns a row that
    holds a NaN into a zero row; an infinite element gives scale inf either way."""
    is_torch = isinstance(x, torch.Tensor)
    if not is_torch:
        x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"expected a (n, d) array, got shape {tuple(x.shape)}")
    n, d = int(x.shape[0]), int(x.shape[1])
    _check_code_dim(d)
    if not is_torch or x.device.type != "cuda":
        codes, scales = _quantize_rows_numpy(x.float().numpy() if is_torch else x)
        return (torch.from_numpy(codes), torch.from_numpy(scales)) if is_torch else (codes, scales)
    codes = torch.empty(n, d, dtype=torch.int8, device=x.device)
    scales = torch.empty(n, dtype=torch.float32, device=x.device)
    _quantize_rows_device(_quantizable(x), codes, scales)
    return codes, scales


def _is_code_pair(x) -> bool:
    return isinstance(x, tuple) and len(x) == 2


class Int8FlatIndex:
    """Maximum-inner-product index over int8 scalar-quantised rows on one GPU (faiss IndexScalarQuantizer QT_8bit with one
    range per row; sentence-transformers "int8"): d bytes + one fp32 scale per vector where FlatIPIndex keeps 2 d bytes.  Same
    surface as FlatIPIndex / BinaryFlatIndex.  The score of a pair is ((float)(q_codes . d_codes) * d_scale) * q_scale with an
    exact integer dot product (cx_search_int8_topk, csrc/search.hip): queries are quantised per row as the corpus is.
    search_int8_rescored re-scores its candidates exactly against the float rows."""

    def __init__(self, d: int, device="cuda", workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        _check_code_dim(d)
        self.d = int(d)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Int8FlatIndex runs on the GPU (cx_search_int8_topk); there is no CPU path")
        self.workspace_bytes = int(workspace_bytes)
        self._store: Optional[torch.Tensor] = None    # (capacity, d) int8; rows [0, ntotal) are the corpus
        self._scale: Optional[torch.Tensor] = None    # (capacity,) fp32
        self.ntotal = 0

    def reset(self) -> None:
        self._store = None
        self._scale = None
        self.ntotal = 0

    @property
    def codes(self) -> torch.Tensor:
        """The stored codes, (ntotal, d) int8 (a view)."""
        if self._store is None:
            return torch.empty(0, self.d, dtype=torch.int8, device=self.device)
        return self._store[: self.ntotal]

    @property
    def scales(self) -> torch.Tensor:
        """The stored scales, (ntotal,) float32 (a view)."""
        if self._scale is None:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        return self._scale[: self.ntotal]

    def reserve(self, n: int) -> None:
        """Allocate room for n vectors in total, so that adding a corpus in chunks never copies it."""
        if n > MAX_NTOTAL:
            raise ValueError(f"Int8FlatIndex holds at most {MAX_NTOTAL} vectors")
        cap = 0 if self._store is None else self._store.shape[0]
        if n > cap:
            grown = torch.empty(n, self.d, dtype=torch.int8, device=self.device)
            gscale = torch.empty(n, dtype=torch.float32, device=self.device)
            if self.ntotal:
                grown[: self.ntotal].copy_(self._store[: self.ntotal])
                gscale[: self.ntotal].copy_(self._scale[: self.ntotal])
            self._store, self._scale = grown, gscale

    def _check_pair(self, pair):
        """A (codes int8 (n, d), scales float32 (n,)) tuple -> host-or-device tensors, shapes and dtypes checked."""
        c, s = (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t)) for t in pair)
        if c.dtype != torch.int8 or c.dim() != 2 or c.shape[1] != self.d:
            raise ValueError(f"expected (n, {self.d}) int8 codes, got {tuple(c.shape)} {c.dtype}")
        if s.dtype != torch.float32 or s.dim() != 1 or s.shape[0] != c.shape[0]:
            raise ValueError(f"expected ({c.shape[0]},) float32 scales, got {tuple(s.shape)} {s.dtype}")
        return c, s

    def _check_rows(self, x) -> int:
        if len(np.shape(x)) != 2 or np.shape(x)[1] != self.d:
            raise ValueError(f"expected a (n, {self.d}) array, got shape {tuple(np.shape(x))}")
        return int(np.shape(x)[0])

    def _quantize_into(self, x, codes: torch.Tensor, scales: torch.Tensor) -> None:
        """Float rows x (a tensor anywhere, an array or a memmap) -> the given device views, QUANTIZE_ROWS rows at a time: a host
        source is never on the device as a whole."""
        for r0, r1, part in _float_chunks(x, codes.shape[0], self.device):
            _quantize_rows_device(part, codes[r0:r1], scales[r0:r1])

    def add(self, x) -> None:
        """Append rows: float vectors are quantised per row on the device (quantize_rows_int8's contract), a
        (codes int8 (n, d), scales float32 (n,)) tuple is taken as it is."""
        if _is_code_pair(x):
            c, s = self._check_pair(x)
            n = c.shape[0]
            self.reserve(self.ntotal + n)
            self._store[self.ntotal: self.ntotal + n].copy_(c)
            self._scale[self.ntotal: self.ntotal + n].copy_(s)
        else:
            n = self._check_rows(x)
            self.reserve(self.ntotal + n)
            self._quantize_into(x, self._store[self.ntotal: self.ntotal + n], self._scale[self.ntotal: self.ntotal + n])
        self.ntotal += n

    def batch_rows(self, M: int, k: int) -> int:
        """The largest query batch (all of M, else halved down to a multiple of 128) whose workspace fits the bound."""
        h = _C.lib()
        m = M
        while m > 128 and h.cx_search_int8_ws_bytes(m, max(self.ntotal, 1), k, 0) > self.workspace_bytes:
            m = max(128, (m // 2) // 128 * 128)
        return m

    def _query_codes(self, queries):
        """float rows or a (codes, scales) tuple -> (codes (M, d) int8, scales (M,) fp32) on the index's device."""
        if _is_code_pair(queries):
            c, s = self._check_pair(queries)
            return c.to(self.device).contiguous(), s.to(self.device).contiguous()
        M = self._check_rows(queries)
        qc = torch.empty(M, self.d, dtype=torch.int8, device=self.device)
        qs = torch.empty(M, dtype=torch.float32, device=self.device)
        self._quantize_into(queries, qc, qs)
        return qc, qs

    def search(self, queries, k: int, exclude=None, below=None, nsplit: int = 0):
        """-> (scores (M, k) float32, ids (M, k) int64): per query the k largest int8 scores, descending, ties to the lower id;
        missing entries are (-inf, -1).  queries: float rows (quantised per row) or a (codes, scales) tuple, as for add.
        exclude, below (a strict bound on the int8 score), nsplit: as FlatIPIndex.search.  numpy in -> numpy out, torch in ->
        torch out on the index's device."""
        first = queries[0] if _is_code_pair(queries) else queries
        as_numpy = not isinstance(first, torch.Tensor)
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        if _is_code_pair(queries):
            M = self._check_pair(queries)[0].shape[0]
        else:
            M = self._check_rows(queries)
        xptr, xids = _exclusion_csr_host(exclude, M)
        bel = None
        if below is not None:
            bel = torch.as_tensor(np.asarray(below) if not isinstance(below, torch.Tensor) else below)
            if bel.numel() != M:
                raise ValueError(f"below has {bel.numel()} entries for {M} queries")
            bel = bel.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        qc, qs = self._query_codes(queries)
        if xptr is not None:
            xptr = xptr.to(self.device)
            xids = (xids if xids.numel() else torch.zeros(1, dtype=torch.int64)).to(self.device)
        scores = torch.empty(M, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(M, k, dtype=torch.int64, device=self.device)
        if M:
            h = _C.lib()
            with torch.cuda.device(self.device):
                stream = _C.cur_stream()
                mb = self.batch_rows(M, k)
                ws = None
                if self.ntotal:
                    last = M - (M - 1) // mb * mb
                    nbytes = max(h.cx_search_int8_ws_bytes(mb, self.ntotal, k, nsplit),
                                 h.cx_search_int8_ws_bytes(last, self.ntotal, k, nsplit))
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                D, ds = self.codes, self.scales
                for b0 in range(0, M, mb):
                    m = min(mb, M - b0)
                    _C.check(h.cx_search_int8_topk(qc[b0].data_ptr(), D.data_ptr() if self.ntotal else None,
                                                   qs[b0:].data_ptr(), ds.data_ptr() if self.ntotal else None, m, self.ntotal,
                                                   self.d, self.d, self.d, k,
                                                   None if xptr is None else xptr[b0:].data_ptr(), _C.ptr(xids),
                                                   None if bel is None else bel[b0:].data_ptr(), int(nsplit), _C.ptr(ws),
                                                   scores[b0].data_ptr(), ids[b0].data_ptr(), stream), "cx_search_int8_topk")
        if as_numpy:
            return scores.cpu().numpy(), ids.cpu().numpy()
        return scores, ids


def search_int8_rescored(index: Int8FlatIndex, vectors, queries, k: int, rescore_factor: int = 2, exclude=None, below=None):
    """Coarse int8 search + exact re-scoring: the min(k * rescore_factor, 4096) best int8 scores of `index` per query, then the
    k best of those by exact inner product with `vectors` (the corpus the codes were made from: device bf16 rows, a host array
    or a memmap; see rescore).  queries: float rows.  exclude applies to the coarse stage, below to the exact score.
    -> (scores, ids) as FlatIPIndex.search; equal to it bit for bit when the candidate lists cover the corpus.  Lists longer
    than the kernel's k bound (1024) are fetched in pages (_paged_candidates)."""
    k = int(k)
    c = _check_rescored_arguments(index, vectors, k, rescore_factor)
    as_numpy = not isinstance(queries, torch.Tensor)
    M = index._check_rows(queries)
    _exclusion_csr_host(exclude, M)   # (malformed filters raise before any launch)
    if below is not None and int(np.size(below)) != M:
        raise ValueError(f"below has {int(np.size(below))} entries for {M} queries")
    qd = _to_device_2d(queries, index.d, index.device)
    qc = index._query_codes(queries)
    cand = _paged_candidates(lambda kp, ex: index.search(qc, kp, exclude=ex)[1], M, c, index.ntotal, exclude)
    return _rescore_candidates(qd, cand, vectors, k, below, index.device, as_numpy)


class IVFInt8Index(_IVFLists):
    """Inverted-file index over int8 scalar-quantised rows on one GPU (faiss IndexIVFScalarQuantizer, QT_8bit with one range per
    row, inner product): IVFFlatIndex's lists -- the same centroids and rows give the same lists -- holding Int8FlatIndex's
    codes and scales, d bytes + one fp32 scale per row.  A search probes the nprobe nearest lists with the bf16 queries, as
    IVFFlatIndex does, and scans them with the queries quantised per row: one cx_search_int8_window_topk launch per query batch
    over the (query, probed list) pairs, one cx_topk_merge_lists call.  Scores have the bits Int8FlatIndex.search gives the
    pair, so probing every list returns exactly its result; search_ivf_int8_rescored re-scores the candidates exactly.

    The sort happens at the first search after an add and may still peak at twice the int8 corpus in device memory (the
    concatenated codes and their gathered copy).  Not here: adding (codes, scales, labels) made elsewhere, an in-place sort,
    int8 re-scoring, save / load, more than one GPU."""

    _ENTRY = "cx_search_int8_window_topk"

    @property
    def codes(self) -> torch.Tensor:
        """The stored codes in list order, (ntotal, d) int8 (a view): row p is the row add() gave the id _order[p]."""
        self._finalise()
        if self._cols is None:
            return torch.empty(0, self.d, dtype=torch.int8, device=self.device)
        return self._cols[0]

    @property
    def scales(self) -> torch.Tensor:
        """The stored scales in list order, (ntotal,) float32 (a view)."""
        self._finalise()
        if self._cols is None:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        return self._cols[1]

    def add(self, x) -> None:
        """Append float rows (a tensor anywhere, an array or a memmap; codes are not taken); row i of the n-th add gets id
        ntotal + i.  The rows go through the device QUANTIZE_ROWS at a time: each chunk is quantised per row exactly as
        Int8FlatIndex.add quantises it, and labelled from its bf16 rounding exactly as IVFFlatIndex.add labels it; only the
        codes, the scales and the labels stay."""
        self._require_trained()
        if _is_code_pair(x):
            raise ValueError("IVFInt8Index.add takes float rows, not a (codes, scales) pair")
        n = self._check_queries(x)
        if self.ntotal + n > MAX_NTOTAL:
            raise ValueError(f"IVFInt8Index holds at most {MAX_NTOTAL} vectors")
        for r0, r1, part in _float_chunks(x, n, self.device):
            codes = torch.empty(r1 - r0, self.d, dtype=torch.int8, device=self.device)
            scales = torch.empty(r1 - r0, dtype=torch.float32, device=self.device)
            _quantize_rows_device(part, codes, scales)
            self._append((codes, scales), part.to(torch.bfloat16).contiguous())

    def _pair_row_bytes(self) -> int:
        return self.d + 4

    def _prepare_queries(self, queries):
        M = int(np.shape(queries)[0])
        qb = torch.empty(M, self.d, dtype=torch.bfloat16, device=self.device)
        qc = torch.empty(M, self.d, dtype=torch.int8, device=self.device)
        qs = torch.empty(M, dtype=torch.float32, device=self.device)
        for r0, r1, part in _float_chunks(queries, M, self.device):
            qb[r0:r1].copy_(part)
            _quantize_rows_device(part, qc[r0:r1], qs[r0:r1])
        return qb, (qc, qs)

    def _scan(self, h, prepared, b0, m, pair_q, k, mid, end, pptr, pids, bg, ws, ls, li, stream) -> None:
        qc, qs = prepared
        cg, sg = qc[b0: b0 + m][pair_q], qs[b0: b0 + m][pair_q]
        D, ds = self._cols
        _C.check(h.cx_search_int8_window_topk(cg.data_ptr(), D.data_ptr(), sg.data_ptr(), ds.data_ptr(), pair_q.numel(),
                                              self.ntotal, self.d, self.d, self.d, k, mid.data_ptr(), end.data_ptr(),
                                              _C.ptr(pptr), _C.ptr(pids), _C.ptr(bg), ws.data_ptr(), ls.data_ptr(),
                                              li.data_ptr(), stream), "cx_search_int8_window_topk")

    def search(self, queries, k: int, nprobe: int, exclude=None, below=None):
        """-> (scores (M, k) float32, ids (M, k) int64), the conventions of Int8FlatIndex.search (descending int8 score, ties to
        the lower id, (-inf, -1) where the probed lists hold fewer than k admissible rows; numpy in -> numpy out) over the rows
        of the nprobe lists nearest to each query, 1 <= nprobe <= min(nlist, 256).  queries: float rows, rounded to bf16 for the
        probe over the centroids and quantised per row for the scan.  ids, and the ids of exclude, are the ids add() gave; below
        is a strict bound on the int8 score.  nprobe == nlist is Int8FlatIndex.search, bit for bit."""
        if _is_code_pair(queries):
            raise ValueError("IVFInt8Index.search takes float queries, not a (codes, scales) pair")
        return super().search(queries, k, nprobe, exclude=exclude, below=below)


def search_ivf_int8_rescored(index: IVFInt8Index, vectors, queries, k: int, nprobe: int, rescore_factor: int = 2, exclude=None,
                             below=None):
    """search_int8_rescored over an IVFInt8Index: the min(k * rescore_factor, 4096) best int8 scores among the rows of the
    nprobe lists nearest to each query, then the k best of those by exact inner product with `vectors` (the corpus the index
    was made from, in add() order: device bf16 rows, a host array or a memmap; see rescore).  queries: float rows.  exclude
    applies to the coarse stage, below to the exact score.  -> (scores, ids) as FlatIPIndex.search; equal to it bit for bit
    when every list is probed and the candidate lists cover the corpus."""
    k, nprobe = int(k), int(nprobe)
    c = _check_rescored_arguments(index, vectors, k, rescore_factor)
    if not 1 <= nprobe <= min(index.nlist, MAX_NPROBE):
        raise ValueError(f"nprobe must be in [1, min(nlist, {MAX_NPROBE})] = [1, {min(index.nlist, MAX_NPROBE)}], got {nprobe}")
    index._require_trained()
    as_numpy = not isinstance(queries, torch.Tensor)
    M = index._check_queries(queries)
    _exclusion_csr_host(exclude, M)   # (malformed filters raise before any launch)
    if below is not None:
        n_below = below.numel() if isinstance(below, torch.Tensor) else int(np.size(below))
        if n_below != M:
            raise ValueError(f"below has {n_below} entries for {M} queries")
    qd = _to_device_2d(queries, index.d, index.device)
    qf = queries if isinstance(queries, torch.Tensor) else torch.from_numpy(np.array(queries, dtype=np.float32))
    qf = _quantizable(qf.to(index.device))   # (once: a page of candidates quantises it again, to the same codes)
    cand = _paged_candidates(lambda kp, ex: index.search(qf, kp, nprobe, exclude=ex)[1], M, c, index.ntotal, exclude)
    return _rescore_candidates(qd, cand, vectors, k, below, index.device, as_numpy)


PQ_KSUB = 256                    # centroids per sub-quantiser: a code is one byte
PQ_DSUBS = (8, 16, 32, 64)       # sub-vector widths: a 16-byte piece of a bf16 row lies inside one centroid
PQ_DEFAULT_SAMPLE = 1 << 16      # PQFlatIndex.train: rows sampled by default, at most
PQ_MAX_SAMPLE = 1 << 18          # ... and the largest explicit sample (the update adds in row order, one thread per cell)


def _check_pq_dims(d: int, dsub: int) -> int:
    """-> m = d / dsub (refusals first)."""
    _check_code_dim(d)
    if dsub not in PQ_DSUBS:
        raise ValueError(f"dsub must be one of {PQ_DSUBS}, got {dsub}")
    return d // dsub


def _np_bf16(a: np.ndarray) -> np.ndarray:
    """fp32 array -> the nearest bf16 values (ties to even) as fp32: the rounding of torch's .to(bfloat16), finite input."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(a.shape)


def _np_fmaf(a, b, c):
    """fp32 fmaf of bf16-valued a, b and fp32 c: the float64 sum is exact for such operands (tests/pq_ref.py), so rounding it
    to fp32 is the one rounding of the fused operation."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _pq_half_norm_numpy(shadow: np.ndarray) -> np.ndarray:
    h = np.zeros(shadow.shape[:-1], np.float32)
    for j in range(shadow.shape[-1]):
        h = _np_fmaf(shadow[..., j], shadow[..., j], h)
    return (np.float32(0.5) * h).astype(np.float32)


def _pq_encode_numpy(x: np.ndarray, shadow: np.ndarray) -> np.ndarray:
    """cx_pq_assign's contract in numpy: every step one IEEE fp32 operation, ties to the lower code."""
    xb = _np_bf16(x)
    m, _, dsub = shadow.shape
    hn = _pq_half_norm_numpy(shadow)
    codes = np.zeros((xb.shape[0], m), np.uint8)
    for s in range(m):
        acc = np.zeros((xb.shape[0], PQ_KSUB), np.float32)
        for j in range(dsub):
            acc = _np_fmaf(xb[:, s * dsub + j, None], shadow[s, None, :, j], acc)
        codes[:, s] = np.argmax((acc - hn[s][None, :]).astype(np.float32), axis=1)
    return codes


def _pq_half_norm_device(shadow: torch.Tensor) -> torch.Tensor:
    m, _, dsub = shadow.shape
    hn = torch.empty(m, PQ_KSUB, dtype=torch.float32, device=shadow.device)
    with torch.cuda.device(shadow.device):
        _C.check(_C.lib().cx_pq_half_norm(shadow.data_ptr(), m * dsub, dsub, hn.data_ptr(), _C.cur_stream()), "cx_pq_half_norm")
    return hn


def _pq_assign_device(xb: torch.Tensor, shadow: torch.Tensor, hn: torch.Tensor, codes: torch.Tensor) -> None:
    """xb (n, d) bf16 on the GPU (unit column stride) -> codes (n, m) uint8 view (unit column stride), in place."""
    n, d = xb.shape
    m, _, dsub = shadow.shape
    if n:
        with torch.cuda.device(xb.device):
            _C.check(_C.lib().cx_pq_assign(xb.data_ptr(), n, d, xb.stride(0) if n > 1 else d, shadow.data_ptr(), hn.data_ptr(),
                                           dsub, codes.data_ptr(), codes.stride(0) if n > 1 else m, _C.cur_stream()),
                     "cx_pq_assign")


def _pq_rows(x: torch.Tensor) -> torch.Tensor:
    """A GPU tensor as cx_pq_assign takes it: bf16 (other dtypes rounded as FlatIPIndex.add rounds), unit column stride, rows
    not overlapping."""
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def _check_codebooks(codebooks, d: Optional[int] = None, dsub: Optional[int] = None):
    shape = tuple(np.shape(codebooks))
    if len(shape) != 3 or shape[1] != PQ_KSUB or shape[2] not in PQ_DSUBS:
        raise ValueError(f"expected (m, {PQ_KSUB}, dsub) codebooks with dsub in {PQ_DSUBS}, got shape {shape}")
    if d is not None and (shape[2] != dsub or shape[0] * shape[2] != d):
        raise ValueError(f"expected ({d // dsub}, {PQ_KSUB}, {dsub}) codebooks, got shape {shape}")
    _check_code_dim(shape[0] * shape[2])
    return shape


def pq_encode(x, codebooks):
    """Product-quantiser codes of the rows of x (n, d) against codebooks (m, 256, dsub), m * dsub = d -> uint8 (n, m): faiss
    IndexPQ's encoding with 8 bits per sub-quantiser under inner-product-free nearest-centroid assignment.  x is rounded to bf16
    (as FlatIPIndex.add rounds) and so are the codebooks (PQFlatIndex.codebooks already is the bf16 shadow); per sub-vector
    the code is the arg-max of fmaf-chain(x . c) - 0.5f * fmaf-chain(c . c), ties to the lower code (tests/pq_ref.py is the
    contract).  A tensor on the GPU goes through cx_pq_assign (a row stride is honoured); a CPU tensor or a numpy array through
    numpy.  Same bytes either way for finite input; torch in -> torch out."""
    is_torch = isinstance(x, torch.Tensor)
    if not is_torch:
        x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"expected a (n, d) array, got shape {tuple(x.shape)}")
    m, _, dsub = _check_codebooks(codebooks)
    n, d = int(x.shape[0]), int(x.shape[1])
    if d != m * dsub:
        raise ValueError(f"expected a (n, {m * dsub}) array for ({m}, {PQ_KSUB}, {dsub}) codebooks, got shape {tuple(x.shape)}")
    if not is_torch or x.device.type != "cuda":
        cb = codebooks.detach().cpu().float().numpy() if isinstance(codebooks, torch.Tensor) else np.asarray(codebooks, np.float32)
        codes = _pq_encode_numpy(x.float().numpy() if is_torch else x, _np_bf16(cb))
        return torch.from_numpy(codes) if is_torch else codes
    shadow = torch.as_tensor(codebooks).to(device=x.device, dtype=torch.bfloat16).contiguous()
    codes = torch.empty(n, m, dtype=torch.uint8, device=x.device)
    _pq_assign_device(_pq_rows(x), shadow, _pq_half_norm_device(shadow), codes)
    return codes


def pq_train_rows(n: int, sample: Optional[int], seed: int):
    """The rows PQFlatIndex.train fits on and starts from -> (sample rows (ns,) int64 ascending, or None = all n rows;
    initial rows (256,) int64, positions INSIDE the sample).  The sample is KMeans.fit(sample=)'s seeded choice; the initial
    centroids of every sub-quantiser are the sub-vectors of the first 256 rows of a permutation seeded the same way."""
    rows = None
    ns = n
    if sample is not None and int(sample) < n:
        g = torch.Generator().manual_seed(seed)
        rows = torch.randperm(n, generator=g)[: int(sample)].sort().values
        ns = int(sample)
    g = torch.Generator().manual_seed(seed)
    return rows, torch.randperm(ns, generator=g)[:PQ_KSUB]


class PQFlatIndex:
    """Maximum-inner-product index over product-quantised rows on one GPU (faiss IndexPQ, 8 bits per sub-quantiser, asymmetric
    scoring): d / dsub bytes per vector -- with dsub = 8 what BinaryFlatIndex keeps -- where FlatIPIndex keeps 2 d.  A row is
    cut into m = d / dsub sub-vectors, each stored as the index of the nearest of 256 trained centroids; queries stay bf16.
    The search kernel (cx_search_pq_topk, csrc/search.hip) is the bf16 tile kernel with the document panel gathered from the
    codebook in LDS-staging order, so `search` equals `FlatIPIndex.search` over `decode()` bit for bit.  Same surface as
    FlatIPIndex / Int8FlatIndex; search_pq_rescored re-scores its candidates exactly against the float rows.

    Not here: IVF lists and residual encoding, OPQ rotations, other code widths, a look-up-table scan, save / load (codebooks go
    in and out as arrays), more than one GPU."""

    def __init__(self, d: int, dsub: int = 8, device="cuda", workspace_bytes: int = DEFAULT_WORKSPACE_BYTES, seed: int = 0):
        self.m = _check_pq_dims(int(d), int(dsub))
        self.d, self.dsub = int(d), int(dsub)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PQFlatIndex runs on the GPU (cx_search_pq_topk); there is no CPU path")
        self.workspace_bytes = int(workspace_bytes)
        self.seed = int(seed)
        self._masters: Optional[torch.Tensor] = None   # (m, 256, dsub) fp32
        self._shadow: Optional[torch.Tensor] = None    # ... rounded to bf16: what encodes, decodes and scores
        self._hn: Optional[torch.Tensor] = None        # (m, 256) fp32 half norms of the shadow
        self._store: Optional[torch.Tensor] = None     # (capacity, m) uint8; rows [0, ntotal) are the corpus
        self.ntotal = 0

    def reset(self) -> None:
        """Drop the stored rows; the codebooks stay."""
        self._store = None
        self.ntotal = 0

    @property
    def is_trained(self) -> bool:
        return self._shadow is not None

    def _require_trained(self) -> None:
        if self._shadow is None:
            raise RuntimeError("PQFlatIndex has no codebooks yet: call train() first")

    @property
    def codebooks(self) -> torch.Tensor:
        """(m, 256, dsub) bf16: the shadow of the trained masters, the only table used to encode, decode and score."""
        self._require_trained()
        return self._shadow

    @property
    def masters(self) -> torch.Tensor:
        """(m, 256, dsub) fp32: what the Lloyd updates wrote."""
        self._require_trained()
        return self._masters

    @property
    def half_norms(self) -> torch.Tensor:
        """(m, 256) fp32: half the squared norm of every shadow centroid, the bias of the assignment."""
        self._require_trained()
        return self._hn

    def train(self, x=None, max_iter: int = 25, sample: Optional[int] = None, codebooks=None) -> None:
        """Fit the m x 256 centroids to x (a tensor anywhere, an array or a memmap; host sources are sampled on the host) with
        max_iter Lloyd steps (cx_pq_assign, cx_pq_update) from seeded initial rows -- the same x and seed give the same bits;
        no convergence test, no restarts -- or take a given (m, 256, dsub) table as the masters.  sample: fit on that many rows,
        a seeded subsample (default min(n, 65 536); explicit values from 256 to 262 144)."""
        if (x is None) == (codebooks is None):
            raise ValueError("train: give either the training rows or codebooks=")
        if self.ntotal:
            raise RuntimeError("train: the index holds rows encoded with the current codebooks; reset() first")
        if codebooks is not None:
            _check_codebooks(codebooks, self.d, self.dsub)
            self._masters = torch.as_tensor(codebooks).to(device=self.device, dtype=torch.float32).clone().contiguous()
            self._shadow = self._masters.to(torch.bfloat16)
            self._hn = _pq_half_norm_device(self._shadow)
            return
        if len(np.shape(x)) != 2 or np.shape(x)[1] != self.d:
            raise ValueError(f"expected a (n, {self.d}) array, got shape {tuple(np.shape(x))}")
        n = int(np.shape(x)[0])
        max_iter = int(max_iter)
        if max_iter < 0:
            raise ValueError(f"max_iter must not be negative, got {max_iter}")
        if sample is not None and not PQ_KSUB <= int(sample) <= PQ_MAX_SAMPLE:
            raise ValueError(f"sample must be in [{PQ_KSUB}, {PQ_MAX_SAMPLE}], got {sample}")
        ns = min(n, PQ_DEFAULT_SAMPLE if sample is None else int(sample))
        if ns < PQ_KSUB:
            raise ValueError(f"train: {PQ_KSUB} centroids need at least {PQ_KSUB} rows, got {ns}")
        rows, first = pq_train_rows(n, ns, self.seed)
        if rows is None:
            xs = x
        elif isinstance(x, torch.Tensor):
            xs = x[rows.to(x.device)]
        else:
            xs = np.asarray(x[rows.numpy()], dtype=np.float32)
        xs = xs if isinstance(xs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(xs, dtype=np.float32)))
        xb = _pq_rows(xs.to(self.device))
        if xb.data_ptr() % 16 or xb.stride(0) % 8:
            xb = xb.clone(memory_format=torch.contiguous_format)
        masters = xb[first.to(self.device)].float().view(PQ_KSUB, self.m, self.dsub).transpose(0, 1).contiguous()
        shadow = masters.to(torch.bfloat16)
        hn = _pq_half_norm_device(shadow)
        codes = torch.empty(ns, self.m, dtype=torch.uint8, device=self.device)
        h = _C.lib()
        with torch.cuda.device(self.device):
            stream = _C.cur_stream()
            for _ in range(max_iter):
                _pq_assign_device(xb, shadow, hn, codes)
                _C.check(h.cx_pq_update(xb.data_ptr(), ns, self.d, xb.stride(0), codes.data_ptr(), self.m, self.dsub,
                                        masters.data_ptr(), shadow.data_ptr(), hn.data_ptr(), stream), "cx_pq_update")
        self._masters, self._shadow, self._hn = masters, shadow, hn

    @property
    def codes(self) -> torch.Tensor:
        """The stored codes, (ntotal, m) uint8 (a view)."""
        if self._store is None:
            return torch.empty(0, self.m, dtype=torch.uint8, device=self.device)
        return self._store[: self.ntotal]

    def reserve(self, n: int) -> None:
        """Allocate room for n codes in total, so that adding a corpus in chunks never copies it."""
        if n > MAX_NTOTAL:
            raise ValueError(f"PQFlatIndex holds at most {MAX_NTOTAL} vectors")
        cap = 0 if self._store is None else self._store.shape[0]
        if n > cap:
            grown = torch.empty(n, self.m, dtype=torch.uint8, device=self.device)
            if self.ntotal:
                grown[: self.ntotal].copy_(self._store[: self.ntotal])
            self._store = grown

    def _is_codes(self, x) -> bool:
        return (x.dtype == torch.uint8) if isinstance(x, torch.Tensor) else (np.asarray(x).dtype == np.uint8)

    def add(self, x) -> None:
        """Append rows: float vectors (a tensor anywhere, an array or a memmap) are encoded on the device 65 536 rows at a time
        (pq_encode's contract), a uint8 (n, m) array is taken as codes."""
        if len(np.shape(x)) != 2:
            raise ValueError(f"expected a 2-d array, got shape {tuple(np.shape(x))}")
        n = int(np.shape(x)[0])
        is_codes = self._is_codes(x)
        if np.shape(x)[1] != (self.m if is_codes else self.d):
            raise ValueError(f"expected a (n, {self.d}) array or (n, {self.m}) uint8 codes, got shape {tuple(np.shape(x))}")
        if self.ntotal + n > MAX_NTOTAL:
            raise ValueError(f"PQFlatIndex holds at most {MAX_NTOTAL} vectors")
        self._require_trained()
        if is_codes:
            self.reserve(self.ntotal + n)
            self._store[self.ntotal: self.ntotal + n].copy_(torch.as_tensor(x if isinstance(x, torch.Tensor) else np.asarray(x)))
        else:
            self.reserve(self.ntotal + n)
            out = self._store[self.ntotal: self.ntotal + n]
            for r0, r1, part in _float_chunks(x, n, self.device):
                _pq_assign_device(_pq_rows(part), self._shadow, self._hn, out[r0:r1])
        self.ntotal += n

    def decode(self, ids=None) -> torch.Tensor:
        """-> (n, d) bf16: the rows the codes stand for (all of them, or those of the given ids), the concatenation of
        codebooks[s][codes[n][s]]."""
        self._require_trained()
        codes = self.codes
        if ids is not None:
            ids = torch.as_tensor(ids if isinstance(ids, torch.Tensor) else np.asarray(ids)).to(device=self.device, dtype=torch.int64)
            if ids.dim() != 1 or (ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.ntotal)):
                raise ValueError(f"decode: expected a 1-d list of ids in [0, {self.ntotal})")
            codes = codes[ids]
        s = torch.arange(self.m, device=self.device)[None, :]
        return self._shadow[s, codes.to(torch.int64)].reshape(codes.shape[0], self.d)

    def batch_rows(self, M: int, k: int) -> int:
        """The largest query batch (all of M, else halved down to a multiple of 128) whose workspace fits the bound."""
        h = _C.lib()
        m = M
        while m > 128 and h.cx_search_pq_ws_bytes(m, max(self.ntotal, 1), k, 0) > self.workspace_bytes:
            m = max(128, (m // 2) // 128 * 128)
        return m

    def search(self, queries, k: int, exclude=None, below=None, nsplit: int = 0):
        """-> (scores (M, k) float32, ids (M, k) int64): FlatIPIndex.search over the decoded rows, bit for bit -- per query the k
        largest inner products of the bf16 query with the decoded vectors, descending, ties to the lower id; missing entries are
        (-inf, -1).  exclude, below, nsplit, numpy in -> numpy out: as FlatIPIndex.search."""
        as_numpy = not isinstance(queries, torch.Tensor)
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        if len(np.shape(queries)) != 2 or np.shape(queries)[1] != self.d:
            raise ValueError(f"expected a (n, {self.d}) array, got shape {tuple(np.shape(queries))}")
        M = int(np.shape(queries)[0])
        xptr, xids = _exclusion_csr_host(exclude, M)
        if below is not None:
            n_below = below.numel() if isinstance(below, torch.Tensor) else int(np.size(below))
            if n_below != M:
                raise ValueError(f"below has {n_below} entries for {M} queries")
        self._require_trained()
        bel = None
        if below is not None:
            bel = torch.as_tensor(np.asarray(below) if not isinstance(below, torch.Tensor) else below)
            bel = bel.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        q = _to_device_2d(queries, self.d, self.device)
        if xptr is not None:
            xptr = xptr.to(self.device)
            xids = (xids if xids.numel() else torch.zeros(1, dtype=torch.int64)).to(self.device)
        scores = torch.empty(M, k, dtype=torch.float32, device=self.device)
        ids = torch.empty(M, k, dtype=torch.int64, device=self.device)
        if M:
            h = _C.lib()
            with torch.cuda.device(self.device):
                stream = _C.cur_stream()
                mb = self.batch_rows(M, k)
                ws = None
                if self.ntotal:
                    last = M - (M - 1) // mb * mb
                    nbytes = max(h.cx_search_pq_ws_bytes(mb, self.ntotal, k, nsplit),
                                 h.cx_search_pq_ws_bytes(last, self.ntotal, k, nsplit))
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                D = self.codes
                for b0 in range(0, M, mb):
                    m = min(mb, M - b0)
                    _C.check(h.cx_search_pq_topk(q[b0].data_ptr(), D.data_ptr() if self.ntotal else None,
                                                 self._shadow.data_ptr(), m, self.ntotal, self.d, self.dsub, self.d, self.m, k,
                                                 None if xptr is None else xptr[b0:].data_ptr(), _C.ptr(xids),
                                                 None if bel is None else bel[b0:].data_ptr(), int(nsplit), _C.ptr(ws),
                                                 scores[b0].data_ptr(), ids[b0].data_ptr(), stream), "cx_search_pq_topk")
        if as_numpy:
            return scores.cpu().numpy(), ids.cpu().numpy()
        return scores, ids


def search_pq_rescored(index: PQFlatIndex, vectors, queries, k: int, rescore_factor: int = 4, exclude=None, below=None):
    """Coarse PQ search + exact re-scoring: the min(k * rescore_factor, 4096) best PQ scores of `index` per query, then the k
    best of those by exact inner product with `vectors` (the corpus the codes were made from: device bf16 rows, a host array or
    a memmap; see rescore).  queries: float rows.  exclude applies to the coarse stage, below to the exact score.
    -> (scores, ids) as FlatIPIndex.search; equal to it bit for bit when the candidate lists cover the corpus.  Lists longer
    than the kernel's k bound (1024) are fetched in pages (_paged_candidates)."""
    k = int(k)
    c = _check_rescored_arguments(index, vectors, k, rescore_factor)
    as_numpy = not isinstance(queries, torch.Tensor)
    if len(np.shape(queries)) != 2 or np.shape(queries)[1] != index.d:
        raise ValueError(f"expected a (n, {index.d}) array, got shape {tuple(np.shape(queries))}")
    M = int(np.shape(queries)[0])
    _exclusion_csr_host(exclude, M)   # (malformed filters raise before any launch)
    if below is not None:
        n_below = below.numel() if isinstance(below, torch.Tensor) else int(np.size(below))
        if n_below != M:
            raise ValueError(f"below has {n_below} entries for {M} queries")
    index._require_trained()
    qd = _to_device_2d(queries, index.d, index.device)
    cand = _paged_candidates(lambda kp, ex: index.search(qd, kp, exclude=ex)[1], M, c, index.ntotal, exclude)
    return _rescore_candidates(qd, cand, vectors, k, below, index.device, as_numpy)


def encode(model, texts: Sequence[str], tokenizer, batch_size: int = 256, max_length: int = 512,
           window: int = 64) -> torch.Tensor:
    """Normalised embeddings (len(texts), d) fp32 of `texts` from a BiEncoder (its no-grad engine pass, eval mode).

    Texts are tokenised `window` batches at a time; inside a window they are sorted by token count (longest first, stable)
    so a batch pads to its own longest member; the rows come back in input order."""
    was_training = model.training
    model.eval()
    out = None
    try:
        with torch.no_grad():
            step = batch_size * max(1, int(window))
            for w0 in range(0, len(texts), step):
                chunk = list(texts[w0: w0 + step])
                tok = tokenizer(chunk, padding="max_length", truncation=True, return_tensors="pt", max_length=max_length)
                ids, mask = tok["input_ids"], tok["attention_mask"]
                lens = mask.sum(1)
                order = torch.sort(-lens, stable=True).indices
                for b0 in range(0, len(chunk), batch_size):
                    sel = order[b0: b0 + batch_size]
                    L = max(1, int(lens[sel].max()))
                    emb = model(input_ids=ids[sel, :L].to(model.device), attention_mask=mask[sel, :L].to(model.device),
                                normalize=True)["embedding"].float()
                    if out is None:
                        out = torch.empty(len(texts), emb.shape[1], dtype=torch.float32, device=emb.device)
                    out[w0 + sel.to(emb.device)] = emb
    finally:
        model.train(was_training)
    if out is None:
        raise ValueError("encode: no texts")
    return out
