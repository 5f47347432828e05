"""Exact inner-product search for the data-curation stage (hard-negative mining, consistency filtering).

`FlatIPIndex` stands where the reference scripts build a faiss `IndexFlatIP` cloned to the GPUs with fp16 storage
(scripts/text/index_filtering.py:364-377, scripts/text/get_negatives.py:163-168): same method names (`add`, `search`,
`ntotal`, `reset`), bf16 storage, one fused HIP kernel per query batch (csrc/search.hip, cx_search_topk) that never writes
the (queries x corpus) scores.  `search` adds what the margin miner needs on top of faiss: per-row excluded ids (the
positives) and a per-row exclusive score bound (margin * s(q, pos)).

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


def _exclusion_csr(exclude, M: int, device) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """exclude: None, a length-M sequence of id lists, or a (row_ptr (M+1), ids) pair -> int64 device CSR."""
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
    if ids.numel() == 0:
        ids = torch.zeros(1, dtype=torch.int64)   # a valid pointer; no row reads it
    return row_ptr.to(device), ids.to(device)


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
