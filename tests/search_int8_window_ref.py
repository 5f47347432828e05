"""numpy reference of the WINDOWED int8 top-k search (tests/test_search_int8_window_ref_cpu.py,
tests/test_search_int8_window_gpu.py).  The score of a pair is tests/int8_ref.scores -- an exact integer dot product, then two
fp32 multiplications -- and the admission rule is tests/search_window_ref.admitted: row m admits document n iff
max(min_id[m], -1) < n < min(max(end_id[m], 0), N)  (None: -1 / N everywhere), score < below[m] (strict) and n is not among the
row's excluded ids.  The answer is the k admitted documents first in (score descending, id ascending), padded with (-inf, -1).
Every output is defined bit for bit, so the kernel is compared by equality."""
import numpy as np
import torch

from tests import int8_ref as R
from tests import search_window_ref as W


def admitted(S, min_id=None, end_id=None, exclude=None, below=None):
    """(M, N) bool numpy for a float32 score matrix S."""
    return W.admitted(torch.from_numpy(np.ascontiguousarray(S)), min_id, end_id, exclude, below).numpy()


def topk_from_mask(S, mask, k):
    """-> (scores (M, k) float32, ids (M, k) int64): the admitted entries of every row, a STABLE descending sort by score over
    ascending ids (ties to the lower id)."""
    M, N = S.shape
    out_s = np.full((M, k), -np.inf, dtype=np.float32)
    out_i = np.full((M, k), -1, dtype=np.int64)
    for m in range(M):
        cols = np.nonzero(mask[m])[0]
        order = cols[np.argsort(-S[m, cols], kind="stable")][:k]
        out_s[m, : order.size] = S[m, order]
        out_i[m, : order.size] = order
    return out_s, out_i


def search(qc, qs, dc, ds, k, min_id=None, end_id=None, exclude=None, below=None):
    S = R.scores(qc, qs, dc, ds)
    return topk_from_mask(S, admitted(S, min_id, end_id, exclude, below), k)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check(got, want):
    """(scores, ids) pairs: equal shapes, dtypes and bits (+0 and -0 are told apart)."""
    (gs, gi), (ws, wi) = got, want
    gs, gi, ws, wi = _bits(gs), _bits(gi), _bits(ws), _bits(wi)
    assert gs.shape == ws.shape and gi.shape == wi.shape and gs.dtype == ws.dtype and gi.dtype == wi.dtype
    assert np.array_equal(gi, wi), "ids differ from the reference"
    assert np.array_equal(gs, ws), "scores differ from the reference"
