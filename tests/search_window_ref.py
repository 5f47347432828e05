"""float64 dense reference of the WINDOWED top-k search and of the list merge (tests/test_search_window_gpu.py,
tests/test_ivf_gpu.py).  Row m admits document n iff  max(min_id[m], -1) < n < min(max(end_id[m], 0), N)  (None: -1 / N
everywhere), score < below[m] (strict) and n is not among the row's excluded ids.  The answer is the k admitted documents
first in the order (score descending, REPORTED id ascending) -- the reported id of position n is id_map[n], or n -- padded with
(-inf, -1).  Works on CPU and device tensors alike."""
import numpy as np
import torch


def scores64(Q, D):
    return Q.double() @ D.double().T


def admitted(S, min_id=None, end_id=None, exclude=None, below=None):
    """(M, N) bool for a score matrix S."""
    M, N = S.shape
    col = torch.arange(N, device=S.device)
    mask = torch.ones(M, N, dtype=torch.bool, device=S.device)
    if min_id is not None:
        lo = torch.as_tensor(min_id, dtype=torch.int64).to(S.device).reshape(-1).clamp(-1, N)
        assert lo.numel() == M
        mask &= col[None, :] > lo[:, None]
    if end_id is not None:
        hi = torch.as_tensor(end_id, dtype=torch.int64).to(S.device).reshape(-1).clamp(0, N)
        assert hi.numel() == M
        mask &= col[None, :] < hi[:, None]
    if below is not None:
        b = torch.as_tensor(below).to(S.device).double().reshape(-1)
        assert b.numel() == M
        mask &= S < b[:, None]
    if exclude is not None:
        assert len(exclude) == M
        for m, ex in enumerate(exclude):
            ex = [e for e in ex if 0 <= e < N]
            if ex:
                mask[m, ex] = False
    return mask


def topk_from_mask(S, mask, k, id_map=None):
    """-> (scores (M, k) float64, ids (M, k) int64): the admitted entries of every row by (score descending, reported id
    ascending): columns into reported-id order first, then a STABLE descending sort by score."""
    M, N = S.shape
    rep = torch.arange(N, device=S.device) if id_map is None else torch.as_tensor(id_map, dtype=torch.int64).to(S.device)
    assert rep.numel() == N
    o1 = torch.sort(rep, stable=True).indices
    s = torch.where(mask, S, torch.full_like(S, -float("inf")))[:, o1]
    ids = torch.where(mask, rep.expand(M, -1), torch.full((M, N), -1, dtype=torch.int64, device=S.device))[:, o1]
    ok = mask[:, o1]
    # inadmissible entries behind every admissible one, whatever their score: sort on (admissible, score)
    o2 = torch.sort(s, dim=1, descending=True, stable=True).indices
    s, ids, ok = s.gather(1, o2), ids.gather(1, o2), ok.gather(1, o2)
    o3 = torch.sort(ok.to(torch.int8), dim=1, descending=True, stable=True).indices[:, :k]
    s, ids = s.gather(1, o3), ids.gather(1, o3)
    if s.shape[1] < k:
        pad = k - s.shape[1]
        s = torch.cat([s, torch.full((M, pad), -float("inf"), dtype=torch.float64, device=S.device)], 1)
        ids = torch.cat([ids, torch.full((M, pad), -1, dtype=torch.int64, device=S.device)], 1)
    return s, ids


def ref_window_topk(Q, D, k, min_id=None, end_id=None, exclude=None, below=None, id_map=None):
    S = scores64(Q, D)
    return topk_from_mask(S, admitted(S, min_id, end_id, exclude, below), k, id_map)


def check_exact(Q, D, k, scores, ids, min_id=None, end_id=None, exclude=None, below=None, id_map=None):
    """A result on operands whose fp32 accumulation is exact: scores and ids EQUAL to the reference."""
    rs, ri = ref_window_topk(Q, D, k, min_id, end_id, exclude, below, id_map)
    scores, ids = torch.as_tensor(scores).to(rs.device), torch.as_tensor(ids).to(rs.device)
    assert scores.shape == rs.shape and ids.shape == ri.shape
    assert torch.equal(ids, ri), "ids differ from the reference"
    assert torch.equal(scores.double(), rs), "scores differ from the reference"


def merge_ref(scores, ids, src, k, id_map=None):
    """Host merge of top-k lists: scores / ids (P, k') padded with (-inf, -1); src (M, L) names the lists of every output
    row (entries outside [0, P) are skipped).  -> numpy (scores (M, k) float32, ids (M, k) int64): the k best entries by
    (score descending, reported id ascending), padded."""
    scores = torch.as_tensor(scores).cpu().numpy()
    ids = torch.as_tensor(ids).cpu().numpy()
    src = torch.as_tensor(src).cpu().numpy()
    rep = None if id_map is None else torch.as_tensor(id_map).cpu().numpy()
    M, P = src.shape[0], scores.shape[0]
    out_s = np.full((M, k), -np.inf, dtype=np.float32)
    out_i = np.full((M, k), -1, dtype=np.int64)
    for m in range(M):
        rows = src[m][(src[m] >= 0) & (src[m] < P)]
        s, i = scores[rows].reshape(-1), ids[rows].reshape(-1)
        keep = i >= 0
        s, i = s[keep], i[keep]
        if rep is not None:
            i = rep[i]
        o = np.lexsort((i, -s.astype(np.float64)))[:k]
        out_s[m, : o.size], out_i[m, : o.size] = s[o], i[o]
    return out_s, out_i
