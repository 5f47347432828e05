"""float64 reference of the rank kernel and of the metrics built on it (tests/test_rank_gpu.py, tests/test_zeroshot_*.py).

Scores are `Q.double() @ D.double().T` on the bf16 operands; a target's rank is its 0-based position in the order
(score descending, id ascending).  The metrics are computed from a DENSE boolean positives matrix, independently of the CSR
code under test.  Everything runs on the operands' device, chunked over rows."""
import torch


def scores64(Q, D):
    return Q.double() @ D.double().T


def ref_rank(Q, D, row_ptr, ids, chunk_rows=1024):
    """-> (ranks int64 (nnz), scores float64 (nnz)) for the CSR (row_ptr, ids) of targets per row of Q."""
    dev = Q.device
    row_ptr = torch.as_tensor(row_ptr, dtype=torch.int64).cpu()
    ids = torch.as_tensor(ids, dtype=torch.int64).to(dev)
    M, N = Q.shape[0], D.shape[0]
    rows = torch.repeat_interleave(torch.arange(M), row_ptr[1:] - row_ptr[:-1]).to(dev)
    ranks = torch.empty(ids.numel(), dtype=torch.int64, device=dev)
    scores = torch.empty(ids.numel(), dtype=torch.float64, device=dev)
    col = torch.arange(N, device=dev)
    Dd = D.double()
    for r0 in range(0, M, chunk_rows):
        r1 = min(M, r0 + chunk_rows)
        e0, e1 = int(row_ptr[r0]), int(row_ptr[r1])
        if e1 == e0:
            continue
        S = Q[r0:r1].double() @ Dd.T                      # (rows, N)
        er, et = rows[e0:e1] - r0, ids[e0:e1]
        st = S[er, et]                                    # (entries)
        Se = S[er]                                        # (entries, N)
        before = (Se > st[:, None]) | ((Se == st[:, None]) & (col[None, :] < et[:, None]))
        ranks[e0:e1] = before.sum(1)
        scores[e0:e1] = st
    return ranks, scores


def near_count(Q, D, row_ptr, ids, band):
    """Per entry: the number of OTHER columns whose float64 score lies within `band` of the target's."""
    dev = Q.device
    row_ptr = torch.as_tensor(row_ptr, dtype=torch.int64).cpu()
    ids = torch.as_tensor(ids, dtype=torch.int64).to(dev)
    rows = torch.repeat_interleave(torch.arange(Q.shape[0]), row_ptr[1:] - row_ptr[:-1]).to(dev)
    S = scores64(Q, D)[rows]
    st = S[torch.arange(ids.numel(), device=dev), ids]
    return ((S - st[:, None]).abs() <= band).sum(1) - 1


def dense_positives(M, N, row_ptr, ids):
    """(M, N) bool: pos[m, n] = n is a target of row m."""
    pos = torch.zeros(M, N, dtype=torch.bool)
    row_ptr = [int(x) for x in row_ptr]
    ids = [int(x) for x in ids]
    for m in range(M):
        for e in range(row_ptr[m], row_ptr[m + 1]):
            pos[m, ids[e]] = True
    return pos


def dense_order(S):
    """(M, N) int64: column ids in (score descending, id ascending) order -- a stable descending sort of ascending ids."""
    return torch.sort(S, dim=1, descending=True, stable=True).indices


def dense_topk_hits(S, labels, ks=(1, 5)):
    """Number of rows whose label is among the first k of the row's order, per k."""
    order = dense_order(S)
    labels = torch.as_tensor(labels, dtype=torch.int64).to(S.device)
    return [int((order[:, :k] == labels[:, None]).any(1).sum()) for k in ks]


def dense_recall(S, pos, ks=(1, 5, 10)):
    """clip_benchmark's `recall_at_k(...) > 0` averaged over rows: the share of rows with a positive among the first k."""
    order = dense_order(S)
    hit = pos.to(S.device).gather(1, order)              # positives in rank order
    return [int(hit[:, :k].any(1).sum()) / S.shape[0] for k in ks]     # an exact count over the number of rows
