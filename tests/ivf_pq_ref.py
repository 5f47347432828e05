"""numpy reference of the IVF-PQ index, on top of tests/pq_ref.py.  This file IS the contract; the kernels are tested against it
by equality.

Residual: x is a bf16 row (fp32 input is rounded first, as `add` rounds it), l its list, c_l the bf16 centroid row the coarse
index stores.  r_j = bf16_rne(f32(x_j) - f32(c_l,j)): one fp32 subtraction and one round-to-nearest-even per element.
Codes: pq_ref.assign applied to r, unchanged.
Score of (pair row = (query q, probed list l), row n of l): s = acc + bias, one fp32 addition, where acc has the bits
cx_search_topk gives (q, decode(code_n)) and bias is the fp32 score the coarse search returned for (q, l).  The window, `below`,
the exclusions, the order (s descending, ties to the lower id) and the (-inf, -1) padding all act on s.
Without residuals (bias None): raw rows are encoded and s = acc with no addition at all, so -0 stays -0."""
import numpy as np

from tests import pq_ref as R

F32 = np.float32


def residual(x, c):
    """x (n, d) float rows, c (n, d) the bf16 centroid row of every row's list -> (n, d) bf16 values as fp32."""
    return R.to_bf16((R.to_bf16(x) - np.asarray(c, F32)).astype(F32))


def encode(x, labels, centroids, shadow):
    """-> codes uint8 (n, m) of the residuals of x to R.to_bf16(centroids)[labels]."""
    return R.assign(residual(x, R.to_bf16(centroids)[np.asarray(labels)]), shadow)


def select(s, ok, k, m, exclude, below):
    """Row m: s (N,) fp32 scores, ok (N,) inside the window / lists -> (scores (k,), ids (k,)), padded with (-inf, -1)."""
    ok = ok & (True if below is None else s < F32(below[m]))
    if exclude is not None:
        ok[[e for e in exclude[m] if 0 <= e < s.shape[0]]] = False
    ids = np.nonzero(ok)[0]
    order = np.lexsort((ids, -s[ids]))[:k]
    out_s, out_i = np.full(k, -np.inf, F32), np.full(k, -1, np.int64)
    out_s[: order.size], out_i[: order.size] = s[ids][order], ids[order]
    return out_s, out_i


def window_topk(acc, bias, k, min_id=None, end_id=None, exclude=None, below=None):
    """cx_search_pq_window_topk from the (M, N) fp32 matrix of acc (M > 0): row m admits min_id[m] < n < end_id[m]."""
    S = acc if bias is None else (acc + np.asarray(bias, F32)[:, None]).astype(F32)
    n = np.arange(acc.shape[1])
    out = [select(S[m], (n > (-1 if min_id is None else min_id[m])) & (n < (n.size if end_id is None else end_id[m])), k, m,
                  exclude, below) for m in range(acc.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def ivf_search(acc, labels, probes, coarse, k, by_residual=True, exclude=None, below=None):
    """IVFPQIndex.search from acc (M, N) in add() order: query m sees the rows whose label is among probes[m] (M, nprobe), each
    with the bias coarse[m, j] of its list's probe j."""
    out = []
    for m in range(acc.shape[0]):
        hit = labels[:, None] == probes[m][None, :]                         # (N, nprobe): at most one probe per row
        s = (acc[m] + (hit * coarse[m][None, :]).sum(1, dtype=F32)).astype(F32) if by_residual else acc[m]
        out.append(select(s, hit.any(1), k, m, exclude, below))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
