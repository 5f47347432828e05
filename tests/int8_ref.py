"""numpy reference of the int8 scalar-quantised search (tests/test_int8_ref_cpu.py, test_int8_search_cpu.py,
test_int8_search_gpu.py).  This file IS the contract; the kernels are tested against it by equality.

Quantiser, per row x of width d:  amax = max_j |x_j| in fp32;  amax < 2^-100: codes 0, scale 0;  otherwise
inv = 127.0f / amax, scale = amax / 127.0f (IEEE fp32 divisions), code_j = clamp(rint(x_j * inv), -127, 127) with an fp32
product and round-half-to-even.
Score of (m, n):  acc = sum_j Q[m][j] D[n][j] (integer, exact);  s = ((float)acc * d_scale[n]) * q_scale[m]: two fp32
multiplications in that order.
Top-k: row m admits document n iff s < below[m] (strict) and n is not among the row's excluded ids; the answer is the k
admitted documents first in (score descending, id ascending), padded with (-inf, -1).
Pipeline: the int8 top-c candidates (exclusions applied), re-scored in float64 against the float rows, `below` on the exact
score, the k best by (score descending, id ascending)."""
import numpy as np

ZERO_AMAX = np.float32(2.0 ** -100)
F127 = np.float32(127)


def quantize(x):
    """x (n, d) -> (codes int8 (n, d), scales float32 (n,))."""
    a = np.asarray(x, dtype=np.float32)
    n, d = a.shape
    codes = np.zeros((n, d), np.int8)
    scales = np.zeros(n, np.float32)
    for r in range(n):
        amax = np.float32(np.max(np.abs(a[r])))
        if amax < ZERO_AMAX:
            continue
        inv = np.float32(F127 / amax)
        scales[r] = np.float32(amax / F127)
        prod = (a[r] * inv).astype(np.float32)
        codes[r] = np.clip(np.rint(prod), -127, 127).astype(np.int8)
    return codes, scales


def acc_matrix(qc, dc):
    """(M, N) int64 exact dot products of int8 codes."""
    return np.asarray(qc, dtype=np.int64) @ np.asarray(dc, dtype=np.int64).T


def scores(qc, qs, dc, ds):
    """(M, N) float32: ((float)acc * d_scale[n]) * q_scale[m], each product rounded to fp32."""
    acc = acc_matrix(qc, dc)
    assert np.abs(acc).max(initial=0) < 2 ** 24          # (float)acc is exact
    f = acc.astype(np.float32)
    t = (f * np.asarray(ds, np.float32)[None, :]).astype(np.float32)
    return (t * np.asarray(qs, np.float32)[:, None]).astype(np.float32)


def topk(S, k, exclude=None, below=None):
    """S (M, N) -> (scores (M, k) of S's dtype, ids (M, k) int64)."""
    M, N = S.shape
    out_s = np.full((M, k), -np.inf, dtype=S.dtype)
    out_i = np.full((M, k), -1, dtype=np.int64)
    for m in range(M):
        ok = np.ones(N, bool)
        if below is not None:
            ok &= S[m] < below[m]
        if exclude is not None:
            ex = [e for e in exclude[m] if 0 <= e < N]
            ok[ex] = False
        cols = np.nonzero(ok)[0]
        order = cols[np.argsort(-S[m, cols], kind="stable")][:k]      # stable over ascending ids: ties to the lower id
        out_s[m, : order.size] = S[m, order]
        out_i[m, : order.size] = order
    return out_s, out_i


def search(qc, qs, dc, ds, k, exclude=None, below=None):
    return topk(scores(qc, qs, dc, ds), k, exclude, below)


def pipeline(Q, D, k, rescore_factor=2, exclude=None, below=None, max_candidates=4096):
    """Two stages on float rows Q (M, d), D (N, d): -> (scores float64 (M, k), ids int64 (M, k))."""
    Q, D = np.asarray(Q, np.float32), np.asarray(D, np.float32)
    c = max(k, min(k * rescore_factor, max_candidates))
    qc, qs = quantize(Q)
    dc, ds = quantize(D)
    _, cand = search(qc, qs, dc, ds, c, exclude=exclude)
    M = Q.shape[0]
    out_s = np.full((M, k), -np.inf, np.float64)
    out_i = np.full((M, k), -1, np.int64)
    for m in range(M):
        ids = np.sort(cand[m][cand[m] >= 0])
        s = D[ids].astype(np.float64) @ Q[m].astype(np.float64)
        if below is not None:
            keep = s < below[m]
            ids, s = ids[keep], s[keep]
        order = np.argsort(-s, kind="stable")[:k]
        out_s[m, : order.size] = s[order]
        out_i[m, : order.size] = ids[order]
    return out_s, out_i


def recall(got_ids, ref_ids):
    """Mean over rows of |got ∩ ref| / |ref| (ids >= 0)."""
    tot = 0.0
    for g, r in zip(got_ids, ref_ids):
        r = set(int(x) for x in r if x >= 0)
        tot += len(r & set(int(x) for x in g if x >= 0)) / max(len(r), 1)
    return tot / len(ref_ids)
