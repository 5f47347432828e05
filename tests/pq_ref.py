"""numpy reference of the product quantiser (tests/test_pq_ref_cpu.py, test_pq_cpu.py, test_pq_gpu.py,
test_search_pq_gpu.py).  This file IS the contract; the kernels are tested against it by equality.

Shapes: d a multiple of 64 in [64, 1024], dsub in {8, 16, 32, 64}, m = d / dsub sub-quantisers of 256 centroids, uint8 codes.
Codebooks: fp32 masters (m, 256, dsub); their bf16 shadow (round to nearest even; held here as fp32 arrays whose values are bf16
values); half_norm (m, 256) fp32 = 0.5f * h with h = 0, h = fmaf(c_j, c_j, h) for j ascending over the SHADOW.  Only the shadow
encodes, decodes and scores.
Assign: x is a bf16 row (fp32 input is rounded first).  Per sub-quantiser s and centroid c: acc = 0, acc = fmaf(x_j, c_j, acc)
for j ascending over the sub-vector, score = acc - half_norm[s][c] (one fp32 subtraction); the code is the arg-max, ties to the
lower c.
Update: per (s, c) the fp32 sum of the bf16 rows' sub-vectors whose code is c, added element-wise in ascending row order;
master = sum / count (fp32 division) where count > 0, an empty cell keeps its master; shadow and half_norm are recomputed.
Train: masters = the sub-vectors of 256 given rows of the sample (the same rows for every s), then max_iter x (assign, update);
no convergence test, no restarts.
Decode: row n is the concatenation of shadow[s][code[n][s]].
Search: the exact top-k over the decoded rows (on the GPU: FlatIPIndex.search over them, bit for bit).

fmaf in numpy: the operands of every product here are bf16 values (8 significant bits), so a product has at most 16 bits and
product + accumulator (24 bits) is exact in float64 whenever the two overlap or nearly do, and where they are more than 29
binades apart the smaller one only decides a rounding that float64 keeps too; rounding that float64 sum to fp32 is therefore the
single rounding of fmaf (tests/test_pq_ref_cpu.py holds it against exact rational arithmetic, denormal results included)."""
import numpy as np

from tests.int8_ref import recall, topk  # noqa: F401  (the dense top-k and recall are shared)

KSUB = 256
F32 = np.float32
DSUBS = (8, 16, 32, 64)


def to_bf16(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32.  Finite input."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(a.shape)


def bf16_bits(x):
    """The uint16 patterns of an array of bf16 values held as fp32."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    assert not (a.view(np.uint32) & 0xFFFF).any()
    return (a.view(np.uint32) >> 16).astype(np.uint16).reshape(a.shape)


def fmaf(a, b, c):
    """fp32 fused multiply-add of bf16-valued a, b and fp32 c (see the module docstring)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def half_norm(shadow):
    """shadow (m, 256, dsub) -> (m, 256) fp32."""
    c = np.asarray(shadow, np.float32)
    h = np.zeros(c.shape[:-1], np.float32)
    for j in range(c.shape[-1]):
        h = fmaf(c[..., j], c[..., j], h)
    return (F32(0.5) * h).astype(np.float32)


def sub_scores(xs, cb, hn):
    """xs (n, dsub) bf16 values, cb (256, dsub) shadow, hn (256,) -> (n, 256) fp32 scores of one sub-quantiser."""
    acc = np.zeros((xs.shape[0], cb.shape[0]), np.float32)
    for j in range(xs.shape[1]):
        acc = fmaf(xs[:, j, None], cb[None, :, j], acc)
    return (acc - np.asarray(hn, np.float32)[None, :]).astype(np.float32)


def assign(x, shadow, hn=None):
    """x (n, d) float rows, shadow (m, 256, dsub) -> codes uint8 (n, m)."""
    xb = to_bf16(x)
    m, _, dsub = shadow.shape
    hn = half_norm(shadow) if hn is None else hn
    codes = np.zeros((xb.shape[0], m), np.uint8)
    for s in range(m):
        sc = sub_scores(xb[:, s * dsub: (s + 1) * dsub], shadow[s], hn[s])
        codes[:, s] = np.argmax(sc, axis=1)                  # the first maximum: ties to the lower c
    return codes


def update(x, codes, masters):
    """One Lloyd step's second half -> (masters, shadow, half_norm), new arrays."""
    xb = to_bf16(x)
    masters = np.array(masters, dtype=np.float32)
    m, _, dsub = masters.shape
    for s in range(m):
        sums = np.zeros((KSUB, dsub), np.float32)
        np.add.at(sums, codes[:, s].astype(np.int64), xb[:, s * dsub: (s + 1) * dsub])   # unbuffered: ascending row order
        cnt = np.bincount(codes[:, s], minlength=KSUB)
        live = cnt > 0
        masters[s][live] = (sums[live] / cnt[live].astype(np.float32)[:, None]).astype(np.float32)
    shadow = to_bf16(masters)
    return masters, shadow, half_norm(shadow)


def init_masters(x, rows, dsub):
    """The sub-vectors of rows `rows` (256 of them) of x, the same rows for every s -> masters (m, 256, dsub)."""
    xb = to_bf16(np.asarray(x, np.float32)[np.asarray(rows)])
    assert xb.shape[0] == KSUB
    return np.ascontiguousarray(xb.reshape(KSUB, -1, dsub).transpose(1, 0, 2))


def train(x, rows, dsub, max_iter):
    """-> (masters, shadow, half_norm) after max_iter x (assign, update) from init_masters(x, rows, dsub)."""
    masters = init_masters(x, rows, dsub)
    shadow = to_bf16(masters)
    hn = half_norm(shadow)
    for _ in range(max_iter):
        masters, shadow, hn = update(x, assign(x, shadow, hn), masters)
    return masters, shadow, hn


def decode(codes, shadow):
    """codes (n, m), shadow (m, 256, dsub) -> (n, d) bf16 values as fp32."""
    codes = np.asarray(codes)
    return np.concatenate([shadow[s][codes[:, s]] for s in range(shadow.shape[0])], axis=1).astype(np.float32)


def search(Q, codes, shadow, k, exclude=None, below=None):
    """Float64 scores of the bf16-rounded queries against the decoded rows -> the dense top-k.  (The GPU result is defined as
    FlatIPIndex.search over decode(); this is that order wherever the fp32 scores are exact or far apart.)"""
    S = to_bf16(Q).astype(np.float64) @ decode(codes, shadow).astype(np.float64).T
    return topk(S, k, exclude, below)


def pipeline(Q, D, shadow, k, rescore_factor=4, exclude=None, below=None, max_candidates=4096):
    """Two stages on float rows Q (M, d), D (N, d): the PQ top-c candidates (exclusions applied), re-scored in float64 against
    the float rows, `below` on the exact score -> (scores float64 (M, k), ids int64 (M, k))."""
    Q, D = np.asarray(Q, np.float32), np.asarray(D, np.float32)
    c = max(k, min(k * rescore_factor, max_candidates))
    _, cand = search(Q, assign(D, shadow), shadow, c, exclude=exclude)
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


def sign_search(Q, D, k):
    """The sign-code comparator (BinaryFlatIndex's order): ascending Hamming distance of the sign bits, ties to the lower id."""
    qb, db = np.asarray(Q) > 0, np.asarray(D) > 0
    dist = (qb[:, None, :] != db[None, :, :]).sum(-1)
    return topk(-dist.astype(np.float64), k)
