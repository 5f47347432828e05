"""numpy reference of the IVF index over sign codes.  This file IS the contract; the kernels are tested against it by equality.
Nothing here is a float.

Codes: uint8 (n, d / 8) in numpy.packbits layout (dimension 0 is bit 7 of byte 0).  Order everywhere: ascending Hamming
distance, ties to the lower (original) id; padding is (INT32_MAX, -1).
Assign: a row's list is the centroid code at the smallest distance, ties to the lower list.
Update (k-majority): centroid bit (l, b) = [2 * ones > size] over the member codes of list l; an empty list keeps its bytes.
Train: initial centroids = the codes of the given rows, then max_iter rounds of (assign, update).
Search: the nprobe nearest centroid codes name the lists; the top-k over their rows by (distance, original id)."""
import numpy as np

PAD = np.int32(2 ** 31 - 1)
POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1, dtype=np.uint8)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def hamming(a, b):
    """a (M, nb), b (N, nb) uint8 -> (M, N) int32 distances."""
    return np.stack([POP[r ^ b].sum(1, dtype=np.int32) for r in a]) if len(a) else np.zeros((0, len(b)), np.int32)


def assign(codes, centroids):
    return np.argmin(hamming(codes, centroids), axis=1).astype(np.int32)        # (argmin: the first minimum)


def update(codes, labels, centroids):
    """-> (new centroids, sizes int32)."""
    out = centroids.copy()
    sizes = np.bincount(labels, minlength=centroids.shape[0]).astype(np.int32)
    bits = np.unpackbits(codes, axis=1).astype(np.int64)
    for l in np.nonzero(sizes)[0]:
        out[l] = np.packbits(2 * bits[labels == l].sum(0) > sizes[l])
    return out, sizes


def train(codes, first, max_iter):
    c = codes[first].copy()
    for _ in range(max_iter):
        c, _ = update(codes, assign(codes, c), c)
    return c


def select(dist, ok, k, m, exclude, max_dist):
    """Row m: dist (N,) int32, ok (N,) inside the window / lists -> (dist (k,), ids (k,)), padded."""
    ok = ok & (True if max_dist is None else dist <= max_dist[m])
    if exclude is not None:
        ok[[e for e in exclude[m] if 0 <= e < dist.shape[0]]] = False
    ids = np.nonzero(ok)[0]
    order = np.lexsort((ids, dist[ids]))[:k]
    out_d, out_i = np.full(k, PAD, np.int32), np.full(k, -1, np.int64)
    out_d[: order.size], out_i[: order.size] = dist[ids][order], ids[order]
    return out_d, out_i


def window_topk(dist, k, min_id=None, end_id=None, exclude=None, max_dist=None):
    """cx_search_hamming_window_topk from the (M, N) distances (M > 0): row m admits min_id[m] < n < end_id[m]."""
    n = np.arange(dist.shape[1])
    out = [select(dist[m], (n > (-1 if min_id is None else min_id[m])) & (n < (n.size if end_id is None else end_id[m])), k, m,
                  exclude, max_dist) for m in range(dist.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def ivf_search(q, codes, centroids, k, nprobe, exclude=None, max_dist=None):
    """IVFBinaryIndex.search: q (M, nb), codes (N, nb) in add() order."""
    labels = assign(codes, centroids)
    probes = window_topk(hamming(q, centroids), nprobe)[1]
    dist = hamming(q, codes)
    out = [select(dist[m], np.isin(labels, probes[m]), k, m, exclude, max_dist) for m in range(q.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
