"""float64 reference of k-means on bf16 points (tests/test_kmeans_gpu.py; checked itself in tests/test_kmeans_ref_cpu.py).

Values are v(x, c) = x.c - half_norm[c] with `X.double() @ C.double().T` on the bf16 operands (half_norm None: the plain inner
product).  The assignment is the arg-max with ties to the LOWER centroid id, `best` the maximum and `second` the second
largest value counted with multiplicity (a maximum attained twice has second == best; K == 1 gives -inf).  The update is the
float64 mean of a cluster's rows, or their sum scaled to unit L2 norm (spherical); an empty cluster keeps its previous
centroid.  Empty clusters are then re-seeded: in ascending cluster id each takes the not-yet-used point with the smallest
`best`, ties to the lower point id.  `band` is the rounding band of the fp32 kernel around a value.  Runs on the operands'
device."""
import torch


def scores64(X, C):
    return X.double() @ C.double().T


def values64(X, C, half_norm=None):
    S = scores64(X, C)
    return S if half_norm is None else S - half_norm.double()[None, :]


def assign64(V, ties="lower"):
    """(N, K) float64 values -> (labels int64, best, second).  ties="upper" is a planted error for the reference's own test."""
    N, K = V.shape
    best = V.max(1).values
    col = torch.arange(K, device=V.device)
    at = V == best[:, None]
    labels = torch.where(at, col, K).min(1).values if ties == "lower" else torch.where(at, col, -1).max(1).values
    rest = V.clone()
    rest[torch.arange(N, device=V.device), labels] = -float("inf")
    second = rest.max(1).values if K > 1 else torch.full_like(best, -float("inf"))
    return labels, best, second


def tied_rows(V):
    """(N,) bool: rows whose maximum is attained more than once."""
    return (V == V.max(1).values[:, None]).sum(1) > 1


def band(X, C, labels, runner, half_norm=None):
    """(N,) float64: the row's rounding band, from its two contenders (the best centroid and the runner-up):
    d * 2^-24 * sum_j |x_j c_j| of both  (the d - 1 fp32 additions of an accumulation in any order; bf16 products are exact)
    + 2^-23 * (|score| + bias of both)   (the one fp32 subtraction of the bias, and the rounding of the stored value)."""
    d = X.shape[1]
    rows = torch.arange(X.shape[0], device=X.device)
    A = X.double().abs() @ C.double().abs().T
    S = scores64(X, C)
    hn = torch.zeros(C.shape[0], dtype=torch.float64, device=X.device) if half_norm is None else half_norm.double().abs()
    both = lambda M: M[rows, labels] + M[rows, runner]
    return d * 2.0 ** -24 * both(A) + 2.0 ** -23 * (both(S.abs()) + hn[labels] + hn[runner])


def runner_up(V, labels):
    """(N,) the id of the second contender: the arg-max (lower id) of the row without its label (K == 1: the label itself)."""
    if V.shape[1] == 1:
        return labels.clone()
    rest = V.clone()
    rest[torch.arange(V.shape[0], device=V.device), labels] = -float("inf")
    return assign64(rest)[0]


def update64(X, labels, prev, spherical=False, count_offset=0):
    """-> (counts (K,) int64, centroids (K, d) float64): the mean of every cluster's bf16 rows (spherical: the sum scaled to
    unit norm); an empty cluster keeps its row of `prev`.  count_offset != 0 is a planted error (divides by the wrong count)."""
    K, d = prev.shape
    lab = labels.to(torch.int64)
    counts = torch.bincount(lab, minlength=K)
    sums = torch.zeros(K, d, dtype=torch.float64, device=X.device).index_add_(0, lab, X.double())
    if spherical:
        cent = sums / sums.norm(dim=1, keepdim=True).clamp_min(1e-300)
    else:
        cent = sums / (counts + count_offset).clamp_min(1).double()[:, None]
    return counts, torch.where((counts > 0)[:, None], cent, prev.double())


def abs_sums64(X, labels, K):
    """(K, d) float64: sum_i |x_i| per cluster and dimension -- the scale of the fp32 running-sum bound."""
    return torch.zeros(K, X.shape[1], dtype=torch.float64, device=X.device).index_add_(0, labels.to(torch.int64), X.double().abs())


def reseed_points(best, counts):
    """{empty cluster id: point id}: ascending cluster id takes the not-yet-used point with the smallest best, ties to the
    lower point id."""
    order = sorted(range(best.numel()), key=lambda i: (float(best[i]), i))
    empty = [int(c) for c in torch.nonzero(counts == 0).flatten().tolist()]
    return {c: order[j] for j, c in enumerate(empty[: len(order)])}


def lloyd_step64(X, C, spherical=False):
    """One iteration from centroids C (K, d; the kernel sees them rounded to bf16): -> (labels, best, counts, new centroids
    float64 with the empty clusters re-seeded to their points)."""
    Cb = C.to(torch.bfloat16)
    hn = None if spherical else 0.5 * Cb.double().square().sum(1)
    labels, best, _ = assign64(values64(X, Cb, hn))
    counts, cent = update64(X, labels, C, spherical)
    for c, i in reseed_points(best.cpu(), counts.cpu()).items():
        row = X[i].double()
        cent[c] = row / row.norm().clamp_min(1e-300) if spherical else row
    return labels, best, counts, cent


def gaussian_operands(N, K, d, unit, seed=None):
    """Seeded Gaussian points and centroids in bf16 (CPU), unit-norm rows or as drawn."""
    g = torch.Generator().manual_seed(1000 * N + K + d + (7 if unit else 0) if seed is None else seed)
    X, C = torch.randn(N, d, generator=g), torch.randn(K, d, generator=g)
    if unit:
        X, C = torch.nn.functional.normalize(X, dim=1), torch.nn.functional.normalize(C, dim=1)
    return X.to(torch.bfloat16), C.to(torch.bfloat16)


def half_norm32(C):
    """|c|^2 / 2 of bf16 rows in fp32, summed over ascending dimension (the definition cx_kmeans_finish implements; the squares
    are exact in fp32)."""
    sq = C.float().square()
    h = torch.zeros(C.shape[0], dtype=torch.float32, device=C.device)
    for j in range(C.shape[1]):
        h = h + sq[:, j]
    return 0.5 * h


RANDOM_SHAPES = [(1000, 129, 64), (1000, 257, 320), (1000, 1000, 1024), (1000, 127, 1024), (300, 2, 64)]
