"""GPU check of the per-batch offsets of the shared search skeletons (contrastors_amd.search._FlatIndex._search_batched and
_IVFLists.search): a workspace bound that cuts 300 queries into batches of 128, 128 and 44 must give the bits of the one-batch
search, with exclusion lists and a per-row bound that differ from row to row -- so a query, a CSR offset, a bound or an output
row taken from the wrong batch position changes the result."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D_, N, M, K = 64, 257, 300, 5
EDGE_ROWS = (0, 127, 128, 255, 256, 299)    # the first and the last row of every batch


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, D_, generator=g), dim=1).to(DEV)


def _flat(kind, **kw):
    from contrastors_amd.search import BinaryFlatIndex, FlatIPIndex, Int8FlatIndex, PQFlatIndex

    ix = {"flat": FlatIPIndex, "binary": BinaryFlatIndex, "int8": Int8FlatIndex, "pq": PQFlatIndex}[kind](D_, device=DEV, **kw)
    if kind == "pq":    # given tables: nothing is fitted
        ix.train(codebooks=torch.randn(D_ // 8, 256, 8, generator=torch.Generator().manual_seed(3)))
    ix.add(_rows(N, 1))
    return ix


def _ivf(kind, **kw):
    from contrastors_amd.search import IVFBinaryIndex, IVFFlatIndex, pack_sign_bits

    c = torch.randn(4, D_, generator=torch.Generator().manual_seed(4))
    if kind == "binary":
        ix = IVFBinaryIndex(D_, 4, device=DEV, **kw)
        ix.train(centroids=pack_sign_bits(c))
    else:
        ix = IVFFlatIndex(D_, 4, device=DEV, **kw)
        ix.train(centroids=c)
    ix.add(_rows(N, 1))
    return ix


def _filters(s0, i0):
    """From the unfiltered result: per row 1 to 3 excluded ids (its best ones) and a bound at its entry 1 to 3."""
    exclude = [i0[r, : r % 3 + 1].tolist() for r in range(M)]
    bound = torch.stack([s0[r, r % 3 + 1] for r in range(M)])
    return exclude, bound


def _check_batched_equals_one_batch(big, small, bound_kw, **kw):
    Q = _rows(M, 2)    # fp32: the int8 index quantises them per row, so its query scales are sliced too
    s0, i0 = big.search(Q, K, **kw)
    exclude, bound = _filters(s0, i0)
    kw = dict(kw, exclude=exclude, **{bound_kw: bound})
    s1, i1 = big.search(Q, K, **kw)
    for r in EDGE_ROWS:    # the filters bite on the rows at the batch edges
        assert not torch.equal(i1[r], i0[r]) and not (set(i1[r].tolist()) - {-1}) & set(exclude[r]), r
    s2, i2 = small.search(Q, K, **kw)
    assert s2.dtype == s1.dtype and torch.equal(s2, s1) and torch.equal(i2, i1)


@pytest.mark.parametrize("kind", ["flat", "binary", "int8", "pq"])
def test_flat_search_in_three_batches_equals_one_batch(kind):
    big, small = _flat(kind), _flat(kind, workspace_bytes=1)
    assert big.batch_rows(M, K) == M and small.batch_rows(M, K) == 128
    assert [min(128, M - b0) for b0 in range(0, M, 128)] == [128, 128, 44]
    _check_batched_equals_one_batch(big, small, "max_dist" if kind == "binary" else "below")


@pytest.mark.parametrize("kind", ["flat", "binary"])
def test_ivf_search_in_three_batches_equals_one_batch(kind):
    nprobe = 2
    big = _ivf(kind)
    per_pair = K * 12 + K * 8 + 4 + big._pair_row_bytes() + 32    # batch_queries' bytes per (query, probed list) pair
    small = _ivf(kind, workspace_bytes=128 * nprobe * per_pair)
    assert big.batch_queries(M, K, nprobe) == M and small.batch_queries(M, K, nprobe) == 128
    _check_batched_equals_one_batch(big, small, "max_dist" if kind == "binary" else "below", nprobe=nprobe)
