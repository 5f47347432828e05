"""IVFPQIndex on the GPU against tests/ivf_pq_ref.py and the existing public pieces, by equality: the residual encoder, train,
search (lists, bias, merge), by_residual=False against PQFlatIndex, and the covering re-scored search."""
import numpy as np
import pytest
import torch

from tests import ivf_pq_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, DSUB = 64, 8


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    ids = [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in (got[1], want[1])]
    return np.array_equal(ids[0], ids[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))


def _unaligned(t):
    """The same bf16 rows at an odd element offset with a row stride of d + 3: the element-load path."""
    n, d = t.shape
    return torch.zeros(n * (d + 3) + 1, dtype=t.dtype, device=DEV)[1:].view(n, d + 3)[:, :d].copy_(t)


@pytest.mark.parametrize("dsub", [8, 16, 32, 64])
@pytest.mark.parametrize("d", [64, 192])
def test_residual_encoder_equals_pq_encode_of_torch_residuals(d, dsub):
    from contrastors_amd import _C
    from contrastors_amd.search import PQFlatIndex, pq_encode

    g = torch.Generator().manual_seed(d + dsub)
    m = d // dsub
    pq = PQFlatIndex(d, dsub, device=DEV)
    pq.train(codebooks=torch.randn(m, 256, dsub, generator=g))
    for n in (1, 63, 65, 300):
        for nlist in (1, 7):
            x = torch.randn(n, d, generator=g).to(DEV, torch.bfloat16)
            cen = torch.randn(nlist, d, generator=g).to(DEV, torch.bfloat16)
            labels = torch.randint(0, nlist, (n,), generator=g, dtype=torch.int32).to(DEV)
            res = (x.float() - cen[labels.long()].float()).to(torch.bfloat16)
            want = pq_encode(res, pq.codebooks)
            if (n, nlist, d) == (63, 7, 64):
                ref = V.encode(x.float().cpu().numpy(), labels.cpu().numpy(), cen.float().cpu().numpy(),
                               pq.codebooks.float().cpu().numpy())
                assert np.array_equal(want.cpu().numpy(), ref)
            for xs, cs in ((x, cen), (_unaligned(x), _unaligned(cen)), (x, _unaligned(cen))):
                codes = torch.full((n, m + 2), 0xAB, dtype=torch.uint8, device=DEV)     # ld > m: the bytes beyond stay
                _C.check(_C.lib().cx_pq_assign_residual(xs.data_ptr(), n, d, xs.stride(0), labels.data_ptr(), cs.data_ptr(), nlist,
                                                        cs.stride(0), pq.codebooks.data_ptr(), pq.half_norms.data_ptr(), dsub,
                                                        codes.data_ptr(), m + 2, _C.cur_stream()))
                assert torch.equal(codes[:, :m], want) and bool((codes[:, m:] == 0xAB).all()), (n, nlist)


def _coarse(centroids):
    from contrastors_amd.search import FlatIPIndex

    co = FlatIPIndex(D, device=DEV)
    co.add(centroids)
    return co


def _acc(rows, Q):
    """FlatIPIndex's score of every (query, row) as an (M, N) matrix, N <= 1024."""
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(D, device=DEV)
    ix.add(rows)
    s, i = ix.search(Q, rows.shape[0])
    return torch.empty_like(s).scatter_(1, i, s).cpu().numpy()


def test_train_equals_the_pipeline_of_the_public_pieces():
    from contrastors_amd.cluster import KMeans
    from contrastors_amd.search import IVFPQIndex, PQFlatIndex

    x = torch.randn(1000, D, generator=torch.Generator().manual_seed(5)).to(DEV)
    ix = IVFPQIndex(D, 4, DSUB, device=DEV, seed=3)
    ix.train(x, max_iter=3, pq_iters=3)
    c = KMeans(4, D, spherical=True, device=DEV, seed=3).fit(x, max_iter=3).centroids
    xb, cb = x.to(torch.bfloat16), c.to(torch.bfloat16)
    labels = _coarse(c).search(xb, 1)[1][:, 0]
    pq = PQFlatIndex(D, DSUB, device=DEV, seed=3)
    pq.train((xb.float() - cb[labels].float()).to(torch.bfloat16), max_iter=3)
    assert torch.equal(ix.centroids, c) and torch.equal(ix.pq.masters, pq.masters)
    assert torch.equal(ix.pq.codebooks, pq.codebooks) and torch.equal(ix.pq.half_norms, pq.half_norms)


@pytest.fixture(scope="module")
def corpus():
    g = torch.Generator().manual_seed(11)
    return torch.randn(1000, D, generator=g).numpy(), torch.randn(37, D, generator=g).numpy()


def _filled(x, nlist, tmp_path, by_residual=True):
    """Trained on x and filled with it in three uneven adds (device, host, memmap), with a search between the first two."""
    from contrastors_amd.search import IVFPQIndex

    ix = IVFPQIndex(D, nlist, DSUB, by_residual=by_residual, device=DEV, seed=1)
    ix.train(torch.from_numpy(x).to(DEV), max_iter=2, pq_iters=2)
    ix.add(torch.from_numpy(x[:100]).to(DEV))
    ix.search(x[:3], 5, 1)
    ix.add(x[100:101])
    np.save(tmp_path / "rows.npy", x[101:])
    ix.add(np.load(tmp_path / "rows.npy", mmap_mode="r"))
    return ix


@pytest.mark.parametrize("nlist", [1, 4, 16])
@pytest.mark.parametrize("N", [300, 1000])
def test_search_equals_the_reference(N, nlist, corpus, tmp_path):
    from contrastors_amd.search import pq_encode, search_ivf_pq_rescored

    x, Q = corpus[0][:N], corpus[1]
    ix = _filled(x, nlist, tmp_path)
    co = _coarse(ix.centroids)
    xb, cb = torch.from_numpy(x).to(DEV, torch.bfloat16), ix.centroids.to(torch.bfloat16)
    labels = co.search(xb, 1)[1][:, 0]
    assert torch.equal(ix.list_sizes, torch.bincount(labels, minlength=nlist))
    dec = ix.pq.decode_codes(pq_encode((xb.float() - cb[labels].float()).to(torch.bfloat16), ix.pq.codebooks))
    assert torch.equal(ix.decode(), dec.float() + cb[labels].float())
    acc, exact, lab = _acc(dec, torch.from_numpy(Q).to(DEV)), _acc(xb, torch.from_numpy(Q).to(DEV)), labels.cpu().numpy()
    for nprobe in sorted({1, min(3, nlist), nlist}):
        coarse, probes = (t.cpu().numpy() for t in co.search(torch.from_numpy(Q).to(DEV), nprobe))
        for k in (1, 10, 1024):                                          # 1024: more than the probed rows
            got = ix.search(Q, k, nprobe)
            assert isinstance(got[0], np.ndarray) and _same(got, V.ivf_search(acc, lab, probes, coarse, k)), (nprobe, k)
        exclude = [[int(t)] for t in got[1][:, 0]]
        below = np.where(np.arange(Q.shape[0]) % 2 == 0, got[0][:, 1], np.inf).astype(np.float32)
        got = ix.search(torch.from_numpy(Q), 10, nprobe, exclude=exclude, below=below)
        assert _same(got, V.ivf_search(acc, lab, probes, coarse, 10, exclude=exclude, below=below)), nprobe
        # a covering candidate list: FlatIPIndex's scores of the original rows, restricted to the probed lists
        got = search_ivf_pq_rescored(ix, x, Q, 10, nprobe, rescore_factor=100)
        assert _same(got, V.ivf_search(exact, lab, probes, coarse, 10, by_residual=False)), nprobe


def test_without_residuals_every_list_probed_is_pqflatindex(corpus, tmp_path):
    from contrastors_amd.search import PQFlatIndex

    x, Q = corpus
    ix = _filled(x, 4, tmp_path, by_residual=False)
    pq = PQFlatIndex(D, DSUB, device=DEV)
    pq.train(codebooks=ix.pq.masters)
    pq.add(x)
    assert torch.equal(ix.decode(), pq.decode().float())
    for k in (1, 10, 1024):
        assert _same(ix.search(Q, k, 4), pq.search(Q, k))
