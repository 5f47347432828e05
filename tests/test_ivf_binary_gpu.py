"""IVFBinaryIndex on the GPU against tests/ivf_binary_ref.py, by equality: the k-majority update, train, add + search, the
exact search at nprobe == nlist and the covering re-scored search."""
import numpy as np
import pytest
import torch

from tests import ivf_binary_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def corpus():
    """1000 float rows around 16 centres (d = 192), their codes, 40 queries."""
    g = torch.Generator().manual_seed(11)
    centres = torch.randn(16, 192, generator=g)
    x = (centres[torch.randint(0, 16, (1000,), generator=g)] + 0.7 * torch.randn(1000, 192, generator=g)).numpy()
    q = (centres[torch.randint(0, 16, (40,), generator=g)] + 0.7 * torch.randn(40, 192, generator=g)).numpy()
    return x, np.packbits(x > 0, axis=1), q, np.packbits(q > 0, axis=1)


@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_kmeans_update_against_the_reference(n, d):
    from contrastors_amd import _C

    h = _C.lib()
    rng = np.random.default_rng(n + d)
    codes = rng.integers(0, 256, (n, d // 8), dtype=np.uint8)
    cen = rng.integers(0, 256, (7, d // 8), dtype=np.uint8)
    cases = [rng.integers(0, 6, n), np.full(n, 3), np.arange(n) % 2 * 4]             # list 6 is empty; one list; 0 and 4
    if n >= 4:                                                                       # list 6 = rows 0 - 3: 2 of 4 on every bit
        codes[:4] = np.array([0, 0, 255, 255], np.uint8)[:, None]
        cases.append(np.concatenate([np.full(4, 6), rng.integers(0, 6, n - 4)]))
    for labels in cases:
        wide = torch.zeros(n, d // 8 + 8, dtype=torch.uint8, device=DEV)             # a leading dimension
        wide[:, : d // 8] = torch.from_numpy(codes)
        lab = torch.from_numpy(labels.astype(np.int32)).to(DEV)
        c = torch.from_numpy(cen).to(DEV)
        sizes = torch.full((7,), -1, dtype=torch.int32, device=DEV)
        ws = torch.empty(h.cx_binary_kmeans_update_ws_bytes(n, d, 7), dtype=torch.uint8, device=DEV)
        _C.check(h.cx_binary_kmeans_update(wide.data_ptr(), n, d, d // 8 + 8, lab.data_ptr(), 7, ws.data_ptr(), c.data_ptr(),
                                           sizes.data_ptr(), _C.cur_stream()))
        want, wsizes = B.update(codes, labels, cen)
        assert np.array_equal(c.cpu().numpy(), want) and np.array_equal(sizes.cpu().numpy(), wsizes)


@pytest.mark.parametrize("sample", [None, 300])
@pytest.mark.parametrize("source", ["device", "host", "memmap"])
def test_train_against_the_reference(corpus, source, sample, tmp_path):
    from contrastors_amd.search import IVFBinaryIndex, pq_train_rows

    x, codes, _, _ = corpus
    rows, first = pq_train_rows(1000, sample, 5, first=16)
    sc = codes if rows is None else codes[rows.numpy()]
    want = B.train(sc, first.numpy(), 3)
    if source == "memmap":
        np.save(tmp_path / "x.npy", x)
        src = np.load(tmp_path / "x.npy", mmap_mode="r")
    else:
        src = torch.from_numpy(x).to(DEV) if source == "device" else x
    for given in (src, torch.from_numpy(codes).to(DEV) if source == "device" else codes):    # float rows, then codes
        ix = IVFBinaryIndex(192, 16, device=DEV, seed=5)
        ix.train(given, max_iter=3, sample=sample)
        assert ix.centroids.dtype == torch.uint8 and np.array_equal(ix.centroids.cpu().numpy(), want)


def test_add_and_search_against_the_reference(corpus):
    from contrastors_amd.search import BinaryFlatIndex, IVFBinaryIndex

    x, codes, q, qc = corpus
    ix = IVFBinaryIndex(192, 16, device=DEV, workspace_bytes=1 << 16)               # several query batches
    ix.train(x, max_iter=3)
    cen = ix.centroids.cpu().numpy()
    ix.add(x[:1])
    ix.add(codes[1:130])
    ix.add(torch.from_numpy(x[130:777]).to(DEV))
    assert B.same(ix.search(qc, 10, 3), B.ivf_search(qc, codes[:777], cen, 10, 3))
    ix.add(codes[777:])                                                             # an add that follows a search
    labels = B.assign(codes, cen)
    assert np.array_equal(ix.list_sizes.cpu().numpy(), np.bincount(labels, minlength=16))
    assert np.array_equal(ix.codes.cpu().numpy(), codes[np.argsort(labels, kind="stable")])
    top = B.ivf_search(qc, codes, cen, 1, 16)[1][:, 0]
    exclude = [[int(t), 5] for t in top]
    md = (B.hamming(qc, codes).min(1) + np.arange(40) % 9 * 4).astype(np.int32)
    for nprobe in (1, 4):
        assert B.same(ix.search(q, 10, nprobe), B.ivf_search(qc, codes, cen, 10, nprobe))            # float queries
        assert B.same(ix.search(qc, 200, nprobe, exclude, md), B.ivf_search(qc, codes, cen, 200, nprobe, exclude, md))
    # every list probed: BinaryFlatIndex.search bit for bit
    flat = BinaryFlatIndex(192, device=DEV)
    flat.add(codes)
    assert B.same(ix.search(qc, 50, 16, exclude, md), flat.search(qc, 50, exclude=exclude, max_dist=md))
    assert B.same(ix.search(qc, 50, 16), flat.search(qc, 50))


def test_covering_rescored_search_is_the_exact_search_of_the_probed_lists(corpus):
    from contrastors_amd.search import FlatIPIndex, IVFBinaryIndex, search_ivf_binary_rescored

    x, codes, q, qc = corpus
    ix = IVFBinaryIndex(192, 16, device=DEV)
    ix.train(x, max_iter=3)
    ix.add(x)
    cen = ix.centroids.cpu().numpy()
    labels, probes = B.assign(codes, cen), B.window_topk(B.hamming(qc, cen), 2)[1]
    flat = FlatIPIndex(192, device=DEV)
    flat.add(x)
    fs, fi = flat.search(q, 1000)                                                   # every row, best first
    gs, gi = search_ivf_binary_rescored(ix, x, q, 10, 2, rescore_factor=100)        # 1000 candidates: covers two lists
    for m in range(40):
        keep = np.isin(labels[fi[m]], probes[m])
        assert np.array_equal(gi[m], fi[m][keep][:10]) and np.array_equal(gs[m].view(np.uint32), fs[m][keep][:10].view(np.uint32))
