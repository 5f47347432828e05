"""GPU checks of IVFInt8Index and search_ivf_int8_rescored (contrastors_amd.search): with every list probed the index IS
Int8FlatIndex.search, bit for bit; its lists are IVFFlatIndex's lists and its codes Int8FlatIndex's codes; with fewer probes it
is the host merge of per-list Int8FlatIndex searches over exactly the lists the coarse search names; and the bookkeeping
(chunked adds from tensors, arrays and memmaps, determinism, query batching, empty lists).  The two-stage search against
FlatIPIndex.search and rescore.  All comparisons are bitwise."""
import gzip
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import search_window_ref as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
DEV = "cuda:0"


def _unit(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, device=DEV, generator=g), dim=1)


def _grid(n, d, seed):
    """Entries in {-1/2, 0, 1/2}: codes in {-127, 0, 127}, equal scales, score ties everywhere."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-1, 2, (n, d), device=DEV, generator=g).float() / 2


def _same(got, want):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[0].shape == want[0].shape
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


def _flat8(D):
    from contrastors_amd.search import Int8FlatIndex

    ix = Int8FlatIndex(D.shape[1], device=DEV)
    if D.shape[0]:
        ix.add(D)
    return ix


def _flat(D):
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(D.shape[1], device=DEV)
    if D.shape[0]:
        ix.add(D)
    return ix


def _ivf8(D, nlist, centroids=None, seed=0, cls=None, **kw):
    from contrastors_amd.search import IVFInt8Index

    ix = (cls or IVFInt8Index)(D.shape[1], nlist, device=DEV, seed=seed, **kw)
    if centroids is None and D.shape[0] >= nlist:
        ix.train(D)
    else:       # fewer rows than lists (or a given table): random unit centroids
        ix.train(centroids=_unit(nlist, D.shape[1], 77) if centroids is None else centroids)
    ix.add(D)
    return ix


def _filters(flat, Q, k, N, seed):
    g = np.random.default_rng(seed)
    es, ei = flat.search(Q, k)
    M = Q.shape[0]
    exclude = [[int(ei[r, 0])] + g.integers(0, N, r % 3).tolist() for r in range(M)]
    below = es[:, min(k, N) // 2].clone()
    below[torch.isinf(below)] = 0.0
    return exclude, below


@pytest.mark.parametrize("make", [_unit, _grid], ids=["gauss", "grid"])
@pytest.mark.parametrize("nlist", [1, 2, 7, 64])
@pytest.mark.parametrize("N", [1, 129, 1000, 5000])
def test_all_lists_probed_is_the_flat_int8_search(N, nlist, make):
    d, M = 64, 150
    D, Q = make(N, d, N + nlist), make(M, d, 5)
    flat, ivf = _flat8(D), _ivf8(D, nlist)
    assert ivf.ntotal == N and int(ivf.list_sizes.sum()) == N and ivf.list_sizes.shape == (nlist,)
    assert ivf.codes.shape == (N, d) and ivf.codes.dtype == torch.int8 and ivf.scales.shape == (N,)
    for k in (1, 10, 300):
        exclude, below = _filters(flat, Q, k, N, k)
        for ex, bel in ((None, None), (exclude, below)):
            want = flat.search(Q, k, exclude=ex, below=bel)
            got = ivf.search(Q, k, nlist, exclude=ex, below=bel)
            assert got[0].shape == (M, k)
            _same(got, want)
    # numpy in -> numpy out
    s, i = ivf.search(Q.cpu().numpy(), 10, nlist)
    es, ei = flat.search(Q.cpu().numpy(), 10)
    assert isinstance(s, np.ndarray) and np.array_equal(i, ei) and np.array_equal(s.view(np.int32), es.view(np.int32))


@pytest.mark.parametrize("make", [_unit, _grid], ids=["gauss", "grid"])
def test_same_lists_as_the_bf16_index_and_the_flat_index_codes(make):
    from contrastors_amd.search import IVFFlatIndex, quantize_rows_int8

    d, N, nlist = 128, 3000, 16
    D = make(N, d, 1)
    ivf = _ivf8(D, nlist)
    ref = _ivf8(D, nlist, centroids=ivf.centroids, cls=IVFFlatIndex)
    assert torch.equal(ivf.list_sizes, ref.list_sizes) and torch.equal(ivf._order, ref._order)
    assert torch.equal(ivf._list_ptr, ref._list_ptr) and torch.equal(ivf._labels, ref._labels)
    codes, scales = quantize_rows_int8(D)
    assert torch.equal(ivf.codes, codes[ivf._order])
    assert torch.equal(ivf.scales.view(torch.int32), scales[ivf._order].view(torch.int32))
    flat = _flat8(D)
    assert torch.equal(ivf.codes, flat.codes[ivf._order]) and torch.equal(ivf.scales, flat.scales[ivf._order])
    # a host source gives the same lists and codes
    host = _ivf8(D.cpu().numpy(), nlist, centroids=ivf.centroids)
    assert torch.equal(host.list_sizes, ivf.list_sizes) and torch.equal(host._order, ivf._order)
    assert torch.equal(host.codes, ivf.codes) and torch.equal(host.scales, ivf.scales)


def _per_list_expected(ivf, Q, k, probes, exclude=None, below=None):
    """Host merge of per-list Int8FlatIndex searches over the lists `probes` names; ids mapped back to the original ones."""
    from contrastors_amd.search import Int8FlatIndex

    M, L = probes.shape
    order, ptr = ivf._order, ivf._list_ptr.tolist()
    inv = {int(o): p for p, o in enumerate(order.tolist())}
    codes, scales = ivf.codes, ivf.scales
    qc, qs = Int8FlatIndex(ivf.d, device=DEV)._query_codes(Q)
    scores = torch.full((M * L, k), -float("inf"), dtype=torch.float32, device=DEV)
    ids = torch.full((M * L, k), -1, dtype=torch.int64, device=DEV)
    for l in sorted(set(probes.flatten().tolist())):
        a, b = ptr[l], ptr[l + 1]
        if b == a:
            continue
        m_idx, j_idx = torch.nonzero(probes == l, as_tuple=True)
        ex = None
        if exclude is not None:
            ex = [[inv[e] - a for e in exclude[m] if e in inv and a <= inv[e] < b] for m in m_idx.tolist()]
        one = Int8FlatIndex(ivf.d, device=DEV)
        one.add((codes[a:b], scales[a:b]))
        s, i = one.search((qc[m_idx], qs[m_idx]), k, exclude=ex, below=None if below is None else below[m_idx])
        rows = m_idx * L + j_idx
        scores[rows], ids[rows] = s, torch.where(i >= 0, i + a, i)
    src = np.arange(M * L).reshape(M, L)
    return W.merge_ref(scores, ids, src, k, order)


@pytest.mark.parametrize("make", [_unit, _grid], ids=["gauss", "grid"])
def test_fewer_lists_probed_is_the_merge_of_per_list_searches(make):
    d, N, M, nlist = 128, 3000, 200, 16
    D, Q = make(N, d, 1), make(M, d, 2)
    ivf = _ivf8(D, nlist)
    ivf.list_sizes                                   # (sorts the rows)
    flat = _flat8(D)
    for nprobe, k in ((1, 10), (3, 40), (5, 300), (15, 10)):
        probes = ivf._coarse.search(Q.to(torch.bfloat16), nprobe)[1]      # the existing coarse search's answer
        exclude, below = _filters(flat, Q, k, N, nprobe)
        for ex, bel in ((None, None), (exclude, below)):
            es, ei = _per_list_expected(ivf, Q, k, probes, ex, bel)
            s, i = ivf.search(Q, k, nprobe, exclude=ex, below=bel)
            assert np.array_equal(i.cpu().numpy(), ei), (nprobe, k, ex is not None)
            assert np.array_equal(s.cpu().numpy().view(np.int32), es.view(np.int32)), (nprobe, k, ex is not None)
    # what is found is a subset of the flat answer's pairs, with the flat search's score bits
    s, i = ivf.search(Q, 10, 3)
    fs, fi = flat.search(Q, 1024)
    for r in range(0, M, 13):
        where = dict(zip(fi[r].tolist(), fs[r].tolist()))
        assert all(where.get(a, b) == b for a, b in zip(i[r].tolist(), s[r].tolist()) if a >= 0)


def test_empty_lists_padding_an_empty_index_and_reset():
    from contrastors_amd.search import IVFInt8Index

    d, N, M = 64, 500, 70
    D, Q = _unit(N, d, 3).abs(), _unit(M, d, 4).abs()          # everything in the positive orthant
    C = _unit(8, d, 5).abs()
    C[[1, 4, 6]] *= -1                                          # three centroids no row ever prefers
    ivf = _ivf8(D, 8, centroids=C)
    sizes = ivf.list_sizes.tolist()
    assert sizes[1] == sizes[4] == sizes[6] == 0 and sum(sizes) == N
    _same(ivf.search(Q, 300, 8), _flat8(D).search(Q, 300))
    # k larger than the probed rows: padding after exactly those rows
    probes = ivf._coarse.search(Q.to(torch.bfloat16), 2)[1]
    s, i = ivf.search(Q, 1024, 2)
    want = torch.tensor(sizes, device=DEV)[probes].sum(1).clamp(max=1024)
    assert torch.equal((i >= 0).sum(1), want) and torch.equal(i >= 0, ~torch.isinf(s))
    assert bool((want < 1024).any())
    # an empty index; then one whose lists are all empty for a query's probes: only padding
    ix = IVFInt8Index(d, 8, device=DEV)
    ix.train(centroids=C)
    s, i = ix.search(Q, 5, 3)
    assert bool((i == -1).all()) and bool(torch.isinf(s).all()) and ix.list_sizes.tolist() == [0] * 8
    assert ix.codes.shape == (0, d) and ix.scales.shape == (0,)
    ix.add(-D[:40])                                             # rows only the negated centroids attract
    assert sum(ix.list_sizes[[1, 4, 6]].tolist()) == 40
    s, i = ix.search(Q, 5, 3)                                   # the queries' three best lists hold nothing
    assert bool((i == -1).all())
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained and ix.codes.shape == (0, d)
    ix.add(D[:10])
    assert ix.ntotal == 10 and ix.codes.shape == (10, d)


def test_adds_in_chunks_from_anywhere_and_after_a_search_equal_one_add(tmp_path):
    from contrastors_amd.search import IVFInt8Index

    d, N, M, nlist, k = 64, 2000, 100, 12, 50
    D, Q = _unit(N, d, 6), _unit(M, d, 7)
    one = _ivf8(D, nlist)
    want = one.search(Q, k, 4)
    np.save(tmp_path / "rows.npy", D.cpu().numpy())
    mm = np.load(tmp_path / "rows.npy", mmap_mode="r")
    for searched_between in (False, True):
        ix = IVFInt8Index(d, nlist, device=DEV)
        ix.train(centroids=one.centroids)
        for n, (a, b) in enumerate(((0, 1), (1, 1300), (1300, N))):
            ix.add((D[a:b], D[a:b].cpu().numpy(), mm[a:b])[n])          # a device tensor, an array, a memmap slice
            if searched_between:
                ix.search(Q[:3], 5, 2)
        assert ix.ntotal == N and torch.equal(ix.list_sizes, one.list_sizes)
        _same(ix.search(Q, k, 4), want)
        assert torch.equal(ix._order, one._order) and torch.equal(ix.codes, one.codes) and torch.equal(ix.scales, one.scales)
    whole = IVFInt8Index(d, nlist, device=DEV)
    whole.train(centroids=one.centroids)
    whole.add(mm)                                                        # the memmap itself
    _same(whole.search(Q, k, 4), want)


def test_training_is_deterministic():
    d, N, M = 64, 3000, 64
    D, Q = _unit(N, d, 8), _unit(M, d, 9)
    a, b = _ivf8(D, 20, seed=3), _ivf8(D, 20, seed=3)
    assert torch.equal(a.centroids, b.centroids) and torch.equal(a.list_sizes, b.list_sizes)
    ra, rb = a.search(Q, 30, 5), b.search(Q, 30, 5)
    _same(ra, rb)
    _same(a.search(Q, 30, 5), ra)


def test_query_batching_by_a_small_workspace():
    d, N, M, nlist, k, nprobe = 64, 3000, 700, 16, 20, 4
    D, Q = _unit(N, d, 10), _unit(M, d, 11)
    big = _ivf8(D, nlist)
    exclude, below = _filters(_flat8(D), Q, k, N, 0)
    want = big.search(Q, k, nprobe, exclude=exclude, below=below)
    assert big.batch_queries(M, k, nprobe) == M
    for ws in (1 << 20, 1 << 17, 1):
        small = _ivf8(D, nlist, centroids=big.centroids, workspace_bytes=ws)
        mq = small.batch_queries(M, k, nprobe)
        assert mq < M and (mq % 128 == 0 or mq < 128)
        if ws == 1:
            assert mq == 1
            _same(small.search(Q[:9], k, nprobe, exclude=exclude[:9], below=below[:9]), (want[0][:9], want[1][:9]))
        else:
            _same(small.search(Q, k, nprobe, exclude=exclude, below=below), want)


# ---- the two-stage search ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [129, 1000])
def test_covering_rescored_search_is_the_exact_search(N, tmp_path):
    from contrastors_amd.search import search_ivf_int8_rescored

    d, M, nlist, k, R = 64, 130, 5, 250, 4                      # k * R = 1000 candidates cover the corpus
    D, Q = _unit(N, d, 20 + N), _unit(M, d, 21)
    flat, ivf = _flat(D), _ivf8(D, nlist)
    exclude, below = _filters(flat, Q, k, N, 1)
    np.save(tmp_path / "rows.npy", D.cpu().numpy())
    sources = (D.to(torch.bfloat16), D.cpu().numpy(), np.load(tmp_path / "rows.npy", mmap_mode="r"))
    for ex, bel in ((None, None), (exclude, below)):
        want = flat.search(Q, k, exclude=ex, below=bel)
        for vectors in sources:
            _same(search_ivf_int8_rescored(ivf, vectors, Q, k, nlist, R, exclude=ex, below=bel), want)
    s, i = search_ivf_int8_rescored(ivf, sources[1], Q.cpu().numpy(), 10, nlist, 100)
    es, ei = flat.search(Q.cpu().numpy(), 10)
    assert isinstance(s, np.ndarray) and np.array_equal(i, ei) and np.array_equal(s.view(np.int32), es.view(np.int32))


def test_partial_rescored_search_is_rescore_of_the_index_candidates_and_paging():
    from contrastors_amd.search import rescore, search_int8_rescored, search_ivf_int8_rescored

    d, N, M, nlist = 64, 5000, 100, 16
    D, Q = _unit(N, d, 30), _unit(M, d, 31)
    ivf = _ivf8(D, nlist)
    Db = D.to(torch.bfloat16)
    exclude, below = _filters(_flat(D), Q, 10, N, 2)
    for k, R, nprobe in ((10, 2, 3), (10, 4, 1), (100, 3, 5)):
        for ex, bel in ((None, None), (exclude, below)):
            cand = ivf.search(Q, k * R, nprobe, exclude=ex)[1]
            _same(search_ivf_int8_rescored(ivf, Db, Q, k, nprobe, R, exclude=ex, below=bel), rescore(Q, cand, Db, k, below=bel))
    # 1200 candidates come in two pages of the same ranking; with every list probed that is the flat int8 pipeline's answer
    flat8 = _flat8(D)
    for ex in (None, exclude):
        _same(search_ivf_int8_rescored(ivf, Db, Q, 300, nlist, 4, exclude=ex), search_int8_rescored(flat8, Db, Q, 300, 4, exclude=ex))


# ---- the tools -------------------------------------------------------------------------------------------------------
def _tool(name, *args):
    r = subprocess.run([sys.executable, "-m", f"contrastors_amd.tools.{name}", *args], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def test_tools_with_int8_lists_write_the_fixture_shards(tmp_path):
    fx = json.loads((GOLD / "search_curation.json").read_text())
    ivf = ("--ivf_lists", "4", "--ivf_nprobe", "4", "--ivf_storage", "int8", "--rescore_factor", "32")
    c = fx["consistency"]
    np.save(tmp_path / "cq.npy", np.asarray(c["q"], np.float32))
    np.save(tmp_path / "cd.npy", np.asarray(c["d"], np.float32))
    (tmp_path / "ids.json").write_text(json.dumps(c["ids"]))
    _tool("consistency_filter", "--output_dir", str(tmp_path / "cf"), "--query_embeddings", str(tmp_path / "cq.npy"),
          "--document_embeddings", str(tmp_path / "cd.npy"), "--ids", str(tmp_path / "ids.json"), *ivf)
    assert json.loads((tmp_path / "cf" / "ids_to_keep_0.json").read_text()) == c["kept"]
    t = fx["topk"]
    with open(tmp_path / "recs.jsonl", "w") as f:
        for r in t["records"]:
            f.write(json.dumps(r) + "\n")
    np.save(tmp_path / "tq.npy", np.asarray(t["q"], np.float32))
    np.save(tmp_path / "td.npy", np.asarray(t["d"], np.float32))
    np.save(tmp_path / "c.npy", np.asarray(t["d"], np.float32)[:4])         # the centroids from a file: four document rows
    for name, extra in (("tk", ("--ivf_sample", "6", "--ivf_iters", "3")), ("tkc", ("--ivf_centroids", str(tmp_path / "c.npy")))):
        _tool("mine_negatives", "--rule", "topk", "--dataset", str(tmp_path / "recs.jsonl"), "--output_dir",
              str(tmp_path / name), "--k", str(t["k"]), "--seed", str(t["seed"]), "--query_embeddings",
              str(tmp_path / "tq.npy"), "--document_embeddings", str(tmp_path / "td.npy"), *ivf, *extra)
        got = []
        for p in sorted((tmp_path / name).glob("shard-*.jsonl.gz")):
            with gzip.open(p, "rt") as f:
                got += [json.loads(line) for line in f]
        for g in got:
            assert g.pop("metadata")["objective"]["triplet"] == [["question", "positive_ctxs", "hard_negative_ctxs"]]
        assert got == t["expected"]
