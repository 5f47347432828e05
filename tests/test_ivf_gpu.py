"""GPU checks of IVFFlatIndex (contrastors_amd.search): with every list probed it IS FlatIPIndex.search, bit for bit; with
fewer it is the host merge of per-list FlatIPIndex searches over exactly the lists the coarse search names; and the index's
bookkeeping (chunked adds, determinism, query batching, empty lists, own list first).  All comparisons are bitwise."""
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
    """Entries in {-1/2, 0, 1/2}: exact fp32 sums and score ties everywhere."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-1, 2, (n, d), device=DEV, generator=g).float() / 2


def _flat(D):
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(D.shape[1], device=DEV)
    if D.shape[0]:
        ix.add(D)
    return ix


def _ivf(D, nlist, centroids=None, seed=0, **kw):
    from contrastors_amd.search import IVFFlatIndex

    ix = IVFFlatIndex(D.shape[1], nlist, device=DEV, seed=seed, **kw)
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
def test_all_lists_probed_is_the_exact_search(N, nlist, make):
    d, M = 64, 150
    D, Q = make(N, d, N + nlist), make(M, d, 5)
    flat, ivf = _flat(D), _ivf(D, nlist)
    assert ivf.ntotal == N and int(ivf.list_sizes.sum()) == N and ivf.list_sizes.shape == (nlist,)
    assert ivf.centroids.shape == (nlist, d) and ivf.centroids.dtype == torch.float32
    for k in (1, 10, 300):
        exclude, below = _filters(flat, Q, k, N, k)
        for ex, bel in ((None, None), (exclude, below)):
            es, ei = flat.search(Q, k, exclude=ex, below=bel)
            s, i = ivf.search(Q, k, nlist, exclude=ex, below=bel)
            assert s.dtype == torch.float32 and i.dtype == torch.int64 and s.shape == (M, k)
            assert torch.equal(i, ei) and torch.equal(s, es), (k, ex is not None)
    # numpy in -> numpy out
    s, i = ivf.search(Q.cpu().numpy(), 10, nlist)
    es, ei = flat.search(Q.cpu().numpy(), 10)
    assert isinstance(s, np.ndarray) and np.array_equal(i, ei) and np.array_equal(s.view(np.int32), es.view(np.int32))


def _per_list_expected(ivf, flat_rows, Q, k, probes, exclude=None, below=None):
    """Host merge of per-list FlatIPIndex searches over the lists `probes` names; ids mapped back to the original ones."""
    M, L = probes.shape
    order, ptr = ivf._order, ivf._list_ptr.tolist()
    inv = {int(o): p for p, o in enumerate(order.tolist())}
    scores = torch.full((M * L, k), -float("inf"), dtype=torch.float32, device=DEV)
    ids = torch.full((M * L, k), -1, dtype=torch.int64, device=DEV)
    for l in sorted(set(probes.flatten().tolist())):
        a, b = ptr[l], ptr[l + 1]
        m_idx, j_idx = torch.nonzero(probes == l, as_tuple=True)
        ex = None
        if exclude is not None:
            ex = [[inv[e] - a for e in exclude[m] if e in inv and a <= inv[e] < b] for m in m_idx.tolist()]
        s, i = _flat(flat_rows[a:b]).search(Q[m_idx], k, exclude=ex, below=None if below is None else below[m_idx])
        rows = m_idx * L + j_idx
        scores[rows], ids[rows] = s, torch.where(i >= 0, i + a, i)
    src = np.arange(M * L).reshape(M, L)
    return W.merge_ref(scores, ids, src, k, order)


@pytest.mark.parametrize("make", [_unit, _grid], ids=["gauss", "grid"])
def test_fewer_lists_probed_is_the_merge_of_per_list_searches(make):
    d, N, M, nlist = 128, 3000, 200, 16
    D, Q = make(N, d, 1), make(M, d, 2)
    ivf = _ivf(D, nlist)
    ivf.list_sizes                                   # (sorts the rows)
    rows = ivf._rows                                 # bf16 rows in list order
    assert torch.equal(rows, D.to(torch.bfloat16)[ivf._order])
    flat = _flat(D)
    for nprobe, k in ((1, 10), (3, 40), (5, 300), (15, 10)):
        probes = ivf._coarse.search(Q.to(torch.bfloat16), nprobe)[1]      # the existing coarse search's answer
        exclude, below = _filters(flat, Q, k, N, nprobe)
        for ex, bel in ((None, None), (exclude, below)):
            es, ei = _per_list_expected(ivf, rows, Q.to(torch.bfloat16), k, probes, ex, bel)
            s, i = ivf.search(Q, k, nprobe, exclude=ex, below=bel)
            assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es), (nprobe, k, ex is not None)
    # what is found is a subset of the exact answer's pairs, with the exact score bits
    s, i = ivf.search(Q, 10, 3)
    fs, fi = flat.search(Q, 1024)
    for r in range(0, M, 13):
        where = dict(zip(fi[r].tolist(), fs[r].tolist()))
        assert all(where.get(a, b) == b for a, b in zip(i[r].tolist(), s[r].tolist()) if a >= 0)


def test_empty_lists_and_padding():
    d, N, M = 64, 500, 70
    D, Q = _unit(N, d, 3).abs(), _unit(M, d, 4).abs()          # everything in the positive orthant
    C = _unit(8, d, 5).abs()
    C[[1, 4, 6]] *= -1                                          # three centroids no row ever prefers
    ivf = _ivf(D, 8, centroids=C)
    sizes = ivf.list_sizes.tolist()
    assert sizes[1] == sizes[4] == sizes[6] == 0 and sum(sizes) == N
    es, ei = _flat(D).search(Q, 300)
    s, i = ivf.search(Q, 300, 8)
    assert torch.equal(i, ei) and torch.equal(s, es)
    # k larger than the probed rows: padding after exactly those rows
    probes = ivf._coarse.search(Q.to(torch.bfloat16), 2)[1]
    s, i = ivf.search(Q, 1024, 2)
    want = torch.tensor(sizes, device=DEV)[probes].sum(1).clamp(max=1024)
    assert torch.equal((i >= 0).sum(1), want) and torch.equal(i >= 0, ~torch.isinf(s))
    assert bool((want < 1024).any())
    # an index whose lists are all empty for a query's probes: only padding; and an empty index
    from contrastors_amd.search import IVFFlatIndex

    ix = IVFFlatIndex(d, 8, device=DEV)
    ix.train(centroids=C)
    s, i = ix.search(Q, 5, 3)
    assert bool((i == -1).all()) and bool(torch.isinf(s).all()) and ix.list_sizes.tolist() == [0] * 8
    ix.add(-D[:40])                                             # rows only the negated centroids attract
    assert sum(ix.list_sizes[[1, 4, 6]].tolist()) == 40
    s, i = ix.search(Q, 5, 3)                                   # the queries' three best lists hold nothing
    assert bool((i == -1).all())
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained


def test_adds_in_chunks_and_after_a_search_equal_one_add():
    d, N, M, nlist, k = 64, 2000, 100, 12, 50
    D, Q = _unit(N, d, 6), _unit(M, d, 7)
    one = _ivf(D, nlist)
    es, ei = one.search(Q, k, 4)
    from contrastors_amd.search import IVFFlatIndex

    for searched_between in (False, True):
        ix = IVFFlatIndex(d, nlist, device=DEV)
        ix.train(centroids=one.centroids)
        for a, b in ((0, 1), (1, 1300), (1300, N)):
            ix.add(D[a:b].cpu().numpy() if a else D[a:b])
            if searched_between:
                ix.search(Q[:3], 5, 2)
        assert ix.ntotal == N and torch.equal(ix.list_sizes, one.list_sizes)
        s, i = ix.search(Q, k, 4)
        assert torch.equal(i, ei) and torch.equal(s, es)
        assert torch.equal(ix._order, one._order) and torch.equal(ix._rows, one._rows)


def test_training_is_deterministic():
    d, N, M = 64, 3000, 64
    D, Q = _unit(N, d, 8), _unit(M, d, 9)
    a, b = _ivf(D, 20, seed=3), _ivf(D, 20, seed=3)
    assert torch.equal(a.centroids, b.centroids) and torch.equal(a.list_sizes, b.list_sizes)
    ra, rb = a.search(Q, 30, 5), b.search(Q, 30, 5)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    r2 = a.search(Q, 30, 5)
    assert torch.equal(ra[0], r2[0]) and torch.equal(ra[1], r2[1])


def test_query_batching_by_a_small_workspace():
    d, N, M, nlist, k, nprobe = 64, 3000, 700, 16, 20, 4
    D, Q = _unit(N, d, 10), _unit(M, d, 11)
    big = _ivf(D, nlist)
    flat = _flat(D)
    exclude, below = _filters(flat, Q, k, N, 0)
    es, ei = big.search(Q, k, nprobe, exclude=exclude, below=below)
    assert big.batch_queries(M, k, nprobe) == M
    for ws in (1 << 20, 1 << 17, 1):
        small = _ivf(D, nlist, centroids=big.centroids, workspace_bytes=ws)
        mq = small.batch_queries(M, k, nprobe)
        assert mq < M and (mq % 128 == 0 or mq < 128)
        if ws == 1:
            assert mq == 1
            s, i = small.search(Q[:9], k, nprobe, exclude=exclude[:9], below=below[:9])
            assert torch.equal(i, ei[:9]) and torch.equal(s, es[:9])
        else:
            s, i = small.search(Q, k, nprobe, exclude=exclude, below=below)
            assert torch.equal(i, ei) and torch.equal(s, es)


def test_own_list_is_the_first_probe():
    d, N, nlist = 128, 4000, 33
    D = torch.cat([_unit(N - 500, d, 12), _grid(500, d, 13)])       # grid rows: exact ties between centroids' scores
    C = torch.cat([_unit(nlist - 3, d, 14), _grid(3, d, 15)])
    C[5] = C[2]                                                      # a duplicated centroid: ties go to the lower list
    ivf = _ivf(D, nlist, centroids=C)
    ivf.list_sizes
    labels = torch.empty(N, dtype=torch.int64, device=DEV)
    labels[ivf._order] = ivf._labels.long()
    first = ivf._coarse.search(D.to(torch.bfloat16), 1)[1][:, 0]
    assert torch.equal(labels, first)
    assert int(ivf.list_sizes[5]) == 0
    # and so one probe searches the row's own list: the best of that list scores at least what the row scores with itself
    s, i = ivf.search(D[:300], 1, 1)
    own = _flat(D).rank(D[:300], torch.arange(300))[1]
    assert bool((s[:, 0] >= own).all()) and torch.equal(labels[i[:, 0]], labels[:300])


# ---- the tools -------------------------------------------------------------------------------------------------------
def _tool(name, *args):
    r = subprocess.run([sys.executable, "-m", f"contrastors_amd.tools.{name}", *args], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def test_tools_with_ivf_write_the_fixture_shards(tmp_path):
    fx = json.loads((GOLD / "search_curation.json").read_text())
    ivf = ("--ivf_lists", "4", "--ivf_nprobe", "4")
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
    # the centroids from a file: four rows of the documents
    np.save(tmp_path / "c.npy", np.asarray(t["d"], np.float32)[:4])
    for name, extra in (("tk", ()), ("tkc", ("--ivf_centroids", str(tmp_path / "c.npy")))):
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
