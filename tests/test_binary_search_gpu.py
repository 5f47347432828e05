"""GPU checks of the binary index (csrc/search_binary.hip via contrastors_amd.search): sign packing against numpy.packbits,
the Hamming top-k against numpy XOR + popcount ordered by (distance, id), ties across corpus splits, exclusions, the
inclusive distance bound, padding, determinism, the operand lane map, exact re-scoring against float64 and -- bit for bit --
against FlatIPIndex, the two-stage search against the exact one, and the curation tools with --coarse binary.
Every expectation is exact equality."""
import functools
import gzip
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
DEV = "cuda:0"
INT32_MAX = 2 ** 31 - 1


# ---- reference: XOR + popcount, then (distance, id) ------------------------------------------------------------------
def _popcount64(x):
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x)
    lut = np.array([bin(i).count("1") for i in range(256)], np.uint8)
    return lut[x.view(np.uint8)].reshape(*x.shape, 8).sum(-1)


def hamming_matrix(qc, dc):
    """(M, N) int32 distances of packed uint8 codes (d / 8 is a multiple of 8)."""
    q64, d64 = np.ascontiguousarray(qc).view(np.uint64), np.ascontiguousarray(dc).view(np.uint64)
    out = np.empty((q64.shape[0], d64.shape[0]), np.int32)
    for r in range(q64.shape[0]):
        out[r] = _popcount64(d64 ^ q64[r]).sum(1)
    return out


def ref_topk(dist, k, exclude=None, max_dist=None):
    """Top-k of the strict order (distance, id) among the admissible columns; padded with (INT32_MAX, -1)."""
    M, N = dist.shape
    od = np.full((M, k), INT32_MAX, np.int32)
    oi = np.full((M, k), -1, np.int64)
    ids = np.arange(N)
    for r in range(M):
        ok = np.ones(N, bool)
        if exclude is not None:
            ok[list(exclude[r])] = False
        if max_dist is not None:
            ok &= dist[r] <= max_dist[r]
        cols = ids[ok]
        if len(cols) > 4 * k:                                   # only columns up to the k-th distance can be in the top-k
            cols = cols[dist[r, cols] <= np.partition(dist[r, cols], k - 1)[k - 1]]
        order = np.lexsort((cols, dist[r, cols]))[:k]
        od[r, : len(order)] = dist[r, cols[order]]
        oi[r, : len(order)] = cols[order]
    return od, oi


def _codes(n, d, seed, spread=None):
    """Random codes; with `spread`, rows are a few bit flips away from a handful of centres, so distances span a wide range
    (and tie) instead of concentrating around d / 2."""
    rng = np.random.default_rng(seed)
    if spread is None:
        return rng.integers(0, 256, (n, d // 8), dtype=np.uint8)
    centres = rng.integers(0, 2, (spread, d), dtype=np.uint8)
    bits = centres[rng.integers(0, spread, n)]
    flips = rng.random((n, d), dtype=np.float32) < rng.random((n, 1), dtype=np.float32) * 0.3
    return np.packbits(bits ^ flips, axis=1)


def _index(dc, d):
    from contrastors_amd.search import BinaryFlatIndex

    ix = BinaryFlatIndex(d, device=DEV)
    ix.add(dc)
    return ix


# ---- packing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("d", [64, 192, 768, 1024])
def test_pack_sign_bits_equals_numpy_packbits(d, rows, dtype):
    from contrastors_amd.search import pack_sign_bits

    x = np.random.default_rng(d + rows).standard_normal((rows, d + 16)).astype(np.float32)
    x[0, :6] = [0.0, -0.0, np.nan, -np.nan, 1e-30, -1e-30]
    x[-1, d - 3: d] = [np.nan, -0.0, 2.0]
    wide = torch.from_numpy(x).to(DEV).to(dtype)
    want = np.packbits(wide[:, :d].float().cpu().numpy() > 0, axis=1)
    view = wide[:, :d]                                      # leading dimension d + 16
    assert view.stride(0) == d + 16
    got = pack_sign_bits(view)
    assert got.dtype == torch.uint8 and got.shape == (rows, d // 8) and got.device == wide.device
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(pack_sign_bits(view.contiguous()).cpu().numpy(), want)
    assert np.array_equal(pack_sign_bits(view.cpu()).numpy(), want)        # the host path gives the same bytes


# ---- the search grid -------------------------------------------------------------------------------------------------
GRID_M = (1, 129, 300)
GRID_K = (1, 100, 1024)


@functools.lru_cache(maxsize=None)
def _grid_case(N, d):
    qc = _codes(max(GRID_M), d, 7 * d + 1, spread=5)
    dc = _codes(N, d, 7 * d + N, spread=5) if N > 1 else _codes(1, d, N)
    return qc, dc, hamming_matrix(qc, dc)


@pytest.mark.parametrize("d", [64, 192, 768, 1024])
@pytest.mark.parametrize("N", [1, 127, 129, 257, 70_001])
def test_hamming_search_grid(N, d):
    """A lone row and document, the tile edges at 128, K padding (d = 64, 192: half of the last 128-bit chunk) and, at
    N = 70 001, 64 corpus splits.  One distance matrix per (N, d): the queries of a smaller M are its first rows."""
    qc, dc, dist = _grid_case(N, d)
    ix = _index(dc, d)
    assert ix.ntotal == N and ix.codes.shape == (N, d // 8)
    rd, ri = ref_topk(dist, max(GRID_K))
    for M in GRID_M:
        for k in GRID_K:
            gd, gi = ix.search(torch.from_numpy(qc[:M]).to(DEV), k)
            assert gd.dtype == torch.int32 and gi.dtype == torch.int64 and gd.shape == (M, k)
            assert np.array_equal(gi.cpu().numpy(), ri[:M, :k]), (M, N, d, k)
            assert np.array_equal(gd.cpu().numpy(), rd[:M, :k]), (M, N, d, k)


def test_float_rows_and_numpy_in_numpy_out():
    d, N, M = 192, 300, 9
    rng = np.random.default_rng(3)
    D, Q = rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((M, d)).astype(np.float32)
    ix = _index(D, d)                                                        # float rows are binarised by sign
    assert np.array_equal(ix.codes.cpu().numpy(), np.packbits(D > 0, axis=1))
    rd, ri = ref_topk(hamming_matrix(np.packbits(Q > 0, axis=1), np.packbits(D > 0, axis=1)), 10)
    gd, gi = ix.search(Q, 10)
    assert isinstance(gd, np.ndarray) and np.array_equal(gd, rd) and np.array_equal(gi, ri)
    gd2, gi2 = ix.search(np.packbits(Q > 0, axis=1), 10)                     # codes as queries
    assert np.array_equal(gd2, rd) and np.array_equal(gi2, ri)
    ix.reserve(1000)
    ix.add(D[:5])
    assert ix.ntotal == N + 5 and np.array_equal(ix.codes[N:].cpu().numpy(), np.packbits(D[:5] > 0, axis=1))
    ix.reset()
    assert ix.ntotal == 0 and ix.codes.shape == (0, d // 8)
    gd, gi = ix.search(Q, 3)                                                 # an empty index: all padding
    assert (gd == INT32_MAX).all() and (gi == -1).all()


def test_ties_do_not_depend_on_the_split_count():
    """8 distinct codes repeated to N = 1000: every distance is shared by ~125 documents, so the k-th entry of every list
    sits inside a run of ties and the tile / split boundaries cut through such runs."""
    d, N, M, k = 128, 1000, 130, 300
    base = _codes(8, d, 11)
    dc = base[np.arange(N) % 8]
    qc = np.concatenate([base, _codes(M - 8, d, 12)])
    rd, ri = ref_topk(hamming_matrix(qc, dc), k)
    ix = _index(dc, d)
    q = torch.from_numpy(qc).to(DEV)
    for nsplit in (1, 3, 7):
        gd, gi = ix.search(q, k, nsplit=nsplit)
        assert np.array_equal(gi.cpu().numpy(), ri), nsplit
        assert np.array_equal(gd.cpu().numpy(), rd), nsplit


def test_exclusions_and_the_inclusive_distance_bound():
    d, N, M, k = 256, 2000, 140, 50
    qc, dc = _codes(M, d, 21, spread=4), _codes(N, d, 22, spread=4)
    dist = hamming_matrix(qc, dc)
    _, nearest = ref_topk(dist, 3)
    rng = np.random.default_rng(23)
    exclude = [sorted({int(nearest[r, 0]), int(nearest[r, 2]), *rng.integers(0, N, r % 5).tolist()}) for r in range(M)]
    exclude[7] = []
    # the bound sits ON a distance that occurs, so "inclusive" decides whether those documents are returned
    max_dist = np.array([np.sort(dist[r])[(r * 13) % 200] for r in range(M)], np.int32)
    max_dist[3], max_dist[4], max_dist[5] = -1, 0, d
    ix = _index(dc, d)
    q = torch.from_numpy(qc).to(DEV)
    for ex, md in ((exclude, None), (None, max_dist), (exclude, max_dist)):
        rd, ri = ref_topk(dist, k, ex, md)
        gd, gi = ix.search(q, k, exclude=ex, max_dist=md)
        gd, gi = gd.cpu().numpy(), gi.cpu().numpy()
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd)
        if ex is not None:
            for r in range(M):
                assert not set(ex[r]) & set(gi[r].tolist())
        if md is not None:
            assert (gd[gi >= 0] <= np.broadcast_to(md[:, None], gd.shape)[gi >= 0]).all()
            assert (gi[3] == -1).all()
            assert any((gd[r] == md[r]).any() for r in range(M))         # entries AT the bound are returned
    # the CSR form gives the same result
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in exclude])])
    flat = np.asarray([i for e in exclude for i in e], np.int64)
    rd, ri = ref_topk(dist, k, exclude)
    gd, gi = ix.search(q, k, exclude=(ptr, flat), nsplit=5)
    assert np.array_equal(gi.cpu().numpy(), ri) and np.array_equal(gd.cpu().numpy(), rd)


def test_padding_when_k_exceeds_the_corpus():
    d, N, M, k = 64, 37, 5, 64
    qc, dc = _codes(M, d, 31), _codes(N, d, 32)
    rd, ri = ref_topk(hamming_matrix(qc, dc), k)
    gd, gi = _index(dc, d).search(qc, k)
    assert np.array_equal(gd, rd) and np.array_equal(gi, ri)
    assert (gd[:, N:] == INT32_MAX).all() and (gi[:, N:] == -1).all() and (gi[:, :N] >= 0).all()


def test_two_runs_are_bit_identical():
    d, N, M, k = 768, 30_000, 200, 100
    qc, dc = _codes(M, d, 41, spread=6), _codes(N, d, 42, spread=6)
    ix = _index(dc, d)
    q = torch.from_numpy(qc).to(DEV)
    a = ix.search(q, k)
    b = ix.search(q, k)
    c = ix.search(q, k, nsplit=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize("d", [192, 768])
def test_operand_lane_map_with_single_bits_against_asymmetric_codes(d):
    """Query i has only bit i set; document j has exactly the bits below j set (and a second block has every (7 j)-th bit
    cleared).  The distance of (i, j) then depends on whether bit i is among document j's: a K position that the query and
    the document operand disagree on, a transposed operand or a permuted result row shows as a wrong distance."""
    eye = np.eye(d, dtype=np.uint8)
    prefix = (np.arange(d)[None, :] < np.arange(d + 1)[:, None]).astype(np.uint8)        # (d + 1, d)
    comb = np.ones((64, d), np.uint8)
    for j in range(64):
        comb[j, (7 * j) % d:: j + 2] = 0
    docs = np.concatenate([prefix, comb])
    qc, dc = np.packbits(eye, axis=1), np.packbits(docs, axis=1)
    want = (docs.sum(1)[None, :] + 1 - 2 * docs.T.astype(np.int64)).astype(np.int32)     # from the bits themselves
    dist = hamming_matrix(qc, dc)
    assert np.array_equal(dist, want)
    k = min(1024, len(docs))
    rd, ri = ref_topk(dist, k)
    gd, gi = _index(dc, d).search(qc, k)
    assert np.array_equal(gd, rd) and np.array_equal(gi, ri)
    # and with the roles swapped: single-bit documents, asymmetric queries
    rd, ri = ref_topk(dist.T.copy(), 100)
    gd, gi = _index(qc, d).search(dc, 100)
    assert np.array_equal(gd, rd) and np.array_equal(gi, ri)


# ---- re-scoring ------------------------------------------------------------------------------------------------------
def _ref_rescore(Q, D, cand, k, below=None):
    """float64 scores, (score descending, id ascending), -1 skipped, padded with (-inf, -1)."""
    M = cand.shape[0]
    os_ = np.full((M, k), -np.inf, np.float64)
    oi = np.full((M, k), -1, np.int64)
    for r in range(M):
        ids = cand[r][cand[r] >= 0]
        s = D[ids].astype(np.float64) @ Q[r].astype(np.float64)
        if below is not None:
            ids, s = ids[s < below[r]], s[s < below[r]]
        order = np.lexsort((ids, -s))[:k]
        os_[r, : len(order)] = s[order]
        oi[r, : len(order)] = ids[order]
    return os_, oi


@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("c", [1, 17, 512])
def test_rescore_against_float64_on_exact_data(c, d, tmp_path):
    """Integer-valued data in {-2 .. 2}: every accumulation order is exact in fp32, so scores AND order must equal the float64
    reference; scores tie often, so the id order is exercised."""
    from contrastors_amd.search import rescore

    M, R = 70, 1000
    rng = np.random.default_rng(100 * c + d)
    Q = rng.integers(-2, 3, (M, d)).astype(np.float32)
    D = rng.integers(-2, 3, (R, d)).astype(np.float32)
    cand = np.stack([rng.permutation(R)[:c] for _ in range(M)]).astype(np.int64)
    cand[rng.random((M, c)) < 0.1] = -1                                      # skipped entries
    cand[5] = -1
    for k in sorted({1, min(c, 100), c}):
        ws, wi = _ref_rescore(Q, D, cand, k)
        for vectors in (torch.from_numpy(D).to(DEV).to(torch.bfloat16), torch.from_numpy(D), D):
            s, i = rescore(torch.from_numpy(Q).to(DEV), torch.from_numpy(cand).to(DEV), vectors, k)
            assert s.dtype == torch.float32 and i.dtype == torch.int64
            assert np.array_equal(i.cpu().numpy(), wi), (c, d, k, type(vectors))
            assert np.array_equal(s.cpu().numpy().astype(np.float64), ws), (c, d, k, type(vectors))
    np.save(tmp_path / "D.npy", D)
    below = np.median(_ref_rescore(Q, D, cand, c)[0], axis=1) if c > 1 else np.full(M, 0.0)
    below[~np.isfinite(below)] = 0.0
    k = min(c, 100)
    ws, wi = _ref_rescore(Q, D, cand, k, below)
    s, i = rescore(Q, cand, np.load(tmp_path / "D.npy", mmap_mode="r"), k, below=below)          # numpy in, numpy out
    assert isinstance(s, np.ndarray) and np.array_equal(i, wi) and np.array_equal(s.astype(np.float64), ws)


@pytest.mark.parametrize("d", [64, 768])
def test_rescore_scores_are_bitwise_those_of_the_exact_search(d):
    from contrastors_amd.search import FlatIPIndex, rescore

    M, N, c = 70, 1000, 512
    g = torch.Generator(device=DEV).manual_seed(d)
    D = torch.nn.functional.normalize(torch.randn(N, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
    Q = torch.nn.functional.normalize(torch.randn(M, d, device=DEV, generator=g), dim=1).to(torch.bfloat16)
    ix = FlatIPIndex(d, device=DEV)
    ix.add(D)
    fs, fi = ix.search(Q, N)                                # N <= 1024: the exact search's score of EVERY pair
    table = torch.empty(M, N, dtype=torch.float32, device=DEV).scatter_(1, fi, fs)
    rng = np.random.default_rng(d)
    cand = torch.from_numpy(np.stack([rng.permutation(N)[:c] for _ in range(M)])).to(DEV)
    s, i = rescore(Q, cand, D, c)
    assert (i >= 0).all()
    assert torch.equal(s.view(torch.int32), table.gather(1, i).view(torch.int32))
    assert torch.equal(torch.sort(i, 1).values, torch.sort(cand, 1).values)
    # the exact search's own top-k, shuffled, comes back as it was
    k = 50
    shuffled = fi[:, :k][:, torch.from_numpy(rng.permutation(k)).to(DEV)]
    s, i = rescore(Q, shuffled, D.cpu(), k)
    assert torch.equal(i, fi[:, :k]) and torch.equal(s.view(torch.int32), fs[:, :k].contiguous().view(torch.int32))


# ---- coarse + exact --------------------------------------------------------------------------------------------------
def test_binary_search_with_full_rescoring_equals_the_exact_search(tmp_path):
    from contrastors_amd.search import BinaryFlatIndex, FlatIPIndex, search_binary_rescored

    N, M, d, k, factor = 3000, 200, 256, 20, 150            # k * factor = N: the candidates cover the corpus (3 pages)
    rng = np.random.default_rng(5)
    D = rng.standard_normal((N, d)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    Q = rng.standard_normal((M, d)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    binary = BinaryFlatIndex(d, device=DEV)
    binary.add(D)
    es, ei = flat.search(Q, k)
    exclude = [[int(ei[r, 0]), int(ei[r, 3])] + rng.integers(0, N, r % 4).tolist() for r in range(M)]
    below = es[:, k // 2].copy()                            # cuts into every row's top-k
    np.save(tmp_path / "D.npy", D)
    sources = {"device": flat.vectors, "memmap": np.load(tmp_path / "D.npy", mmap_mode="r")}
    for ex, bel in ((None, None), (exclude, None), (None, below), (exclude, below)):
        es, ei = flat.search(Q, k, exclude=ex, below=bel)
        for name, vectors in sources.items():
            s, i = search_binary_rescored(binary, vectors, Q, k, factor, exclude=ex, below=bel)
            assert isinstance(s, np.ndarray)
            assert np.array_equal(i, ei), (name, ex is not None, bel is not None)
            assert np.array_equal(s.view(np.int32), es.view(np.int32)), (name, ex is not None, bel is not None)
    # a short candidate list is a subset of the corpus: every returned pair still carries the exact search's score
    s, i = search_binary_rescored(binary, flat.vectors, torch.from_numpy(Q).to(DEV), k, 4)
    full_s, full_i = flat.search(torch.from_numpy(Q).to(DEV), 1024)
    for r in range(0, M, 17):
        where = {int(a): b for a, b in zip(full_i[r].tolist(), full_s[r].tolist())}
        for a, b in zip(i[r].tolist(), s[r].tolist()):
            assert a not in where or where[a] == b


# ---- the tools -------------------------------------------------------------------------------------------------------
def _tool(name, *args):
    r = subprocess.run([sys.executable, "-m", f"contrastors_amd.tools.{name}", *args], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def test_tools_with_binary_coarse_search_write_the_fixture_shards(tmp_path):
    fx = json.loads((GOLD / "search_curation.json").read_text())
    coarse = ("--coarse", "binary", "--rescore_factor", "32")          # 2 * 32 >= 40 pairs, 10 * 32 >= 9 documents
    c = fx["consistency"]
    np.save(tmp_path / "cq.npy", np.asarray(c["q"], np.float32))
    np.save(tmp_path / "cd.npy", np.asarray(c["d"], np.float32))
    (tmp_path / "ids.json").write_text(json.dumps(c["ids"]))
    _tool("consistency_filter", "--output_dir", str(tmp_path / "cf"), "--query_embeddings", str(tmp_path / "cq.npy"),
          "--document_embeddings", str(tmp_path / "cd.npy"), "--ids", str(tmp_path / "ids.json"), *coarse)
    assert json.loads((tmp_path / "cf" / "ids_to_keep_0.json").read_text()) == c["kept"]
    t = fx["topk"]
    with open(tmp_path / "recs.jsonl", "w") as f:
        for r in t["records"]:
            f.write(json.dumps(r) + "\n")
    np.save(tmp_path / "tq.npy", np.asarray(t["q"], np.float32))
    np.save(tmp_path / "td.npy", np.asarray(t["d"], np.float32))
    _tool("mine_negatives", "--rule", "topk", "--dataset", str(tmp_path / "recs.jsonl"), "--output_dir",
          str(tmp_path / "tk"), "--k", str(t["k"]), "--seed", str(t["seed"]), "--query_embeddings", str(tmp_path / "tq.npy"),
          "--document_embeddings", str(tmp_path / "td.npy"), *coarse)
    got = []
    for p in sorted((tmp_path / "tk").glob("shard-*.jsonl.gz")):
        with gzip.open(p, "rt") as f:
            got += [json.loads(line) for line in f]
    for g in got:
        assert g.pop("metadata")["objective"]["triplet"] == [["question", "positive_ctxs", "hard_negative_ctxs"]]
    assert got == t["expected"]
