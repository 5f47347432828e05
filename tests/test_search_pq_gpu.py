"""GPU checks of the product-quantised search (cx_search_pq_topk in csrc/search.hip via contrastors_amd.search).  The kernel is
the bf16 tile kernel with its document panel gathered from the codebook, so PQFlatIndex.search must equal FlatIPIndex.search
over the decoded rows bit for bit: every comparison here is an equality of bits, with no tolerance anywhere."""
import functools
import gzip
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import pq_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
DEV = "cuda:0"
F32 = np.float32


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(got, want):
    """(scores, ids) pairs: equal shapes, dtypes and bits (+0 and -0 are told apart)."""
    for g, w in zip(got, want):
        g, w = _bits(g), _bits(w)
        assert g.shape == w.shape and g.dtype == w.dtype
        assert np.array_equal(g, w)


@functools.lru_cache(maxsize=None)
def _coded(N, d, dsub, seed):
    """Random codes and a random bf16 codebook (shared: the tests copy before they change one)."""
    rng = np.random.default_rng(seed)
    m = d // dsub
    shadow = R.to_bf16(rng.standard_normal((m, R.KSUB, dsub)).astype(F32))
    return rng.integers(0, 256, (N, m), dtype=np.uint8), shadow


def _pair(codes, shadow):
    """(the PQ index over the codes, the flat index over its decoded rows)."""
    from contrastors_amd.search import FlatIPIndex, PQFlatIndex

    m, _, dsub = shadow.shape
    ix = PQFlatIndex(m * dsub, dsub, device=DEV)
    ix.train(codebooks=shadow)
    ix.add(codes)
    flat = FlatIPIndex(m * dsub, device=DEV)
    flat.add(ix.decode())
    return ix, flat


def _queries(M, d, seed):
    return np.random.default_rng(seed).standard_normal((M, d)).astype(F32)


GRID = [(1, 1, 64, 8, 1), (127, 129, 192, 16, 10), (129, 127, 320, 32, 130), (300, 1000, 1024, 64, 1024), (1000, 300, 64, 8, 130),
        (1, 1000, 320, 8, 1024), (1000, 1, 192, 8, 1), (129, 300, 1024, 8, 10), (300, 129, 64, 16, 1024)]


@pytest.mark.parametrize("M, N, d, dsub, k", GRID)
def test_search_equals_the_flat_search_over_the_decoded_rows_for_every_split_count(M, N, d, dsub, k):
    codes, shadow = _coded(N, d, dsub, 2)
    ix, flat = _pair(codes, shadow)
    assert np.array_equal(_bits(flat.vectors.view(torch.int16)).view(np.uint16), R.bf16_bits(R.decode(codes, shadow)))
    Q = _queries(M, d, 1)
    want = flat.search(Q, k)
    for nsplit in (0, 1, 3, 7):
        got = ix.search(Q, k, nsplit=nsplit)
        assert isinstance(got[0], np.ndarray) and got[0].dtype == F32 and got[1].dtype == np.int64
        _assert_same(got, want)
    got = ix.search(torch.from_numpy(Q).to(DEV), k)
    assert isinstance(got[0], torch.Tensor) and got[0].is_cuda
    _assert_same(got, want)
    if N < k:
        assert np.isneginf(want[0][:, N:]).all() and (want[1][:, N:] == -1).all() and (want[1][:, :N] >= 0).all()   # padding


def test_exclusions_bounds_padding_and_empty_sides():
    d, dsub, N, M, k = 192, 8, 700, 150, 20
    codes, shadow = _coded(N, d, dsub, 3)
    ix, flat = _pair(codes, shadow)
    Q = _queries(M, d, 4)
    full = flat.search(Q, k)
    excl = [[int(full[1][m, 0]), int(full[1][m, 3])] if m % 3 else [] for m in range(M)]        # the top hit among them
    _assert_same(ix.search(Q, k, exclude=excl), flat.search(Q, k, exclude=excl))
    assert all(full[1][m, 0] not in ix.search(Q, k, exclude=excl)[1][m] for m in range(M) if m % 3)
    at = full[0][:, 2].copy()                                # at an attained score: strict, the third hit drops out
    above = np.nextafter(at, F32(np.inf), dtype=F32)
    under = np.nextafter(at, F32(-np.inf), dtype=F32)
    for bel in (at, above, under, np.full(M, -np.inf, F32)):
        got = ix.search(Q, k, below=bel)
        _assert_same(got, flat.search(Q, k, below=bel))
    assert (ix.search(Q, k, below=at)[1][:, 0] == full[1][:, 3]).all()
    assert (ix.search(Q, k, below=above)[1][:, 0] == full[1][:, 2]).all()
    _assert_same(ix.search(Q, k, exclude=excl, below=above, nsplit=5), flat.search(Q, k, exclude=excl, below=above))
    s, i = ix.search(Q, k, below=np.full(M, -np.inf, F32))
    assert np.isneginf(s).all() and (i == -1).all()
    # M = 0 and N = 0
    s, i = ix.search(np.zeros((0, d), F32), k)
    assert s.shape == (0, k) and i.shape == (0, k)
    ix.reset()
    flat.reset()
    s, i = ix.search(Q, k)
    assert np.isneginf(s).all() and (i == -1).all()
    _assert_same((s, i), flat.search(Q, k))


@pytest.mark.parametrize("code", [0, 255])
def test_all_codes_equal(code):
    d, dsub, N = 128, 16, 300
    _, shadow = _coded(N, d, dsub, 5)
    ix, flat = _pair(np.full((N, d // dsub), code, np.uint8), shadow)
    Q = _queries(70, d, 6)
    got = ix.search(Q, 10)
    _assert_same(got, flat.search(Q, 10))
    assert (got[1] == np.arange(10)[None, :]).all()          # every score ties: id order
    dec = R.decode(np.full((1, d // dsub), code, np.uint8), shadow)[0]
    assert np.array_equal(flat.vectors.float().cpu().numpy(), np.repeat(dec[None, :], N, axis=0))


def test_code_rows_with_a_leading_dimension_and_an_unaligned_base_give_the_same_result():
    """The index stores packed, aligned codes (one 16-byte copy per tile); any byte leading dimension >= m and any base address
    are legal at the C entry and take the byte path."""
    from contrastors_amd import _C

    d, dsub, N, M, k = 192, 16, 333, 40, 12
    m = d // dsub
    codes, shadow = _coded(N, d, dsub, 7)
    ix, flat = _pair(codes, shadow)
    Q = _queries(M, d, 8)
    want = flat.search(Q, k)
    lib = _C.lib()
    q = torch.from_numpy(Q).to(DEV).to(torch.bfloat16)
    ws = torch.empty(lib.cx_search_pq_ws_bytes(M, N, k, 0), dtype=torch.uint8, device=DEV)
    for ld, off in ((m, 0), (m, 1), (m + 4, 0), (m + 5, 3), (64, 16)):
        buf = torch.zeros(N * ld + 64, dtype=torch.uint8, device=DEV)
        view = buf[off: off + N * ld].view(N, ld)
        view[:, :m] = torch.from_numpy(codes).to(DEV)
        s = torch.empty(M, k, dtype=torch.float32, device=DEV)
        i = torch.empty(M, k, dtype=torch.int64, device=DEV)
        rc = lib.cx_search_pq_topk(q.data_ptr(), view.data_ptr(), ix.codebooks.data_ptr(), M, N, d, dsub, d, ld, k, None, None,
                                   None, 0, ws.data_ptr(), s.data_ptr(), i.data_ptr(), _C.cur_stream())
        torch.cuda.synchronize()
        assert rc == 0
        _assert_same((s, i), want)


def test_lane_map_every_codebook_entry_distinct_one_hot_queries_documents_differing_in_one_code():
    """Every (s, code, j) of the codebook decodes to its own bf16 value (finite, normal, both signs); a one-hot query at j reads
    column j of the decoded corpus exactly, so a piece gathered from the wrong centroid, sub-quantiser or offset, or landed in
    the wrong lane, changes a score."""
    d, dsub = 192, 8
    m = d // dsub
    pats = np.concatenate([np.arange(0x0080, 0x7F80), np.arange(0x8080, 0xFF80)]).astype(np.uint32)       # normal bf16 patterns
    pick = np.random.default_rng(9).permutation(pats.size)[: m * R.KSUB * dsub]
    shadow = (pats[pick] << 16).astype(np.uint32).view(F32).reshape(m, R.KSUB, dsub)
    assert np.unique(shadow).size == shadow.size and np.isfinite(shadow).all()
    rng = np.random.default_rng(10)
    base = rng.integers(0, 256, m, dtype=np.uint8)
    codes = np.repeat(base[None, :], 1 + 6 * m, axis=0)
    for n in range(1, codes.shape[0]):                       # document n differs from document 0 in one code only
        s = (n - 1) % m
        codes[n, s] = (int(base[s]) + 1 + 40 * ((n - 1) // m)) % 256
    N = codes.shape[0]
    ix, flat = _pair(codes, shadow)
    dec = R.decode(codes, shadow)
    Q = np.eye(d, dtype=F32)                                 # one-hot at every j
    got = ix.search(Q, N)
    _assert_same(got, flat.search(Q, N))
    for j in range(d):
        order = np.argsort(-dec[:, j], kind="stable")
        assert np.array_equal(got[1][j], order) and np.array_equal(got[0][j].view(np.uint32), dec[order, j].view(np.uint32))
    for j in (0, 7, 8, 63, 64, 100, 191):
        one = ix.search(Q[j: j + 1], N)                      # M = 1
        _assert_same(one, (got[0][j: j + 1], got[1][j: j + 1]))
        rep = ix.search(np.repeat(Q[j: j + 1], 129, axis=0), N)                  # ... and replicated to 129 rows
        _assert_same(rep, (np.repeat(got[0][j: j + 1], 129, axis=0), np.repeat(got[1][j: j + 1], 129, axis=0)))


# ---- the two-stage search ------------------------------------------------------------------------------------------------
def _exact_rows(n, d, seed):
    """Rows whose bf16 rounding and fp32 dot products are exact: multiples of 1 / 8 in [-1, 1]."""
    return (np.random.default_rng(seed).integers(-8, 9, (n, d)) / 8).astype(F32)


@pytest.mark.parametrize("N", [300, 1000])
def test_rescored_search_covering_the_corpus_equals_the_exact_search_bit_for_bit(N, tmp_path):
    from contrastors_amd.search import FlatIPIndex, PQFlatIndex, search_pq_rescored

    d, M, k = 128, 40, 10
    rng = np.random.default_rng(N)
    D = rng.standard_normal((N, d)).astype(F32)
    D[50] = D[7]                                             # a tie in the exact score
    Q = rng.standard_normal((M, d)).astype(F32)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    ix = PQFlatIndex(d, 8, device=DEV)
    ix.train(D, max_iter=2)
    ix.add(D)
    full = flat.search(Q, k)
    excl = [[int(full[1][m, 0])] if m % 2 else [] for m in range(M)]
    below = full[0][:, 1].copy()
    np.save(tmp_path / "D.npy", D)
    sources = {"device": flat.vectors, "host": D, "memmap": np.load(tmp_path / "D.npy", mmap_mode="r")}
    factor = -(-N // k)
    for name, vectors in sources.items():
        for ex, bel in ((None, None), (excl, None), (None, below), (excl, below)):
            got = search_pq_rescored(ix, vectors, Q, k, factor, exclude=ex, below=bel)
            assert isinstance(got[0], np.ndarray)
            _assert_same(got, flat.search(Q, k, exclude=ex, below=bel))
    got = search_pq_rescored(ix, flat.vectors, torch.from_numpy(Q).to(DEV), k, factor)
    assert isinstance(got[0], torch.Tensor) and got[0].is_cuda
    _assert_same(got, full)


@functools.lru_cache(maxsize=None)
def _exact_codebook(d, dsub, seed):
    return (np.random.default_rng(seed).integers(-8, 9, (d // dsub, R.KSUB, dsub)) / 8).astype(F32)


def test_rescored_search_with_partial_candidates_equals_the_reference_pipeline():
    from contrastors_amd.search import PQFlatIndex, search_pq_rescored

    d, N, M, k = 64, 600, 20, 10
    D, Q, shadow = _exact_rows(N, d, 21), _exact_rows(M, d, 22), _exact_codebook(d, 8, 25)
    ix = PQFlatIndex(d, 8, device=DEV)
    ix.train(codebooks=shadow)
    ix.add(D)
    assert np.array_equal(ix.codes.cpu().numpy(), R.assign(D, shadow))
    excl = [[m, m + 1] for m in range(M)]
    below = np.full(M, 3.0, F32)
    for factor, ex, bel in ((1, None, None), (4, excl, None), (3, excl, below)):
        ws, wi = R.pipeline(Q, D, shadow, k, factor, exclude=ex, below=bel)
        s, i = search_pq_rescored(ix, D, Q, k, factor, exclude=ex, below=bel)
        assert np.array_equal(i, wi) and np.array_equal(s.astype(np.float64), ws) and s.dtype == F32
    s4, i4 = search_pq_rescored(ix, D, Q, k, exclude=excl)  # the default factor is 4
    assert np.array_equal(i4, R.pipeline(Q, D, shadow, k, 4, exclude=excl)[1])


def test_candidate_lists_longer_than_1024_are_fetched_in_pages():
    from contrastors_amd.search import PQFlatIndex, search_pq_rescored

    d, N, M, k = 64, 5000, 5, 300
    D, Q, shadow = _exact_rows(N, d, 23), _exact_rows(M, d, 24), _exact_codebook(d, 8, 25)
    ix = PQFlatIndex(d, 8, device=DEV)
    ix.train(codebooks=shadow)
    ix.add(D)
    excl = [[int(x) for x in range(m, 40, 5)] for m in range(M)]
    ws, wi = R.pipeline(Q, D, shadow, k, 4, exclude=excl)    # 1200 candidates: two pages
    s, i = search_pq_rescored(ix, torch.from_numpy(D).to(DEV).to(torch.bfloat16), Q, k, 4, exclude=excl)
    assert np.array_equal(i, wi) and np.array_equal(s.astype(np.float64), ws)


# ---- the tools -----------------------------------------------------------------------------------------------------------
def _shards(path):
    got = []
    for p in sorted(Path(path).glob("shard-*.jsonl.gz")):
        with gzip.open(p, "rt") as f:
            got += [json.loads(line) for line in f]
    return got


def test_tools_with_pq_codes_write_what_the_default_run_writes(tmp_path):
    from contrastors_amd.tools import consistency_filter, mine_negatives

    fx = json.loads((GOLD / "search_curation.json").read_text())
    c, t = fx["consistency"], fx["topk"]
    np.save(tmp_path / "cq.npy", np.asarray(c["q"], F32))
    np.save(tmp_path / "cd.npy", np.asarray(c["d"], F32))
    (tmp_path / "ids.json").write_text(json.dumps(c["ids"]))
    with open(tmp_path / "recs.jsonl", "w") as f:
        for r in t["records"]:
            f.write(json.dumps(r) + "\n")
    np.save(tmp_path / "tq.npy", np.asarray(t["q"], F32))
    np.save(tmp_path / "td.npy", np.asarray(t["d"], F32))
    flags = {}
    for name, docs in (("c", np.asarray(c["d"], F32)), ("t", np.asarray(t["d"], F32))):
        pq = ["--pq_dsub", "8", "--rescore_factor", "32"]    # 2 * 32 >= 40 pairs, 10 * 32 >= 9 documents: covering
        if docs.shape[0] < 256:                              # too few rows to fit 256 centroids: codebooks from a file
            table = np.random.default_rng(docs.shape[1]).standard_normal((docs.shape[1] // 8, 256, 8)).astype(F32)
            np.save(tmp_path / f"cb_{name}.npy", table * F32(np.abs(docs).mean()))
            pq += ["--pq_codebooks", str(tmp_path / f"cb_{name}.npy")]
        flags[name] = pq
    kept, mined = {}, {}
    for name in ("default", "pq"):
        assert consistency_filter.main(["--output_dir", str(tmp_path / f"cf_{name}"), "--query_embeddings",
                                        str(tmp_path / "cq.npy"), "--document_embeddings", str(tmp_path / "cd.npy"), "--ids",
                                        str(tmp_path / "ids.json"), "--device", DEV,
                                        *(flags["c"] if name == "pq" else [])]) == 0
        kept[name] = (tmp_path / f"cf_{name}" / "ids_to_keep_0.json").read_bytes()
        assert mine_negatives.main(["--rule", "topk", "--dataset", str(tmp_path / "recs.jsonl"), "--output_dir",
                                    str(tmp_path / f"tk_{name}"), "--k", str(t["k"]), "--seed", str(t["seed"]),
                                    "--query_embeddings", str(tmp_path / "tq.npy"), "--document_embeddings",
                                    str(tmp_path / "td.npy"), "--device", DEV, *(flags["t"] if name == "pq" else [])]) == 0
        mined[name] = _shards(tmp_path / f"tk_{name}")
    assert kept["pq"] == kept["default"] and json.loads(kept["default"]) == c["kept"]
    assert mined["pq"] == mined["default"] and len(mined["default"]) == len(t["expected"])
