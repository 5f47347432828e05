"""GPU checks of the int8 scalar-quantised index (csrc/quantize_int8.hip, csrc/search.hip via contrastors_amd.search) against
the numpy reference tests/int8_ref.py.  Every output of the new kernels is defined bit for bit by that reference (an exact
integer dot product, then two fp32 multiplications), so every comparison here is an equality of bits."""
import functools
import gzip
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import int8_ref as R

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


def _index(dc, ds, d):
    from contrastors_amd.search import Int8FlatIndex

    ix = Int8FlatIndex(d, device=DEV)
    ix.add((dc, ds))
    return ix


@functools.lru_cache(maxsize=None)
def _coded(n, d, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(-127, 128, (n, d), dtype=np.int8)
    s = rng.uniform(1e-3, 3e-2, n).astype(F32)
    return c, s                                              # (shared: the tests copy before they change one)


# ---- the quantiser -----------------------------------------------------------------------------------------------------
def _float_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(F32) * rng.uniform(1e-3, 50, (n, 1)).astype(F32)
    if n >= 8:
        x[0] = 0                                            # a zero row
        x[1] = F32(2.0 ** -101)                             # amax below 2^-100
        x[2] = F32(2.0 ** -100)                             # at the bound: quantised
        x[3, d // 2] = -1e4                                 # the amax element negative
        x[4, -1] = 2e4                                      # the amax element last
        x[5, :] = 0
        x[5, :32] = (np.arange(32, dtype=F32) + F32(0.5)) / 32        # inv = 32: k + 0.5 for even and odd k
        x[5, 32:64] = -(np.arange(95, 127, dtype=F32) + F32(0.5)) / 32
        x[5, -1] = -127 / 32 if d > 64 else x[5, -1]
        x[6] = x[5]
        x[6, 40] = 127 / 32                                 # (d = 64: the amax element inside the row)
        x[7, 0] = -x[7, 0]
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [0, 1, 63, 65, 300])
@pytest.mark.parametrize("d", [64, 192, 1024])
def test_quantize_rows_int8_equals_the_reference(d, n, dtype):
    from contrastors_amd.search import quantize_rows_int8

    x = torch.from_numpy(_float_rows(n, d, 100 * d + n)).to(dtype)
    wc, ws = R.quantize(x.float().numpy())
    if n >= 8 and dtype == torch.float32:
        assert not wc[0].any() and not wc[1].any() and ws[1] == 0 and (wc[2] == 127).all()
        assert wc[3, d // 2] == -127 and wc[4, -1] == 127 and wc[6, :4].tolist() == [0, 2, 2, 4]
    c, s = quantize_rows_int8(x.to(DEV))
    assert c.dtype == torch.int8 and c.shape == (n, d) and s.dtype == torch.float32 and s.shape == (n,) and c.is_cuda
    _assert_same((c, s), (wc, ws))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_rows_int8_honours_row_strides_and_unaligned_views(dtype):
    from contrastors_amd.search import quantize_rows_int8

    wide = torch.from_numpy(_float_rows(70, 256, 5)).to(dtype).to(DEV)
    for view in (wide[:, :192], wide[:, 64:128], wide[:, 1:65], wide[3:, 2:194]):          # the last two: element loads
        want = R.quantize(view.float().cpu().numpy())
        _assert_same(quantize_rows_int8(view), want)


def test_non_finite_rows_quantise_as_documented():
    """Unspecified by the contract beyond "no out-of-bounds access"; what the kernel does is documented, and held here."""
    from contrastors_amd.search import quantize_rows_int8

    x = np.ones((3, 192), F32)
    x[:, 1] = 0.5
    x[0, 3], x[1, 5], x[2, 7] = np.nan, np.inf, -np.inf
    c, s = (t.cpu().numpy() for t in quantize_rows_int8(torch.from_numpy(x).to(DEV)))
    assert s[0] == F32(1) / F32(127) and c[0, 3] == -127 and c[0, 0] == 127 and c[0, 1] == 64     # NaN skipped by the maximum
    for r, j in ((1, 5), (2, 7)):
        assert np.isposinf(s[r]) and c[r, j] == -127 and not np.delete(c[r], j).any()


# ---- the search against the reference ----------------------------------------------------------------------------------
GRID = [(1, 1, 64, 1), (127, 129, 192, 10), (129, 127, 320, 130), (300, 1000, 1024, 1024), (1000, 300, 64, 130),
        (1, 1000, 320, 1024), (1000, 1, 192, 1), (129, 300, 1024, 10), (300, 129, 64, 1024)]


@pytest.mark.parametrize("M, N, d, k", GRID)
def test_search_grid_equals_the_reference_for_every_split_count(M, N, d, k):
    qc, qs = _coded(M, d, 1)
    dc, ds = _coded(N, d, 2)
    want = R.search(qc, qs, dc, ds, k)
    ix = _index(dc, ds, d)
    for nsplit in (0, 1, 3, 7):
        got = ix.search((qc, qs), k, nsplit=nsplit)
        assert isinstance(got[0], np.ndarray) and got[0].dtype == F32 and got[1].dtype == np.int64
        _assert_same(got, want)
    got = ix.search((torch.from_numpy(qc).to(DEV), torch.from_numpy(qs).to(DEV)), k)       # torch in -> torch out
    assert isinstance(got[0], torch.Tensor) and got[0].is_cuda
    _assert_same(got, want)


@pytest.mark.parametrize("sign", [1, -1])
def test_saturated_rows_reach_the_largest_accumulator(sign):
    d = 1024
    qc = np.full((3, d), 127, np.int8)
    dc = np.full((140, d), sign * 127, np.int8)
    dc[1::2] = -dc[1::2]
    qs, ds = np.ones(3, F32), np.ones(140, F32)
    ds[5] = F32(0.3)
    want = R.search(qc, qs, dc, ds, 140)
    assert abs(float(want[0][0, 0])) == 16516096.0 and float(want[0][0, -1]) == -16516096.0
    _assert_same(_index(dc, ds, d).search((qc, qs), 140), want)


@pytest.mark.parametrize("d", [192, 320])
def test_operand_lane_map_with_single_codes_against_asymmetric_documents(d):
    """A query with one non-zero code at position j reads column j of the documents.  The documents' codes are an asymmetric
    function of (row, column) -- a prefix pattern and a comb whose period depends on the row -- with a distinct scale per row:
    a lane that feeds the wrong row, a K position paired with another on the other operand, or a result written to another
    (row, column) changes the ranking.  Every j of the second 128-chunk and j = d - 1 (d = 192: that chunk is the half-used
    one), with M = 1 and with the query replicated to 129 rows."""
    N = 300
    n, col = np.arange(N)[:, None], np.arange(d)[None, :]
    prefix = np.where(col <= (n * 7) % d, 1 + n % 100, -(1 + col % 90))
    comb = np.where(col % (2 + n % 5) == 0, 3 + col % 120, -(2 + n % 11))
    dc = np.where(n % 2 == 0, prefix, comb).astype(np.int8)
    ds = (F32(1) + np.arange(N, dtype=F32) / F32(512)).astype(F32)
    js = list(range(128, min(256, d))) + [d - 1] if d > 256 else list(range(64, 192))
    js = sorted(set(js) | {d - 1})
    qc = np.zeros((len(js), d), np.int8)
    qc[np.arange(len(js)), js] = (np.arange(len(js)) % 2 * 2 - 1) * (1 + np.arange(len(js)) % 127)
    qs = np.full(len(js), F32(0.25))
    want_s, want_i = R.search(qc, qs, dc, ds, N)
    assert len({tuple(r) for r in want_i.tolist()}) > len(js) // 2            # the rankings tell the columns apart
    ix = _index(dc, ds, d)
    for r in range(len(js)):
        _assert_same(ix.search((qc[r: r + 1], qs[r: r + 1]), N), (want_s[r: r + 1], want_i[r: r + 1]))
    rep = np.repeat(np.arange(len(js)), 129)
    _assert_same(ix.search((qc[rep], qs[rep]), N), (want_s[rep], want_i[rep]))


def test_ties_go_to_the_lower_id_across_tiles_and_splits():
    d = 64
    base_c, base_s = _coded(8, d, 3)
    rep = np.arange(1000) % 8
    dc, ds = base_c[rep], base_s[rep]
    qc, qs = _coded(5, d, 4)
    want = R.search(qc, qs, dc, ds, 300)
    assert (np.diff(want[0], axis=1) == 0).sum() > 5 * 250
    ix = _index(dc, ds, d)
    for nsplit in (0, 1, 3, 7):
        _assert_same(ix.search((qc, qs), 300, nsplit=nsplit), want)


def test_bounds_exclusions_padding_and_an_empty_index():
    from contrastors_amd.search import Int8FlatIndex

    d, M, N, k = 192, 130, 300, 10
    qc, qs = _coded(M, d, 5)
    dc, ds = _coded(N, d, 6)
    S = R.scores(qc, qs, dc, ds)
    ix = _index(dc, ds, d)
    third = np.sort(S, 1)[:, -3].copy()                      # an attained score: at, just above and just below it
    for below in (third, np.nextafter(third, F32(np.inf)), np.nextafter(third, F32(-np.inf))):
        _assert_same(ix.search((qc, qs), k, below=below), R.topk(S, k, None, below))
    excl = [[int(np.argmax(S[m]))] + [int(x) for x in np.argsort(-S[m])[3: 3 + m % 4]] for m in range(M)]
    want = R.topk(S, k, excl)
    assert all(want[1][m, 0] != excl[m][0] for m in range(M))
    _assert_same(ix.search((qc, qs), k, exclude=excl), want)
    _assert_same(ix.search((qc, qs), k, exclude=excl, below=third, nsplit=3), R.topk(S, k, excl, third))
    # fewer than k admissible documents: everything but a few ids excluded, and a bound below every score
    keep = [[int(x) for x in range(N) if x % 97 != m % 5] for m in range(M)]
    want = R.topk(S, k, keep)
    assert (want[1][:, 4:] == -1).all() and (want[1][:, :3] >= 0).all()
    _assert_same(ix.search((qc, qs), k, exclude=keep), want)
    low = np.full(M, -np.inf, F32)
    _assert_same(ix.search((qc, qs), k, below=low), R.topk(S, k, None, low))
    _assert_same(ix.search((qc, qs), 400), R.topk(S, 400))   # k > N
    empty = Int8FlatIndex(d, device=DEV)
    s, i = empty.search((qc, qs), 7)
    assert s.shape == (M, 7) and np.isneginf(s).all() and (i == -1).all()
    s, i = ix.search((qc[:0], qs[:0]), 7)
    assert s.shape == (0, 7) and i.shape == (0, 7)


def test_zero_scales_score_signed_zeros_and_tie_by_id():
    d = 64
    qc, qs = (a.copy() for a in _coded(6, d, 7))
    dc, ds = (a.copy() for a in _coded(200, d, 8))
    qs[1] = 0
    ds[::3] = 0
    want = R.search(qc, qs, dc, ds, 200)
    assert np.signbit(want[0][1]).any() and not np.signbit(want[0][1]).all()
    _assert_same(_index(dc, ds, d).search((qc, qs), 200), want)


def test_c_entry_refuses_misaligned_operands_and_bad_shapes():
    from contrastors_amd import _C

    lib = _C.lib()
    d, M, N, k = 64, 4, 8, 2
    q = torch.zeros(M * 2, 128, dtype=torch.int8, device=DEV)
    D = torch.zeros(N * 2, 128, dtype=torch.int8, device=DEV)
    qs, ds = torch.ones(M, device=DEV), torch.ones(N, device=DEV)
    ws = torch.empty(lib.cx_search_int8_ws_bytes(M, N, k, 0) + 16, dtype=torch.uint8, device=DEV)
    s = torch.empty(M, k, device=DEV)
    i = torch.empty(M, k, dtype=torch.int64, device=DEV)

    def call(qp=0, dp=0, ldq=128, ldd=128, d=d, k=k, wp=0, qsp=True):
        return lib.cx_search_int8_topk(q.data_ptr() + qp, D.data_ptr() + dp, qs.data_ptr() if qsp else None, ds.data_ptr(), M, N,
                                       d, ldq, ldd, k, None, None, None, 0, ws.data_ptr() + wp, s.data_ptr(), i.data_ptr(),
                                       _C.cur_stream())

    SHAPE, ALIGN, ARG = -1, -2, -3
    with torch.cuda.device(DEV):
        assert call() == 0
        assert call(qp=8) == ALIGN and call(dp=4) == ALIGN and call(wp=8) == ALIGN
        assert call(ldq=72) == ALIGN and call(ldd=136) == ALIGN and call(ldq=48) == ALIGN
        assert call(d=96) == SHAPE and call(k=1025) == SHAPE and call(k=0) == SHAPE
        assert call(qsp=False) == ARG
        x = torch.zeros(4, 64, device=DEV)
        c = torch.zeros(4, 80, dtype=torch.int8, device=DEV)
        sc = torch.zeros(4, device=DEV)
        quant = functools.partial(lib.cx_quantize_rows_int8, x.data_ptr(), 0, 4, 64, 64)
        assert quant(c.data_ptr(), 80, sc.data_ptr(), _C.cur_stream()) == 0
        assert quant(c.data_ptr(), 72, sc.data_ptr(), _C.cur_stream()) == ALIGN
        assert quant(c.data_ptr() + 4, 80, sc.data_ptr(), _C.cur_stream()) == ALIGN
        assert quant(c.data_ptr(), 48, sc.data_ptr(), _C.cur_stream()) == ALIGN
    torch.cuda.synchronize()
    assert np.isneginf(s.cpu().numpy()).sum() == 0 and (i.cpu().numpy()[:, 0] == 0).all()      # all-zero codes: ties, id order


# ---- the index and the pipeline ----------------------------------------------------------------------------------------
def _exact_rows(n, d, seed):
    """Rows whose bf16 rounding and fp32 dot products are exact: multiples of 1 / 8 in [-1, 1]."""
    return (np.random.default_rng(seed).integers(-8, 9, (n, d)) / 8).astype(F32)


def test_uneven_adds_tuples_and_float_rows_give_the_same_index_and_results():
    from contrastors_amd.search import Int8FlatIndex, quantize_rows_int8

    d, N = 192, 700
    rng = np.random.default_rng(9)
    D, Q = rng.standard_normal((N, d)).astype(F32), rng.standard_normal((33, d)).astype(F32)
    wc, ws = R.quantize(D)
    one = Int8FlatIndex(d, device=DEV)
    one.add(D)
    assert one.ntotal == N and one.codes.shape == (N, d) and one.scales.shape == (N,)
    _assert_same((one.codes, one.scales), (wc, ws))
    three = Int8FlatIndex(d, device=DEV)
    three.add(D[:1])
    three.add(torch.from_numpy(D[1:130]).to(DEV))
    three.add((wc[130:], torch.from_numpy(ws[130:])))
    _assert_same((three.codes, three.scales), (wc, ws))
    reserved = Int8FlatIndex(d, device=DEV)
    reserved.reserve(N)
    ptr = reserved._store.data_ptr()
    reserved.add(D[:300])
    reserved.add(quantize_rows_int8(torch.from_numpy(D[300:]).to(DEV)))
    assert reserved._store.data_ptr() == ptr
    _assert_same((reserved.codes, reserved.scales), (wc, ws))
    want = R.search(*R.quantize(Q), wc, ws, 20)
    for ix in (one, three, reserved):
        _assert_same(ix.search(Q, 20), want)
        _assert_same(ix.search(R.quantize(Q), 20), want)
    assert one.batch_rows(33, 20) == 33
    one.reset()
    assert one.ntotal == 0 and one.codes.shape == (0, d) and one.scales.shape == (0,)


@pytest.mark.parametrize("N", [129, 1000])
def test_rescored_search_covering_the_corpus_equals_the_exact_search_bit_for_bit(N, tmp_path):
    from contrastors_amd.search import FlatIPIndex, Int8FlatIndex, search_int8_rescored

    d, M, k = 128, 40, 10
    rng = np.random.default_rng(N)
    D = rng.standard_normal((N, d)).astype(F32)
    D[50] = D[7]                                             # a tie in the exact score
    Q = rng.standard_normal((M, d)).astype(F32)
    flat = FlatIPIndex(d, device=DEV)
    flat.add(D)
    ix = Int8FlatIndex(d, device=DEV)
    ix.add(D)
    full = flat.search(Q, k)
    excl = [[int(full[1][m, 0])] if m % 2 else [] for m in range(M)]
    below = full[0][:, 1].copy()
    np.save(tmp_path / "D.npy", D)
    sources = {"device": flat.vectors, "host": D, "memmap": np.load(tmp_path / "D.npy", mmap_mode="r")}
    factor = -(-N // k)
    for name, vectors in sources.items():
        for ex, bel in ((None, None), (excl, None), (None, below), (excl, below)):
            got = search_int8_rescored(ix, vectors, Q, k, factor, exclude=ex, below=bel)
            assert isinstance(got[0], np.ndarray)
            _assert_same(got, flat.search(Q, k, exclude=ex, below=bel))
    got = search_int8_rescored(ix, flat.vectors, torch.from_numpy(Q).to(DEV), k, factor)
    assert isinstance(got[0], torch.Tensor) and got[0].is_cuda
    _assert_same(got, full)


def test_rescored_search_with_partial_candidates_equals_the_reference_pipeline():
    from contrastors_amd.search import Int8FlatIndex, search_int8_rescored

    d, N, M, k = 64, 600, 20, 10
    D, Q = _exact_rows(N, d, 21), _exact_rows(M, d, 22)
    ix = Int8FlatIndex(d, device=DEV)
    ix.add(D)
    excl = [[m, m + 1] for m in range(M)]
    below = np.full(M, 3.0, F32)
    for factor, ex, bel in ((1, None, None), (2, excl, None), (3, excl, below)):
        ws, wi = R.pipeline(Q, D, k, factor, exclude=ex, below=bel)
        s, i = search_int8_rescored(ix, D, Q, k, factor, exclude=ex, below=bel)
        assert np.array_equal(i, wi) and np.array_equal(s.astype(np.float64), ws) and s.dtype == F32


def test_candidate_lists_longer_than_1024_are_fetched_in_pages():
    from contrastors_amd.search import Int8FlatIndex, search_int8_rescored

    d, N, M, k = 64, 5000, 5, 300
    D, Q = _exact_rows(N, d, 23), _exact_rows(M, d, 24)
    ix = Int8FlatIndex(d, device=DEV)
    ix.add(D)
    excl = [[int(x) for x in range(m, 40, 5)] for m in range(M)]
    ws, wi = R.pipeline(Q, D, k, 4, exclude=excl)            # 1200 candidates: two pages
    s, i = search_int8_rescored(ix, torch.from_numpy(D).to(DEV).to(torch.bfloat16), Q, k, 4, exclude=excl)
    assert np.array_equal(i, wi) and np.array_equal(s.astype(np.float64), ws)


# ---- the tools ---------------------------------------------------------------------------------------------------------
def _shards(path):
    got = []
    for p in sorted(Path(path).glob("shard-*.jsonl.gz")):
        with gzip.open(p, "rt") as f:
            got += [json.loads(line) for line in f]
    return got


def test_tools_with_int8_storage_write_what_the_default_run_writes(tmp_path):
    from contrastors_amd.tools import consistency_filter, mine_negatives

    fx = json.loads((GOLD / "search_curation.json").read_text())
    int8 = ["--storage", "int8", "--rescore_factor", "32"]   # 2 * 32 >= 40 pairs, 10 * 32 >= 9 documents
    c = fx["consistency"]
    np.save(tmp_path / "cq.npy", np.asarray(c["q"], F32))
    np.save(tmp_path / "cd.npy", np.asarray(c["d"], F32))
    (tmp_path / "ids.json").write_text(json.dumps(c["ids"]))
    t = fx["topk"]
    with open(tmp_path / "recs.jsonl", "w") as f:
        for r in t["records"]:
            f.write(json.dumps(r) + "\n")
    np.save(tmp_path / "tq.npy", np.asarray(t["q"], F32))
    np.save(tmp_path / "td.npy", np.asarray(t["d"], F32))
    kept, mined = {}, {}
    for name, flags in (("default", []), ("int8", int8)):
        assert consistency_filter.main(["--output_dir", str(tmp_path / f"cf_{name}"), "--query_embeddings",
                                        str(tmp_path / "cq.npy"), "--document_embeddings", str(tmp_path / "cd.npy"), "--ids",
                                        str(tmp_path / "ids.json"), "--device", DEV, *flags]) == 0
        kept[name] = (tmp_path / f"cf_{name}" / "ids_to_keep_0.json").read_bytes()
        assert mine_negatives.main(["--rule", "topk", "--dataset", str(tmp_path / "recs.jsonl"), "--output_dir",
                                    str(tmp_path / f"tk_{name}"), "--k", str(t["k"]), "--seed", str(t["seed"]),
                                    "--query_embeddings", str(tmp_path / "tq.npy"), "--document_embeddings",
                                    str(tmp_path / "td.npy"), "--device", DEV, *flags]) == 0
        mined[name] = _shards(tmp_path / f"tk_{name}")
    assert kept["int8"] == kept["default"] and json.loads(kept["default"]) == c["kept"]
    assert mined["int8"] == mined["default"] and len(mined["default"]) == len(t["expected"])
