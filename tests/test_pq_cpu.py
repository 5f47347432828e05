"""CPU checks of the product-quantised index: its C-ABI entries (header, ctypes lists, ABI version, refusals decided before any
pointer is touched), pq_encode on the host against the reference, the argument errors of PQFlatIndex / search_pq_rescored, and
the curation tools' --pq_* flags.  No GPU call is made."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import pq_ref as R

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "contrastors_hip.h"
PQ_SYMBOLS = {"cx_pq_half_norm", "cx_pq_assign", "cx_pq_update", "cx_search_pq_ws_bytes", "cx_search_pq_topk"}
SHAPE, ALIGN, ARG = -1, -2, -3


@pytest.fixture(scope="module")
def built():
    from contrastors_amd import build

    return build.build()


def test_pq_symbols_in_header_ctypes_and_product_library(built):
    from contrastors_amd import _C

    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", HDR.read_text()))
    assert PQ_SYMBOLS <= declared
    assert declared == set(_C.EXPORTED_SYMBOLS)
    assert not PQ_SYMBOLS & set(_C.DEV_EXPORTED_SYMBOLS)
    lib = _C.lib()
    assert lib.cx_abi_version() == 10          # additive: no existing signature changed
    for name in PQ_SYMBOLS:
        assert hasattr(lib, name)
    for args in ((128, 128, 10, 1), (128, 128 * 100, 10, 7), (1000, 10 ** 6, 1024, 0), (0, 10, 10, 0)):
        assert lib.cx_search_pq_ws_bytes(*args) == lib.cx_search_ws_bytes(*args)


def test_pq_prototypes_match_ctypes_arity_under_gcc(tmp_path, built):
    from contrastors_amd import _C

    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include "contrastors_hip.h"\n'
                   "int main(void){long (*a)(int, long, int, int) = cx_search_pq_ws_bytes;"
                   " int (*b)(const uint16_t*, const uint8_t*, const uint16_t*, int, long, int, int, long, long, int,"
                   " const int64_t*, const int64_t*, const float*, int, void*, float*, int64_t*, void*) = cx_search_pq_topk;"
                   " int (*c)(const uint16_t*, long, int, long, const uint16_t*, const float*, int, uint8_t*, long, void*)"
                   " = cx_pq_assign;"
                   " int (*e)(const uint16_t*, long, int, long, const uint8_t*, long, int, float*, uint16_t*, float*, void*)"
                   " = cx_pq_update;"
                   " int (*f)(const uint16_t*, int, int, float*, void*) = cx_pq_half_norm;"
                   " printf(\"%d\\n\", a != 0 && b != 0 && c != 0 && e != 0 && f != 0); return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])
    res, args = _C._SIGS["cx_search_pq_topk"]
    base = _C._SIGS["cx_search_topk"][1]       # (Q, D, M, N, d, ldq, ldd, k, ...): + the codebook and dsub
    assert res is C.c_int and args == base[:2] + [C.c_void_p] + base[2:5] + [C.c_int] + base[5:]
    assert _C._SIGS["cx_search_pq_ws_bytes"] == _C._SIGS["cx_search_ws_bytes"]
    assert len(_C._SIGS["cx_pq_assign"][1]) == 10 and len(_C._SIGS["cx_pq_update"][1]) == 11


def test_pq_entry_points_refuse_bad_shapes_arguments_and_alignment_before_touching_pointers(built):
    from contrastors_amd import _C

    lib = _C.lib()
    one = C.c_void_p(16)                       # never dereferenced: every call below is refused first

    def search(N, d, dsub, k, Q=None, codes=None, cb=None, ldq=None, ldc=None, ws=None, out=None):
        return lib.cx_search_pq_topk(Q, codes, cb, 1, N, d, dsub, d if ldq is None else ldq, d // max(dsub, 1) if ldc is None
                                     else ldc, k, None, None, None, 0, ws, out, out, None)

    for d, dsub, k in ((96, 8, 1), (32, 8, 1), (1088, 8, 1), (64, 8, 0), (64, 8, 1025), (64, 4, 1), (64, 12, 1), (128, 128, 1),
                       (64, 0, 1)):
        assert search(10, d, dsub, k) == SHAPE
    assert search(2 ** 31 - 128, 64, 8, 1) == SHAPE
    assert search(2 ** 31 - 129, 64, 8, 1) == ARG            # in bounds: the null pointers are refused
    assert search(10, 64, 8, 1, Q=one, out=one) == ARG       # N > 0 without codes, codebook and workspace
    assert search(10, 64, 8, 1, Q=one, codes=one, ws=one, out=one) == ARG         # ... without a codebook
    full = dict(Q=one, codes=one, cb=one, ws=one, out=one)
    assert search(10, 64, 8, 1, **{**full, "ldq": 60}) == ALIGN
    assert search(10, 64, 8, 1, **{**full, "ldq": 68}) == ALIGN
    assert search(10, 64, 8, 1, **{**full, "ldc": 7}) == ALIGN                    # a code row shorter than m
    assert search(10, 64, 8, 1, **{**full, "cb": C.c_void_p(8)}) == ALIGN
    assert search(10, 64, 8, 1, **{**full, "Q": C.c_void_p(8)}) == ALIGN
    assert search(10, 64, 8, 1, **{**full, "ws": C.c_void_p(8)}) == ALIGN
    assert lib.cx_search_pq_topk(None, None, None, 0, 10, 64, 8, 64, 8, 1, None, None, None, 0, None, None, None, None) == 0

    def assign(n, d, dsub, X=None, sh=None, hn=None, codes=None, ldx=None, ldc=None):
        return lib.cx_pq_assign(X, n, d, d if ldx is None else ldx, sh, hn, dsub, codes,
                                d // max(dsub, 1) if ldc is None else ldc, None)

    assert assign(4, 96, 8) == SHAPE and assign(4, 64, 24) == SHAPE and assign(-1, 64, 8) == SHAPE
    assert assign(0, 64, 8) == 0                             # n = 0: nothing to do, nothing is looked at
    assert assign(4, 64, 8) == ARG and assign(4, 64, 8, X=one, sh=one, hn=one) == ARG
    ok = dict(X=one, sh=one, hn=one, codes=one)
    assert assign(4, 64, 8, **{**ok, "ldx": 63}) == ALIGN
    assert assign(4, 64, 8, **{**ok, "ldc": 7}) == ALIGN
    assert assign(4, 64, 64, **{**ok, "ldc": 0}) == ALIGN    # m = 1: ldc == 1 is the smallest legal value
    assert assign(4, 64, 8, **{**ok, "X": C.c_void_p(17)}) == ALIGN
    assert assign(4, 64, 8, **{**ok, "sh": C.c_void_p(8)}) == ALIGN

    def update(n, d, dsub, X=None, codes=None, ma=None, sh=None, hn=None, ldx=None, ldc=None):
        return lib.cx_pq_update(X, n, d, d if ldx is None else ldx, codes, d // max(dsub, 1) if ldc is None else ldc, dsub, ma,
                                sh, hn, None)

    assert update(4, 96, 8) == SHAPE and update(4, 64, 5) == SHAPE and update(2 ** 24 + 1, 64, 8) == SHAPE
    assert update(0, 64, 8) == 0
    assert update(4, 64, 8) == ARG and update(4, 64, 8, X=one, codes=one, ma=one, sh=one) == ARG
    oku = dict(X=one, codes=one, ma=one, sh=one, hn=one)
    assert update(4, 64, 8, **{**oku, "ldx": 32}) == ALIGN and update(4, 64, 8, **{**oku, "ldc": 4}) == ALIGN
    assert update(4, 64, 8, **{**oku, "ma": C.c_void_p(18)}) == ALIGN
    assert lib.cx_pq_half_norm(None, 64, 8, None, None) == ARG and lib.cx_pq_half_norm(None, 64, 3, None, None) == SHAPE


@pytest.mark.parametrize("d, dsub", [(64, 8), (64, 64), (192, 16), (320, 32)])
def test_pq_encode_on_the_host_equals_the_reference(d, dsub):
    """The host path of pq_encode is written the way the reference is (the same float64 product-and-sum for fmaf, the same
    rounding to bf16), so this comparison checks the plumbing -- shapes, dtypes, the rounding of rows and codebooks, torch in ->
    torch out -- and not the arithmetic a second time.  The arithmetic is held independently in tests/test_pq_ref_cpu.py, against
    scalar loops in exact rational arithmetic, and on the GPU by the kernel's equality with the reference."""
    from contrastors_amd.search import pq_encode

    rng = np.random.default_rng(d + dsub)
    m = d // dsub
    masters = rng.standard_normal((m, 256, dsub)).astype(np.float32)
    masters[0, 9] = masters[0, 4]                            # duplicate centroids: the lower code
    x = rng.standard_normal((37, d)).astype(np.float32)
    x[3, :dsub] = R.to_bf16(masters)[0, 9]                   # ... a row that sits on them
    x[4] = 0
    want = R.assign(x, R.to_bf16(masters))
    assert want[3, 0] == 4
    got = pq_encode(x, masters)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (37, m) and np.array_equal(got, want)
    gt = pq_encode(torch.from_numpy(x), torch.from_numpy(masters).to(torch.bfloat16))
    assert isinstance(gt, torch.Tensor) and gt.dtype == torch.uint8 and np.array_equal(gt.numpy(), want)
    gb = pq_encode(torch.from_numpy(x).to(torch.bfloat16), masters)
    assert np.array_equal(gb.numpy(), want)
    assert pq_encode(np.zeros((0, d), np.float32), masters).shape == (0, m)


def test_argument_errors_raise_before_any_launch():
    from contrastors_amd.search import PQFlatIndex, pq_encode, pq_train_rows, search_pq_rescored

    with pytest.raises(ValueError, match="multiple of 64"):
        PQFlatIndex(96)
    with pytest.raises(ValueError, match="multiple of 64"):
        PQFlatIndex(2048)
    for dsub in (0, 4, 12, 128):
        with pytest.raises(ValueError, match="dsub must be"):
            PQFlatIndex(128, dsub)
    with pytest.raises(RuntimeError, match="GPU"):
        PQFlatIndex(64, device="cpu")
    with pytest.raises(ValueError, match="codebooks"):
        pq_encode(np.zeros((2, 64), np.float32), np.zeros((8, 255, 8), np.float32))
    with pytest.raises(ValueError, match="codebooks"):
        pq_encode(np.zeros((2, 64), np.float32), np.zeros((16, 256, 4), np.float32))
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        pq_encode(np.zeros((2, 128), np.float32), np.zeros((8, 256, 8), np.float32))
    with pytest.raises(ValueError, match="multiple of 64"):
        pq_encode(np.zeros((2, 96), np.float32), np.zeros((12, 256, 8), np.float32))
    ix = PQFlatIndex(64)
    assert ix.ntotal == 0 and ix.d == 64 and ix.dsub == 8 and ix.m == 8 and not ix.is_trained and ix.seed == 0
    assert PQFlatIndex(128, 32).m == 4
    with pytest.raises(ValueError, match="at most"):
        ix.reserve(2 ** 31 - 128)
    for attr in ("codebooks", "masters", "half_norms"):
        with pytest.raises(RuntimeError, match="train"):
            getattr(ix, attr)
    with pytest.raises(RuntimeError, match="train"):
        ix.decode()
    # train
    with pytest.raises(ValueError, match="either"):
        ix.train()
    with pytest.raises(ValueError, match="either"):
        ix.train(np.zeros((300, 64), np.float32), codebooks=np.zeros((8, 256, 8), np.float32))
    with pytest.raises(ValueError, match=r"\(8, 256, 8\)"):
        ix.train(codebooks=np.zeros((4, 256, 16), np.float32))
    with pytest.raises(ValueError, match="codebooks"):
        ix.train(codebooks=np.zeros((8, 256), np.float32))
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        ix.train(np.zeros((300, 128), np.float32))
    with pytest.raises(ValueError, match="at least 256 rows"):
        ix.train(np.zeros((255, 64), np.float32))
    for sample in (255, 262145, 0):
        with pytest.raises(ValueError, match="sample must be"):
            ix.train(np.zeros((300, 64), np.float32), sample=sample)
    with pytest.raises(ValueError, match="max_iter"):
        ix.train(np.zeros((300, 64), np.float32), max_iter=-1)
    assert not ix.is_trained
    # add
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        ix.add(np.zeros((3, 128), np.float32))
    with pytest.raises(ValueError, match="uint8 codes"):
        ix.add(np.zeros((3, 64), np.uint8))
    with pytest.raises(ValueError, match="2-d"):
        ix.add(np.zeros(64, np.float32))
    with pytest.raises(RuntimeError, match="train"):
        ix.add(np.zeros((3, 64), np.float32))
    with pytest.raises(RuntimeError, match="train"):
        ix.add(np.zeros((3, 8), np.uint8))
    assert ix.ntotal == 0
    # search
    q = np.zeros((3, 64), np.float32)
    vec = np.zeros((0, 64), np.float32)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k must be"):
            ix.search(q, k)
        with pytest.raises(ValueError, match="k must be"):
            search_pq_rescored(ix, vec, q, k)
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        ix.search(np.zeros((3, 128), np.float32), 1)
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.search(q, 1, exclude=(np.array([0, 2, 1, 3]), np.array([1, 2, 3])))
    with pytest.raises(ValueError, match="rows for 3 queries"):
        ix.search(q, 1, exclude=[[1], [2]])
    with pytest.raises(ValueError, match="below has 2 entries"):
        ix.search(q, 1, below=np.zeros(2, np.float32))
    with pytest.raises(RuntimeError, match="train"):
        ix.search(q, 1)
    with pytest.raises(ValueError, match="rescore_factor"):
        search_pq_rescored(ix, vec, q, 1, rescore_factor=0)
    with pytest.raises(ValueError, match="10 vectors for an index of 0"):
        search_pq_rescored(ix, np.zeros((10, 64), np.float32), q, 1)
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        search_pq_rescored(ix, vec, np.zeros((3, 128), np.float32), 1)
    with pytest.raises(ValueError, match="rows for 3 queries"):
        search_pq_rescored(ix, vec, q, 1, exclude=[[1], [2]])
    with pytest.raises(ValueError, match="below has 2 entries"):
        search_pq_rescored(ix, vec, q, 1, below=np.zeros(2, np.float32))
    with pytest.raises(RuntimeError, match="train"):
        search_pq_rescored(ix, vec, q, 1)
    # the seeded rows of a fit: KMeans.fit(sample=)'s choice, then the first 256 of a permutation of the sample
    rows, first = pq_train_rows(1000, 300, 5)
    g = torch.Generator().manual_seed(5)
    assert torch.equal(rows, torch.randperm(1000, generator=g)[:300].sort().values)
    g = torch.Generator().manual_seed(5)
    assert torch.equal(first, torch.randperm(300, generator=g)[:256]) and first.unique().numel() == 256
    rows, first = pq_train_rows(300, 300, 5)
    assert rows is None and torch.equal(first, torch.randperm(300, generator=torch.Generator().manual_seed(5))[:256])


def test_tool_parsers_take_the_pq_flags_and_refuse_what_they_cannot_serve(capsys):
    from contrastors_amd.tools import _common, consistency_filter, mine_negatives

    assert _common.COARSE == ("exact", "binary")
    assert _common.STORAGE == ("bf16", "int8")
    assert _common.IVF_STORAGE == ("bf16", "int8")
    base = {mine_negatives: ["--rule", "topk", "--dataset", "x", "--output_dir", "o"],
            consistency_filter: ["--output_dir", "o"]}
    for tool, argv in base.items():
        ap = tool.build_parser()
        args = ap.parse_args(argv)
        assert args.pq_dsub == 0 and args.pq_sample is None and args.pq_iters == 25 and args.pq_codebooks is None
        assert args.storage == "bf16" and args.coarse == "exact" and args.rescore_factor == 4
        assert _common.check_search_arguments(ap, args) == {} and not _common.host_documents(args)
        args = ap.parse_args(argv + ["--pq_dsub", "8"])
        assert _common.host_documents(args)                  # the document .npy is memory-mapped
        assert _common.check_search_arguments(ap, args) == {"pq_dsub": 8, "pq_sample": None, "pq_iters": 25,
                                                            "pq_codebooks": None}
        args = ap.parse_args(argv + ["--pq_dsub", "16", "--pq_sample", "1000", "--pq_iters", "3", "--pq_codebooks", "c.npy",
                                     "--rescore_factor", "8"])
        assert _common.check_search_arguments(ap, args) == {"pq_dsub": 16, "pq_sample": 1000, "pq_iters": 3,
                                                            "pq_codebooks": "c.npy"} and args.rescore_factor == 8
        for bad in ("4", "12", "128"):
            with pytest.raises(SystemExit):
                ap.parse_args(argv + ["--pq_dsub", bad])
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--storage", "pq"])
        capsys.readouterr()
        for bad in (["--coarse", "binary"], ["--storage", "int8"], ["--ivf_lists", "4"]):
            with pytest.raises(SystemExit):
                _common.check_search_arguments(ap, ap.parse_args(argv + ["--pq_dsub", "8"] + bad))
            assert "--pq_dsub" in capsys.readouterr().err
        for bad in (["--pq_sample", "1000"], ["--pq_codebooks", "c.npy"]):
            with pytest.raises(SystemExit):
                _common.check_search_arguments(ap, ap.parse_args(argv + bad))
            assert "need --pq_dsub" in capsys.readouterr().err
        for bad in (["--pq_sample", "255"], ["--pq_sample", "262145"], ["--pq_iters", "-1"]):
            with pytest.raises(SystemExit):
                _common.check_search_arguments(ap, ap.parse_args(argv + ["--pq_dsub", "8"] + bad))
        with pytest.raises(SystemExit):                     # the tool's own main refuses it too, before any file is read
            tool.main(argv + ["--pq_dsub", "8", "--coarse", "binary"])


def test_common_search_refuses_pq_with_binary_int8_or_ivf_before_any_launch():
    from contrastors_amd.tools import _common

    d, q = np.zeros((4, 64), np.float32), np.zeros((2, 64), np.float32)
    with pytest.raises(ValueError, match="pq_dsub must be"):
        _common.search(d, q, 1, "cuda", pq_dsub=12)
    with pytest.raises(ValueError, match="pq_dsub goes with"):
        _common.search(d, q, 1, "cuda", coarse="binary", pq_dsub=8)
    with pytest.raises(ValueError, match="pq_dsub goes with"):
        _common.search(d, q, 1, "cuda", storage="int8", pq_dsub=8)
    with pytest.raises(ValueError, match="pq_dsub goes with"):
        _common.search(d, q, 1, "cuda", ivf_lists=2, pq_dsub=8)
