"""CPU checks of the binary index: its C-ABI entries (header, ctypes lists, ABI version, shape errors that are decided before
any pointer is touched), pack_sign_bits on the host against numpy.packbits, the argument errors of BinaryFlatIndex / rescore,
and the curation tools' new flags.  No GPU call is made."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "contrastors_hip.h"
BINARY_SYMBOLS = {"cx_pack_sign_bits", "cx_search_hamming_topk", "cx_search_hamming_ws_bytes", "cx_rescore_topk"}


@pytest.fixture(scope="module")
def built():
    from contrastors_amd import build

    return build.build()


def test_binary_symbols_in_header_ctypes_and_product_library(built):
    from contrastors_amd import _C

    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", HDR.read_text()))
    assert BINARY_SYMBOLS <= declared
    assert declared == set(_C.EXPORTED_SYMBOLS)
    assert not BINARY_SYMBOLS & set(_C.DEV_EXPORTED_SYMBOLS)
    lib = _C.lib()
    assert lib.cx_abi_version() == 10          # additive: no existing signature changed
    for name in BINARY_SYMBOLS:
        assert hasattr(lib, name)
    # workspace: (M, splits, k) lists of (int32 distance, int32 id) + one count per (row, split) + 16
    assert lib.cx_search_hamming_ws_bytes(128, 128, 10, 1) == 128 * (10 * 8 + 4) + 16
    assert lib.cx_search_hamming_ws_bytes(128, 128 * 100, 10, 7) == 128 * 7 * (10 * 8 + 4) + 16
    assert lib.cx_search_hamming_ws_bytes(128, 128 * 3, 10, 7) == 128 * 3 * (10 * 8 + 4) + 16
    assert lib.cx_search_hamming_ws_bytes(0, 10, 10, 0) == 0


def test_binary_entry_points_refuse_bad_shapes_before_touching_pointers(built):
    from contrastors_amd import _C

    lib = _C.lib()
    SHAPE, ARG = -1, -3

    def hamming(N, d, k):
        return lib.cx_search_hamming_topk(None, None, 1, N, d, d // 8, d // 8, k, None, None, None, 0, None, None, None, None)

    assert hamming(10, 96, 1) == SHAPE
    assert hamming(10, 32, 1) == SHAPE
    assert hamming(10, 1088, 1) == SHAPE
    assert hamming(10, 64, 0) == SHAPE
    assert hamming(10, 64, 1025) == SHAPE
    assert hamming(2 ** 31 - 128, 64, 1) == SHAPE
    assert hamming(2 ** 31 - 129, 64, 1) == ARG          # in bounds: the null pointers are refused
    assert lib.cx_pack_sign_bits(None, 0, 4, 96, 96, None, 12, None) == SHAPE
    assert lib.cx_pack_sign_bits(None, 2, 4, 64, 64, None, 8, None) == ARG
    assert lib.cx_pack_sign_bits(None, 0, 4, 64, 64, None, 8, None) == ARG

    def rescore(d, c, k):
        return lib.cx_rescore_topk(None, None, None, None, 1, 10, d, d, d, c, k, None, None, None, None)

    assert rescore(96, 4, 1) == SHAPE
    assert rescore(64, 0, 1) == SHAPE
    assert rescore(64, 4097, 1) == SHAPE
    assert rescore(64, 4, 5) == SHAPE                   # k <= c
    assert rescore(64, 4096, 1025) == SHAPE
    assert rescore(64, 4096, 1024) == ARG


def test_binary_prototypes_match_ctypes_arity_under_gcc(tmp_path, built):
    from contrastors_amd import _C

    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include "contrastors_hip.h"\n'
                   "int main(void){long (*a)(int, long, int, int) = cx_search_hamming_ws_bytes;"
                   " int (*b)(const uint8_t*, const uint8_t*, int, long, int, long, long, int, const int64_t*,"
                   " const int64_t*, const int32_t*, int, void*, int32_t*, int64_t*, void*) = cx_search_hamming_topk;"
                   " int (*c)(const void*, int, long, int, long, uint8_t*, long, void*) = cx_pack_sign_bits;"
                   " int (*e)(const uint16_t*, const uint16_t*, const int64_t*, const int64_t*, int, long, int, long, long,"
                   " int, int, const float*, float*, int64_t*, void*) = cx_rescore_topk;"
                   " printf(\"%d\\n\", a != 0 && b != 0 && c != 0 && e != 0); return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])
    res, args = _C._SIGS["cx_search_hamming_topk"]
    assert res is C.c_int and len(args) == 16 and args == _C._SIGS["cx_search_topk"][1]   # argument for argument
    res, args = _C._SIGS["cx_search_hamming_ws_bytes"]
    assert res is C.c_long and args == [C.c_int, C.c_long, C.c_int, C.c_int]
    res, args = _C._SIGS["cx_pack_sign_bits"]
    assert res is C.c_int and args[1:5] == [C.c_int, C.c_long, C.c_int, C.c_long] and len(args) == 8
    res, args = _C._SIGS["cx_rescore_topk"]
    assert res is C.c_int and len(args) == 15
    assert args[4:11] == [C.c_int, C.c_long, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int]


def _signed_edge_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    x[0, :8] = [0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45]     # +-0 and NaN -> 0; the denormal counts
    x[-1, -4:] = [np.nan, 0.0, -0.0, 3.0]
    return x


@pytest.mark.parametrize("d", [64, 192, 1024])
def test_pack_sign_bits_on_the_host_equals_numpy_packbits(d):
    from contrastors_amd.search import pack_sign_bits

    x = _signed_edge_rows(5, d, d)
    want = np.packbits(x > 0, axis=1)
    assert want[0, 0] == 0b00001010                         # dimension 0 is bit 7: only +inf and the positive denormal
    got = pack_sign_bits(x)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (5, d // 8)
    assert np.array_equal(got, want)
    got_t = pack_sign_bits(torch.from_numpy(x))
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.uint8 and np.array_equal(got_t.numpy(), want)
    xb = torch.from_numpy(x).to(torch.bfloat16)             # the denormal rounds to zero: compare against the rounded rows
    assert np.array_equal(pack_sign_bits(xb).numpy(), np.packbits(xb.float().numpy() > 0, axis=1))


def test_argument_errors():
    from contrastors_amd.search import BinaryFlatIndex, pack_sign_bits, rescore

    with pytest.raises(ValueError, match="multiple of 64"):
        BinaryFlatIndex(96)
    with pytest.raises(ValueError, match="multiple of 64"):
        BinaryFlatIndex(2048)
    with pytest.raises(ValueError, match="multiple of 64"):
        pack_sign_bits(np.zeros((2, 96), np.float32))
    with pytest.raises(ValueError):
        pack_sign_bits(np.zeros(64, np.float32))
    with pytest.raises(RuntimeError, match="GPU"):
        BinaryFlatIndex(64, device="cpu")
    ix = BinaryFlatIndex(64)
    assert ix.ntotal == 0 and ix.d == 64
    q = np.zeros((3, 64), np.float32)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k must be"):
            ix.search(q, k)
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.search(q, 1, exclude=(np.array([0, 2, 1, 3]), np.array([1, 2, 3])))       # decreasing offsets
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.search(q, 1, exclude=(np.array([0, 1, 2]), np.array([1, 2])))              # M + 1 offsets wanted
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.search(q, 1, exclude=(np.array([0, 1, 2, 5]), np.array([1, 2, 3])))        # past the id array
    with pytest.raises(ValueError, match="rows for 3 queries"):
        ix.search(q, 1, exclude=[[1], [2]])
    vec = np.zeros((10, 64), np.float32)
    with pytest.raises(ValueError, match="candidate lists"):
        rescore(q, np.zeros((3, 4097), np.int64), vec, 1)
    with pytest.raises(ValueError, match="k must be"):
        rescore(q, np.zeros((3, 4), np.int64), vec, 5)
    with pytest.raises(ValueError, match="multiple of 64"):
        rescore(np.zeros((3, 96), np.float32), np.zeros((3, 4), np.int64), np.zeros((10, 96), np.float32), 1)


def test_tool_parsers_take_the_coarse_flags_and_default_to_exact():
    from contrastors_amd.tools import consistency_filter, mine_negatives

    base = {mine_negatives: ["--rule", "topk", "--dataset", "x", "--output_dir", "o"],
            consistency_filter: ["--output_dir", "o"]}
    for tool, argv in base.items():
        ap = tool.build_parser()
        args = ap.parse_args(argv)
        assert args.coarse == "exact" and args.rescore_factor == 4
        args = ap.parse_args(argv + ["--coarse", "binary", "--rescore_factor", "16"])
        assert args.coarse == "binary" and args.rescore_factor == 16
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--coarse", "ivf"])
