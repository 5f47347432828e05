"""CPU checks of the int8 index: its C-ABI entries (header, ctypes lists, ABI version, shape errors decided before any pointer is
touched), quantize_rows_int8 on the host against the reference, the argument errors of Int8FlatIndex / search_int8_rescored, and
the curation tools' --storage flag.  No GPU call is made."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import int8_ref as R

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "contrastors_hip.h"
INT8_SYMBOLS = {"cx_quantize_rows_int8", "cx_search_int8_ws_bytes", "cx_search_int8_topk"}


@pytest.fixture(scope="module")
def built():
    from contrastors_amd import build

    return build.build()


def test_int8_symbols_in_header_ctypes_and_product_library(built):
    from contrastors_amd import _C

    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", HDR.read_text()))
    assert INT8_SYMBOLS <= declared
    assert declared == set(_C.EXPORTED_SYMBOLS)
    assert not INT8_SYMBOLS & set(_C.DEV_EXPORTED_SYMBOLS)
    lib = _C.lib()
    assert lib.cx_abi_version() == 10          # additive: no existing signature changed
    for name in INT8_SYMBOLS:
        assert hasattr(lib, name)
    for args in ((128, 128, 10, 1), (128, 128 * 100, 10, 7), (128, 128 * 3, 10, 7), (1000, 10 ** 6, 1024, 0), (0, 10, 10, 0)):
        assert lib.cx_search_int8_ws_bytes(*args) == lib.cx_search_ws_bytes(*args)
    assert lib.cx_search_int8_ws_bytes(128, 128 * 100, 10, 7) == 128 * 7 * (10 * 8 + 4) + 16


def test_int8_entry_points_refuse_bad_shapes_before_touching_pointers(built):
    from contrastors_amd import _C

    lib = _C.lib()
    SHAPE, ARG = -1, -3

    def search(N, d, k):
        return lib.cx_search_int8_topk(None, None, None, None, 1, N, d, d, d, k, None, None, None, 0, None, None, None, None)

    assert search(10, 96, 1) == SHAPE
    assert search(10, 32, 1) == SHAPE
    assert search(10, 1088, 1) == SHAPE
    assert search(10, 64, 0) == SHAPE
    assert search(10, 64, 1025) == SHAPE
    assert search(2 ** 31 - 128, 64, 1) == SHAPE
    assert search(2 ** 31 - 129, 64, 1) == ARG          # in bounds: the null pointers are refused
    assert lib.cx_quantize_rows_int8(None, 0, 4, 96, 96, None, 96, None, None) == SHAPE
    assert lib.cx_quantize_rows_int8(None, 2, 4, 64, 64, None, 64, None, None) == ARG
    assert lib.cx_quantize_rows_int8(None, 0, 4, 64, 64, None, 64, None, None) == ARG
    assert lib.cx_quantize_rows_int8(None, 0, 0, 64, 64, None, 64, None, None) == 0


def test_int8_prototypes_match_ctypes_arity_under_gcc(tmp_path, built):
    from contrastors_amd import _C

    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include "contrastors_hip.h"\n'
                   "int main(void){long (*a)(int, long, int, int) = cx_search_int8_ws_bytes;"
                   " int (*b)(const int8_t*, const int8_t*, const float*, const float*, int, long, int, long, long, int,"
                   " const int64_t*, const int64_t*, const float*, int, void*, float*, int64_t*, void*) = cx_search_int8_topk;"
                   " int (*c)(const void*, int, long, int, long, int8_t*, long, float*, void*) = cx_quantize_rows_int8;"
                   " printf(\"%d\\n\", a != 0 && b != 0 && c != 0); return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])
    res, args = _C._SIGS["cx_search_int8_topk"]
    base = _C._SIGS["cx_search_topk"][1]
    assert res is C.c_int and args == base[:2] + [C.c_void_p, C.c_void_p] + base[2:]     # cx_search_topk + the two scales
    assert _C._SIGS["cx_search_int8_ws_bytes"] == _C._SIGS["cx_search_ws_bytes"]
    res, args = _C._SIGS["cx_quantize_rows_int8"]
    assert res is C.c_int and args[1:5] == [C.c_int, C.c_long, C.c_int, C.c_long] and args[6] == C.c_long and len(args) == 9


def _edge_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32) * rng.uniform(1e-3, 50, (n, 1)).astype(np.float32)
    x[0] = 0
    x[1] = np.float32(2.0 ** -101)
    x[2, -1] = -1e4                                         # the amax element: last and negative
    x[3, :16] = (np.arange(16, dtype=np.float32) + 0.5) / 32
    x[3, 16:] = 0
    x[3, 20] = 127 / 32                                     # inv = 32: the first 16 elements land on k + 0.5
    return x


@pytest.mark.parametrize("d", [64, 192, 1024])
def test_quantize_rows_int8_on_the_host_equals_the_reference(d):
    from contrastors_amd.search import quantize_rows_int8

    x = _edge_rows(7, d, d)
    wc, ws = R.quantize(x)
    assert not wc[0].any() and ws[0] == 0 and not wc[1].any() and ws[1] == 0 and wc[2, -1] == -127
    assert wc[3, :4].tolist() == [0, 2, 2, 4]
    c, s = quantize_rows_int8(x)
    assert isinstance(c, np.ndarray) and c.dtype == np.int8 and c.shape == (7, d) and s.dtype == np.float32 and s.shape == (7,)
    assert np.array_equal(c, wc) and np.array_equal(s, ws)
    ct, st = quantize_rows_int8(torch.from_numpy(x))
    assert isinstance(ct, torch.Tensor) and ct.dtype == torch.int8 and st.dtype == torch.float32
    assert np.array_equal(ct.numpy(), wc) and np.array_equal(st.numpy(), ws)
    xb = torch.from_numpy(x).to(torch.bfloat16)             # bf16 is widened exactly: the reference of the rounded rows
    cb, sb = quantize_rows_int8(xb)
    wb = R.quantize(xb.float().numpy())
    assert np.array_equal(cb.numpy(), wb[0]) and np.array_equal(sb.numpy(), wb[1])
    e = quantize_rows_int8(np.zeros((0, d), np.float32))
    assert e[0].shape == (0, d) and e[1].shape == (0,)


def test_non_finite_rows_quantise_without_an_error_on_the_host():
    from contrastors_amd.search import quantize_rows_int8

    x = np.ones((3, 64), np.float32)
    x[0, 3], x[1, 5], x[2, 7] = np.nan, np.inf, -np.inf
    c, s = quantize_rows_int8(x)
    assert c.dtype == np.int8 and c.min() >= -127 and s.shape == (3,)


def test_argument_errors_raise_before_any_launch():
    from contrastors_amd.search import Int8FlatIndex, quantize_rows_int8, search_int8_rescored

    with pytest.raises(ValueError, match="multiple of 64"):
        Int8FlatIndex(96)
    with pytest.raises(ValueError, match="multiple of 64"):
        Int8FlatIndex(2048)
    with pytest.raises(ValueError, match="multiple of 64"):
        quantize_rows_int8(np.zeros((2, 96), np.float32))
    with pytest.raises(ValueError):
        quantize_rows_int8(np.zeros(64, np.float32))
    with pytest.raises(RuntimeError, match="GPU"):
        Int8FlatIndex(64, device="cpu")
    ix = Int8FlatIndex(64)
    assert ix.ntotal == 0 and ix.d == 64
    with pytest.raises(ValueError, match="at most"):
        ix.reserve(2 ** 31 - 128)
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        ix.add(np.zeros((3, 128), np.float32))
    with pytest.raises(ValueError, match="int8 codes"):
        ix.add((np.zeros((3, 64), np.uint8), np.zeros(3, np.float32)))
    with pytest.raises(ValueError, match="int8 codes"):
        ix.add((np.zeros((3, 128), np.int8), np.zeros(3, np.float32)))
    with pytest.raises(ValueError, match="float32 scales"):
        ix.add((np.zeros((3, 64), np.int8), np.zeros(4, np.float32)))
    with pytest.raises(ValueError, match="float32 scales"):
        ix.add((np.zeros((3, 64), np.int8), np.zeros(3, np.float64)))
    assert ix.ntotal == 0
    q = np.zeros((3, 64), np.float32)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k must be"):
            ix.search(q, k)
        with pytest.raises(ValueError, match="k must be"):
            search_int8_rescored(ix, np.zeros((0, 64), np.float32), q, k)
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        ix.search(np.zeros((3, 128), np.float32), 1)
    with pytest.raises(ValueError, match="int8 codes"):
        ix.search((np.zeros((3, 128), np.int8), np.zeros(3, np.float32)), 1)
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.search(q, 1, exclude=(np.array([0, 2, 1, 3]), np.array([1, 2, 3])))       # decreasing offsets
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.search(q, 1, exclude=(np.array([0, 1, 2, 5]), np.array([1, 2, 3])))        # past the id array
    with pytest.raises(ValueError, match="rows for 3 queries"):
        ix.search(q, 1, exclude=[[1], [2]])
    with pytest.raises(ValueError, match="below has 2 entries"):
        ix.search(q, 1, below=np.zeros(2, np.float32))
    vec = np.zeros((0, 64), np.float32)
    with pytest.raises(ValueError, match="rescore_factor"):
        search_int8_rescored(ix, vec, q, 1, rescore_factor=0)
    with pytest.raises(ValueError, match="10 vectors for an index of 0"):
        search_int8_rescored(ix, np.zeros((10, 64), np.float32), q, 1)
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        search_int8_rescored(ix, vec, np.zeros((3, 128), np.float32), 1)
    with pytest.raises(ValueError, match="rows for 3 queries"):
        search_int8_rescored(ix, vec, q, 1, exclude=[[1], [2]])
    with pytest.raises(ValueError, match="below has 2 entries"):
        search_int8_rescored(ix, vec, q, 1, below=np.zeros(2, np.float32))


def test_tool_parsers_take_the_storage_flag_and_refuse_what_it_cannot_serve(capsys):
    from contrastors_amd.tools import _common, consistency_filter, mine_negatives

    assert _common.COARSE == ("exact", "binary")
    assert _common.STORAGE == ("bf16", "int8")
    base = {mine_negatives: ["--rule", "topk", "--dataset", "x", "--output_dir", "o"],
            consistency_filter: ["--output_dir", "o"]}
    for tool, argv in base.items():
        ap = tool.build_parser()
        args = ap.parse_args(argv)
        assert args.storage == "bf16" and args.coarse == "exact" and args.rescore_factor == 4
        assert _common.check_search_arguments(ap, args) == {}
        args = ap.parse_args(argv + ["--storage", "int8"])
        assert args.storage == "int8" and args.rescore_factor == 4
        assert _common.check_search_arguments(ap, args) == {}
        args = ap.parse_args(argv + ["--storage", "int8", "--rescore_factor", "2"])
        assert args.rescore_factor == 2
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--storage", "fp8"])
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--coarse", "int8"])
        for bad in (["--coarse", "binary"], ["--ivf_lists", "4"]):
            with pytest.raises(SystemExit):
                _common.check_search_arguments(ap, ap.parse_args(argv + ["--storage", "int8"] + bad))
            assert "--storage int8" in capsys.readouterr().err
        with pytest.raises(SystemExit):                     # the tool's own main refuses it too, before any file is read
            tool.main(argv + ["--storage", "int8", "--coarse", "binary"])


def test_common_search_refuses_int8_with_binary_or_ivf_before_any_launch():
    from contrastors_amd.tools import _common

    d, q = np.zeros((4, 64), np.float32), np.zeros((2, 64), np.float32)
    with pytest.raises(ValueError, match="storage"):
        _common.search(d, q, 1, "cuda", storage="fp8")
    with pytest.raises(ValueError, match="int8"):
        _common.search(d, q, 1, "cuda", coarse="binary", storage="int8")
    with pytest.raises(ValueError, match="int8"):
        _common.search(d, q, 1, "cuda", ivf_lists=2, storage="int8")
