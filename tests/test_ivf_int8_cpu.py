"""CPU checks of the int8 IVF index: the windowed int8 entry points (header, ctypes lists, ABI version, the refusals decided
before any pointer is touched), the argument errors of IVFInt8Index / search_ivf_int8_rescored, which all come before anything
is allocated or launched (this machine has no GPU), and the curation tools' --ivf_storage flag."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "contrastors_hip.h"
SYMBOLS = {"cx_search_int8_window_ws_bytes", "cx_search_int8_window_topk"}


@pytest.fixture(scope="module")
def built():
    from contrastors_amd import build

    return build.build()


def test_symbols_in_header_ctypes_and_product_library(built):
    from contrastors_amd import _C

    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", HDR.read_text()))
    assert SYMBOLS <= declared and SYMBOLS <= set(_C.EXPORTED_SYMBOLS)
    assert not SYMBOLS & set(_C.DEV_EXPORTED_SYMBOLS)
    lib = _C.lib()
    assert lib.cx_abi_version() == 10          # additive: no existing signature changed
    for name in SYMBOLS:
        assert hasattr(lib, name)
    for args in ((1000, 100), (1, 1), (128, 1024), (129, 7), (0, 100), (100, 0)):
        assert lib.cx_search_int8_window_ws_bytes(*args) == lib.cx_search_window_ws_bytes(*args)
    assert lib.cx_search_int8_window_ws_bytes(1000, 100) == 1000 * (100 * 8 + 4) + 16
    # cx_search_int8_topk's operands with cx_search_window_topk's window in place of nsplit
    res, args = _C._SIGS["cx_search_int8_window_topk"]
    flat, win = _C._SIGS["cx_search_int8_topk"][1], _C._SIGS["cx_search_window_topk"][1]
    assert res is C.c_int and len(args) == 19 and args[:10] == flat[:10] and args[10:] == win[8:]
    assert _C._SIGS["cx_search_int8_window_ws_bytes"] == _C._SIGS["cx_search_window_ws_bytes"]


def test_prototypes_match_the_header_under_gcc(tmp_path):
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include "contrastors_hip.h"\n'
                   "int main(void){long (*a)(int, int) = cx_search_int8_window_ws_bytes;"
                   " int (*b)(const int8_t*, const int8_t*, const float*, const float*, int, long, int, long, long, int,"
                   " const int64_t*, const int64_t*, const int64_t*, const int64_t*, const float*, void*, float*, int64_t*,"
                   " void*) = cx_search_int8_window_topk;"
                   " printf(\"%d\\n\", a != 0 && b != 0); return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])


def test_entry_point_refuses_before_touching_pointers(built):
    from contrastors_amd import _C

    lib = _C.lib()
    SHAPE, ALIGN, ARG = -1, -2, -3

    def search(M, N, d, k, ldq=None, ldd=None, ptr=None):
        return lib.cx_search_int8_window_topk(ptr, ptr, ptr, ptr, M, N, d, d if ldq is None else ldq, d if ldd is None else ldd,
                                              k, None, None, None, None, None, ptr, ptr, ptr, None)

    for d in (96, 32, 0, 1088):
        assert search(1, 10, d, 1) == SHAPE
    for k in (0, 1025):
        assert search(1, 10, 64, k) == SHAPE
    assert search(-1, 10, 64, 1) == SHAPE and search(1, -1, 64, 1) == SHAPE
    assert search(1, 2 ** 31 - 128, 64, 1) == SHAPE
    assert search(1, 2 ** 31 - 129, 64, 1) == ARG           # in bounds: the null pointers are refused
    assert search(0, 10, 64, 1) == 0                        # M = 0: nothing to do, nothing is read
    # with (never dereferenced) non-null pointers: leading dimensions in bytes, % 16 and >= d; 16-byte aligned pointers
    assert search(1, 10, 64, 1, ldq=72, ptr=4096) == ALIGN
    assert search(1, 10, 64, 1, ldd=72, ptr=4096) == ALIGN
    assert search(1, 10, 128, 1, ldq=64, ptr=4096) == ALIGN
    assert search(1, 10, 64, 1, ptr=4104) == ALIGN
    # an exclusion row pointer without ids
    assert lib.cx_search_int8_window_topk(4096, 4096, 4096, 4096, 1, 10, 64, 64, 64, 1, None, None, 4096, None, None, 4096,
                                          4096, 4096, None) == ARG
    for null in (0, 1, 2, 3, 15, 16, 17):                   # Q, D, q_scale, d_scale, ws, out_scores, out_ids
        a = [4096, 4096, 4096, 4096, 1, 10, 64, 64, 64, 1, None, None, None, None, None, 4096, 4096, 4096, None]
        a[null] = None
        assert lib.cx_search_int8_window_topk(*a) == ARG, null


def _trained(nlist=4, d=64):
    """An index that passes the `trained` check without a device: the refusals under test come before any use of it."""
    from contrastors_amd.search import IVFInt8Index

    ix = IVFInt8Index(d, nlist)
    ix._centroids = torch.zeros(nlist, d)
    return ix


def test_index_refusals_come_before_any_launch():
    from contrastors_amd.search import MAX_NPROBE, IVFFlatIndex, IVFInt8Index, _IVFLists

    assert issubclass(IVFInt8Index, _IVFLists) and issubclass(IVFFlatIndex, _IVFLists)      # one copy of the bookkeeping
    for name in ("train", "_finalise", "list_sizes", "batch_queries", "reset", "_append"):
        assert name not in vars(IVFInt8Index) and name not in vars(IVFFlatIndex)
    for d in (0, 32, 96, 1088):
        with pytest.raises(ValueError, match="d must be"):
            IVFInt8Index(d, 4)
    for nlist in (0, -3):
        with pytest.raises(ValueError, match="nlist"):
            IVFInt8Index(64, nlist)
    with pytest.raises(RuntimeError, match="GPU"):
        IVFInt8Index(64, 4, device="cpu")
    ix = IVFInt8Index(64, 1000)
    assert ix.ntotal == 0 and not ix.is_trained and MAX_NPROBE == 256
    q = np.zeros((3, 64), np.float32)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k must be"):
            ix.search(q, k, 1)
    for nprobe in (0, 257, 1001):
        with pytest.raises(ValueError, match="nprobe"):
            ix.search(q, 10, nprobe)
    with pytest.raises(ValueError, match="nprobe"):
        IVFInt8Index(64, 4).search(q, 10, 5)                     # nprobe > nlist
    for call in (lambda: ix.search(q, 10, 8), lambda: ix.add(q), lambda: ix.centroids, lambda: ix.list_sizes):
        with pytest.raises(RuntimeError, match="IVFInt8Index has no centroids"):
            call()
    with pytest.raises(ValueError, match="centroids"):
        ix.train(centroids=np.zeros((999, 64), np.float32))
    with pytest.raises(ValueError, match="either"):
        ix.train()
    # batch_queries counts int8 pair rows plus their scale: d + 4 bytes where the bf16 sibling counts 2 d
    a, b = IVFInt8Index(768, 8, workspace_bytes=1 << 24), IVFFlatIndex(768, 8, workspace_bytes=1 << 24)
    assert a._pair_row_bytes() == 772 and b._pair_row_bytes() == 1536
    assert a.batch_queries(10 ** 6, 10, 8) == (1 << 24) // (8 * (200 + 4 + 772 + 32)) // 128 * 128
    assert b.batch_queries(10 ** 6, 10, 8) == (1 << 24) // (8 * (200 + 4 + 1536 + 32)) // 128 * 128
    # a trained index: shapes, float rows only, exclusions, below
    ix = _trained()
    for call in (lambda x: ix.search(x, 1, 1), ix.add):
        with pytest.raises(ValueError, match=r"\(n, 64\)"):
            call(np.zeros((3, 128), np.float32))
        with pytest.raises(ValueError, match=r"\(n, 64\)"):
            call(np.zeros(64, np.float32))
        with pytest.raises(ValueError, match="float"):
            call((np.zeros((3, 64), np.int8), np.zeros(3, np.float32)))
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.search(q, 1, 1, exclude=(np.array([0, 2, 1, 3]), np.array([1, 2, 3])))       # decreasing offsets
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.search(q, 1, 1, exclude=(np.array([0, 1, 2, 5]), np.array([1, 2, 3])))        # past the id array
    with pytest.raises(ValueError, match="rows for 3 queries"):
        ix.search(q, 1, 1, exclude=[[1], [2]])
    with pytest.raises(ValueError, match="below has 2 entries"):
        ix.search(q, 1, 1, below=np.zeros(2, np.float32))
    assert ix.ntotal == 0


def test_rescored_search_refusals_come_before_any_launch():
    from contrastors_amd.search import IVFInt8Index, search_ivf_int8_rescored

    q, vec = np.zeros((3, 64), np.float32), np.zeros((0, 64), np.float32)
    ix = IVFInt8Index(64, 4)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k must be"):
            search_ivf_int8_rescored(ix, vec, q, k, 1)
    with pytest.raises(ValueError, match="rescore_factor"):
        search_ivf_int8_rescored(ix, vec, q, 1, 1, rescore_factor=0)
    with pytest.raises(ValueError, match="10 vectors for an index of 0"):
        search_ivf_int8_rescored(ix, np.zeros((10, 64), np.float32), q, 1, 1)
    for nprobe in (0, 5, 257):
        with pytest.raises(ValueError, match="nprobe"):
            search_ivf_int8_rescored(ix, vec, q, 1, nprobe)
    with pytest.raises(RuntimeError, match="train"):
        search_ivf_int8_rescored(ix, vec, q, 1, 1)
    ix = _trained()
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        search_ivf_int8_rescored(ix, vec, np.zeros((3, 128), np.float32), 1, 1)
    with pytest.raises(ValueError, match="rows for 3 queries"):
        search_ivf_int8_rescored(ix, vec, q, 1, 1, exclude=[[1], [2]])
    with pytest.raises(ValueError, match="malformed CSR"):
        search_ivf_int8_rescored(ix, vec, q, 1, 1, exclude=(np.array([0, 2, 1, 3]), np.array([1, 2, 3])))
    with pytest.raises(ValueError, match="below has 2 entries"):
        search_ivf_int8_rescored(ix, vec, q, 1, 1, below=np.zeros(2, np.float32))


# ---- the tools ---------------------------------------------------------------------------------------------------------
def test_tool_parsers_take_ivf_storage_and_refuse_what_it_cannot_serve(capsys):
    from contrastors_amd.tools import _common, consistency_filter, mine_negatives

    assert _common.COARSE == ("exact", "binary")
    assert _common.STORAGE == ("bf16", "int8")
    base = {mine_negatives: ["--rule", "topk", "--dataset", "x", "--output_dir", "o"],
            consistency_filter: ["--output_dir", "o"]}
    for tool, argv in base.items():
        ap = tool.build_parser()
        args = ap.parse_args(argv)
        assert args.ivf_storage == "bf16" and not _common.host_documents(args)
        assert _common.check_search_arguments(ap, args) == {}
        ivf = ["--ivf_lists", "64", "--ivf_nprobe", "4"]
        plain = _common.check_search_arguments(ap, ap.parse_args(argv + ivf + ["--ivf_storage", "bf16"]))
        assert plain == _common.check_search_arguments(ap, ap.parse_args(argv + ivf)) and "ivf_storage" not in plain
        args = ap.parse_args(argv + ivf + ["--ivf_storage", "int8", "--rescore_factor", "2"])
        assert _common.check_search_arguments(ap, args) == {**plain, "ivf_storage": "int8"}
        assert _common.host_documents(args) and args.rescore_factor == 2 and args.storage == "bf16"
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ivf + ["--ivf_storage", "fp8"])
        capsys.readouterr()
        with pytest.raises(SystemExit):                                             # not without --ivf_lists K
            _common.check_search_arguments(ap, ap.parse_args(argv + ["--ivf_storage", "int8"]))
        assert "--ivf_storage needs --ivf_lists" in capsys.readouterr().err
        with pytest.raises(SystemExit):                                             # the tool's own main refuses it too
            tool.main(argv + ["--ivf_storage", "int8"])
        with pytest.raises(SystemExit):                                             # --storage int8 still does not take lists
            _common.check_search_arguments(ap, ap.parse_args(argv + ivf + ["--storage", "int8"]))
        assert "--storage int8 does not go with --ivf_lists" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            _common.check_search_arguments(ap, ap.parse_args(argv + ivf + ["--storage", "int8", "--ivf_storage", "int8"]))
        with pytest.raises(SystemExit):
            _common.check_search_arguments(ap, ap.parse_args(argv + ivf + ["--ivf_storage", "int8", "--coarse", "binary"]))


def test_common_search_refuses_before_any_launch():
    from contrastors_amd.tools import _common

    d, q = np.zeros((4, 64), np.float32), np.zeros((2, 64), np.float32)
    with pytest.raises(ValueError, match="ivf_storage must be one of"):
        _common.search(d, q, 1, "cuda", ivf_lists=2, ivf_storage="fp8")
    with pytest.raises(ValueError, match="ivf_storage goes with ivf_lists"):
        _common.search(d, q, 1, "cuda", ivf_storage="int8")
    with pytest.raises(ValueError, match="ivf_lists"):
        _common.search(d, q, 1, "cuda", coarse="binary", ivf_lists=2, ivf_storage="int8")
    with pytest.raises(ValueError, match="int8"):
        _common.search(d, q, 1, "cuda", ivf_lists=2, storage="int8")                 # still refused
    with pytest.raises(ValueError, match="int8"):
        _common.search(d, q, 1, "cuda", ivf_lists=2, storage="int8", ivf_storage="int8")


def test_fit_sample_is_kmeans_fits_subsample(tmp_path):
    """The rows gathered on the host for the fit are the rows KMeans.fit(x, sample=) draws: the same generator, sorted."""
    from contrastors_amd.tools import _common

    x = np.arange(50 * 64, dtype=np.float32).reshape(50, 64)
    np.save(tmp_path / "x.npy", x)
    mm = np.load(tmp_path / "x.npy", mmap_mode="r")
    assert _common._fit_sample(mm, None) is mm and _common._fit_sample(mm, 50) is mm and _common._fit_sample(mm, 80) is mm
    rows = torch.randperm(50, generator=torch.Generator().manual_seed(0))[:7].sort().values.numpy()
    got = _common._fit_sample(mm, 7, 0)
    assert got.dtype == np.float32 and np.array_equal(got, x[rows])
