"""CPU checks of the IVF-PQ index: the residual of tests/ivf_pq_ref.py against scalar loops, the Python refusals (all before a
launch), the new C entries in the header / ctypes table / library and their refusals before any pointer is touched."""
import re
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ivf_pq_ref as V
from tests import pq_ref as R

HDR = Path(__file__).resolve().parent.parent / "include" / "contrastors_hip.h"
NEW = {"cx_pq_assign_residual", "cx_search_pq_window_ws_bytes", "cx_search_pq_window_topk"}
SHAPE, ALIGN, ARG = -1, -2, -3


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]            # one rounding to nearest even from the exact double


def _bf16(v):
    u = struct.unpack("I", struct.pack("f", v))[0]
    return struct.unpack("f", struct.pack("I", ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16))[0]


def test_residual_equals_scalar_loops():
    rng = np.random.default_rng(7)
    x = R.to_bf16(rng.standard_normal((5, 64)).astype(np.float32))
    c = R.to_bf16(rng.standard_normal((3, 64)).astype(np.float32))
    x[0, 0], c[0, 0] = 1.0, 2.0 ** -20 * 1.0078125               # 1 - c needs 28 bits: inexact in fp32
    x[0, 1], c[0, 1] = 1.0, -2.0 ** -8                           # 1 + 2^-8: a bf16 tie, to the even 1.0
    x[0, 2], c[0, 2] = 1.0 + 2.0 ** -7, -2.0 ** -8               # ... and to the even 1 + 2^-6
    labels = np.array([0, 1, 2, 0, 1])
    got = V.residual(x, c[labels])
    # bf16 operands make the double difference exact, so _f32 is the single rounding of the fp32 subtraction
    want = np.array([[_bf16(_f32(float(x[i, j]) - float(c[labels[i], j]))) for j in range(64)] for i in range(5)], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert float(x[0, 0]) - float(c[0, 0]) != got[0, 0] and got[0, 1] == 1.0 and got[0, 2] == 1.0 + 2.0 ** -6
    assert not np.array_equal(got, V.residual(x, c[(labels + 1) % 3]))          # the wrong centroid row differs


def test_python_refusals_come_before_any_launch():
    from contrastors_amd.search import IVFPQIndex, _IVFLists, search_ivf_pq_rescored

    assert issubclass(IVFPQIndex, _IVFLists) and "_finalise" not in vars(IVFPQIndex)
    for args, match in (((64, 4, 4), "dsub"), ((64, 4, 12), "dsub"), ((64, 4, 128), "dsub"), ((96, 4), "multiple of 64"),
                        ((64, 0), "nlist")):
        with pytest.raises(ValueError, match=match):
            IVFPQIndex(*args)
    with pytest.raises(RuntimeError, match="GPU"):
        IVFPQIndex(64, 4, device="cpu")
    ix = IVFPQIndex(768, 8, workspace_bytes=1 << 24)
    assert ix.m == 96 and ix.by_residual and not ix.is_trained and ix._pair_row_bytes() == 1540
    assert ix.batch_queries(10 ** 6, 10, 8) == (1 << 24) // (8 * (200 + 4 + 1540 + 32)) // 128 * 128
    q, none = np.zeros((3, 64), np.float32), np.zeros((0, 64), np.float32)
    ix = IVFPQIndex(64, 4)
    for call in (lambda: ix.search(q, 1, 1), lambda: ix.add(q), lambda: ix.decode(), lambda: ix.list_sizes,
                 lambda: search_ivf_pq_rescored(ix, none, q, 1, 1)):
        with pytest.raises(RuntimeError, match="train"):
            call()
    big, cen = np.zeros((300, 64), np.float32), np.zeros((4, 64))
    for kw, match in ((dict(), "give the training rows"), (dict(centroids=cen), "give the training rows"),
                      (dict(x=np.zeros((300, 32))), r"\(n, 64\)"), (dict(x=big, centroids=np.zeros((5, 64))), "centroids"),
                      (dict(centroids=cen, codebooks=np.zeros((8, 256, 16))), "codebooks"), (dict(x=big, pq_sample=100), "pq_sample"),
                      (dict(x=big[:200]), "at least 256"), (dict(x=big, pq_iters=-1), "pq_iters")):
        with pytest.raises(ValueError, match=match):
            ix.train(**kw)
    assert not ix.is_trained
    ix._centroids, ix.pq._shadow = torch.zeros(4, 64), torch.zeros(8, 256, 8, dtype=torch.bfloat16)   # "trained", no device
    for kw, match in ((dict(k=0), "k must be"), (dict(k=1025), "k must be"), (dict(nprobe=0), "nprobe"), (dict(nprobe=5), "nprobe"),
                      (dict(queries=np.zeros((3, 128), np.float32)), r"\(n, 64\)"), (dict(below=np.zeros(2)), "below has 2 entries"),
                      (dict(exclude=[[1], [2]]), "rows for 3 queries")):
        for call in (ix.search, lambda **a: search_ivf_pq_rescored(ix, none, **a)):
            with pytest.raises(ValueError, match=match):
                call(**{**dict(queries=q, k=1, nprobe=1), **kw})
    with pytest.raises(ValueError, match=r"\(n, 64\)"):
        ix.add(np.zeros((3, 128), np.float32))
    with pytest.raises(ValueError, match="rescore_factor"):
        search_ivf_pq_rescored(ix, none, q, 1, 1, rescore_factor=0)
    with pytest.raises(ValueError, match="10 vectors for an index of 0"):
        search_ivf_pq_rescored(ix, np.zeros((10, 64)), q, 1, 1)
    assert ix.ntotal == 0


def test_new_entries_are_declared_exported_and_refuse_before_touching_pointers():
    from contrastors_amd import _C, build

    build.build()
    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", HDR.read_text()))
    assert NEW <= declared and declared == set(_C.EXPORTED_SYMBOLS)
    lib = _C.lib()
    assert lib.cx_abi_version() == 10 and all(hasattr(lib, n) for n in NEW)
    for args in ((128, 10), (1000, 1024), (0, 10), (5, 0)):
        assert lib.cx_search_pq_window_ws_bytes(*args) == lib.cx_search_window_ws_bytes(*args)
    p = 4096                                                     # never dereferenced: every call below is refused first

    def search(M=1, N=10, d=64, dsub=8, k=1, Q=p, codes=p, cb=p, ldq=64, ldc=8, bias=None, xptr=None, ws=p, out=p):
        return lib.cx_search_pq_window_topk(Q, codes, cb, M, N, d, dsub, ldq, ldc, k, None, None, bias, xptr, None, None, ws, out,
                                            out, None)

    def assign(n=4, d=64, dsub=8, X=p, lab=p, cen=p, nlist=3, ldx=64, ldcen=64, sh=p, hn=p, codes=p, ldc=8):
        return lib.cx_pq_assign_residual(X, n, d, ldx, lab, cen, nlist, ldcen, sh, hn, dsub, codes, ldc, None)

    for kw in (dict(d=96), dict(d=32), dict(d=1088), dict(k=0), dict(k=1025), dict(dsub=4), dict(dsub=12), dict(dsub=128),
               dict(M=-1), dict(N=-1), dict(N=2 ** 31 - 128)):
        assert search(**kw) == SHAPE, kw
    for kw in (dict(d=96), dict(dsub=24), dict(n=-1), dict(nlist=0)):
        assert assign(**kw) == SHAPE, kw
    # M = 0 / n = 0: nothing to do, nothing is read
    assert search(M=0, Q=None, codes=None, cb=None, ws=None, out=None) == 0
    assert assign(n=0, X=None, lab=None, cen=None, sh=None, hn=None, codes=None) == 0
    for kw in (dict(Q=None), dict(codes=None), dict(cb=None), dict(ws=None), dict(out=None), dict(xptr=p)):
        assert search(**kw) == ARG, kw
    for name in ("X", "lab", "cen", "sh", "hn", "codes"):
        assert assign(**{name: None}) == ARG, name
    for kw in (dict(ldq=60), dict(ldq=68), dict(ldc=7), dict(Q=p + 8), dict(cb=p + 8), dict(ws=p + 8), dict(bias=p + 2)):
        assert search(**kw) == ALIGN, kw
    for kw in (dict(ldx=63), dict(ldcen=63), dict(ldc=7), dict(X=p + 1), dict(cen=p + 1), dict(lab=p + 2), dict(sh=p + 8),
               dict(hn=p + 2)):
        assert assign(**kw) == ALIGN, kw
