"""CPU checks of the IVF index over sign codes: tests/ivf_binary_ref.py against scalar loops and brute force, the Python
refusals (all before a launch), the new C entries in the header / ctypes table / library and their refusals before any pointer
is touched."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ivf_binary_ref as B

HDR = Path(__file__).resolve().parent.parent / "include" / "contrastors_hip.h"
NEW = {"cx_search_hamming_window_ws_bytes", "cx_search_hamming_window_topk", "cx_hamming_merge_lists",
       "cx_binary_kmeans_update_ws_bytes", "cx_binary_kmeans_update"}
SHAPE, ALIGN, ARG = -1, -2, -3


def test_update_equals_a_scalar_loop():
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 256, (9, 8), dtype=np.uint8)
    codes[:4] = np.array([0, 0, 255, 255], np.uint8)[:, None]        # list 0: a tie on every bit but bit 0
    codes[:4, 0] = 0x80, 0x80, 0xFF, 0x7F                            # ... which 3 of 4 members have
    labels = np.array([0, 0, 0, 0, 2, 2, 2, 3, 3])                   # list 1 is empty
    cen = rng.integers(0, 256, (4, 8), dtype=np.uint8)
    got, sizes = B.update(codes, labels, cen)
    want = cen.copy()
    for l in (0, 2, 3):
        rows = [i for i in range(9) if labels[i] == l]
        for b in range(64):
            ones = sum((int(codes[i, b // 8]) >> (7 - b % 8)) & 1 for i in rows)
            want[l, b // 8] = (int(want[l, b // 8]) & ~(1 << (7 - b % 8))) | (int(2 * ones > len(rows)) << (7 - b % 8))
    assert np.array_equal(got, want) and sizes.tolist() == [4, 0, 3, 2] and np.array_equal(got[1], cen[1])
    assert got[0, 0] == 0x80 and not got[0, 1:].any()                # bit 0 is bit 7 of byte 0; 2 * ones == size gives 0
    assert B.assign(np.array([[1, 0], [0, 0]], np.uint8), np.array([[0, 1], [1, 0], [0, 0], [0, 0]], np.uint8)).tolist() == [1, 2]


def test_search_equals_brute_force():
    rng = np.random.default_rng(5)
    codes, cen, q = (rng.integers(0, 4, (n, 8), dtype=np.uint8) for n in (60, 5, 7))               # few distinct bits: ties
    dist = np.array([[bin(int.from_bytes(bytes(a ^ b), "big")).count("1") for b in codes] for a in q], np.int32)
    assert np.array_equal(B.hamming(q, codes), dist)
    labels, cdist = B.assign(codes, cen), B.hamming(q, cen)
    exclude = [[int(np.argmin(dist[m]))] for m in range(7)]
    gd, gi = B.ivf_search(q, codes, cen, 9, 2, exclude=exclude, max_dist=np.full(7, 6))
    for m in range(7):
        probes = np.lexsort((np.arange(5), cdist[m]))[:2]
        ids = np.array([n for n in range(60) if labels[n] in probes and n not in exclude[m] and dist[m, n] <= 6], np.int64)
        ids = ids[np.lexsort((ids, dist[m, ids]))][:9]
        assert np.array_equal(gi[m, : ids.size], ids) and np.array_equal(gd[m, : ids.size], dist[m, ids])
        assert np.all(gi[m, ids.size:] == -1) and np.all(gd[m, ids.size:] == 2 ** 31 - 1)
    assert B.same(B.ivf_search(q, codes, cen, 9, 5), B.window_topk(dist, 9))


def test_python_refusals_come_before_any_launch():
    from contrastors_amd.search import IVFBinaryIndex, _IVFLists, search_ivf_binary_rescored

    assert issubclass(IVFBinaryIndex, _IVFLists) and not {"_finalise", "_push", "reset"} & set(vars(IVFBinaryIndex))
    for args, match in (((96, 4), "multiple of 64"), ((1088, 4), "multiple of 64"), ((64, 0), "nlist")):
        with pytest.raises(ValueError, match=match):
            IVFBinaryIndex(*args)
    with pytest.raises(RuntimeError, match="GPU"):
        IVFBinaryIndex(64, 4, device="cpu")
    ix = IVFBinaryIndex(768, 8, workspace_bytes=1 << 24)
    assert not ix.is_trained and ix._pair_row_bytes() == 100
    assert ix.batch_queries(10 ** 6, 10, 8) == (1 << 24) // (8 * (200 + 4 + 100 + 32)) // 128 * 128
    q, qc, none = np.zeros((3, 64), np.float32), np.zeros((3, 8), np.uint8), np.zeros((0, 64), np.float32)
    ix = IVFBinaryIndex(64, 4)
    for call in (lambda: ix.search(q, 1, 1), lambda: ix.add(q), lambda: ix.list_sizes, lambda: ix.centroids,
                 lambda: search_ivf_binary_rescored(ix, none, q, 1, 1)):
        with pytest.raises(RuntimeError, match="train"):
            call()
    big, u8 = np.zeros((300, 64), np.float32), lambda *s: np.zeros(s, np.uint8)
    for kw, match in ((dict(), "either the training rows"), (dict(x=big, centroids=u8(4, 8)), "either the training rows"),
                      (dict(x=np.zeros((300, 32))), r"\(n, 64\)"), (dict(x=u8(300, 64)), r"\(n, 8\) uint8"),
                      (dict(centroids=u8(5, 8)), "centroids"), (dict(centroids=np.zeros((4, 8))), "centroids"),
                      (dict(x=big, sample=100), "sample"), (dict(x=big, sample=1 << 19), "sample"),
                      (dict(x=big[:3]), "at least 4"), (dict(x=big, max_iter=-1), "max_iter")):
        with pytest.raises(ValueError, match=match):
            ix.train(**kw)
    assert not ix.is_trained
    ix._centroids = torch.zeros(4, 8, dtype=torch.uint8)             # "trained", no device
    both = (ix.search, lambda **a: search_ivf_binary_rescored(ix, none, **a))
    for kw, match, calls in ((dict(k=0), "k must be", both), (dict(k=1025), "k must be", both), (dict(nprobe=0), "nprobe", both),
                             (dict(nprobe=5), "nprobe", both), (dict(queries=np.zeros((3, 128), np.float32)), r"\(n, 64\)", both),
                             (dict(exclude=[[1], [2]]), "rows for 3 queries", both),
                             (dict(queries=u8(3, 64)), r"\(n, 8\) uint8", both[:1]), (dict(max_dist=np.zeros(2)), "max_dist has 2", both[:1]),
                             (dict(queries=qc), "float queries", both[1:]), (dict(rescore_factor=0), "rescore_factor", both[1:]),
                             (dict(below=np.zeros(2)), "below has 2", both[1:])):
        for call in calls:
            with pytest.raises(ValueError, match=match):
                call(**{**dict(queries=q, k=1, nprobe=1), **kw})
    for x in (np.zeros((3, 128), np.float32), u8(3, 9)):
        with pytest.raises(ValueError, match="expected"):
            ix.add(x)
    with pytest.raises(ValueError, match="10 vectors for an index of 0"):
        search_ivf_binary_rescored(ix, np.zeros((10, 64)), q, 1, 1)
    assert ix.ntotal == 0


def test_new_entries_are_declared_exported_and_refuse_before_touching_pointers():
    from contrastors_amd import _C, build

    build.build()
    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", HDR.read_text()))
    assert NEW <= declared and declared == set(_C.EXPORTED_SYMBOLS)
    lib = _C.lib()
    assert lib.cx_abi_version() == 10 and all(hasattr(lib, n) for n in NEW)
    for args in ((128, 10), (1000, 1024), (0, 10), (5, 0)):
        assert lib.cx_search_hamming_window_ws_bytes(*args) == lib.cx_search_hamming_ws_bytes(args[0], 1, args[1], 1)
    assert lib.cx_binary_kmeans_update_ws_bytes(1000, 192, 16) >= 4 * (16 * 192 + 3 * 16 + 2 + 1000)
    assert lib.cx_binary_kmeans_update_ws_bytes(0, 192, 16) == 0
    p = 4096                                                     # never dereferenced: every call below is refused first

    def search(M=1, N=10, d=64, k=1, Q=p, D=p, ldq=8, ldd=8, xptr=None, ws=p, out=p):
        return lib.cx_search_hamming_window_topk(Q, D, M, N, d, ldq, ldd, k, None, None, xptr, None, None, ws, out, out, None)

    def merge(M=1, P=2, k=1, L=1, dist=p, ids=p, src=p, id_map=None, N=0, out=p):
        return lib.cx_hamming_merge_lists(dist, ids, P, k, src, M, L, id_map, N, out, out, None)

    def update(n=4, d=64, ldc=8, nlist=3, codes=p, lab=p, ws=p, cen=p, sizes=p):
        return lib.cx_binary_kmeans_update(codes, n, d, ldc, lab, nlist, ws, cen, sizes, None)

    for fn, code, cases in (
            (search, SHAPE, (dict(d=96), dict(d=32), dict(d=1088), dict(k=0), dict(k=1025), dict(M=-1), dict(N=-1), dict(N=2 ** 31 - 128))),
            (merge, SHAPE, (dict(M=-1), dict(P=-1), dict(k=0), dict(k=1025), dict(L=0), dict(L=257), dict(id_map=p, N=0))),
            (update, SHAPE, (dict(d=96), dict(d=1088), dict(n=-1), dict(n=2 ** 31), dict(nlist=0))),
            # M = 0 / n = 0: nothing to do, nothing is read
            (search, 0, (dict(M=0, Q=None, D=None, ws=None, out=None),)),
            (merge, 0, (dict(M=0, dist=None, ids=None, src=None, out=None),)),
            (update, 0, (dict(n=0, codes=None, lab=None, ws=None, cen=None, sizes=None),)),
            (search, ARG, (dict(Q=None), dict(D=None), dict(ws=None), dict(out=None), dict(xptr=p))),
            (merge, ARG, (dict(dist=None), dict(ids=None), dict(src=None), dict(out=None))),
            (update, ARG, (dict(codes=None), dict(lab=None), dict(ws=None), dict(cen=None), dict(sizes=None))),
            (search, ALIGN, (dict(ldq=4), dict(ldq=12), dict(ldd=4), dict(ldd=12), dict(Q=p + 4), dict(D=p + 4), dict(ws=p + 8))),
            (update, ALIGN, (dict(ldc=4), dict(ldc=12), dict(codes=p + 4), dict(lab=p + 2), dict(ws=p + 8), dict(sizes=p + 2)))):
        for kw in cases:
            assert fn(**kw) == code, (fn.__name__, kw)
