"""cx_search_hamming_window_topk and cx_hamming_merge_lists against tests/ivf_binary_ref.py, by equality (everything is an
integer)."""
import numpy as np
import pytest
import torch

from tests import ivf_binary_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(DEV, dtype).contiguous()


def window(Q, D, k, mid=None, end=None, exclude=None, max_dist=None):
    """numpy codes Q (M, nb), D (N, nb) -> numpy (dist, ids) of cx_search_hamming_window_topk."""
    from contrastors_amd import _C

    h = _C.lib()
    M, N, nb = Q.shape[0], D.shape[0], Q.shape[1]
    xptr = xids = None
    if exclude is not None:
        xptr = _dev(np.cumsum([0] + [len(e) for e in exclude]), torch.int64)
        xids = _dev(np.concatenate([np.asarray(e, np.int64) for e in exclude] + [np.zeros(1, np.int64)]), torch.int64)
    q, dd = _dev(Q, torch.uint8), _dev(D, torch.uint8)
    mid, end, md = _dev(mid, torch.int64), _dev(end, torch.int64), _dev(max_dist, torch.int32)
    ws = torch.empty(h.cx_search_hamming_window_ws_bytes(M, k) + 16, dtype=torch.uint8, device=DEV)
    d = torch.empty(M, k, dtype=torch.int32, device=DEV)
    i = torch.empty(M, k, dtype=torch.int64, device=DEV)
    _C.check(h.cx_search_hamming_window_topk(_C.ptr(q) if M else None, _C.ptr(dd) if N else None, M, N, nb * 8, nb, nb, k,
                                             _C.ptr(mid), _C.ptr(end), _C.ptr(xptr), _C.ptr(xids), _C.ptr(md), ws.data_ptr(),
                                             d.data_ptr(), i.data_ptr(), _C.cur_stream()))
    return d.cpu().numpy(), i.cpu().numpy()


def make(M, N, d):
    """Codes a few bits apart from one base code, so distances are small and tie all the time; rows 1 and N - 1 repeat row 0."""
    rng = np.random.default_rng(1000 * M + N + d)
    base = rng.integers(0, 256, d // 8, dtype=np.uint8)
    flip = lambda n: np.packbits(rng.random((n, d)) < 6 / d, axis=1)
    Q, D = base ^ flip(M), base ^ flip(N)
    if N:
        D[1 % N], D[N - 1] = D[0], D[0]
    return Q, D


def windows(M, N):
    """Query tile 0 mixes every kind of window, the ends of the corpus among them; tile 1 (rows 128 - 255) is all empty; the
    rows after it are random."""
    rng = np.random.default_rng(M + N)
    kinds = [(5, 5), None, (126, 130), (-1, N), (-7, N + 50), (-1, 3), (N - 4, N), (N + 3, N + 9), (40, 300)]
    mid, end = rng.integers(-3, N + 3, M), rng.integers(-3, N + 3, M)
    for r in range(min(M, 256)):
        kind = kinds[(r + M) % len(kinds)] if r < 128 else (r, r)
        mid[r], end[r] = kind if kind is not None else (r % N - 1, r % N + 1)          # one row
    return mid.astype(np.int64), end.astype(np.int64)


@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("N", [1, 127, 129, 300, 1000])
@pytest.mark.parametrize("M", [1, 129, 300])
def test_window_max_dist_exclude_against_the_reference(M, N, d):
    Q, D = make(M, N, d)
    dist = B.hamming(Q, D)
    mid, end = windows(M, N)
    for k in (1, 10, 200):
        assert B.same(window(Q, D, k, mid, end), B.window_topk(dist, k, mid, end)), k
    assert B.same(window(Q, D, 10), B.window_topk(dist, 10))                              # NULL windows: the whole corpus
    # max_dist at, just below and far below the row's 3rd nearest distance, and negative; the top hit excluded
    third = np.sort(dist, 1)[:, min(2, N - 1)]
    md = (third + np.array([0, -1, -1000, -10 ** 6])[np.arange(M) % 4]).astype(np.int32)
    top = B.window_topk(dist, 1, mid, end)[1][:, 0]
    exclude = [[t] if t >= 0 else [] for t in top]
    assert B.same(window(Q, D, 10, mid, end, exclude, md), B.window_topk(dist, 10, mid, end, exclude, md))
    if M > 1 and N > 128:                                         # NULL windows: the flat kernel's result at any nsplit
        from contrastors_amd.search import BinaryFlatIndex

        ix = BinaryFlatIndex(d, device=DEV)
        ix.add(D)
        for nsplit in (1, 3):
            assert B.same(window(Q, D, 10, max_dist=md), ix.search(Q, 10, max_dist=md, nsplit=nsplit))


def test_constant_ties_overflow_the_pending_buffer():
    rng = np.random.default_rng(8)
    eight = rng.integers(0, 256, (8, 24), dtype=np.uint8)
    D = np.tile(eight, (125, 1))                                  # 1000 rows: every distance 125 times
    Q = np.concatenate([eight, rng.integers(0, 256, (122, 24), dtype=np.uint8)])
    dist = B.hamming(Q, D)
    mid, end = np.full(130, -1, np.int64), np.full(130, 1000, np.int64)
    mid[1::3], end[2::3] = 333, 801                               # windows that start / end inside a run of ties
    assert B.same(window(Q, D, 200, mid, end), B.window_topk(dist, 200, mid, end))
    assert B.same(window(Q, D, 200), B.window_topk(dist, 200))


@pytest.mark.parametrize("M, N", [(0, 300), (5, 0)])
def test_empty_operands(M, N):
    Q, D = make(M, N, 64)
    gd, gi = window(Q, D, 7)
    assert gd.shape == (M, 7) and np.all(gd == 2 ** 31 - 1) and np.all(gi == -1)


def test_merge_lists_ranks_by_the_mapped_id():
    from contrastors_amd import _C

    pad = 2 ** 31 - 1
    # positions 0 - 5 report ids 7, 9, 2, 4, 1, 8: each list is sorted by (distance, reported id)
    id_map = np.array([7, 9, 2, 4, 1, 8], np.int64)
    dist = np.array([[3, 3, pad, pad], [3, 3, 5, pad], [1, pad, pad, pad], [pad] * 4], np.int32)
    ids = np.array([[0, 1, -1, -1], [2, 3, 4, -1], [5, -1, -1, -1], [-1] * 4], np.int64)
    src = np.array([[0, 1, 2], [1, 7, 0], [3, -1, 2], [3, 3, 3]], np.int64)           # 7 and -1 name no list
    want_d = np.array([[1, 3, 3, 3], [3, 3, 3, 3], [1, pad, pad, pad], [pad] * 4], np.int32)
    want_i = np.array([[8, 2, 4, 7], [2, 4, 7, 9], [8, -1, -1, -1], [-1] * 4], np.int64)
    od = torch.empty(4, 4, dtype=torch.int32, device=DEV)
    oi = torch.empty(4, 4, dtype=torch.int64, device=DEV)
    td, ti, ts, tm = _dev(dist, torch.int32), _dev(ids, torch.int64), _dev(src, torch.int64), _dev(id_map, torch.int64)
    _C.check(_C.lib().cx_hamming_merge_lists(td.data_ptr(), ti.data_ptr(), 4, 4, ts.data_ptr(), 4, 3, tm.data_ptr(), 6,
                                             od.data_ptr(), oi.data_ptr(), _C.cur_stream()))
    assert np.array_equal(od.cpu().numpy(), want_d) and np.array_equal(oi.cpu().numpy(), want_i)
