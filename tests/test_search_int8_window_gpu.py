"""GPU checks of the windowed int8 top-k kernel (csrc/search.hip: cx_search_int8_window_topk, through _C).  A pair's score is
defined bit for bit by tests/int8_ref.py and the admission rule by tests/search_int8_window_ref.py, so everything is compared
BITWISE: against cx_search_int8_topk over the slice a window names, and against the numpy reference.  Operands come as code
pairs: random codes in [-127, 127] with distinct random positive scales (a wrong tile's scales changes bits), or grid codes in
{-1, 0, 1} with scales in {0.5, 1, 2} (exact ties everywhere)."""
import functools

import numpy as np
import pytest
import torch

from tests import search_int8_window_ref as IW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
WRAP = 1 << 32


@functools.lru_cache(maxsize=None)
def _coded(n, d, seed):
    """Random codes, distinct positive scales (host arrays, shared: nobody writes into them)."""
    g = np.random.default_rng(seed)
    c = g.integers(-127, 128, (n, d), dtype=np.int8)
    s = (g.permutation(n).astype(F32) + F32(1)) * F32(2.0 ** -12) + g.uniform(1e-3, 2e-3, n).astype(F32)
    return c, s


@functools.lru_cache(maxsize=None)
def _grid(n, d, seed):
    g = np.random.default_rng(seed)
    return g.integers(-1, 2, (n, d), dtype=np.int8), g.choice(np.array([0.5, 1, 2], F32), n)


def _dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i64(x):
    return None if x is None else torch.as_tensor(x, dtype=torch.int64).to(DEV).contiguous()


def _csr(exclude):
    if exclude is None:
        return None, None
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(e) for e in exclude])]), dtype=torch.int64, device=DEV)
    ids = torch.tensor([i for e in exclude for i in e] or [0], dtype=torch.int64, device=DEV)
    return ptr, ids


def win8(qc, qs, dc, ds, k, min_id=None, end_id=None, exclude=None, below=None, out=None, ws_fill=None):
    """cx_search_int8_window_topk on code pairs (host arrays or device tensors) -> (rc, scores, ids)."""
    from contrastors_amd import _C

    h = _C.lib()
    qc, qs, dc, ds = _dev(qc), _dev(qs), _dev(dc), _dev(ds)
    M, N, d = qc.shape[0], dc.shape[0], qc.shape[1]
    mid, end = _i64(min_id), _i64(end_id)
    xptr, xids = _csr(exclude)
    bel = None if below is None else torch.as_tensor(below, dtype=torch.float32).to(DEV).contiguous()
    ws = torch.empty(max(16, h.cx_search_int8_window_ws_bytes(M, k)), dtype=torch.uint8, device=DEV)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    s, i = out if out is not None else (torch.empty(M, max(k, 1), dtype=torch.float32, device=DEV),
                                        torch.empty(M, max(k, 1), dtype=torch.int64, device=DEV))
    rc = h.cx_search_int8_window_topk(qc.data_ptr() if M else None, dc.data_ptr() if N else None, qs.data_ptr() if M else None,
                                      ds.data_ptr() if N else None, M, N, d, qc.stride(0) if M else d,
                                      dc.stride(0) if N else d, k, _C.ptr(mid), _C.ptr(end), _C.ptr(xptr), _C.ptr(xids),
                                      _C.ptr(bel), ws.data_ptr(), s.data_ptr(), i.data_ptr(), _C.cur_stream())
    torch.cuda.synchronize()
    return rc, s, i


def flat8(qc, qs, dc, ds, k, exclude=None, below=None):
    """cx_search_int8_topk through Int8FlatIndex on device code pairs."""
    from contrastors_amd.search import Int8FlatIndex

    ix = Int8FlatIndex(qc.shape[1], device=DEV)
    ix.add((dc, ds))
    return ix.search((qc, qs), k, exclude=exclude, below=below)


def _same(got, want):
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


def _slice_expected(qc, qs, dc, ds, k, windows, rows_of, exclude=None, below=None):
    """Per distinct window (lo, hi): the flat int8 search over D[lo + 1 : hi] by the rows that have it, ids shifted back."""
    M, N = qc.shape[0], dc.shape[0]
    es = torch.full((M, k), -float("inf"), dtype=torch.float32, device=DEV)
    ei = torch.full((M, k), -1, dtype=torch.int64, device=DEV)
    for (lo, hi), rows in zip(windows, rows_of):
        a, b = min(max(lo, -1), N) + 1, min(max(hi, 0), N)
        if not len(rows) or b <= a:
            continue
        rows_t = torch.as_tensor(rows, device=DEV)
        ex = None if exclude is None else [[e - a for e in exclude[r] if a <= e < b] for r in rows]
        s, i = flat8(qc[rows_t], qs[rows_t], dc[a:b], ds[a:b], k, ex, None if below is None else below[rows_t])
        es[rows_t], ei[rows_t] = s, torch.where(i >= 0, i + a, i)
    return es, ei


def _bound_windows(N):
    """Bounds at -3, -1, 0, 1, 127, 128, 129, N - 1, N, N + 500: full, one-id, tile-edge, empty and inverted windows."""
    return [(-1, N), (-3, N + 500), (-3, 1), (0, 128), (0, 129), (1, 127), (126, 128), (127, 129), (127, N), (128, N + 500),
            (129, N - 1), (N - 1, N), (N - 1, N + 500), (-1, 0), (129, 128), (N, N + 500), (0, N)]


@pytest.mark.parametrize("N", [1, 127, 129, 300, 1000])
@pytest.mark.parametrize("d", [64, 192, 320, 1024])
def test_windows_equal_the_flat_int8_search_over_the_slice(d, N):
    dc, ds = (_dev(t) for t in _coded(N, d, 10 + N))
    wins = _bound_windows(N)
    for M in (1, 129, 300):
        qc, qs = (_dev(t) for t in _coded(M, d, 20 + M))
        which = [(3 * r + r // 7) % len(wins) for r in range(M)]           # windows mixed inside every query tile
        mid, end = [wins[w][0] for w in which], [wins[w][1] for w in which]
        rows_of = [[r for r in range(M) if which[r] == w] for w in range(len(wins))]
        for k in (1, 10, 130, 1024):
            want = _slice_expected(qc, qs, dc, ds, k, wins, rows_of)
            rc, s, i = win8(qc, qs, dc, ds, k, mid, end)
            assert rc == 0
            _same((s, i), want)


def test_null_and_full_windows_equal_the_plain_int8_search():
    for N, M, d, k in ((1000, 300, 128, 10), (129, 129, 64, 130), (4097, 130, 320, 100)):
        qc, qs = (_dev(t) for t in _coded(M, d, 1))
        dc, ds = (_dev(t) for t in _coded(N, d, 2))
        g = np.random.default_rng(N)
        exclude = [g.integers(0, N, int(g.integers(0, 4))).tolist() for _ in range(M)]
        es, _ = flat8(qc, qs, dc, ds, k)
        below = es[:, min(k, N) // 2].contiguous()
        for ex, bel in ((None, None), (exclude, below)):
            want = flat8(qc, qs, dc, ds, k, ex, bel)
            for mid, end in ((None, None), ([-1] * M, [N] * M), ([-1] * M, None), (None, [N] * M), ([-9] * M, [N + 9] * M)):
                rc, s, i = win8(qc, qs, dc, ds, k, mid, end, ex, bel)
                assert rc == 0
                _same((s, i), want)


def test_grid_codes_equal_the_reference():
    for N, M, d, k in ((300, 129, 64, 10), (1000, 300, 320, 130), (129, 127, 1024, 1024), (127, 1, 192, 1)):
        qc, qs = _grid(M, d, 3)
        dc, ds = _grid(N, d, 4)
        wins = _bound_windows(N)
        mid = [wins[(5 * r) % len(wins)][0] for r in range(M)]
        end = [wins[(5 * r) % len(wins)][1] for r in range(M)]
        g = np.random.default_rng(M)
        exclude = [g.integers(-1, N + 1, int(g.integers(0, 4))).tolist() for _ in range(M)]
        S = IW.R.scores(qc, qs, dc, ds)
        below = np.quantile(S, 0.9, axis=1, method="nearest").astype(F32)       # ON an attained score: strictness matters
        for ex, bel in ((None, None), (exclude, None), (None, below), (exclude, below)):
            rc, s, i = win8(qc, qs, dc, ds, k, mid, end, ex, bel)
            assert rc == 0
            IW.check((s, i), IW.topk_from_mask(S, IW.admitted(S, mid, end, ex, bel), k))


def test_single_hits_at_the_band_edges():
    """Windows (a, b) with a and b 127, 128 and 129 positions into a tile; the two best documents sit AT a and AT b, outside the
    window, the next best at a + 1 and b - 1, inside it.  The band starts in corpus tile 3 of 8, so the walk starts at t0 = 3 and
    a tile's scales must be those of tile t, not t - t0: document n has the scale 1 + n / 1024."""
    d, N, M = 64, 1024, 130
    qc = np.zeros((M, d), np.int8)
    qc[:, 0] = 1
    qs = np.ones(M, F32)
    ds = (F32(1) + np.arange(N, dtype=F32) / F32(1024))
    for a in (2 * 128 + 127, 3 * 128, 3 * 128 + 1):
        for b in (5 * 128 + 127, 6 * 128, 6 * 128 + 1):
            assert (a + 1) // 128 == 3
            dc = np.zeros((N, d), np.int8)
            dc[a, 0], dc[b, 0], dc[a + 1, 0], dc[b - 1, 0] = 9, 9, 3, 2
            rc, s, i = win8(qc, qs, dc, ds, 3, [a] * M, [b] * M)
            assert rc == 0
            IW.check((s, i), IW.search(qc, qs, dc, ds, 3, [a] * M, [b] * M))
            for r in (0, 127, 128, M - 1):
                assert i[r].tolist() == [a + 1, b - 1, a + 2]
                assert s[r].tolist() == [float(F32(3) * ds[a + 1]), float(F32(2) * ds[b - 1]), 0.0]


def test_empty_clamped_and_beyond_int32_windows():
    """Rows 0 .. 127 live, rows 128 .. 255 a whole tile of empty windows, rows 256 .. 383 live again with bounds far outside the
    corpus and beyond int32 (clamped, never narrowed first)."""
    d, N, M, k = 64, 700, 384, 10
    qc, qs = _coded(M, d, 31)
    dc, ds = _coded(N, d, 32)
    live = [(-1, N), (130, 650), (0, 2), (511, 513), (255, 700)]
    empty = [(5, 6), (7, 7), (9, 3), (N - 1, N), (N, N + 500), (N + 5, N + 900), (-7, 0), (-WRAP, -5), (1 << 40, 1 << 41),
             (N - 1, WRAP + 3)]
    far = [(-(1 << 40), 1 << 40), (-WRAP + 5, WRAP + 3), (-WRAP + 5, 300), (300, WRAP + 3), ((1 << 31) - 700, 1 << 31),
           (-(1 << 31) - 1, (1 << 31) + 5)]
    wins = ([live[r % len(live)] for r in range(128)] + [empty[r % len(empty)] for r in range(128)]
            + [(far + empty[:2])[r % (len(far) + 2)] for r in range(128)])
    mid, end = [w[0] for w in wins], [w[1] for w in wins]
    rc, s, i = win8(qc, qs, dc, ds, k, mid, end)
    assert rc == 0
    IW.check((s, i), IW.search(qc, qs, dc, ds, k, mid, end))
    assert bool((i[128:256] == -1).all()) and bool(torch.isinf(s[128:256]).all())
    assert bool((i[256, :] >= 0).all()) and bool((i[257, :] >= 0).all())          # the far bounds are the full window
    # only empty windows in the whole launch: nothing is walked, everything is padding
    rc, s, i = win8(qc[:130], qs[:130], dc, ds, k, [e[0] for e in (empty * 13)[:130]], [e[1] for e in (empty * 13)[:130]])
    assert rc == 0 and bool((i == -1).all()) and bool(torch.isinf(s).all())


def test_below_and_exclusions_inside_a_window():
    d, N, M, k = 192, 600, 200, 20
    qc, qs = _coded(M, d, 5)
    dc, ds = _coded(N, d, 6)
    wins = [(99, 400), (-1, 130), (255, 600), (300, 310)]
    mid, end = [wins[r % 4][0] for r in range(M)], [wins[r % 4][1] for r in range(M)]
    S = IW.R.scores(qc, qs, dc, ds)
    es, ei = IW.topk_from_mask(S, IW.admitted(S, mid, end), k)
    assert (ei[:, :9] >= 0).all()
    # below relative to the row's sixth attained score inside its window: at it, just above it and just below it
    v = es[:, 5].copy()
    for bel, first in ((v, 6), (np.nextafter(v, F32(np.inf)), 5), (np.nextafter(v, F32(-np.inf)), 6)):
        rc, s, i = win8(qc, qs, dc, ds, k, mid, end, None, bel)
        assert rc == 0
        IW.check((s, i), IW.topk_from_mask(S, IW.admitted(S, mid, end, None, bel), k))
        assert np.array_equal(i[:, 0].cpu().numpy(), ei[:, first])                # (random scores: no ties at the bound)
    # exclusions: the best and the fourth of every row's window, plus ids outside the window and outside the corpus
    exclude = [[int(ei[r, 0]), int(ei[r, 3]), (mid[r] + 500) % N, max(mid[r], 0), N + 3, -1] for r in range(M)]
    for bel in (None, v):
        rc, s, i = win8(qc, qs, dc, ds, k, mid, end, exclude, bel)
        assert rc == 0
        IW.check((s, i), IW.topk_from_mask(S, IW.admitted(S, mid, end, exclude, bel), k))
    rc, s, i = win8(qc, qs, dc, ds, k, mid, end, exclude)
    assert np.array_equal(i[:, 0].cpu().numpy(), ei[:, 1])
    # everything excluded in a one-id window
    rc, s, i = win8(qc[:3], qs[:3], dc, ds, 4, [7, 7, 7], [9, 9, 9], [[8], [], [7, 9]])
    assert i[:, 0].tolist() == [-1, 8, 8] and bool((i[:, 1:] == -1).all()) and bool(torch.isinf(s[0]).all())


def test_pair_rows_sorted_by_list_every_tile_spans_several():
    """The IVF shape: 600 pair rows sorted by the list they probe, 12 lists of uneven length in 3000 rows."""
    d, k = 192, 130
    sizes = [1, 2, 127, 128, 129, 300, 1, 255, 500, 700, 57, 800]
    probed_by = [3, 130, 1, 127, 129, 2, 64, 100, 20, 10, 7, 7]        # rows per list: tiles start and end inside a list's run
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N, M = int(ptr[-1]), sum(probed_by)
    assert (N, M) == (3000, 600)
    wins = [(int(ptr[l]) - 1, int(ptr[l + 1])) for l in range(len(sizes))]
    which = [l for l, c in enumerate(probed_by) for _ in range(c)]
    mid, end = [wins[w][0] for w in which], [wins[w][1] for w in which]
    rows_of = [[r for r in range(M) if which[r] == w] for w in range(len(sizes))]
    qc, qs = (_dev(t) for t in _coded(M, d, 7))
    dc, ds = (_dev(t) for t in _coded(N, d, 8))
    rc, s, i = win8(qc, qs, dc, ds, k, mid, end)
    assert rc == 0
    _same((s, i), _slice_expected(qc, qs, dc, ds, k, wins, rows_of))
    gq, gd = _grid(M, d, 9), _grid(N, d, 10)
    rc, s, i = win8(*gq, *gd, k, mid, end)
    assert rc == 0
    IW.check((s, i), IW.search(*gq, *gd, k, mid, end))


def test_saturated_rows_and_zero_scales():
    """|acc| = 127 * 127 * 1024 = 16 516 096 with both signs, the largest the integer accumulator holds; and scales of zero on
    either side, whose products are signed zeros."""
    d, N, M, k = 1024, 300, 130, 12
    qc, qs = (a.copy() for a in _coded(M, d, 41))
    dc, ds = (a.copy() for a in _coded(N, d, 42))
    qc[0], qc[1], qc[129] = 127, -127, 127
    dc[5], dc[131], dc[299] = 127, -127, 127
    ds[[5, 131, 299]] = 1                                              # (the largest scales: the saturated pairs win)
    acc = IW.R.acc_matrix(qc, dc)
    assert acc[0, 5] == acc[1, 131] == acc[129, 299] == 16516096 and acc[0, 131] == acc[1, 5] == -16516096
    wins = [(-1, N), (4, 132), (130, N), (0, 6)]
    mid, end = [wins[r % 4][0] for r in range(M)], [wins[r % 4][1] for r in range(M)]
    rc, s, i = win8(qc, qs, dc, ds, k, mid, end)
    assert rc == 0
    IW.check((s, i), IW.search(qc, qs, dc, ds, k, mid, end))
    assert i[0, :2].tolist() == [5, 299] and i[1, 0].item() == 131
    # a window of three documents lists them all: the negative saturated pair of row 0 too
    rc, s, i = win8(qc, qs, dc, ds, k, [129] * M, [133] * M)
    assert rc == 0
    IW.check((s, i), IW.search(qc, qs, dc, ds, k, [129] * M, [133] * M))
    assert i[0, 2].item() == 131 and s[0, 2].item() == float(F32(F32(-16516096) * F32(1)) * qs[0]) and i[1, 0].item() == 131
    ds[::3] = 0
    qs[2::5] = 0
    rc, s, i = win8(qc, qs, dc, ds, k, mid, end)
    assert rc == 0
    IW.check((s, i), IW.search(qc, qs, dc, ds, k, mid, end))


def test_workspace_contents_determinism_and_empty_shapes():
    d, N, M, k = 64, 900, 257, 50
    qc, qs = _grid(M, d, 11)
    dc, ds = _grid(N, d, 12)
    g = np.random.default_rng(0)
    mid = g.integers(-3, N, M).tolist()
    end = [a + int(b) for a, b in zip(mid, g.integers(0, 400, M))]
    want = IW.search(qc, qs, dc, ds, k, mid, end)
    for fill in (None, 0xFF, 0x00):                                    # the workspace need not be initialised
        rc, s, i = win8(qc, qs, dc, ds, k, mid, end, ws_fill=fill)
        assert rc == 0
        IW.check((s, i), want)
    rc, s2, i2 = win8(qc, qs, dc, ds, k, mid, end)
    assert torch.equal(s, s2) and torch.equal(i, i2)
    # N = 0: every row is padding (null D and d_scale); M = 0: nothing is written
    rc, s, i = win8(qc, qs, dc[:0], ds[:0], k, mid, end)
    assert rc == 0 and bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool((s < 0).all())
    out = torch.full((4, k), 7.0, device=DEV), torch.full((4, k), -7, dtype=torch.int64, device=DEV)
    rc, s, i = win8(qc[:0], qs[:0], dc, ds, k, None, None, out=out)
    assert rc == 0 and bool((s == 7).all()) and bool((i == -7).all())


def test_refusals_come_before_any_launch():
    """An error code, and the outputs keep what they held."""
    from contrastors_amd import _C

    d, N, M, k = 128, 300, 130, 10
    qc, qs = (_dev(t) for t in _coded(M, d, 51))
    dc, ds = (_dev(t) for t in _coded(N, d, 52))
    mid, end = [0] * M, [N] * M

    def out():
        return torch.full((M, 2048), 7.0, device=DEV), torch.full((M, 2048), -7, dtype=torch.int64, device=DEV)

    def refused(rc, s, i, code):
        return rc == code and bool((s == 7).all()) and bool((i == -7).all())

    SHAPE, ALIGN, ARG = -1, -2, -3
    for kk in (0, 1025):
        assert refused(*win8(qc, qs, dc, ds, kk, mid, end, out=out()), SHAPE)
    assert refused(*win8(qc[:, :32], qs, dc[:, :32], ds, k, mid, end, out=out()), SHAPE)             # d = 32
    assert refused(*win8(qc[:, :96], qs, dc[:, :96], ds, k, mid, end, out=out()), SHAPE)             # d = 96
    wide = torch.zeros(M, 1088, dtype=torch.int8, device=DEV)
    assert refused(*win8(wide, qs, wide, qs, k, mid[:M], end[:M], out=out()), SHAPE)                 # d = 1088
    odd = torch.zeros(M, d + 8, dtype=torch.int8, device=DEV)[:, :d]                                  # a stride of 136 bytes
    assert refused(*win8(odd, qs, dc, ds, k, mid, end, out=out()), ALIGN)
    assert refused(*win8(qc, qs, odd, qs, k, mid, end, out=out()), ALIGN)
    off = torch.zeros(M * d + 16, dtype=torch.int8, device=DEV)[8: 8 + M * d].view(M, d)              # 8-byte aligned only
    assert refused(*win8(off, qs, dc, ds, k, mid, end, out=out()), ALIGN)
    assert refused(*win8(qc, qs, off, qs, k, mid, end, out=out()), ALIGN)
    h = _C.lib()
    ws = torch.empty(h.cx_search_int8_window_ws_bytes(M, k), dtype=torch.uint8, device=DEV)
    s, i = out()
    base = [qc.data_ptr(), dc.data_ptr(), qs.data_ptr(), ds.data_ptr(), M, N, d, d, d, k, None, None, None, None, None,
            ws.data_ptr(), s.data_ptr(), i.data_ptr(), _C.cur_stream()]
    for arg in (0, 1, 2, 3, 15, 16, 17):                                                              # a null pointer each
        a = list(base)
        a[arg] = None
        assert h.cx_search_int8_window_topk(*a) == ARG, arg
    a = list(base)
    a[12] = torch.zeros(M + 1, dtype=torch.int64, device=DEV).data_ptr()                              # excl_ptr without ids
    assert h.cx_search_int8_window_topk(*a) == ARG
    a = list(base)
    a[5] = (1 << 31) - 128                                                                            # N past the int columns
    assert h.cx_search_int8_window_topk(*a) == SHAPE
    a = list(base)
    a[4] = -1
    assert h.cx_search_int8_window_topk(*a) == SHAPE
    torch.cuda.synchronize()
    assert bool((s == 7).all()) and bool((i == -7).all())
