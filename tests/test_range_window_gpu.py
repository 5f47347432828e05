"""GPU checks of the windowed range search (cx_range_window_count / cx_range_window_emit via FlatIPIndex.range_count /
range_search(end_id=...) and the C ABI): lims, ids and scores equal to the float64 reference bit for bit on operands whose fp32
accumulation is exact, windows at every tile edge (mixed within a query tile, constant per tile, empty, a whole tile of empty
ones), bit equality with the unwindowed kernel, radius -inf / NaN, hits in the first / last / partial last tile of the band,
independence of split count / query batching / run, an uninitialised workspace, a band description that understates the
windows, the refusals, and the label-sorted self-join (tests/range_window_ref.py)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import range_ref as R
from tests import range_window_ref as W
from tests.test_range_search_gpu import _grid_operands, _index, _mixed_radii, _same, _unit_operands

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 127, 129, 300, 1000]


def _edges(N):
    return [-3, -1, 0, 1, 127, 128, 129, N - 1, N, N + 500]


def _windows(kind, M, N):
    """(min_id, end_id) int64 (M,).  mixed: every pairing of the edge values inside every query tile (empty and inverted
    windows among them); per_tile: one window per 128-row query tile; dead_tile: mixed, but the rows of the LAST query tile
    all have empty windows."""
    e = _edges(N)
    m = torch.arange(M)
    if kind == "per_tile":
        t = m // 128
        return torch.tensor(e)[t % len(e)], torch.tensor(e)[(3 * t + 7) % len(e)]
    mid, end = torch.tensor(e)[m % len(e)], torch.tensor(e)[(m // len(e) + m) % len(e)]
    if kind == "dead_tile":
        last = m >= (M - 1) // 128 * 128
        end = torch.where(last, mid.clamp(min=-1) + 1 - (m % 3), end)      # end <= min_id + 1
    return mid, end


@functools.lru_cache(maxsize=None)
def _case(kind, M, N, d):
    """Operands, radii and the index, made once per case and shared (never modified)."""
    if kind == "unit":
        Q, D = _unit_operands(M, N, d)
        rad = torch.full((M,), 2.0 / math.sqrt(d), dtype=torch.float32, device=DEV)
    else:
        Q, D = _grid_operands(M, N, d, 8 if kind == "grid8" else 2, 1000 * M + N + d)
        rad = _mixed_radii(R.scores64(Q, D))
    return dict(Q=Q, D=D, rad=rad, ix=_index(D))


def _filtered(res, end, N):
    """An unwindowed result (lims, scores, ids) cut to id < end_id[row]."""
    lims, scores, ids = res
    M = lims.numel() - 1
    rows = torch.repeat_interleave(torch.arange(M, device=ids.device), lims[1:] - lims[:-1])
    keep = ids < end.to(ids.device).clamp(0, N)[rows]
    out = torch.zeros(M + 1, dtype=torch.int64, device=ids.device)
    out[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=M), 0)
    return out, scores[keep], ids[keep]


# ---- 1. exact operands: bit for bit, every row --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("M", SIZES)
def test_window_exact_grid(M, N):
    d = 320 if (M, N) in ((300, 1000), (129, 129)) else 64
    c = _case("grid8" if (M + N) % 2 else "grid2", M, N, d)
    admitted = 0
    for kind in ("mixed", "per_tile", "dead_tile"):
        mid, end = _windows(kind, M, N)
        got = c["ix"].range_search(c["Q"], c["rad"], min_id=mid, end_id=end)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
        W.check_exact(c["Q"], c["D"], c["rad"], mid, end, *got)
        assert torch.equal(c["ix"].range_count(c["Q"], c["rad"], min_id=mid, end_id=end), got[0][1:] - got[0][:-1])
        if kind == "dead_tile":
            t0 = (M - 1) // 128 * 128
            assert int(got[0][-1] - got[0][t0]) == 0
        admitted += got[2].numel()
    assert admitted > 0 or min(M, N) == 1


def test_window_constant_edges_and_no_min_id():
    """One value of end_id for all rows, at every edge, with and without min_id; numpy in, numpy out."""
    M, N = 300, 1000
    c = _case("grid2", M, N, 64)
    for v in _edges(N):
        end = torch.full((M,), v)
        got = c["ix"].range_search(c["Q"], c["rad"], end_id=end)
        W.check_exact(c["Q"], c["D"], c["rad"], None, end, *got)
        got = c["ix"].range_search(c["Q"], c["rad"], min_id=torch.full((M,), 126), end_id=end)
        W.check_exact(c["Q"], c["D"], c["rad"], torch.full((M,), 126), end, *got)
    mid, end = _windows("mixed", M, N)
    want = c["ix"].range_search(c["Q"], c["rad"], min_id=mid, end_id=end)
    ln, sn, idn = c["ix"].range_search(c["Q"].float().cpu().numpy(), c["rad"].cpu().numpy(), min_id=mid.numpy(),
                                       end_id=end.tolist())
    assert isinstance(ln, np.ndarray) and ln.tolist() == want[0].tolist() and idn.tolist() == want[2].tolist()
    assert sn.dtype == np.float32 and sn.tolist() == want[1].tolist()


# ---- 2. the same bits as the unwindowed kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [("unit", 320), ("grid2", 64)])
def test_window_bit_equal_to_the_existing_kernel(kind, d):
    M, N = 300, 1000
    c = _case(kind, M, N, d)
    ix, Q, rad = c["ix"], c["Q"], c["rad"]
    min_id = torch.arange(M) * 3 - 5
    plain, plain_mid = ix.range_search(Q, rad), ix.range_search(Q, rad, min_id=min_id)
    assert int(plain[0][-1]) > 1000
    assert _same(ix.range_search(Q, rad, end_id=None), plain)
    assert _same(ix.range_search(Q, rad, end_id=torch.full((M,), N)), plain)
    assert _same(ix.range_search(Q, rad, min_id=min_id, end_id=torch.full((M,), N)), plain_mid)
    assert _same(ix.range_search(Q, rad, min_id=min_id, end_id=torch.full((M,), N + 77)), plain_mid)
    for wk in ("mixed", "per_tile"):
        mid, end = _windows(wk, M, N)
        want = _filtered(ix.range_search(Q, rad, min_id=mid), end, N)
        assert _same(ix.range_search(Q, rad, min_id=mid, end_id=end), want)
    end = min_id + 1 + torch.arange(M) % 400                                   # windows of 0 .. 399 ids sliding over the corpus
    want = _filtered(plain_mid, end, N)
    assert int(want[0][-1]) > 100
    assert _same(ix.range_search(Q, rad, min_id=min_id, end_id=end), want)


# ---- 3. radius -inf and NaN ----------------------------------------------------------------------------------------------------
def test_window_radius_minus_inf_is_the_window_and_nan_is_nothing():
    M, N = 300, 1000
    c = _case("grid8", M, N, 320)
    for wk in ("mixed", "per_tile", "dead_tile"):
        mid, end = _windows(wk, M, N)
        want = W.window_counts(mid, end, N)
        lims, scores, ids = c["ix"].range_search(c["Q"], -math.inf, min_id=mid, end_id=end)
        assert torch.equal((lims[1:] - lims[:-1]).cpu(), want)
        assert torch.equal(c["ix"].range_count(c["Q"], -math.inf, min_id=mid, end_id=end).cpu(), want)
        first = (mid + 1).clamp(min=0)
        want_ids = torch.cat([torch.arange(int(a), int(a) + int(n)) for a, n in zip(first, want)])
        assert torch.equal(ids.cpu(), want_ids)
        W.check_exact(c["Q"], c["D"], -math.inf, mid, end, lims, scores, ids)
        lims, scores, ids = c["ix"].range_search(c["Q"], math.nan, min_id=mid, end_id=end)
        assert lims.tolist() == [0] * (M + 1) and ids.numel() == 0 and scores.numel() == 0
        assert c["ix"].range_count(c["Q"], math.nan, min_id=mid, end_id=end).tolist() == [0] * M


# ---- 4. the band's first, last and partial last tile ----------------------------------------------------------------------------
def test_window_single_hits_at_the_band_edges():
    """128 unrelated unit-norm query rows, one of them a copy of a corpus row: the only pair above 0.9 is that copy, and only
    when its id lies in the window.  N % 128 != 0: the band of the last cases ends in the partial last tile."""
    N, d = 1000, 64
    _, D = _unit_operands(1, N, d)
    Qr, _ = _unit_operands(128, 1, d)                        # (another seed: |cos| with the corpus rows stays below 0.7)
    ix = _index(D)
    for lo, hi, target, hit in ((130, 900, 131, True),      # first id of the band's first tile region that is admitted
                                (130, 900, 130, False),     # min_id itself: same tile, not admitted
                                (130, 900, 899, True), (130, 900, 900, False),       # the band's last tile (7 of 1 .. 7)
                                (127, 897, 128, True), (127, 897, 896, True),        # tiles 1 .. 7: exactly the first / last id
                                (127, 896, 896, False),                              # end on a tile edge: tile 7 is outside
                                (500, N, N - 1, True), (-1, N + 9, N - 1, True),     # the partial last tile
                                (-1, N - 1, N - 1, False), (-1, 128, 0, True), (-1, 128, 127, True), (-1, 128, 128, False)):
        Q = Qr.clone()
        Q[77] = D[target]
        mid, end = torch.full((128,), lo), torch.full((128,), hi)
        lims, scores, ids = ix.range_search(Q, 0.9, min_id=mid, end_id=end)
        want = _filtered(ix.range_search(Q, 0.9, min_id=mid), end, N)
        assert _same((lims, scores, ids), want)
        assert ids.tolist() == ([target] if hit else []), (lo, hi, target)
        assert (lims[1:] - lims[:-1]).tolist() == [int(hit and m == 77) for m in range(128)]
        # one row of the tile alone has the wide window: the band is its window, the others still admit nothing outside theirs
        end2 = torch.full((128,), lo + 1)
        end2[5] = hi
        assert ix.range_search(Q, 0.9, min_id=mid, end_id=end2)[2].numel() == 0


# ---- 5. independence of splits, batches, runs and the workspace's contents ------------------------------------------------------
def test_window_independent_of_splits_batches_and_runs():
    from contrastors_amd.search import FlatIPIndex

    for c in (_case("grid2", 300, 1000, 64), _case("unit", 300, 1000, 320)):
        for wk in ("mixed", "per_tile"):
            mid, end = _windows(wk, 300, 1000)
            want = c["ix"].range_search(c["Q"], c["rad"], min_id=mid, end_id=end)
            assert int(want[0][-1]) > 300
            for nsplit in (1, 2, 3, 64):
                for _ in range(2):
                    assert _same(c["ix"].range_search(c["Q"], c["rad"], min_id=mid, end_id=end, nsplit=nsplit), want)
                    assert torch.equal(c["ix"].range_count(c["Q"], c["rad"], min_id=mid, end_id=end, nsplit=nsplit),
                                       want[0][1:] - want[0][:-1])
            small = FlatIPIndex(c["D"].shape[1], device=DEV, workspace_bytes=1024)     # three query batches
            small.add(c["D"])
            assert _same(small.range_search(c["Q"], c["rad"], min_id=mid, end_id=end), want)
            assert torch.equal(small.range_count(c["Q"], c["rad"], min_id=mid, end_id=end), want[0][1:] - want[0][:-1])
            total = int(want[0][-1])
            with pytest.raises(ValueError, match=rf"\b{total}\b.*max_results = {total - 1}\b"):
                c["ix"].range_search(c["Q"], c["rad"], min_id=mid, end_id=end, max_results=total - 1)
            with pytest.raises(ValueError, match=rf"\b{total}\b"):                       # the running total over batches
                small.range_search(c["Q"], c["rad"], min_id=mid, end_id=end, max_results=total - 1)


def _abi_case():
    from contrastors_amd import _C
    from contrastors_amd.search import window_band

    M, N = 300, 1000
    c = _case("grid2", M, N, 64)
    mid, end = (t.to(DEV) for t in _windows("mixed", M, N))
    band = window_band(mid, end, M, N)
    ptr = torch.zeros(band.numel() + 1, dtype=torch.int64, device=DEV)
    ptr[1:] = torch.cumsum(band, 0)
    want = c["ix"].range_search(c["Q"], c["rad"], min_id=mid, end_id=end)
    return _C.lib(), c, mid, end, ptr, int(ptr[-1]), want


def _abi_run(h, c, mid, end, ptr, total, ws, nsplit=0, M=300, N=1000):
    """count -> lims -> emit through the C ABI -> (lims, scores, ids)."""
    cnt = torch.empty(M, dtype=torch.int64, device=DEV)
    args = (c["Q"].data_ptr(), c["D"].data_ptr(), M, N, 64, 64, 64, c["rad"].data_ptr(), mid.data_ptr(), end.data_ptr(),
            ptr.data_ptr(), total, nsplit, ws.data_ptr())
    assert h.cx_range_window_count(*args, cnt.data_ptr(), None) == 0
    lims = torch.zeros(M + 1, dtype=torch.int64, device=DEV)
    lims[1:] = torch.cumsum(cnt, 0)
    n = int(lims[-1])
    s = torch.empty(max(n, 1), dtype=torch.float32, device=DEV)
    i = torch.empty(max(n, 1), dtype=torch.int64, device=DEV)
    assert h.cx_range_window_emit(*args, lims.data_ptr(), s.data_ptr(), i.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return lims, s[:n], i[:n]


def test_window_cabi_uninitialised_workspace_and_understated_band():
    h, c, mid, end, ptr, total, want = _abi_case()
    for nsplit in (0, 1, 5):
        nbytes = h.cx_range_window_ws_bytes(300, 1000, total, nsplit)
        for fill in (0xFF, 0x00, 0x5A):
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
            assert _same(_abi_run(h, c, mid, end, ptr, total, ws, nsplit), want)
    # a band description that holds fewer tiles than the windows ask for: the walk is cut to it -- a subset of the rows'
    # results, and not one byte outside the (smaller) workspace is written
    for small_ptr in (ptr // 2, torch.zeros_like(ptr), ptr.clamp(max=3), -ptr, ptr * 1000):
        small_total = max(0, int(small_ptr.clamp(0, total // 2).max()))
        nbytes = h.cx_range_window_ws_bytes(300, 1000, small_total, 0)
        ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        lims, s, i = _abi_run(h, c, mid, end, small_ptr, small_total, ws)
        assert bool((ws[nbytes:] == 0xA5).all())
        R.check_layout(lims, i, 300)
        got, full = R.to_mask(lims, i, 300, 1000), R.to_mask(want[0], want[2], 300, 1000)
        assert bool((got <= full).all())
        if small_total == 0:
            assert i.numel() == 0


def test_window_refusals():
    from contrastors_amd.search import FlatIPIndex

    h, c, mid, end, ptr, total, want = _abi_case()
    ix, Q, rad = c["ix"], c["Q"], c["rad"]
    with pytest.raises(ValueError, match="end_id has 301 entries for 300"):
        ix.range_search(Q, rad, end_id=torch.arange(301))
    with pytest.raises(ValueError, match="end_id has 1 entries for 300"):
        ix.range_count(Q, rad, end_id=[3])
    with pytest.raises(ValueError, match="end_id: expected integer"):
        ix.range_search(Q, rad, end_id=torch.zeros(300))
    with pytest.raises(ValueError, match="end_id: expected integer"):
        ix.range_count(Q, rad, end_id=torch.zeros(300, dtype=torch.bool))
    empty = FlatIPIndex(64, device=DEV)
    l0, s0, i0 = empty.range_search(Q, 0.0, end_id=end)
    assert l0.tolist() == [0] * 301 and s0.numel() == 0 and i0.numel() == 0
    assert ix.range_count(Q[:0], rad[:0], end_id=end[:0]).numel() == 0
    l0, s0, i0 = ix.range_search(Q, math.inf, min_id=mid, end_id=end)               # a zero total: no emit
    assert l0.tolist() == [0] * 301 and s0.numel() == 0
    # the C ABI: the error codes of cx_range_count / cx_range_emit, returned before any launch
    ws = torch.empty(h.cx_range_window_ws_bytes(300, 1000, total, 0), dtype=torch.uint8, device=DEV)
    cnt = torch.empty(300, dtype=torch.int64, device=DEV)
    D = c["D"]

    def base():
        return dict(Q=Q.data_ptr(), D=D.data_ptr(), M=300, N=1000, d=64, ldq=64, ldd=64, radius=rad.data_ptr(),
                    min_id=mid.data_ptr(), end_id=end.data_ptr(), band_ptr=ptr.data_ptr(), band_tiles=total, nsplit=0,
                    ws=ws.data_ptr())

    def count_rc(**kw):
        a = dict(base(), counts=cnt.data_ptr())
        a.update(kw)
        return h.cx_range_window_count(*a.values(), None)

    def emit_rc(**kw):
        a = dict(base(), lims=want[0].data_ptr(), out_scores=want[1].data_ptr(), out_ids=want[2].data_ptr())
        a.update(kw)
        return h.cx_range_window_emit(*a.values(), None)

    for rc in (count_rc, emit_rc):
        assert rc(Q=None) == -3 and rc(D=None) == -3 and rc(radius=None) == -3 and rc(ws=None) == -3      # CX_ERR_ARG
        assert rc(band_ptr=None) == -3 and rc(band_tiles=-1) == -3
        assert rc(ldq=60) == -2 and rc(ldq=68) == -2 and rc(ldd=68) == -2                                  # CX_ERR_ALIGN
        assert rc(Q=Q.data_ptr() + 2) == -2 and rc(ws=ws.data_ptr() + 4) == -2
        assert rc(N=2 ** 31 - 128) == -1 and rc(d=96, ldq=96, ldd=96) == -1 and rc(d=2048, ldq=2048, ldd=2048) == -1
        assert rc(M=-1) == -1                                                                              # CX_ERR_SHAPE
        assert rc(M=0, Q=None, ws=None) == 0 and rc(N=0, D=None, ws=None) == 0
    assert count_rc(counts=None) == -3
    assert emit_rc(lims=None) == -3 and emit_rc(out_scores=None) == -3 and emit_rc(out_ids=None) == -3
    assert count_rc(min_id=None, end_id=None) == 0                                   # both optional: the whole corpus
    torch.cuda.synchronize()


# ---- 6. the label-sorted self-join ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,rad", [("grid2", 64, 1.0), ("grid8", 320, 1.0), ("unit", 64, 0.2)])
def test_window_sorted_self_join_is_the_join_within_runs(kind, d, rad):
    runs = [1, 2, 127, 128, 129, 300, 1, 255]
    n = sum(runs)
    _, D = _unit_operands(1, n, d) if kind == "unit" else _grid_operands(1, n, d, 8 if kind == "grid8" else 2, 29)
    ix = _index(D)
    run_of = torch.repeat_interleave(torch.arange(len(runs)), torch.tensor(runs)).to(DEV)
    end = torch.repeat_interleave(torch.cumsum(torch.tensor(runs), 0), torch.tensor(runs))
    pos = torch.arange(n)
    lims, scores, ids = ix.range_search(D, rad, min_id=pos)                          # the exact self-join
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), lims[1:] - lims[:-1])
    same = run_of[rows] == run_of[ids]
    assert 100 < int(same.sum()) < ids.numel()
    jl, js, ji = ix.range_search(D, rad, min_id=pos, end_id=end)                      # one call over the band
    assert torch.equal(ji, ids[same]) and torch.equal(js.view(torch.int32), scores[same].view(torch.int32))
    assert torch.equal(jl[1:] - jl[:-1], torch.bincount(rows[same], minlength=n))
    if kind != "unit":
        W.check_exact(D, D, rad, pos, end, jl, js, ji)
