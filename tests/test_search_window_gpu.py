"""GPU checks of the windowed top-k kernel and the list merge (csrc/search.hip: cx_search_window_topk, cx_topk_merge_lists).
Scores keep cx_search_topk's single instruction sequence, so everything is compared BITWISE (torch.equal on scores and ids):
against FlatIPIndex over the slice a window names, against the float64 reference on operands whose fp32 sums are exact, and
against a host merge."""
import numpy as np
import pytest
import torch

from tests import search_window_ref as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _unit_bf16(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, d, device=DEV, generator=g)
    return torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)


def _grid_bf16(n, d, seed, denom=8, levels=3):
    """Entries j / denom, |j| <= levels: every product and every partial sum is exact in fp32 (denom=2, levels=1: few
    distinct scores, ties everywhere)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randint(-levels, levels + 1, (n, d), device=DEV, generator=g).float() / denom).to(torch.bfloat16)


def _i64(x):
    return None if x is None else torch.as_tensor(x, dtype=torch.int64).to(DEV).contiguous()


def _csr(exclude):
    if exclude is None:
        return None, None
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(e) for e in exclude])]), dtype=torch.int64, device=DEV)
    ids = torch.tensor([i for e in exclude for i in e] or [0], dtype=torch.int64, device=DEV)
    return ptr, ids


def window_topk(Q, D, k, min_id=None, end_id=None, exclude=None, below=None, out=None):
    """cx_search_window_topk on device operands -> (rc, scores, ids)."""
    from contrastors_amd import _C

    h = _C.lib()
    M, N, d = Q.shape[0], D.shape[0], Q.shape[1]
    mid, end = _i64(min_id), _i64(end_id)
    xptr, xids = _csr(exclude)
    bel = None if below is None else torch.as_tensor(below, dtype=torch.float32).to(DEV).contiguous()
    ws = torch.empty(max(16, h.cx_search_window_ws_bytes(M, k)), dtype=torch.uint8, device=DEV)
    s, i = out if out is not None else (torch.empty(M, max(k, 1), dtype=torch.float32, device=DEV),
                                        torch.empty(M, max(k, 1), dtype=torch.int64, device=DEV))
    rc = h.cx_search_window_topk(Q.data_ptr(), D.data_ptr() if N else None, M, N, d, Q.stride(0), D.stride(0) if N else d, k,
                                 _C.ptr(mid), _C.ptr(end), _C.ptr(xptr), _C.ptr(xids), _C.ptr(bel), ws.data_ptr(),
                                 s.data_ptr(), i.data_ptr(), _C.cur_stream())
    torch.cuda.synchronize()
    return rc, s, i


def merge_lists(scores, ids, src, k, id_map=None):
    from contrastors_amd import _C

    scores, ids, src = scores.contiguous(), ids.contiguous(), _i64(src)
    M, L = src.shape
    rep = _i64(id_map)
    out_s = torch.full((M, k), 7.0, dtype=torch.float32, device=DEV)
    out_i = torch.full((M, k), -7, dtype=torch.int64, device=DEV)
    rc = _C.lib().cx_topk_merge_lists(scores.data_ptr(), ids.data_ptr(), scores.shape[0], k, src.data_ptr(), M, L,
                                      _C.ptr(rep), 0 if rep is None else rep.numel(), out_s.data_ptr(), out_i.data_ptr(),
                                      _C.cur_stream())
    torch.cuda.synchronize()
    return rc, out_s, out_i


def _flat(D):
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(D.shape[1], device=DEV)
    if D.shape[0]:
        ix.add(D)
    return ix


def _slice_expected(Q, D, k, windows, rows_of, exclude=None, below=None):
    """Per distinct window (lo, hi): FlatIPIndex over D[lo + 1 : hi] searched by the rows that have it, ids shifted back."""
    M, N = Q.shape[0], D.shape[0]
    es = torch.empty(M, k, dtype=torch.float32, device=DEV)
    ei = torch.empty(M, k, dtype=torch.int64, device=DEV)
    for (lo, hi), rows in zip(windows, rows_of):
        if not len(rows):
            continue
        a, b = min(max(lo, -1), N) + 1, min(max(hi, 0), N)
        rows_t = torch.as_tensor(rows, device=DEV)
        ex = None if exclude is None else [[e - a for e in exclude[r] if a <= e < b] for r in rows]
        s, i = _flat(D[a: max(a, b)]).search(Q[rows_t], k, exclude=ex, below=None if below is None else below[rows_t])
        es[rows_t], ei[rows_t] = s, torch.where(i >= 0, i + a, i)
    return es, ei


def _bound_windows(N):
    """Bounds at -3, -1, 0, 1, 127, 128, 129, N - 1, N, N + 500: full, one-id, tile-edge, empty and inverted windows."""
    return [(-1, N), (-3, N + 500), (-3, 1), (0, 128), (0, 129), (1, 127), (126, 128), (127, 129), (127, N), (128, N + 500),
            (129, N - 1), (N - 1, N), (N - 1, N + 500), (-1, 0), (129, 128), (N, N + 500), (0, N)]


@pytest.mark.parametrize("N", [1, 127, 129, 300, 1000])
@pytest.mark.parametrize("d", [64, 320, 1024])
def test_windows_equal_flat_search_over_the_slice(d, N):
    D = _unit_bf16(N, d, 10 + N)
    wins = _bound_windows(N)
    empty = [w for w, (lo, hi) in enumerate(wins) if min(max(hi, 0), N) <= min(max(lo, -1), N) + 1]
    assert len(empty) >= 4
    for M in (1, 127, 129, 300, 1000):
        Q = _unit_bf16(M, d, 20 + M)
        # windows mixed inside every query tile; M = 1000: rows 256 .. 383, a whole tile, have empty windows
        which = [(3 * r + r // 7) % len(wins) for r in range(M)]
        if M == 1000:
            which[256:384] = [empty[r % len(empty)] for r in range(128)]
        mid, end = [wins[w][0] for w in which], [wins[w][1] for w in which]
        rows_of = [[r for r in range(M) if which[r] == w] for w in range(len(wins))]
        for k in (1, 10, 130, 1024):
            es, ei = _slice_expected(Q, D, k, wins, rows_of)
            rc, s, i = window_topk(Q, D, k, mid, end)
            assert rc == 0
            assert torch.equal(i, ei) and torch.equal(s, es), (M, k)
            if M == 1000:
                assert bool((i[256:384] == -1).all()) and bool(torch.isinf(s[256:384]).all())


def test_null_and_full_windows_equal_the_plain_search():
    for N, M, d, k in ((1000, 300, 128, 10), (129, 129, 64, 130), (4097, 130, 256, 100)):
        Q, D = _unit_bf16(M, d, 1), _unit_bf16(N, d, 2)
        g = np.random.default_rng(N)
        exclude = [g.integers(0, N, int(g.integers(0, 4))).tolist() for _ in range(M)]
        es, ei = _flat(D).search(Q, k)
        below = es[:, min(k, N) // 2].contiguous()
        for ex, bel in ((None, None), (exclude, below)):
            es, ei = _flat(D).search(Q, k, exclude=ex, below=bel)
            for mid, end in ((None, None), ([-1] * M, [N] * M), ([-1] * M, None), (None, [N] * M), ([-9] * M, [N + 9] * M)):
                rc, s, i = window_topk(Q, D, k, mid, end, ex, bel)
                assert rc == 0 and torch.equal(i, ei) and torch.equal(s, es)


@pytest.mark.parametrize("denom,levels", [(8, 3), (2, 1)])
def test_grid_operands_equal_the_float64_reference(denom, levels):
    for N, M, d, k in ((300, 129, 64, 10), (1000, 300, 320, 130), (129, 127, 1024, 1024), (127, 1, 64, 1)):
        Q, D = _grid_bf16(M, d, 3, denom, levels), _grid_bf16(N, d, 4, denom, levels)
        wins = _bound_windows(N)
        mid = [wins[(5 * r) % len(wins)][0] for r in range(M)]
        end = [wins[(5 * r) % len(wins)][1] for r in range(M)]
        g = np.random.default_rng(M)
        exclude = [g.integers(-1, N + 1, int(g.integers(0, 4))).tolist() for _ in range(M)]
        S = W.scores64(Q, D)
        below = S.float().quantile(0.9, dim=1).contiguous()          # ON or between attained scores: strictness matters
        below = S.gather(1, (S - below[:, None].double()).abs().argmin(1, keepdim=True)).flatten().float()
        for ex, bel in ((None, None), (exclude, None), (None, below), (exclude, below)):
            rc, s, i = window_topk(Q, D, k, mid, end, ex, bel)
            assert rc == 0
            W.check_exact(Q, D, k, s, i, mid, end, ex, bel)


def test_single_hits_at_the_band_edges():
    """All scores are 0 but one: the hit is found in the band's first tile, its last full tile and its partial last tile, and
    not just outside either bound (then the window's lowest id wins the all-zero tie)."""
    d, N, M = 64, 700, 130
    Q = torch.ones(M, d, device=DEV, dtype=torch.bfloat16)
    lo, hi = 130, 650                                    # band tiles 1 .. 5; tile 5 = ids 640 .. 699 is partial twice over
    mid, end = [lo] * M, [hi] * M
    for hit, found in ((131, True), (255, True), (639, True), (640, True), (649, True), (130, False), (650, False),
                       (127, False), (699, False)):
        D = torch.zeros(N, d, device=DEV, dtype=torch.bfloat16)
        D[hit, 0] = 1
        rc, s, i = window_topk(Q, D, 2, mid, end)
        assert rc == 0
        W.check_exact(Q, D, 2, s, i, mid, end)
        want = [hit, lo + 1 if hit != lo + 1 else lo + 2] if found else [lo + 1, lo + 2]
        assert i[0].tolist() == want and i[M - 1].tolist() == want and s[0, 0].item() == float(found)


def test_below_and_exclusions_inside_a_window():
    d, N, M, k = 128, 600, 200, 20
    Q, D = _unit_bf16(M, d, 5), _unit_bf16(N, d, 6)
    wins = [(99, 400), (-1, 130), (255, 600), (300, 310)]
    which = [r % 4 for r in range(M)]
    mid, end = [wins[w][0] for w in which], [wins[w][1] for w in which]
    rows_of = [[r for r in range(M) if which[r] == w] for w in range(4)]
    es, ei = _slice_expected(Q, D, k, wins, rows_of)
    # exclude the best and the fourth of every row's window, plus ids outside it; bound at the row's sixth score
    exclude = [[int(ei[r, 0]), int(ei[r, 3]), (mid[r] + 500) % N, max(mid[r], 0)] for r in range(M)]
    below = es[:, 5].contiguous()
    for ex, bel in ((exclude, None), (None, below), (exclude, below)):
        es2, ei2 = _slice_expected(Q, D, k, wins, rows_of, ex, bel)
        rc, s, i = window_topk(Q, D, k, mid, end, ex, bel)
        assert rc == 0 and torch.equal(i, ei2) and torch.equal(s, es2)
        if ex is not None:
            assert not bool((i[:, :1] == ei[:, :1]).any())
    # everything excluded in a one-id window
    rc, s, i = window_topk(Q[:3], D, 4, [7, 7, 7], [9, 9, 9], [[8], [], [7, 9]])
    assert i[:, 0].tolist() == [-1, 8, 8] and bool((i[:, 1:] == -1).all()) and bool(torch.isinf(s[0]).all())


def test_sorted_windows_every_tile_spans_several():
    """The IVF shape: lists [1, 2, 127, 128, 129, 300, 1, 255] in a row, the query rows sorted by the list they probe."""
    d, k = 192, 130
    sizes = [1, 2, 127, 128, 129, 300, 1, 255]
    probed_by = [3, 130, 1, 127, 129, 2, 64, 100]                 # rows per list: tiles start and end inside a list's run
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N, M = int(ptr[-1]), sum(probed_by)
    wins = [(int(ptr[l]) - 1, int(ptr[l + 1])) for l in range(len(sizes))]
    which = [l for l, c in enumerate(probed_by) for _ in range(c)]
    mid, end = [wins[w][0] for w in which], [wins[w][1] for w in which]
    rows_of = [[r for r in range(M) if which[r] == w] for w in range(len(sizes))]
    Q, D = _unit_bf16(M, d, 7), _unit_bf16(N, d, 8)
    es, ei = _slice_expected(Q, D, k, wins, rows_of)
    rc, s, i = window_topk(Q, D, k, mid, end)
    assert rc == 0 and torch.equal(i, ei) and torch.equal(s, es)
    Q, D = _grid_bf16(M, d, 9, 2, 1), _grid_bf16(N, d, 10, 2, 1)
    rc, s, i = window_topk(Q, D, k, mid, end)
    W.check_exact(Q, D, k, s, i, mid, end)


def test_determinism_and_refusals():
    d, N, M, k = 64, 900, 257, 50
    Q, D = _grid_bf16(M, d, 11, 2, 1), _grid_bf16(N, d, 12, 2, 1)
    g = np.random.default_rng(0)
    mid = g.integers(-3, N, M).tolist()
    end = [a + int(b) for a, b in zip(mid, g.integers(0, 400, M))]
    _, s1, i1 = window_topk(Q, D, k, mid, end)
    _, s2, i2 = window_topk(Q, D, k, mid, end)
    assert torch.equal(s1, s2) and torch.equal(i1, i2)
    # refusals: an error code, and the outputs keep what they held
    from contrastors_amd import _C

    def untouched(s, i):
        return bool((s == 7).all()) and bool((i == -7).all())

    def out():
        return torch.full((M, 2048), 7.0, device=DEV), torch.full((M, 2048), -7, dtype=torch.int64, device=DEV)

    for kk in (0, 1025):
        rc, s, i = window_topk(Q, D, kk, mid, end, out=out())
        assert rc != 0 and untouched(s, i)
    rc, s, i = window_topk(Q[:, :32], D[:, :32], k, mid, end, out=out())            # d = 32
    assert rc != 0 and untouched(s, i)
    rc, s, i = window_topk(Q[:, 8:], D, k, mid, end, out=out())                     # d = 56, and an odd stride pairing
    assert rc != 0 and untouched(s, i)
    Qo = torch.zeros(M * d + 8, device=DEV, dtype=torch.bfloat16)[4: 4 + M * d].view(M, d)   # 8-byte aligned only
    rc, s, i = window_topk(Qo, D, k, mid, end, out=out())
    assert rc != 0 and untouched(s, i)
    h = _C.lib()
    assert h.cx_topk_merge_lists(None, None, 4, 10, None, 2, 2, None, 0, None, None, None) != 0     # null src / outputs
    sc, ids = torch.zeros(4, 10, device=DEV), torch.zeros(4, 10, dtype=torch.int64, device=DEV)
    for L, kk in ((0, 10), (257, 10), (2, 0), (2, 1025)):
        src = torch.zeros(2, max(L, 1), dtype=torch.int64, device=DEV)
        o_s, o_i = out()
        rc = h.cx_topk_merge_lists(sc.data_ptr(), ids.data_ptr(), 4, kk, src.data_ptr(), 2, L, None, 0, o_s.data_ptr(),
                                   o_i.data_ptr(), _C.cur_stream())
        torch.cuda.synchronize()
        assert rc != 0 and untouched(o_s, o_i)


# ---- the merge ---------------------------------------------------------------------------------------------------------
def _lists(M, L, k, N, seed, levels=3):
    """M * L sorted lists over disjoint positions per output row; scores on a coarse grid (ties inside and across lists,
    resolved by the MAPPED id); lengths 0 / 1 / k / random; some src entries -1; a random id_map."""
    g = np.random.default_rng(seed)
    id_map = g.permutation(N).astype(np.int64)
    scores = np.full((M * L, k), -np.inf, dtype=np.float32)
    ids = np.full((M * L, k), -1, dtype=np.int64)
    src = g.permutation(M * L).astype(np.int64).reshape(M, L)          # a query's lists are scattered over the rows
    for m in range(M):
        pool = g.permutation(N)
        used = 0
        for l in range(L):
            n = [0, 1, k, int(g.integers(0, k + 1))][(m + l) % 4]
            n = min(n, N - used)
            pos = pool[used: used + n]
            used += n
            s = g.integers(-levels, levels + 1, n).astype(np.float32) / 2
            o = np.lexsort((id_map[pos], -s))
            scores[src[m, l], :n], ids[src[m, l], :n] = s[o], pos[o]
    drop = g.random((M, L)) < 0.15
    return scores, ids, np.where(drop, -1, src), id_map


@pytest.mark.parametrize("L", [1, 2, 3, 64, 256])
def test_merge_lists_against_the_host_merge(L):
    M, k = 9, 33 if L < 64 else 17
    N = 4 * L * k + 50
    scores, ids, src, id_map = _lists(M, L, k, N, seed=L)
    ds, di = torch.tensor(scores, device=DEV), torch.tensor(ids, device=DEV)
    for rep in (id_map, None):
        if rep is None:      # lists sorted by (score, position): re-sort the ties inside every list
            o = np.lexsort((np.where(ids >= 0, ids, N), -scores.astype(np.float64)), axis=1)
            scores, ids = np.take_along_axis(scores, o, 1), np.take_along_axis(ids, o, 1)
            ds, di = torch.tensor(scores, device=DEV), torch.tensor(ids, device=DEV)
        for kk in (k,):
            es, ei = W.merge_ref(scores, ids, src, kk, rep)
            rc, s, i = merge_lists(ds, di, src, kk, rep)
            assert rc == 0
            assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es), (L, rep is None)
            rc, s2, i2 = merge_lists(ds, di, src, kk, rep)
            assert torch.equal(s, s2) and torch.equal(i, i2)
    # every list empty or unnamed: padding
    rc, s, i = merge_lists(ds, di, np.full((M, L), -1), k, None)
    assert rc == 0 and bool((i == -1).all()) and bool(torch.isinf(s).all())


def test_merge_of_the_split_lists_of_one_search_is_the_search():
    """Cut the corpus into L consecutive windows, search every (query, window) pair and merge with id_map = NULL."""
    d, N, M, k = 128, 3000, 70, 100
    Q, D = _unit_bf16(M, d, 13), _unit_bf16(N, d, 14)
    es, ei = _flat(D).search(Q, k)
    for L in (1, 2, 3, 64):
        cuts = np.linspace(0, N, L + 1).astype(np.int64)
        rows = torch.arange(M, device=DEV).repeat_interleave(L)
        mid = np.tile(cuts[:-1] - 1, M)
        end = np.tile(cuts[1:], M)
        rc, ls, li = window_topk(Q[rows].contiguous(), D, k, mid, end)
        assert rc == 0
        rc, s, i = merge_lists(ls, li, np.arange(M * L).reshape(M, L), k, None)
        assert rc == 0 and torch.equal(i, ei) and torch.equal(s, es), L
