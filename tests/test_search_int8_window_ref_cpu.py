"""The numpy reference of the windowed int8 top-k search (tests/search_int8_window_ref.py) against scalar Python loops on tiny
inputs, and against planted errors: each mistake at a window's bounds, in its clamping, in an empty window or in the tie order
that the GPU tests exist to find must make the checker fail, on a case named here."""
import numpy as np
import pytest

from tests import search_int8_window_ref as IW

F32 = np.float32
WRAP = 1 << 32


def _tiny(M=10, N=23, d=64, seed=0):
    """Codes in {-1, 0, 1}, scales in {0.5, 1, 2}, duplicated rows: exact ties in every query row."""
    g = np.random.default_rng(seed)
    qc = g.integers(-1, 2, (M, d)).astype(np.int8)
    dc = g.integers(-1, 2, (N, d)).astype(np.int8)
    dc[N // 2:] = dc[: N - N // 2]
    qs = g.choice(np.array([0.5, 1, 2], F32), M)
    ds = g.choice(np.array([0.5, 1, 2], F32), N)
    ds[N // 2:] = ds[: N - N // 2]
    return qc, qs, dc, ds


def _score(qc, qs, dc, ds, m, n):
    acc = 0
    for a, b in zip(qc[m].tolist(), dc[n].tolist()):
        acc += a * b
    return F32(F32(F32(acc) * ds[n]) * qs[m])


def _bounds(qc, qs, dc, ds):
    """Windows with bounds at -1, 0, 1, N - 1, N, above N, negative, empty (end == min_id + 1), inverted, and beyond int32 on
    either side (row 9: a full window whose bounds, truncated to 32 bits, would read (5, 3)); below ON an attained score."""
    M, N = qc.shape[0], dc.shape[0]
    S = np.array([[_score(qc, qs, dc, ds, m, n) for n in range(N)] for m in range(M)], F32)
    min_id = [-1, 0, 5, N - 2, -1, 3, 11, 7, -5, -WRAP + 5]
    end_id = [N, N - 1, N + 7, N, 1, 4, 0, -3, 12, WRAP + 3]
    below = [float("inf")] * M
    below[0] = float(S[0].max())                      # the best score itself is not below it
    below[2] = float(np.median(S[2]))
    exclude = [[] for _ in range(M)]
    exclude[0] = [int(S[0].argmax()), N + 3]
    exclude[1] = [1, 2, 0]
    exclude[8] = [0, 11]
    return S, min_id, end_id, exclude, below


def _brute(S, k, min_id, end_id, exclude, below):
    M, N = S.shape
    out_s = np.full((M, k), -np.inf, F32)
    out_i = np.full((M, k), -1, np.int64)
    for m in range(M):
        cands = []
        for n in range(N):
            if min_id[m] < n < end_id[m] and float(S[m, n]) < below[m] and n not in exclude[m]:      # (0 <= n < N already)
                cands.append((-float(S[m, n]), n))
        cands.sort()
        for j, (_, n) in enumerate(cands[:k]):
            out_s[m, j], out_i[m, j] = S[m, n], n
    return out_s, out_i


@pytest.mark.parametrize("k", [1, 4, 30])
def test_reference_equals_scalar_loops(k):
    for seed in range(3):
        qc, qs, dc, ds = _tiny(seed=seed)
        N = dc.shape[0]
        S, min_id, end_id, exclude, below = _bounds(qc, qs, dc, ds)
        assert np.array_equal(IW.R.scores(qc, qs, dc, ds).view(np.uint32), S.view(np.uint32))
        got = IW.search(qc, qs, dc, ds, k, min_id, end_id, exclude, below)
        IW.check(got, _brute(S, k, min_id, end_id, exclude, below))
        i = got[1]
        assert (i[5] == -1).all() and (i[6] == -1).all() and (i[7] == -1).all()      # empty and inverted windows
        assert i[4].tolist() == [0] + [-1] * (k - 1)                                 # the window (-1, 1) holds id 0
        assert (i[9] >= 0).sum() == min(k, N)                                        # beyond int32 both ways: the full window
        # no bounds at all is the plain int8 top-k
        IW.check(IW.search(qc, qs, dc, ds, k), IW.R.search(qc, qs, dc, ds, k))
        IW.check(IW.search(qc, qs, dc, ds, k), _brute(S, k, [-1] * 10, [N] * 10, [[]] * 10, [float("inf")] * 10))


def _planted(S, min_id, end_id, exclude, below):
    M, N = S.shape
    mid, end = np.array(min_id, np.int64), np.array(end_id, np.int64)
    cmid, cend = np.clip(mid, -1, N), np.clip(end, 0, N)
    col = np.arange(N)[None, :]
    rest = IW.admitted(S, None, None, exclude, below)
    lo_ok, hi_ok = col > cmid[:, None], col < cend[:, None]
    good = IW.admitted(S, min_id, end_id, exclude, below)
    assert np.array_equal(good, rest & lo_ok & hi_ok)
    # what a kernel that narrows the bounds to int before clamping would see
    mid32 = ((mid + (1 << 31)) % WRAP - (1 << 31))
    end32 = ((end + (1 << 31)) % WRAP - (1 << 31))
    empty = cend <= cmid + 1
    return good, {
        "non-strict lower bound": rest & (col >= cmid[:, None]) & hi_ok,
        "non-strict upper bound": rest & lo_ok & (col <= cend[:, None]),
        "min_id < -1 not clamped": rest & (col > np.clip(mid32, -1, N)[:, None]) & hi_ok,
        "end_id > N not clamped": rest & lo_ok & (col < np.clip(end32, 0, N)[:, None]),
        "empty window treated as full": np.where(empty[:, None], rest, good),
    }


def test_planted_errors_are_caught():
    qc, qs, dc, ds = _tiny(seed=1)
    k = 6
    S, min_id, end_id, exclude, below = _bounds(qc, qs, dc, ds)
    want = IW.search(qc, qs, dc, ds, k, min_id, end_id, exclude, below)
    good, planted = _planted(S, min_id, end_id, exclude, below)
    IW.check(IW.topk_from_mask(S, good, k), want)
    for name, mask in planted.items():
        assert not np.array_equal(mask, good), f"{name}: the inputs do not exercise it"
        with pytest.raises(AssertionError):
            IW.check(IW.topk_from_mask(S, mask, k), want)
    # ties broken upward: equal scores by DESCENDING id
    s, i = IW.topk_from_mask(S[:, ::-1], good[:, ::-1], k)
    i = np.where(i >= 0, S.shape[1] - 1 - i, i)
    assert np.array_equal(s.view(np.uint32), want[0].view(np.uint32))                # the same scores ...
    with pytest.raises(AssertionError, match="ids differ"):
        IW.check((s, i), want)                                                       # ... in another id order
    # a score off by one ulp, the ids right
    s = want[0].copy()
    s[3, 0] = np.nextafter(s[3, 0], F32(np.inf))
    with pytest.raises(AssertionError, match="scores differ"):
        IW.check((s, want[1]), want)
