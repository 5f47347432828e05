"""The float64 reference of the windowed range search (tests/range_window_ref.py) against a brute-force loop on tiny inputs,
and against planted errors: each mistake at the window's end that the GPU tests exist to find must make the checker fail."""
import math

import numpy as np
import pytest
import torch

from tests import range_ref as R
from tests import range_window_ref as W


def _tiny(M=9, N=23, d=64, levels=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randint(-levels, levels + 1, (M, d), generator=g).float() / levels).to(torch.bfloat16)
    D = (torch.randint(-levels, levels + 1, (N, d), generator=g).float() / levels).to(torch.bfloat16)
    return Q, D


def _brute(Q, D, radius, min_id, end_id):
    lims, scores, ids = [0], [], []
    q, dd = Q.double().numpy(), D.double().numpy()
    N = dd.shape[0]
    for m in range(q.shape[0]):
        for n in range(N):
            s = float(np.dot(q[m], dd[n]))
            if s > radius[m] and min_id[m] < n < end_id[m]:      # (n < N already: no clamp needed in the loop)
                scores.append(s)
                ids.append(n)
        lims.append(len(ids))
    return lims, scores, ids


def _bounds(Q, D):
    """Radii ON attained scores plus -inf / +inf / NaN rows; windows with ends at 0, 1, N - 1, N, above N, negative, empty
    (end == min_id + 1) and inverted (end < min_id)."""
    S = R.scores64(Q, D)
    M, N = S.shape
    radius = [float(S[m, (3 * m) % N]) for m in range(M)]
    radius[1], radius[2], radius[3] = -math.inf, math.inf, math.nan
    min_id = [-1, 0, 5, N - 2, -1, 3, 11, 7, -5][:M]
    end_id = [N, N - 1, N + 7, N, 1, 4, 0, -3, 12][:M]
    return radius, min_id, end_id


def test_reference_equals_brute_force():
    for seed in range(3):
        Q, D = _tiny(seed=seed)
        radius, min_id, end_id = _bounds(Q, D)
        lims, scores, ids = W.ref_range(Q, D, radius, min_id, end_id)
        bl, bs, bi = _brute(Q, D, radius, min_id, end_id)
        assert lims.tolist() == bl and ids.tolist() == bi and scores.tolist() == bs
        assert len(bi) > 20                                   # not vacuous
        W.check_exact(Q, D, radius, min_id, end_id, lims, scores.float(), ids)
        # empty and inverted windows hold nothing; a -inf radius holds its whole window
        counts = (lims[1:] - lims[:-1]).tolist()
        assert counts[5] == counts[6] == counts[7] == 0
        assert ids[int(lims[1]): int(lims[2])].tolist() == list(range(1, D.shape[0] - 1))
        assert W.window_counts(min_id, end_id, D.shape[0])[1] == D.shape[0] - 2
    # end_id None is range_ref itself
    Q, D = _tiny(seed=4)
    radius, min_id, _ = _bounds(Q, D)
    for a, b in zip(W.ref_range(Q, D, radius, min_id, None), R.ref_range(Q, D, radius, min_id)):
        assert torch.equal(a, b)


def test_window_counts_against_a_loop():
    N = 23
    vals = [-7, -1, 0, 1, 5, N - 1, N, N + 4]
    for a in vals:
        for b in vals:
            assert int(W.window_counts([a], [b], N)[0]) == sum(1 for n in range(N) if a < n < b)


def test_planted_errors_are_caught():
    Q, D = _tiny(seed=1)
    N = D.shape[0]
    radius, min_id, end_id = _bounds(Q, D)
    S = R.scores64(Q, D)
    rad = torch.tensor(radius, dtype=torch.float64)
    mid, end = torch.tensor(min_id), torch.tensor(end_id)
    col = torch.arange(N)
    low = (S > rad[:, None]) & (col[None, :] > mid[:, None])
    good = W.admitted(S, radius, min_id, end_id)
    planted = {
        "<= in place of <": low & (col[None, :] <= end.clamp(0, N)[:, None]),
        "window one short (n < end - 1)": low & (col[None, :] < end.clamp(0, N)[:, None] - 1),
        # a negative end that is not clamped to 0 and then read as unsigned: the window is open above
        "unclamped negative end": low & ((col[None, :] < end[:, None]) | (end[:, None] < 0)),
    }
    # an end above N that is not clamped shows in the counts of a -inf radius: the window formula without min(end, N)
    unclamped = (end - (mid + 1).clamp(min=0)).clamp(min=0)
    full = W.ref_range(Q, D, -math.inf, min_id, end_id)[0]
    assert torch.equal(full[1:] - full[:-1], W.window_counts(min_id, end_id, N))
    assert not torch.equal(unclamped, W.window_counts(min_id, end_id, N))
    for name, mask in planted.items():
        assert not torch.equal(mask, good), f"{name}: the inputs do not exercise it"
        lims, scores, ids = R.from_mask(S, mask)
        with pytest.raises(AssertionError):
            W.check_exact(Q, D, radius, min_id, end_id, lims, scores.float(), ids)
    # the unwindowed answer is not the windowed one
    lims, scores, ids = R.ref_range(Q, D, radius, min_id)
    with pytest.raises(AssertionError):
        W.check_exact(Q, D, radius, min_id, end_id, lims, scores.float(), ids)
