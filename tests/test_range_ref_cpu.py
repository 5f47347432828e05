"""The float64 range-search reference (tests/range_ref.py) against a brute-force loop on tiny inputs, and against planted
errors: each kind of mistake the GPU tests exist to find must make the checker fail."""
import math

import numpy as np
import pytest
import torch

from tests import range_ref as R


def _tiny(M=7, N=23, d=64, levels=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randint(-levels, levels + 1, (M, d), generator=g).float() / levels).to(torch.bfloat16)
    D = (torch.randint(-levels, levels + 1, (N, d), generator=g).float() / levels).to(torch.bfloat16)
    return Q, D


def _brute(Q, D, radius, min_id):
    lims, scores, ids = [0], [], []
    q, dd = Q.double().numpy(), D.double().numpy()
    for m in range(q.shape[0]):
        for n in range(dd.shape[0]):
            s = float(np.dot(q[m], dd[n]))
            if s > radius[m] and n > min_id[m]:
                scores.append(s)
                ids.append(n)
        lims.append(len(ids))
    return lims, scores, ids


def _bounds(Q, D):
    """Radii that sit ON attained scores (strictness matters), plus -inf / +inf / NaN rows; min_ids across the range."""
    S = R.scores64(Q, D)
    M, N = S.shape
    radius = [float(S[m, (3 * m) % N]) for m in range(M)]
    radius[1], radius[2], radius[3] = -math.inf, math.inf, math.nan
    min_id = [-1, 0, 5, N - 2, N - 1, N + 3, 11][:M]
    return radius, min_id


def test_reference_equals_brute_force():
    for seed in range(3):
        Q, D = _tiny(seed=seed)
        radius, min_id = _bounds(Q, D)
        lims, scores, ids = R.ref_range(Q, D, radius, min_id)
        bl, bs, bi = _brute(Q, D, radius, min_id)
        assert lims.tolist() == bl and ids.tolist() == bi and scores.tolist() == bs
        assert len(bi) > 20                                   # not vacuous
        R.check_layout(lims, ids, Q.shape[0])
        assert R.check_against_ref(Q, D, radius, min_id, lims, scores.float(), ids, exact=True) == 0
        # rows with a -inf radius and min_id -1 hold the whole corpus, NaN / +inf rows nothing
        l0, _, i0 = R.ref_range(Q, D, [-math.inf, math.nan, math.inf] + [0.0] * 4, None)
        assert i0[: int(l0[1])].tolist() == list(range(D.shape[0])) and int(l0[3]) == int(l0[1])


def test_scalar_radius_and_no_min_id():
    Q, D = _tiny(seed=5)
    lims, scores, ids = R.ref_range(Q, D, 1.0)
    bl, bs, bi = _brute(Q, D, [1.0] * Q.shape[0], [-1] * Q.shape[0])
    assert lims.tolist() == bl and ids.tolist() == bi and scores.tolist() == bs


def _result_with(Q, D, radius, min_id, mask_fn):
    S = R.scores64(Q, D)
    return R.from_mask(S, mask_fn(S))


def test_planted_errors_are_caught():
    Q, D = _tiny(seed=1)
    M, N = Q.shape[0], D.shape[0]
    radius, min_id = _bounds(Q, D)
    S = R.scores64(Q, D)
    rad = torch.tensor(radius, dtype=torch.float64)
    mid = torch.tensor(min_id)
    col = torch.arange(N)
    good = R.admitted(S, radius, min_id)
    planted = {
        ">= in place of >": (S >= rad[:, None]) & (col[None, :] > mid[:, None]),
        "min_id off by one (n >= min_id)": (S > rad[:, None]) & (col[None, :] >= mid[:, None]),
        "min_id off by one (n > min_id + 1)": (S > rad[:, None]) & (col[None, :] > mid[:, None] + 1),
    }
    for name, mask in planted.items():
        assert not torch.equal(mask, good), f"{name}: the inputs do not exercise it"
        lims, scores, ids = R.from_mask(S, mask)
        # a tie with the radius lies inside every band: only the exact comparison can tell >= from >.  The min_id mistakes
        # move pairs that are far from the radius (the grid's scores are 1/4 apart): the banded comparison finds them too.
        for exact in ((True,) if name.startswith(">=") else (True, False)):
            with pytest.raises(AssertionError):
                R.check_against_ref(Q, D, radius, min_id, lims, scores.float(), ids, exact=exact)
    # unsorted ids: swap two entries of one row (scores along with them: the SET is right, the order is not)
    lims, scores, ids = R.from_mask(S, good)
    row = int(torch.nonzero(lims[1:] - lims[:-1] >= 2)[0])
    a = int(lims[row])
    ids2, scores2 = ids.clone(), scores.clone()
    ids2[[a, a + 1]] = ids[[a + 1, a]]
    scores2[[a, a + 1]] = scores[[a + 1, a]]
    for exact in (True, False):
        with pytest.raises(AssertionError, match="ascending"):
            R.check_against_ref(Q, D, radius, min_id, lims, scores2.float(), ids2, exact=exact)
    with pytest.raises(AssertionError):                       # a wrong score bit
        bad = scores.float().clone()
        bad[0] = torch.nextafter(bad[0], torch.tensor(float("inf")))
        R.check_against_ref(Q, D, radius, min_id, lims, bad, ids, exact=True)
    with pytest.raises(AssertionError):                       # lims that do not delimit ids
        R.check_layout(lims[:-1], ids, M)


def test_band_bounds_fp32_accumulation_in_any_order():
    """The band is what it claims: fp32 accumulations of the exact products, in three different orders, stay inside it."""
    g = torch.Generator().manual_seed(3)
    Q = torch.nn.functional.normalize(torch.randn(16, 320, generator=g), dim=1).to(torch.bfloat16)
    D = torch.nn.functional.normalize(torch.randn(40, 320, generator=g), dim=1).to(torch.bfloat16)
    S, B = R.scores64(Q, D), R.band(Q, D)
    prod = Q.float()[:, None, :] * D.float()[None, :, :]      # exact in fp32
    fwd = torch.zeros(16, 40)
    for i in range(320):
        fwd = fwd + prod[:, :, i]
    rev = torch.zeros(16, 40)
    for i in reversed(range(320)):
        rev = rev + prod[:, :, i]
    pair = prod.reshape(16, 40, 10, 32).sum(3).sum(2)
    for got in (fwd, rev, pair):
        assert bool(((got.double() - S).abs() <= B).all())
    # and it is narrow: sum |q_i d_i| <= |q| |d| ~ 1 for unit-norm rows (Cauchy-Schwarz), so at most ~ d * 2^-24 = 1.9e-5 here
    assert float(B.max()) < 1.02 * 1.01 * 320 * 2.0 ** -24
