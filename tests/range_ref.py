"""float64 dense reference of the range search (tests/test_range_search_gpu.py, tests/test_dedup_gpu.py).

Scores are `Q.double() @ D.double().T` on the bf16 operands.  Row m admits document n iff score > radius[m] (strict) and
n > min_id[m]; the admitted ids of a row come out ascending, in faiss's range_search layout (lims, scores, ids).  `band` is
the per-pair rounding band of an fp32 accumulation in ANY order: bf16 products are exact in fp32 (8 + 8 significand bits),
so only the d - 1 additions round, each by at most 2^-24 relative to a partial sum that is at most sum_i |q_i d_i| --
1.01 * d * 2^-24 * sum_i |q_i d_i| covers it with the usual (1 + u)^d slack.  Runs on the operands' device."""
import torch


def scores64(Q, D):
    return Q.double() @ D.double().T


def band(Q, D):
    """(M, N) float64: |fp32-accumulated score - float64 score| is at most this, whatever the accumulation order."""
    return 1.01 * Q.shape[1] * 2.0 ** -24 * (Q.double().abs() @ D.double().abs().T)


def _bounds(radius, min_id, M, dev):
    rad = torch.as_tensor(radius, dtype=torch.float64).to(dev).reshape(-1)
    rad = rad.expand(M) if rad.numel() == 1 else rad
    mid = torch.full((M,), -1, dtype=torch.int64, device=dev) if min_id is None else \
        torch.as_tensor(min_id, dtype=torch.int64).to(dev).reshape(-1)
    assert rad.numel() == M and mid.numel() == M
    return rad, mid


def admitted(S, radius, min_id=None):
    """(M, N) bool for a score matrix S: S > radius[m] (strict; a NaN radius admits nothing) and n > min_id[m]."""
    M, N = S.shape
    rad, mid = _bounds(radius, min_id, M, S.device)
    col = torch.arange(N, device=S.device)
    return (S > rad[:, None]) & (col[None, :] > mid[:, None])


def from_mask(S, mask):
    """-> (lims (M + 1) int64, scores (nnz) float64, ids (nnz) int64) of a dense admission mask: row-major order, that is rows
    ascending and ids ascending within a row."""
    M = S.shape[0]
    lims = torch.zeros(M + 1, dtype=torch.int64, device=S.device)
    lims[1:] = torch.cumsum(mask.sum(1), 0)
    rows, ids = torch.nonzero(mask, as_tuple=True)     # row-major: the order wanted
    return lims, S[rows, ids], ids


def ref_range(Q, D, radius, min_id=None):
    """The reference answer (lims, scores float64, ids) for operands Q (M, d), D (N, d)."""
    S = scores64(Q, D)
    return from_mask(S, admitted(S, radius, min_id))


def check_layout(lims, ids, M):
    """The structural contract of a result: lims starts at 0, is non-decreasing, ends at len(ids); ids ascend strictly within
    every row.  Raises AssertionError naming the first violation."""
    lims, ids = torch.as_tensor(lims).cpu(), torch.as_tensor(ids).cpu()
    assert lims.numel() == M + 1 and int(lims[0]) == 0 and int(lims[-1]) == ids.numel(), "lims do not delimit ids"
    assert bool((lims[1:] >= lims[:-1]).all()), "lims decrease"
    if ids.numel() > 1:
        starts = torch.zeros(ids.numel(), dtype=torch.bool)
        inner = lims[1:-1]
        starts[inner[inner < ids.numel()]] = True          # first entry of a row: no order constraint with the previous one
        bad = (ids[1:] <= ids[:-1]) & ~starts[1:]
        assert not bool(bad.any()), f"ids not ascending within a row at entry {int(torch.nonzero(bad)[0]) + 1}"


def to_mask(lims, ids, M, N):
    """(M, N) bool of a result (CPU)."""
    lims, ids = torch.as_tensor(lims).cpu(), torch.as_tensor(ids).cpu()
    rows = torch.repeat_interleave(torch.arange(M), lims[1:] - lims[:-1])
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[rows, ids] = True
    return mask


def check_against_ref(Q, D, radius, min_id, lims, scores, ids, exact):
    """A result against the float64 reference.  exact: lims, ids and scores must EQUAL the reference (operands whose fp32
    accumulation is exact).  Otherwise: every pair whose float64 score is further than its band from the radius is classified
    as the reference says, and every returned score is within the band of float64.  -> the number of in-band pairs."""
    M, N = Q.shape[0], D.shape[0]
    check_layout(lims, ids, M)
    S = scores64(Q, D)
    want = admitted(S, radius, min_id)
    lims, scores, ids = (torch.as_tensor(x).to(S.device) for x in (lims, scores, ids))
    if exact:
        rl, rs, ri = from_mask(S, want)
        assert torch.equal(lims, rl), "lims differ from the reference"
        assert torch.equal(ids, ri), "ids differ from the reference"
        assert torch.equal(scores.double(), rs), "scores differ from the reference"
        return 0
    got = to_mask(lims, ids, M, N).to(S.device)
    rad, _ = _bounds(radius, min_id, M, S.device)
    B = band(Q, D)
    inband = ((S - rad[:, None]).abs() <= B) & admitted(torch.full_like(S, float("inf")), -1.0, min_id)
    wrong = (got != want) & ~inband
    assert not bool(wrong.any()), f"{int(wrong.sum())} pairs outside their band are misclassified"
    rows = torch.repeat_interleave(torch.arange(M, device=S.device), lims[1:] - lims[:-1])
    err = (scores.double() - S[rows, ids]).abs()
    assert bool((err <= B[rows, ids]).all()), f"a returned score is {float(err.max()):.3e} from float64, outside its band"
    return int(inband.sum())
