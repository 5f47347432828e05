"""float64 dense reference of the WINDOWED range search (tests/test_range_window_gpu.py, tests/test_clustered_dedup_gpu.py):
tests/range_ref.py with an exclusive upper id per row.  Row m admits document n iff score > radius[m] (strict) and
min_id[m] < n < min(max(end_id[m], 0), N); end_id None is N everywhere.  Everything else (scores64, from_mask, the layout and
the comparison) is range_ref's, imported and not changed."""
import torch

from tests import range_ref as R


def admitted(S, radius, min_id=None, end_id=None):
    """(M, N) bool for a score matrix S: range_ref.admitted and n < end_id[m], end_id clamped to [0, N]."""
    M, N = S.shape
    mask = R.admitted(S, radius, min_id)
    if end_id is None:
        return mask
    end = torch.as_tensor(end_id, dtype=torch.int64).to(S.device).reshape(-1).clamp(0, N)
    assert end.numel() == M
    col = torch.arange(N, device=S.device)
    return mask & (col[None, :] < end[:, None])


def ref_range(Q, D, radius, min_id=None, end_id=None):
    """The reference answer (lims, scores float64, ids) for operands Q (M, d), D (N, d)."""
    S = R.scores64(Q, D)
    return R.from_mask(S, admitted(S, radius, min_id, end_id))


def check_exact(Q, D, radius, min_id, end_id, lims, scores, ids):
    """A result on operands whose fp32 accumulation is exact: layout, then lims, ids and scores EQUAL to the reference."""
    R.check_layout(lims, ids, Q.shape[0])
    S = R.scores64(Q, D)
    rl, rs, ri = R.from_mask(S, admitted(S, radius, min_id, end_id))
    lims, scores, ids = (torch.as_tensor(x).to(S.device) for x in (lims, scores, ids))
    assert torch.equal(lims, rl), "lims differ from the reference"
    assert torch.equal(ids, ri), "ids differ from the reference"
    assert torch.equal(scores.double(), rs), "scores differ from the reference"


def window_counts(min_id, end_id, N):
    """(M,) int64: the ids in each row's window, max(0, min(end, N) - max(min_id + 1, 0))."""
    mid = torch.as_tensor(min_id, dtype=torch.int64)
    end = torch.as_tensor(end_id, dtype=torch.int64)
    return (end.clamp(max=N) - (mid + 1).clamp(min=0)).clamp(min=0)
