"""Host side of the logit-free MLM head (contrastors_amd/linear_xent.py): refusals that need no GPU, and the ctypes signatures."""
import pytest
import torch

from contrastors_amd import _C
from contrastors_amd.linear_xent import linear_cross_entropy


def _args(M=4, V=10, K=64, n_labels=None):
    return (torch.zeros(M, K, dtype=torch.bfloat16), torch.zeros(V, K, dtype=torch.bfloat16), None,
            torch.zeros(M if n_labels is None else n_labels, dtype=torch.int64))


@pytest.mark.parametrize("kwargs, extra, exc", [
    (dict(K=96), {}, ValueError),                       # K % 64 != 0
    (dict(K=1088), {}, ValueError),                     # K > 1024
    (dict(n_labels=3), {}, ValueError),                 # label count mismatch
    (dict(), dict(reduction="batchmean"), ValueError),  # bad reduction
    (dict(), {}, RuntimeError),                         # CPU tensors: there is no CPU path
])
def test_host_refusals(kwargs, extra, exc):
    with pytest.raises(exc):
        linear_cross_entropy(*_args(**kwargs), **extra)


@pytest.mark.parametrize("name, nargs", [("cx_linear_xent_ws_floats", 2), ("cx_linear_xent_fwd", 13), ("cx_linear_xent_grad", 17)])
def test_sigs_arity(name, nargs):
    assert name in _C.EXPORTED_SYMBOLS and len(_C._SIGS[name][1]) == nargs
