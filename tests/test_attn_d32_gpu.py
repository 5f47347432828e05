"""Self-attention at head_dim 32 (csrc/attn_d32.hip) through the public flash-attn functions: parity with the float64 yardstick
at the 32-, 64-, 128- and 256-row edges of the query and the key walk, full head pairs (H = 4) and a lone last head (H = 3), a
sharp softmax, the fixed-length form, run-to-run identical gradients, and the host refusals."""
import math

import pytest
import torch

from contrastors_amd.flash_attn_api import flash_attn_interface as fa
from tests import attn_ref as ar

gpu = pytest.mark.gpu
DEV = "cuda"
D = 32
LENS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 300, 513]


def _cu(lens):
    return torch.tensor([0] + lens, device=DEV).cumsum(0).to(torch.int32)


def _inputs(H, gain, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(sum(LENS), 3, H, D, generator=g)
    qkv[:, :2] *= gain
    return qkv.bfloat16(), torch.randn(sum(LENS), H, D, generator=g).bfloat16()


def run(qkv, dout, **kw):
    """out, lse, dq, dk, dv of the public varlen function and autograd."""
    x = qkv.to(DEV).requires_grad_(True)
    out = fa.flash_attn_varlen_qkvpacked_func(x, _cu(LENS), max(LENS), **kw)
    lse = out.grad_fn.saved_tensors[2].clone()
    out.backward(dout.to(DEV))
    return {"out": out.detach().cpu(), "lse": lse.cpu(), "dq": x.grad[:, 0].cpu(), "dk": x.grad[:, 1].cpu(), "dv": x.grad[:, 2].cpu()}


@gpu
@pytest.mark.parametrize("H,gain,scale", [(3, 1.0, None), (4, 1.0, None), (3, 4.0, None), (4, 4.0, None), (3, 1.0, 0.3)])
def test_parity(H, gain, scale):
    qkv, dout = _inputs(H, gain, seed=7 + H)
    got = run(qkv, dout, softmax_scale=scale)
    sc = 1 / math.sqrt(D) if scale is None else scale
    model, ref = ar.bf16_model(qkv, LENS, None, None, sc, dout), ar.reference(qkv, LENS, None, None, sc, dout)
    fig, fails = ar.judge(got, model, ref, LENS, zero_bounds=ar.zero_grad_bounds(qkv, LENS, sc, dout))
    print(H, gain, scale, fig)
    assert not fails, fails


@gpu
@pytest.mark.parametrize("H", (3, 4))
def test_fixed_length_form_equals_varlen_and_repeats(H):
    B, S = 2, 200
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * S, 3, H, D, generator=g).bfloat16().to(DEV)
    dout = torch.randn(B * S, H, D, generator=g).bfloat16().to(DEV)
    res = []
    for fixed in (True, False, False):
        x = qkv.clone().requires_grad_(True)
        if fixed:
            out = fa.flash_attn_qkvpacked_func(x.view(B, S, 3, H, D)).reshape(B * S, H, D)
        else:
            out = fa.flash_attn_varlen_qkvpacked_func(x, torch.tensor([0, S, 2 * S], device=DEV, dtype=torch.int32), S)
        out.backward(dout)
        res.append((out.detach(), x.grad))
    for out, grad in res[1:]:
        assert torch.equal(out, res[0][0]) and torch.equal(grad, res[0][1])


def test_host_refusals():
    qkv, cu = torch.zeros(4, 3, 2, D, dtype=torch.bfloat16), torch.tensor([0, 4], dtype=torch.int32)
    q, kv = qkv[:, 0].contiguous(), qkv[:, 1:].contiguous()
    with pytest.raises(NotImplementedError, match="dropout"):
        fa.flash_attn_varlen_qkvpacked_func(qkv, cu, 4, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="window"):
        fa.flash_attn_varlen_qkvpacked_func(qkv, cu, 4, window_size=(1, 1))
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        fa.flash_attn_varlen_kvpacked_func(q, kv, cu, cu, 4, 4)
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        fa.flash_attn_kvpacked_func(q[None], kv[None])
    with pytest.raises(NotImplementedError, match="32 or 64"):
        fa.flash_attn_varlen_qkvpacked_func(torch.zeros(4, 3, 2, 48, dtype=torch.bfloat16), cu, 4)
