"""Sliding-window attention (attn_window.inc) through the public flash-attn functions: parity with the banded yardsticks at the
tile (64), wave-block (32) and workgroup (128) edges of the query and the key walk, the exact diagonal, the fixed-length form,
the unchanged default path and the host checks."""
import math

import pytest
import torch

from contrastors_amd.flash_attn_api import flash_attn_interface as fa
from tests import attn_ref as ar
from tests.attn_window_ref import window_model, window_reference

gpu = pytest.mark.gpu
DEV = "cuda"
H = 2
SCALE = 1 / math.sqrt(64)
LENS = [1, 63, 64, 65, 127, 129, 255, 257, 300, 513]
WINDOWS = [(0, 0), (1, 0), (0, 1), (17, 5), (63, 64), (64, 64), (128, 128), (-1, 0), (0, -1), (-1, 64)]


@pytest.fixture(scope="module")
def inputs():
    qkv, dout = ar.make_inputs("gauss", LENS, H, seed=11)
    return qkv.to(DEV), dout.to(DEV)


def _cu(lens):
    return torch.tensor([0] + lens, device=DEV).cumsum(0).to(torch.int32)


def run(qkv, dout, **kw):
    """out, lse, dq, dk, dv of the public varlen function and autograd."""
    x = qkv.clone().requires_grad_(True)
    out = fa.flash_attn_varlen_qkvpacked_func(x, _cu(LENS), max(LENS), **kw)
    lse = out.grad_fn.saved_tensors[2].clone()
    out.backward(dout)
    return {"out": out.detach(), "lse": lse, "dq": x.grad[:, 0], "dk": x.grad[:, 1], "dv": x.grad[:, 2]}


@gpu
@pytest.mark.parametrize("window", WINDOWS, ids=str)
def test_parity(inputs, window):
    qkv, dout = inputs
    got = run(qkv, dout, window_size=window)
    model, ref = window_model(qkv, LENS, window, SCALE, dout), window_reference(qkv, LENS, window, SCALE, dout)
    # rows whose exact dq / dk is 0 (one visible key): the length-1 sequence, and under (0, 0) every row
    zero = ar.zero_grad_bounds(qkv, [1] * sum(LENS) if window == (0, 0) else LENS, SCALE, dout)
    fig, fails = ar.judge(got, model, ref, LENS, zero_bounds=zero)
    print(window, fig)
    assert not fails, fails


@gpu
def test_diagonal_window_is_exact(inputs):
    qkv, dout = inputs
    got = run(qkv, dout, window_size=(0, 0))
    assert torch.equal(got["out"].view(torch.int16), qkv[:, 2].view(torch.int16))   # P is exactly 1
    assert (got["dq"] == 0).all()


@gpu
def test_fixed_length_form_equals_varlen():
    B, S = 2, 200
    qkv, dout = ar.make_inputs("gauss", [S] * B, H, seed=5)
    res = []
    for fixed in (True, False):
        x = qkv.to(DEV).requires_grad_(True)
        if fixed:
            out = fa.flash_attn_qkvpacked_func(x.view(B, S, 3, H, 64), window_size=(64, 64)).reshape(B * S, H, 64)
        else:
            out = fa.flash_attn_varlen_qkvpacked_func(x, _cu([S] * B), S, window_size=(64, 64))
        out.backward(dout.to(DEV))
        res.append((out.detach(), x.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], fa.flash_attn_varlen_qkvpacked_func(qkv.to(DEV), _cu([S] * B), S))


@gpu
@pytest.mark.parametrize("window", [(-1, -1), (512, 512)], ids=str)
def test_covering_window_is_the_default_path(inputs, window):
    qkv, dout = inputs
    got, base = run(qkv, dout, window_size=window), run(qkv, dout)
    for name in base:
        assert torch.equal(got[name], base[name]), name


def test_host_checks():
    qkv, cu = torch.zeros(4, 3, H, 64, dtype=torch.bfloat16), torch.tensor([0, 4], dtype=torch.int32)
    q, kv = qkv[:, 0].contiguous(), qkv[:, 1:].contiguous()
    with pytest.raises(ValueError):
        fa.flash_attn_varlen_qkvpacked_func(qkv, cu, 4, window_size=(-2, 0))
    with pytest.raises(NotImplementedError):
        fa.flash_attn_varlen_qkvpacked_func(qkv, cu, 4, dropout_p=0.1, window_size=(1, 1))
    with pytest.raises(NotImplementedError):
        fa.flash_attn_qkvpacked_func(qkv[None], dropout_p=0.1, window_size=(1, 1))
    with pytest.raises(NotImplementedError):
        fa.flash_attn_varlen_kvpacked_func(q, kv, cu, cu, 4, 4, window_size=(1, 1))
    with pytest.raises(NotImplementedError):
        fa.flash_attn_kvpacked_func(q[None], kv[None], window_size=(0, -1))
