"""Self-attention with ALiBi (csrc/attn_alibi.inc) through the public flash-attn functions: parity with the biased yardsticks at
the 32 / 64-row block, 64-key tile and 256-row workgroup edges of both walks, a head without a bias, per-sequence slopes, a
sharp softmax, zero slopes next to the plain path, the fixed-length form, run-to-run identical bits, the untouched default path
and the host checks."""
import math

import pytest
import torch

from contrastors_amd.flash_attn_api import flash_attn_interface as fa
from tests import attn_ref as ar
from tests.attn_alibi_ref import alibi_model, alibi_reference

gpu = pytest.mark.gpu
DEV = "cuda"
H = 4
LENS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 300, 513]
STD = [2.0 ** -2, 2.0 ** -4, 2.0 ** -6, 2.0 ** -8]              # the standard 4-head slope set
SLOPES = {"std": torch.tensor(STD), "zero_head": torch.tensor([STD[0], 0.0, STD[2], STD[3]]), "zeros": torch.zeros(H),
          "per_seq": torch.tensor(STD)[None, :] * (0.3 + 0.17 * torch.arange(len(LENS)))[:, None]}


def _cu(lens):
    return torch.tensor([0] + lens, device=DEV).cumsum(0).to(torch.int32)


def _inputs(lens, gain, seed):
    qkv, dout = ar.make_inputs("gauss", lens, H, seed=seed)
    qkv = qkv.float()
    qkv[:, :2] *= gain
    return qkv.bfloat16(), dout


def run(qkv, dout, lens, **kw):
    """out, lse, dq, dk, dv of the public varlen function and autograd."""
    x = qkv.to(DEV).requires_grad_(True)
    out = fa.flash_attn_varlen_qkvpacked_func(x, _cu(lens), max(lens), **kw)
    lse = out.grad_fn.saved_tensors[2].clone()
    out.backward(dout.to(DEV))
    return {"out": out.detach().cpu(), "lse": lse.cpu(), "dq": x.grad[:, 0].cpu(), "dk": x.grad[:, 1].cpu(), "dv": x.grad[:, 2].cpu()}


def judged(got, qkv, dout, lens, slopes, sc):
    model, ref = alibi_model(qkv, lens, slopes, sc, dout), alibi_reference(qkv, lens, slopes, sc, dout)
    return ar.judge(got, model, ref, lens, zero_bounds=ar.zero_grad_bounds(qkv, lens, sc, dout))


@gpu
@pytest.mark.parametrize("slopes,gain,scale", [("std", 1.0, None), ("std", 4.0, None), ("zero_head", 1.0, None), ("zero_head", 4.0, None),
                                               ("per_seq", 1.0, None), ("per_seq", 4.0, None), ("std", 1.0, 0.3), ("zeros", 1.0, None)])
def test_parity(slopes, gain, scale):
    qkv, dout = _inputs(LENS, gain, seed=21)
    sc = 1 / math.sqrt(64) if scale is None else scale
    got = run(qkv, dout, LENS, alibi_slopes=SLOPES[slopes].to(DEV), softmax_scale=scale)
    fig, fails = judged(got, qkv, dout, LENS, SLOPES[slopes], sc)
    print(slopes, gain, scale, fig)
    assert not fails, fails


@gpu
def test_zero_slopes_next_to_the_plain_path():
    lens = [300, 300]
    qkv, dout = _inputs(lens, 1.0, seed=22)
    for kw in ({"alibi_slopes": torch.zeros(H)}, {}):      # the ALiBi kernels at slope 0, then cx_attn_varlen_fwd / _bwd
        fig, fails = judged(run(qkv, dout, lens, **kw), qkv, dout, lens, torch.zeros(H), 0.125)
        print(sorted(kw), fig)
        assert not fails, fails


@gpu
def test_fixed_length_form_equals_varlen_and_repeats():
    B, S = 2, 200
    qkv, dout = (t.to(DEV) for t in _inputs([S] * B, 1.0, seed=5))
    slopes, res = SLOPES["zero_head"].to(DEV), []
    for fixed in (True, False, False):
        x = qkv.clone().requires_grad_(True)
        if fixed:
            out = fa.flash_attn_qkvpacked_func(x.view(B, S, 3, H, 64), alibi_slopes=slopes).reshape(B * S, H, 64)
        else:
            out = fa.flash_attn_varlen_qkvpacked_func(x, _cu([S] * B), S, alibi_slopes=slopes)
        out.backward(dout)
        res.append((out.detach(), x.grad))
    for out, grad in res[1:]:
        assert torch.equal(out, res[0][0]) and torch.equal(grad, res[0][1])
    assert not torch.equal(res[0][0], fa.flash_attn_varlen_qkvpacked_func(qkv, _cu([S] * B), S))


@gpu
def test_no_slopes_is_the_default_path(monkeypatch):
    lens = [300, 77]
    qkv, dout = _inputs(lens, 1.0, seed=6)
    base = run(qkv, dout, lens)
    lib = fa._C.lib()

    class NoAlibi:   # the library without the two new entries
        def __getattr__(self, name):
            assert "alibi" not in name, name
            return getattr(lib, name)

    monkeypatch.setattr(fa._C, "lib", lambda: NoAlibi())
    got = run(qkv, dout, lens, alibi_slopes=None)
    for name in base:
        assert torch.equal(got[name], base[name]), name


def test_host_checks():
    qkv, cu = torch.zeros(4, 3, H, 64, dtype=torch.bfloat16), torch.tensor([0, 4], dtype=torch.int32)
    q, kv, ok = qkv[:, 0].contiguous(), qkv[:, 1:].contiguous(), torch.ones(H)
    for bad in (torch.ones(H + 1), torch.ones(2, H), torch.ones(1, 1, H), -ok, ok * float("inf"), ok * float("nan")):
        with pytest.raises(ValueError, match="alibi_slopes"):
            fa.flash_attn_varlen_qkvpacked_func(qkv, cu, 4, alibi_slopes=bad)
    with pytest.raises(ValueError, match="softmax_scale"):
        fa.flash_attn_qkvpacked_func(qkv[None], alibi_slopes=ok, softmax_scale=0.0)
    with pytest.raises(NotImplementedError, match="alibi_slopes with attention dropout"):
        fa.flash_attn_varlen_qkvpacked_func(qkv, cu, 4, alibi_slopes=ok, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="alibi_slopes with a finite window_size"):
        fa.flash_attn_qkvpacked_func(qkv[None], alibi_slopes=ok, window_size=(1, 1))
    with pytest.raises(NotImplementedError, match="alibi_slopes at head_dim 32"):
        fa.flash_attn_varlen_qkvpacked_func(torch.zeros(4, 3, H, 32, dtype=torch.bfloat16), cu, 4, alibi_slopes=ok)
    with pytest.raises(NotImplementedError, match="alibi_slopes is built for the qkv-packed"):
        fa.flash_attn_varlen_kvpacked_func(q, kv, cu, cu, 4, 4, alibi_slopes=ok)
    with pytest.raises(NotImplementedError, match="alibi_slopes is built for the qkv-packed"):
        fa.flash_attn_kvpacked_func(q[None], kv[None], alibi_slopes=ok)
