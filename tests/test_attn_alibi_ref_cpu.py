"""The ALiBi yardsticks themselves (tests/attn_alibi_ref.py): with zero slopes they are attn_ref's, bit for bit; with slopes
alibi_reference is what torch autograd gives for softmax(scores + bias) V."""
import torch

from tests import attn_ref as ar
from tests.attn_alibi_ref import alibi_model, alibi_reference, bias

LENS, H, SCALE = [1, 7, 33, 70], 3, 0.125


def test_zero_slopes_are_the_plain_yardsticks():
    qkv, dout = ar.make_inputs("gauss", LENS, H, seed=3)
    for got, want in ((alibi_reference(qkv, LENS, torch.zeros(H), SCALE, dout), ar.reference(qkv, LENS, None, None, SCALE, dout)),
                      (alibi_model(qkv, LENS, torch.zeros(len(LENS), H), SCALE, dout), ar.bf16_model(qkv, LENS, None, None, SCALE, dout))):
        for name in want:
            assert torch.equal(got[name], want[name]), name


def test_reference_is_autograd_of_the_explicit_form():
    qkv, dout = ar.make_inputs("gauss", LENS, H, seed=4)
    slopes = torch.tensor([[0.5, 0.0, 0.03]]) * torch.arange(1, len(LENS) + 1)[:, None]     # (B, H), one head without a bias
    ref = alibi_reference(qkv, LENS, slopes, SCALE, dout)
    x = qkv.double().requires_grad_(True)
    t0 = 0
    for b, l in enumerate(LENS):
        q, k, v = x[t0:t0 + l].unbind(1)
        P = torch.softmax(torch.einsum("qhd,khd->hqk", q, k) * SCALE + bias(slopes, b, l, torch.float64, "cpu"), -1)
        out = torch.einsum("hqk,khd->qhd", P, v)
        assert (out - ref["out"][t0:t0 + l]).abs().max() <= 1e-12
        (out * dout[t0:t0 + l].double()).sum().backward()
        t0 += l
    for i, name in enumerate(("dq", "dk", "dv")):
        assert (x.grad[:, i] - ref[name]).abs().max() <= 1e-12, name
