"""The sliding-window yardsticks are anchored to the existing ones: a window that covers every pair changes nothing."""
import torch

from tests import attn_ref as ar
from tests.attn_window_ref import window_model, window_reference


def test_covering_window_is_the_full_reference_bit_for_bit():
    lens = [1, 5, 33, 64, 70]
    qkv, dout = ar.make_inputs("gauss", lens, 2, seed=7)
    for window in ((max(lens) - 1, max(lens) - 1), (-1, -1), (-1, 100)):
        ref, full = window_reference(qkv, lens, window, 0.125, dout), ar.reference(qkv, lens, None, None, 0.125, dout)
        mod, fullm = window_model(qkv, lens, window, 0.125, dout), ar.bf16_model(qkv, lens, None, None, 0.125, dout)
        for name in (*ar.OUTPUTS, "lse"):
            assert torch.equal(ref[name], full[name]), (window, name)
            assert torch.equal(mod[name], fullm[name]), (window, name)
    # ... and a finite one does change it
    assert not torch.equal(window_reference(qkv, lens, (3, 3), 0.125, dout)["out"], full["out"])
