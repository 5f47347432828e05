"""The `flash_attn` symbol surface (contrastors_amd.flash_attn_api) exports every name the reference's layer modules import
from flash_attn (the composition of those names on the real kernels: tests/test_shim_compose_gpu.py).  Also checks the
pure-index helpers on CPU."""
import importlib

import torch


def test_bert_padding_roundtrip_cpu():
    from contrastors_amd.flash_attn_api.bert_padding import index_first_axis, pad_input, unpad_input

    mask = torch.tensor([[1, 1, 0], [1, 0, 0], [1, 1, 1]])
    h = torch.arange(18.0).view(3, 3, 2)
    u, idx, cu, mx = unpad_input(h, mask)  # 4-tuple, as the reference expects
    assert idx.tolist() == [0, 1, 3, 6, 7, 8] and cu.tolist() == [0, 2, 3, 6] and mx == 3
    assert cu.dtype == torch.int32
    back = pad_input(u, idx, 3, 3)
    assert torch.equal(back, h * mask.unsqueeze(-1))
    assert torch.equal(index_first_axis(h.view(9, 2), idx), u)


def test_surface_exports_every_symbol_contrastors_imports():
    import contrastors_amd.flash_attn_api as fa

    fa.install("flash_attn_cx_test")
    need = {
        "flash_attn_cx_test": ["flash_attn_qkvpacked_func", "flash_attn_varlen_qkvpacked_func",
                               "flash_attn_kvpacked_func", "flash_attn_varlen_kvpacked_func"],
        "flash_attn_cx_test.bert_padding": ["unpad_input", "pad_input", "index_first_axis"],
        "flash_attn_cx_test.ops.layer_norm": ["dropout_add_layer_norm", "dropout_add_layer_norm_parallel_residual",
                                              "layer_norm"],
        "flash_attn_cx_test.ops.rms_norm": ["RMSNorm", "rms_norm", "dropout_add_rms_norm",
                                            "dropout_add_rms_norm_parallel_residual"],
        "flash_attn_cx_test.ops.fused_dense": ["FusedDense"],
        "flash_attn_cx_test.ops.activations": ["swiglu"],
        "flash_attn_cx_test.layers.rotary": ["RotaryEmbedding", "apply_rotary_emb_func", "apply_rotary_emb_qkv_",
                                             "apply_rotary_emb_kv_"],
        "flash_attn_cx_test.losses.cross_entropy": ["CrossEntropyLoss"],
    }
    for mod, names in need.items():
        m = importlib.import_module(mod)
        for n in names:
            assert hasattr(m, n), f"{mod}.{n}"
