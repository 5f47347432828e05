"""Writes tests/golden/vit_eva02_tiny.npz and tests/golden/eva02_timm_remap.npz (CPU, fp32).

Runs the reference's own ViTModel (through oracle.ref_import.load_vit: exact softmax attention in place of the
third-party kernel) on a tiny EVA-02 configuration with the options of timm_name_to_vit_config's EVA-02 entry
(sc/models/vit/timm_vit.py:71-167): 2-D RoPE, SwiGLU MLP with its LayerNorm, no final LayerNorm.  Two replacements make it
run on a CPU-only host: `n_inner` is passed as an int (the installed transformers refuses the float 4 * 2 / 3 * d), and
the GatedMLP's `swiglu` (a HIP kernel behind this repository's flash_attn shim) becomes the exact silu(gate) * y.
The timm fixture is a synthetic timm-keyed EVA-02 state dict and what the reference's remap_timm_state_dict makes of it.

    python scripts/make_golden_eva02.py
"""
from __future__ import annotations

import importlib
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_import  # noqa: E402
from tests import eva02_ref  # noqa: E402

GOLD = ROOT / "tests" / "golden"
TINY_EVA = dict(n_embd=256, n_layer=2, n_head=4, n_inner=512, img_size=32, patch_size=8, num_channels=3,
                layer_norm_epsilon=1e-6, ref_feat_shape=(14, 14))
REMAP = dict(n_embd=32, n_layer=2, n_inner=64, img_size=8, patch_size=4)   # (a key mapping: small is enough)
B16 = dict(n_embd=768, n_layer=12, n_head=12, n_inner=2048, img_size=224, patch_size=16, num_channels=3,
           layer_norm_epsilon=1e-6, ref_feat_shape=(14, 14))


def gpt2_config(cfgd):
    from transformers import GPT2Config

    c = SimpleNamespace(**cfgd)
    return GPT2Config(
        n_embd=c.n_embd, n_layer=c.n_layer, n_head=c.n_head, n_inner=int(c.n_inner), activation_function="swiglu",
        vocab_size=0, n_positions=0, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, layer_norm_epsilon=c.layer_norm_epsilon,
        initializer_range=0.02, bos_token_id=None, eos_token_id=None, drop_path_rate=0.0, prepre_layernom=False,
        layer_scale=False, layer_scale_init=1.0, img_size=c.img_size, patch_size=c.patch_size, num_channels=c.num_channels,
        prenorm=True, parallel_block=False, parallel_block_tied_norm=False, rotary_emb_fraction=0, tie_word_embeddings=False,
        fused_dropout_add_ln=False, fused_bias_fc=False, patch_embed_bias=True, use_flash_attn=True, qkv_proj_bias=True,
        mlp_fc1_bias=True, mlp_fc2_bias=True, use_rms_norm=False, causal=False, hidden_features_scaling_factor=1.0,
        mask_token=False, learned_pos_embedding=False, patch_dropout=0, sinusoidal_pos_embedding=False, register_tokens=0,
        no_cls_token=False, no_embed_class=False, use_rotary_pos_emb=True, ref_feat_shape=tuple(c.ref_feat_shape),
        use_pos_embed=True, eva_qkv_bias=False, no_last_ln=True, norm_mlp=True, global_pool=None)


def load_reference():
    vit = ref_import.load_vit()
    mlp = importlib.import_module("contrastors.layers.mlp")
    mlp.swiglu = lambda gate, y: F.silu(gate) * y
    return vit


def rope_table(vit_mod, cfgd):
    emb = importlib.import_module("contrastors.layers.embedding")
    g = cfgd["img_size"] // cfgd["patch_size"]
    r = emb.RotaryEmbeddingCat(cfgd["n_embd"] // cfgd["n_head"], in_pixels=False, feat_shape=(g, g),
                               ref_feat_shape=tuple(cfgd["ref_feat_shape"]))
    t = r.get_embed()   # (n_patch, 128) = [sin (64) | cos (64)], each the repeat_interleave(2) of 32 angles
    sin, cos = t[:, :64], t[:, 64:]
    assert torch.equal(sin[:, 0::2], sin[:, 1::2]) and torch.equal(cos[:, 0::2], cos[:, 1::2])
    return np.stack([cos[:, 0::2].numpy(), sin[:, 0::2].numpy()])   # (2, n_patch, 32): cos, sin


def gen_tower(vit, name, cfgd, seed):
    ns = SimpleNamespace(**cfgd)
    m = vit.ViTModel(gpt2_config(cfgd)).float()
    sd = eva02_ref.random_state_dict(ns, seed)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    m.eval()
    g = torch.Generator().manual_seed(seed + 1)
    pixels = torch.randn(5, ns.num_channels, ns.img_size, ns.img_size, generator=g)
    hid = m(pixels).last_hidden_state
    out = {"pixels": pixels.numpy(), "hidden": hid.detach().numpy(), "seed": np.array(seed), "rope": rope_table(vit, cfgd),
           "rope_b16": rope_table(vit, B16)}
    for pooling in ("cls", "mean"):
        m.zero_grad()
        e = hid[:, 0] if pooling == "cls" else hid.mean(1)
        emb = F.normalize(e, dim=-1)
        probe = torch.randn(emb.shape, generator=torch.Generator().manual_seed(seed + 2))
        (emb * probe).sum().backward(retain_graph=True)
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        out[f"{pooling}/embedding"] = emb.detach().numpy()
        out[f"{pooling}/probe"] = probe.numpy()
        for k, gt in grads.items():
            out[f"{pooling}/gnorm/" + k] = np.array(float(gt.norm()))
        out[f"{pooling}/g/embeddings.cls_token"] = grads["embeddings.cls_token"].numpy()
        out[f"{pooling}/g/embeddings.pos_embed"] = grads["embeddings.pos_embed"].numpy()
        for k in ("layers.0.attn.Wqkv.weight", "layers.0.mlp.fc11.weight", "layers.0.mlp.fc12.weight", "layers.1.mlp.fc2.weight"):
            out[f"{pooling}/g/{k}[:16,:16]"] = grads[k][:16, :16].numpy()
        for k in ("layers.0.mlp.norm.weight", "layers.1.mlp.norm.bias", "layers.0.mlp.fc11.bias", "layers.0.mlp.fc12.bias"):
            out[f"{pooling}/g/{k}"] = grads[k].numpy()
    cfg_rec = {"cfg/" + k: np.array(v) for k, v in cfgd.items()}
    np.savez_compressed(GOLD / f"{name}.npz", **out, **cfg_rec)
    print(name, "hidden", tuple(hid.shape))


def gen_timm_remap(seed):
    """A timm-keyed EVA-02 state dict (q / v biases, no k bias, fc1_x / fc1_g, mlp.norm, 4-D patch kernel, head / fc_norm)
    at the tiny sizes, and the reference's remap of it."""
    from transformers import GPT2Config

    tv = importlib.import_module("contrastors.models.vit.timm_vit")
    c = SimpleNamespace(**REMAP)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d, I, p = c.n_embd, c.n_inner, c.patch_size
    P = (c.img_size // p) ** 2
    sd = {"cls_token": rn(1, 1, d), "pos_embed": rn(1, P + 1, d), "patch_embed.proj.weight": rn(d, 3, p, p),
          "patch_embed.proj.bias": rn(d), "head.weight": rn(10, d), "head.bias": rn(10), "fc_norm.weight": rn(d),
          "fc_norm.bias": rn(d)}
    for l in range(c.n_layer):
        b = f"blocks.{l}."
        sd.update({b + "norm1.weight": rn(d), b + "norm1.bias": rn(d), b + "attn.qkv.weight": rn(3 * d, d),
                   b + "attn.q_bias": rn(d), b + "attn.v_bias": rn(d), b + "attn.proj.weight": rn(d, d),
                   b + "attn.proj.bias": rn(d), b + "norm2.weight": rn(d), b + "norm2.bias": rn(d),
                   b + "mlp.fc1_x.weight": rn(I, d), b + "mlp.fc1_x.bias": rn(I), b + "mlp.fc1_g.weight": rn(I, d),
                   b + "mlp.fc1_g.bias": rn(I), b + "mlp.norm.weight": rn(I), b + "mlp.norm.bias": rn(I),
                   b + "mlp.fc2.weight": rn(d, I), b + "mlp.fc2.bias": rn(d)})
    cfg = GPT2Config(n_embd=d, n_layer=c.n_layer, patch_size=p)
    out = tv.remap_timm_state_dict(dict(sd), cfg)
    rec = {"cfg/" + k: np.array(v) for k, v in REMAP.items()}
    rec.update({"in/" + k: v.numpy() for k, v in sd.items()})
    rec.update({"out/" + k: v.detach().numpy() for k, v in out.items()})
    np.savez_compressed(GOLD / "eva02_timm_remap.npz", **rec)
    print("eva02_timm_remap", len(sd), "->", len(out), "keys")


if __name__ == "__main__":
    torch.manual_seed(0)
    vit = load_reference()
    gen_tower(vit, "vit_eva02_tiny", TINY_EVA, 31)
    gen_timm_remap(41)
