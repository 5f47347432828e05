"""Pure-torch restatement of the EVA-02 image tower (test infrastructure; the product never imports it).

Follows in behaviour the reference's ViTModel built from timm_name_to_vit_config("...vit_eva02_base_patch16_224...")
(sc/models/vit/timm_vit.py:71-167):
  * PatchEmbedding (sc/layers/embedding.py:465-516): Linear over (c, p1, p2) patches, [cls | patches] + pos_embed over all
    P + 1 positions, and the RoPE table of RotaryEmbeddingCat(in_pixels=False, ref_feat_shape) (:118-360);
  * FlashAttention with `rope` (sc/layers/attention.py:136-147): q and k of the patch tokens (not [cls]) rotated as
    x * cos + rot(x) * sin on interleaved pairs, in fp32, cast back to q's dtype;
  * GatedMLP with norm_layer (sc/layers/mlp.py:37-83): fc2(LayerNorm_1e-5(silu(fc12 x) * fc11 x));
  * pre-norm blocks, no final LayerNorm: the output is mlp_out + residual of the last block (sc/models/vit/vit.py:263-273).
Run it under torch.autocast(bfloat16) for the bf16-eager yardstick of the err(native) <= 3 err(bf16 eager) rule.
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn.functional as F

SUBLN_EPS = 1e-5


def random_state_dict(cfg, seed: int) -> Dict[str, torch.Tensor]:
    """Deterministic test weights with the reference's keys (std 0.05 matrices, LayerNorm gamma ~ 1, small biases)."""
    g = torch.Generator().manual_seed(seed)
    d, I = cfg.n_embd, cfg.n_inner
    P = (cfg.img_size // cfg.patch_size) ** 2
    pd = cfg.num_channels * cfg.patch_size ** 2
    rn = lambda *s, std=0.05: torch.randn(*s, generator=g) * std  # noqa: E731
    sd = {"embeddings.cls_token": rn(1, 1, d, std=0.5), "embeddings.pos_embed": rn(1, P + 1, d, std=0.5),
          "embeddings.proj.weight": rn(d, pd), "embeddings.proj.bias": rn(d)}
    for l in range(cfg.n_layer):
        p = f"layers.{l}."
        sd[p + "attn.Wqkv.weight"], sd[p + "attn.Wqkv.bias"] = rn(3 * d, d), rn(3 * d)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = rn(d, d), rn(d)
        sd[p + "mlp.fc11.weight"], sd[p + "mlp.fc11.bias"] = rn(I, d), rn(I)
        sd[p + "mlp.fc12.weight"], sd[p + "mlp.fc12.bias"] = rn(I, d), rn(I)
        sd[p + "mlp.norm.weight"], sd[p + "mlp.norm.bias"] = 1 + rn(I, std=0.1), rn(I, std=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(d, I), rn(d)
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = 1 + rn(d, std=0.1), rn(d, std=0.1)
    return sd


def rope_tables(cfg):
    """(n_patch, 32) fp32 cos / sin, angles [16 from the row | 16 from the column] per patch (before repeat_interleave)."""
    gsz = cfg.img_size // cfg.patch_size
    bands = 1.0 / (10000.0 ** (torch.arange(16, dtype=torch.float32) / 16))
    ref = getattr(cfg, "ref_feat_shape", None) or (gsz, gsz)
    t = [torch.arange(gsz, dtype=torch.float32) / gsz * r for r in ref]
    grid = torch.stack(torch.meshgrid(*t, indexing="ij"), -1).unsqueeze(-1) * bands
    return grid.cos().reshape(gsz * gsz, 32), grid.sin().reshape(gsz * gsz, 32)


def rope_apply(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, sign: int = 1) -> torch.Tensor:
    """x (..., P, H, 64) any dtype -> fp32 rotation of the interleaved pairs; sign = -1: the inverse rotation."""
    xf = x.float()
    c = cos.repeat_interleave(2, -1)[:, None, :]
    s = sign * sin.repeat_interleave(2, -1)[:, None, :]
    rot = torch.stack([-xf[..., 1::2], xf[..., ::2]], -1).reshape(xf.shape)
    return xf * c + rot * s


def patchify(pixels: torch.Tensor, p: int) -> torch.Tensor:
    B, C, H, W = pixels.shape
    x = pixels.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B, (H // p) * (W // p), C * p * p)


def eva_hidden(sd: Dict[str, torch.Tensor], cfg, pixels: torch.Tensor) -> torch.Tensor:
    """-> (B, P + 1, d): the residual stream after the last block."""
    d, H = cfg.n_embd, cfg.n_head
    eps = cfg.layer_norm_epsilon
    cos, sin = (t.to(pixels.device) for t in rope_tables(cfg))
    x = patchify(pixels.float(), cfg.patch_size) @ sd["embeddings.proj.weight"].T + sd["embeddings.proj.bias"]
    B = x.shape[0]
    x = torch.cat([sd["embeddings.cls_token"].expand(B, 1, d).to(x.dtype), x], 1) + sd["embeddings.pos_embed"]
    hidden, residual = x, None
    for l in range(cfg.n_layer):
        p = f"layers.{l}."
        residual = hidden if residual is None else hidden + residual
        h = F.layer_norm(residual, (d,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        qkv = (h @ sd[p + "attn.Wqkv.weight"].T + sd[p + "attn.Wqkv.bias"]).view(B, -1, 3, H, d // H)
        q, k, v = qkv.unbind(2)
        q = torch.cat([q[:, :1], rope_apply(q[:, 1:], cos, sin).to(q.dtype)], 1)
        k = torch.cat([k[:, :1], rope_apply(k[:, 1:], cos, sin).to(k.dtype)], 1)
        att = torch.einsum("bshd,bthd->bhst", q, k) / math.sqrt(d // H)
        ctx = torch.einsum("bhst,bthd->bshd", att.softmax(-1).to(v.dtype), v).reshape(B, -1, d)
        a = ctx @ sd[p + "attn.out_proj.weight"].T + sd[p + "attn.out_proj.bias"]
        residual = a + residual
        h = F.layer_norm(residual, (d,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
        y = h @ sd[p + "mlp.fc11.weight"].T + sd[p + "mlp.fc11.bias"]
        gate = h @ sd[p + "mlp.fc12.weight"].T + sd[p + "mlp.fc12.bias"]
        act = (F.silu(gate.float()) * y.float()).to(y.dtype)
        z = F.layer_norm(act, (act.shape[-1],), sd[p + "mlp.norm.weight"], sd[p + "mlp.norm.bias"], SUBLN_EPS)
        hidden = z @ sd[p + "mlp.fc2.weight"].T + sd[p + "mlp.fc2.bias"]
    return hidden + residual


def eva_embedding(sd, cfg, pixels, pooling: str = "cls", normalize: bool = True) -> torch.Tensor:
    h = eva_hidden(sd, cfg, pixels)
    e = h[:, 0] if pooling == "cls" else h.mean(1)
    return F.normalize(e.float(), dim=-1) if normalize else e.float()
