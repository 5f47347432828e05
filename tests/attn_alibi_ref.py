"""Yardsticks for self-attention with ALiBi: attn_ref.reference and attn_ref.bf16_model with - slope[b, h] * |i - j| added to the
scaled scores of query i and key j of one sequence (flash-attn's alibi_slopes, non-causal).  slopes: (H,) or (B, H).  Same
layouts and result dicts as attn_ref; no rotary, no dropout; the slopes get no gradient.  Plain torch, calls no kernel."""
import torch

from tests.attn_ref import _round_bf16
from tests.attn_window_ref import _empty


def bias(slopes, b, l, dtype, device):
    """(H, l, l): - slope[b, h] * |i - j|."""
    s = torch.as_tensor(slopes, device=device).to(dtype)
    pos = torch.arange(l, device=device)
    return -(s[b] if s.dim() == 2 else s)[:, None, None] * (pos[:, None] - pos[None, :]).abs().to(dtype)


def alibi_reference(qkv, lens, slopes, scale, dout):
    """Float64, one sequence at a time, all heads at once."""
    f64 = torch.float64
    res, t0 = _empty(qkv, f64), 0
    for b, l in enumerate(lens):
        if l == 0:
            continue
        x = qkv[t0:t0 + l].to(f64)
        q, k, v, do = x[:, 0], x[:, 1], x[:, 2], dout[t0:t0 + l].to(f64)
        sc = torch.einsum("qhd,khd->hqk", q, k) * scale + bias(slopes, b, l, f64, qkv.device)
        lse = torch.logsumexp(sc, -1)                                   # (H, l)
        P = torch.exp(sc - lse[..., None])
        out = torch.einsum("hqk,khd->qhd", P, v)
        dP = torch.einsum("qhd,khd->hqk", do, v)
        delta = (do * out).sum(-1).transpose(0, 1)                      # (H, l)
        dS = P * (dP - delta[..., None])
        res["out"][t0:t0 + l], res["lse"][:, t0:t0 + l] = out, lse
        res["dq"][t0:t0 + l] = torch.einsum("hqk,khd->qhd", dS, k) * scale
        res["dk"][t0:t0 + l] = torch.einsum("hqk,qhd->khd", dS, q) * scale
        res["dv"][t0:t0 + l] = torch.einsum("hqk,qhd->khd", P, do)
        t0 += l
    return res


def alibi_model(qkv, lens, slopes, scale, dout):
    """fp32 with the kernels' documented rounding points (see attn_ref.bf16_model): the bias formed in fp32; P rounded to bf16 for
    P V, the row sum from the unrounded P; out stored bf16; P recomputed from the stored lse; delta from the stored out; dS
    rounded to bf16; dq / dk / dv stored bf16."""
    f32 = torch.float32
    res, t0 = _empty(qkv, f32), 0
    for b, l in enumerate(lens):
        if l == 0:
            continue
        x = qkv[t0:t0 + l].to(f32)
        q, k, v, do = x[:, 0], x[:, 1], x[:, 2], dout[t0:t0 + l].to(f32)
        sc = torch.einsum("qhd,khd->hqk", q, k) * scale + bias(slopes, b, l, f32, qkv.device)
        m = sc.amax(-1, keepdim=True)
        E = torch.exp(sc - m)
        rowsum = E.sum(-1, keepdim=True)
        lse = (m + torch.log(rowsum))[..., 0]                           # (H, l) stored fp32
        out = _round_bf16(torch.einsum("hqk,khd->qhd", _round_bf16(E), v) / rowsum[..., 0].transpose(0, 1)[..., None])
        P = torch.exp(sc - lse[..., None])
        dP = torch.einsum("qhd,khd->hqk", do, v)
        delta = (do * out).sum(-1).transpose(0, 1)
        dS = _round_bf16(P * (dP - delta[..., None]))
        res["out"][t0:t0 + l], res["lse"][:, t0:t0 + l] = out, lse
        res["dq"][t0:t0 + l] = _round_bf16(torch.einsum("hqk,khd->qhd", dS, k) * scale)
        res["dk"][t0:t0 + l] = _round_bf16(torch.einsum("hqk,qhd->khd", dS, q) * scale)
        res["dv"][t0:t0 + l] = _round_bf16(torch.einsum("hqk,qhd->khd", _round_bf16(P), do))
        t0 += l
    return res
