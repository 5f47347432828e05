"""Yardsticks for sliding-window self-attention: attn_ref.reference and attn_ref.bf16_model with the band mask added to the
scores.  Query i of a sequence sees key j of the same sequence iff i - left <= j <= i + right (-1 = unbounded on that side).
Same layouts and result dicts as attn_ref; no rotary, no dropout.  Plain torch, calls no kernel."""
import torch

from tests.attn_ref import OUTPUTS, _round_bf16


def band(l, window, device):
    """(l, l) bool: True where query row i sees key column j."""
    d = torch.arange(l, device=device)[None, :] - torch.arange(l, device=device)[:, None]    # j - i
    left, right = window
    return (d >= (-left if left >= 0 else -l)) & (d <= (right if right >= 0 else l))


def _empty(qkv, dtype):
    T, _, H, D = qkv.shape
    res = {k: torch.zeros(T, H, D, dtype=dtype, device=qkv.device) for k in OUTPUTS}
    res["lse"] = torch.zeros(H, T, dtype=dtype, device=qkv.device)
    return res


def window_reference(qkv, lens, window, scale, dout):
    """Float64, one sequence at a time, all heads at once."""
    f64 = torch.float64
    res, t0 = _empty(qkv, f64), 0
    for l in lens:
        if l == 0:
            continue
        x = qkv[t0:t0 + l].to(f64)
        q, k, v, do = x[:, 0], x[:, 1], x[:, 2], dout[t0:t0 + l].to(f64)
        sc = (torch.einsum("qhd,khd->hqk", q, k) * scale).masked_fill(~band(l, window, qkv.device), float("-inf"))
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


def window_model(qkv, lens, window, scale, dout):
    """fp32 with the kernels' documented rounding points (see attn_ref.bf16_model): P rounded to bf16 for P V, the row sum from
    the unrounded P; out stored bf16; P recomputed from the stored lse; delta from the stored out; dS rounded to bf16; dq / dk /
    dv stored bf16."""
    f32 = torch.float32
    res, t0 = _empty(qkv, f32), 0
    for l in lens:
        if l == 0:
            continue
        x = qkv[t0:t0 + l].to(f32)
        q, k, v, do = x[:, 0], x[:, 1], x[:, 2], dout[t0:t0 + l].to(f32)
        sc = (torch.einsum("qhd,khd->hqk", q, k) * scale).masked_fill(~band(l, window, qkv.device), float("-inf"))
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
