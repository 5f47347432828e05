"""flash_attn.flash_attn_interface: K1/K2 (sc/layers/attention.py:158-182,220-226)."""
from __future__ import annotations

import math

import torch

from .. import _C


def _scale(softmax_scale, d):
    if softmax_scale is None:
        return 1.0 / math.sqrt(d)
    return float(softmax_scale)  # contrastors passes a 0-dim tensor (attention.py:46,163)


def _draw_philox(device):
    """(seed, offset) from the device generator, advanced as a torch dropout op would (RandContext replays it)."""
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    off = gen.get_offset()
    gen.set_offset(off + 4)
    return gen.initial_seed() & (2**64 - 1), off


class _VarlenQKVPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, scale, dropout_p=0.0, window=None, slopes=None):
        if qkv.dtype != torch.bfloat16 or qkv.dim() != 4 or qkv.shape[1] != 3 or qkv.shape[3] not in (32, 64):
            raise NotImplementedError("qkv must be bf16 (T,3,H,D) with head_dim D = 32 or 64")
        d32 = qkv.shape[3] == 32  # the head-pair kernels of csrc/attn_d32.hip
        if d32 and dropout_p:
            raise NotImplementedError("attention dropout > 0 at head_dim 32 is not built")
        if d32 and window is not None:
            raise NotImplementedError("a finite window_size at head_dim 32 is not built")
        if d32 and slopes is not None:
            raise NotImplementedError("alibi_slopes at head_dim 32 is not built")
        qkv = qkv.contiguous()
        T, _, H, D = qkv.shape
        B = cu_seqlens.numel() - 1
        cu = cu_seqlens.to(torch.int32)
        out = torch.empty(T, H, D, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(H, T, dtype=torch.float32, device=qkv.device)
        rng = None
        if slopes is not None:  # ALiBi: the kernels of csrc/attn_alibi.inc (no dropout, no window: _alibi_of refused them)
            slopes = _alibi_slopes(slopes, B, H, qkv.device)
            _C.check(_C.lib().cx_attn_varlen_alibi_fwd(qkv.data_ptr(), cu.data_ptr(), slopes.data_ptr(),
                                                       H if slopes.dim() == 2 else 0, out.data_ptr(), lse.data_ptr(), B, H, T,
                                                       int(max_seqlen), scale, _C.cur_stream()), "attn fwd (alibi)")
        elif d32:
            _C.check(_C.lib().cx_attn_varlen_d32_fwd(qkv.data_ptr(), cu.data_ptr(), out.data_ptr(), lse.data_ptr(), B, H, T,
                                                     int(max_seqlen), scale, _C.cur_stream()), "attn fwd (head_dim 32)")
        elif window is not None:  # a finite window: the banded kernels (no dropout, _window_of refused it)
            _C.check(_C.lib().cx_attn_varlen_window_fwd(qkv.data_ptr(), cu.data_ptr(), out.data_ptr(), lse.data_ptr(), B, H, T,
                                                        int(max_seqlen), window[0], window[1], scale, _C.cur_stream()),
                     "attn fwd (window)")
        elif dropout_p:
            rng = _draw_philox(qkv.device)
            _C.check(_C.lib().cx_attn_varlen_dropout_fwd(qkv.data_ptr(), cu.data_ptr(), None, None, out.data_ptr(),
                                                         lse.data_ptr(), B, H, T, int(max_seqlen), scale, float(dropout_p),
                                                         rng[0], rng[1], 0, _C.cur_stream()), "attn fwd (dropout)")
        else:
            _C.check(_C.lib().cx_attn_varlen_fwd(qkv.data_ptr(), cu.data_ptr(), None, None, out.data_ptr(), lse.data_ptr(),
                                                 B, H, T, int(max_seqlen), scale, _C.cur_stream()), "attn fwd")
        ctx.save_for_backward(qkv, out, lse, cu)
        ctx.meta = (B, H, T, int(max_seqlen), scale, float(dropout_p), rng, window)
        ctx.slopes = slopes
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, cu = ctx.saved_tensors
        B, H, T, mx, scale, p_drop, rng, window = ctx.meta
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        delta = torch.empty(H, T, dtype=torch.float32, device=qkv.device)
        if ctx.slopes is not None:
            sl = ctx.slopes
            _C.check(_C.lib().cx_attn_varlen_alibi_bwd(dout.data_ptr(), qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                       cu.data_ptr(), sl.data_ptr(), H if sl.dim() == 2 else 0, delta.data_ptr(),
                                                       dqkv.data_ptr(), B, H, T, mx, scale, _C.cur_stream()), "attn bwd (alibi)")
        elif qkv.shape[3] == 32:
            _C.check(_C.lib().cx_attn_varlen_d32_bwd(dout.data_ptr(), qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                     cu.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, H, T, mx, scale,
                                                     _C.cur_stream()), "attn bwd (head_dim 32)")
        elif window is not None:
            _C.check(_C.lib().cx_attn_varlen_window_bwd(dout.data_ptr(), qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                        cu.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, H, T, mx, window[0],
                                                        window[1], scale, _C.cur_stream()), "attn bwd (window)")
        elif p_drop:
            _C.check(_C.lib().cx_attn_varlen_dropout_bwd(dout.data_ptr(), qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                         cu.data_ptr(), None, None, delta.data_ptr(), dqkv.data_ptr(), B, H, T,
                                                         mx, scale, p_drop, rng[0], rng[1], 0, _C.cur_stream()),
                     "attn bwd (dropout)")
        else:
            _C.check(_C.lib().cx_attn_varlen_bwd(dout.data_ptr(), qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                 cu.data_ptr(), None, None, delta.data_ptr(), dqkv.data_ptr(), B, H, T, mx,
                                                 scale, _C.cur_stream()), "attn bwd")
        return dqkv, None, None, None, None, None, None


def _alibi_slopes(slopes, B, H, device):
    """alibi_slopes as the kernels read them: fp32, contiguous, on the qkv device, (H,) or (B, H), finite and >= 0."""
    slopes = torch.as_tensor(slopes).to(device=device, dtype=torch.float32).contiguous()
    if tuple(slopes.shape) not in ((H,), (B, H)):
        raise ValueError(f"alibi_slopes must have shape ({H},) or ({B}, {H}), got {tuple(slopes.shape)}")
    if not bool((torch.isfinite(slopes) & (slopes >= 0)).all()):
        raise ValueError("alibi_slopes must be finite and >= 0")
    return slopes


def _alibi_of(alibi_slopes, scale, dropout_p, window):
    """None without slopes (today's kernels, unchanged); else the slopes, after refusing what the ALiBi kernels do not serve."""
    if alibi_slopes is None:
        return None
    if dropout_p:
        raise NotImplementedError("alibi_slopes with attention dropout > 0 is not built")
    if window is not None:
        raise NotImplementedError("alibi_slopes with a finite window_size is not built")
    if not scale > 0:
        raise ValueError("alibi_slopes needs softmax_scale > 0")
    return alibi_slopes


def _no_alibi(alibi_slopes):
    if alibi_slopes is not None:
        raise NotImplementedError("alibi_slopes is built for the qkv-packed self-attention forms only")


def _window_of(window_size, max_seqlen, dropout_p):
    """flash-attn's window_size = (left, right), -1 = unbounded: query i sees the keys i - left .. i + right of its own sequence.
    None when the window covers every pair of a sequence of max_seqlen rows (today's kernels, unchanged), else (left, right)."""
    left, right = (int(w) for w in window_size)
    if left < -1 or right < -1:
        raise ValueError("window_size: each side is -1 (unbounded) or >= 0")
    if all(w < 0 or w >= int(max_seqlen) - 1 for w in (left, right)):
        return None
    if dropout_p:
        raise NotImplementedError("attention dropout > 0 with a finite window_size is not built")
    return left, right


def _no_window(window_size):
    left, right = (int(w) for w in window_size)
    if left < -1 or right < -1:
        raise ValueError("window_size: each side is -1 (unbounded) or >= 0")
    if left >= 0 or right >= 0:
        raise NotImplementedError("a finite window_size is built for the qkv-packed self-attention forms only")


def _check(dropout_p, causal, return_attn_probs, dropout_ok=False):
    if dropout_p and not dropout_ok:
        raise NotImplementedError("attention dropout > 0 is built for the qkv-packed self-attention forms only")
    if dropout_p and not 0.0 < dropout_p < 1.0:
        raise ValueError("dropout_p must be in [0, 1)")
    if causal:
        raise NotImplementedError("causal attention is out of the encoder hot-path scope")
    if return_attn_probs:
        raise NotImplementedError("return_attn_probs")


def flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                                     window_size=(-1, -1), alibi_slopes=None, deterministic=False,
                                     return_attn_probs=False):
    _check(dropout_p, causal, return_attn_probs, dropout_ok=True)
    scale, window = _scale(softmax_scale, qkv.shape[-1]), _window_of(window_size, max_seqlen, dropout_p)
    return _VarlenQKVPacked.apply(qkv, cu_seqlens, max_seqlen, scale, float(dropout_p), window,
                                  _alibi_of(alibi_slopes, scale, dropout_p, window))


def flash_attn_qkvpacked_func(qkv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                              alibi_slopes=None, deterministic=False, return_attn_probs=False):
    """(B,S,3,H,64 or 32) fixed-length form (the ViT path, attention.py:220-226): same kernel, cu_seqlens = arange * S."""
    _check(dropout_p, causal, return_attn_probs, dropout_ok=True)
    B, S = qkv.shape[:2]
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=qkv.device)
    scale, window = _scale(softmax_scale, qkv.shape[-1]), _window_of(window_size, S, dropout_p)
    out = _VarlenQKVPacked.apply(qkv.reshape(B * S, *qkv.shape[2:]), cu, S, scale, float(dropout_p), window,
                                 _alibi_of(alibi_slopes, scale, dropout_p, window))
    return out.view(B, S, *out.shape[1:])


class _VarlenKVPacked(torch.autograd.Function):
    """K3: q (Tq,H,64) x kv (Tk,2,H,64) cross-attention per batch entry (cx_attn_varlen_kvpacked_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, q, kv, cu_q, cu_k, max_q, max_k, scale):
        if q.dim() == 3 and q.shape[2] == 32:
            raise NotImplementedError("head_dim 32 is built for the qkv-packed self-attention forms only (kv-packed: 64)")
        if q.dtype != torch.bfloat16 or q.dim() != 3 or q.shape[2] != 64:
            raise NotImplementedError("q must be bf16 (Tq,H,64)")
        if kv.dtype != torch.bfloat16 or kv.dim() != 4 or kv.shape[1] != 2 or kv.shape[3] != 64:
            raise NotImplementedError("kv must be bf16 (Tk,2,H,64)")
        if kv.shape[2] != q.shape[1]:
            raise NotImplementedError("MQA / GQA (num_heads_kv != num_heads) is not built (the reference does not use it)")
        q, kv = q.contiguous(), kv.contiguous()
        Tq, H, D = q.shape
        B = cu_q.numel() - 1
        if cu_k.numel() != B + 1:
            raise ValueError("cu_seqlens_q and cu_seqlens_k must describe the same batch")
        cu_q, cu_k = cu_q.to(torch.int32), cu_k.to(torch.int32)
        out = torch.empty(Tq, H, D, dtype=q.dtype, device=q.device)
        lse = torch.empty(H, max(Tq, 1), dtype=torch.float32, device=q.device)
        _C.check(_C.lib().cx_attn_varlen_kvpacked_fwd(q.data_ptr(), kv.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(),
                                                      out.data_ptr(), lse.data_ptr(), B, H, Tq, int(max_q), int(max_k), scale,
                                                      _C.cur_stream()), "cross-attn fwd")
        ctx.save_for_backward(q, kv, out, lse, cu_q, cu_k)
        ctx.meta = (B, H, Tq, int(max_q), int(max_k), scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, out, lse, cu_q, cu_k = ctx.saved_tensors
        B, H, Tq, mq, mk, scale = ctx.meta
        dout = dout.contiguous()
        dq = torch.empty_like(q)
        dkv = torch.zeros_like(kv)   # (keys outside every cu_seqlens_k range, if any, get a zero gradient)
        delta = torch.empty(H, max(Tq, 1), dtype=torch.float32, device=q.device)
        _C.check(_C.lib().cx_attn_varlen_kvpacked_bwd(dout.data_ptr(), q.data_ptr(), kv.data_ptr(), out.data_ptr(),
                                                      lse.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), delta.data_ptr(),
                                                      dq.data_ptr(), dkv.data_ptr(), B, H, Tq, mq, mk, scale,
                                                      _C.cur_stream()), "cross-attn bwd")
        return dq, dkv, None, None, None, None, None


def flash_attn_varlen_kvpacked_func(q, kv, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0,
                                    softmax_scale=None, causal=False, window_size=(-1, -1), alibi_slopes=None,
                                    deterministic=False, return_attn_probs=False):
    """(Tq,H,64) x (Tk,2,H,64) -> (Tq,H,64): FlashAttentionPooling's varlen branch (sc/layers/attention.py:391-419)."""
    _check(dropout_p, causal, return_attn_probs)
    _no_window(window_size)
    _no_alibi(alibi_slopes)
    return _VarlenKVPacked.apply(q, kv, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                 _scale(softmax_scale, q.shape[-1]))


def flash_attn_kvpacked_func(q, kv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                             alibi_slopes=None, deterministic=False, return_attn_probs=False):
    """(B,Sq,H,64) x (B,Sk,2,H,64) -> (B,Sq,H,64): FlashAttentionPooling's fixed-length branch (attention.py:420-428)."""
    _check(dropout_p, causal, return_attn_probs)
    _no_window(window_size)
    _no_alibi(alibi_slopes)
    B, Sq = q.shape[:2]
    Sk = kv.shape[1]
    cu_q = torch.arange(0, (B + 1) * Sq, Sq, dtype=torch.int32, device=q.device)
    cu_k = torch.arange(0, (B + 1) * Sk, Sk, dtype=torch.int32, device=q.device)
    out = _VarlenKVPacked.apply(q.reshape(B * Sq, *q.shape[2:]), kv.reshape(B * Sk, *kv.shape[2:]), cu_q, cu_k, Sq, Sk,
                                _scale(softmax_scale, q.shape[-1]))
    return out.view(B, Sq, *out.shape[1:])
