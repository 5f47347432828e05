"""Logit-free linear + cross-entropy: `cross_entropy(x @ weight.T + bias, labels)` for a vocabulary-sized
`weight` without the (M, V) logits.  Forward: `cx_linear_xent_fwd` (csrc/linear_xent.hip) keeps an online log-sum-exp per token row
while it walks the vocabulary.  Backward: per chunk of `chunk_cols` vocabulary columns `cx_linear_xent_grad` recomputes the logits
and writes the bf16 gradient G and its transpose; the bf16 GEMM family then forms dX += G W[chunk] (fp32 across chunks, rounded
once) and dW[chunk] = G^T X.  The working set is two (M, chunk_cols) bf16 buffers, whatever V is.  No CPU path.
"""
from __future__ import annotations

import torch

from . import _C

_TILE = 128


def _up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


class _LinearXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, labels, ignore_index, chunk_cols):
        lib, s = _C.lib(), _C.cur_stream()
        M, K = x.shape
        V = weight.shape[0]
        x16 = x.to(torch.bfloat16)
        if x16.stride(1) != 1 or x16.stride(0) % 8 or x16.stride(0) < K or x16.data_ptr() % 16:
            x16 = x16.contiguous()
        w16 = weight.to(torch.bfloat16).contiguous()   # cast once (a no-op for a bf16 weight); the backward reuses it
        b32 = None if bias is None else bias.float().contiguous()
        ws = torch.empty(lib.cx_linear_xent_ws_floats(M, V), dtype=torch.float32, device=x.device)
        lse = torch.empty(M, dtype=torch.float32, device=x.device)
        loss = torch.empty(M, dtype=torch.float32, device=x.device)
        _C.check(lib.cx_linear_xent_fwd(x16.data_ptr(), w16.data_ptr(), _C.ptr(b32), labels.data_ptr(), ws.data_ptr(),
                                        lse.data_ptr(), loss.data_ptr(), M, V, K, x16.stride(0), ignore_index, s),
                 "cx_linear_xent_fwd")
        ctx.save_for_backward(x16, w16, b32, labels, lse)
        ctx.meta = (ignore_index, chunk_cols, x.dtype, weight.dtype, None if bias is None else bias.dtype)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib, s = _C.lib(), _C.cur_stream()
        x16, w16, b32, labels, lse = ctx.saved_tensors
        ignore_index, chunk_cols, xdtype, wdtype, bdtype = ctx.meta
        M, K = x16.shape
        V = w16.shape[0]
        dev = x16.device
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], b32 is not None and ctx.needs_input_grad[2]
        dloss = dloss.to(torch.float32).contiguous()
        Vc = min(_up(chunk_cols, _TILE), _up(V, _TILE))
        Mp = _up(M, _TILE)
        g = torch.empty(M, Vc, dtype=torch.bfloat16, device=dev)
        gt = torch.empty(Vc, Mp, dtype=torch.bfloat16, device=dev)
        dx32 = dw = db = dwc = xt = wt = None
        ws_floats = 0
        if need_x:
            dx32 = torch.zeros(M, K, dtype=torch.float32, device=dev)
            wt = torch.empty(K, Vc, dtype=torch.bfloat16, device=dev)
            ws_floats = M * K
        if need_w:
            dw = torch.empty(V, K, dtype=wdtype, device=dev)
            dwc = torch.empty(Vc, K, dtype=torch.float32, device=dev)
            xt = torch.empty(K, Mp, dtype=torch.bfloat16, device=dev)   # X^T once: the NT operand of every chunk's wgrad
            _C.check(lib.cx_transpose_bf16(x16.data_ptr(), xt.data_ptr(), M, K, x16.stride(0), Mp, Mp, s), "transpose x")
            ws_floats = max(ws_floats, Vc * K)
        if need_b:
            db = torch.empty(V, dtype=torch.float32, device=dev)
        # split-K workspace of the accumulating GEMMs: one slab is required, up to 8 let more K slices run at once
        gws = torch.empty(min(8 * ws_floats, max(ws_floats, 1 << 25)), dtype=torch.float32, device=dev) if ws_floats else None
        for v0 in range(0, V, Vc):
            vc = min(Vc, V - v0)
            _C.check(lib.cx_linear_xent_grad(x16.data_ptr(), w16.data_ptr(), _C.ptr(b32), labels.data_ptr(), lse.data_ptr(),
                                             dloss.data_ptr(), g.data_ptr(), gt.data_ptr(),
                                             db[v0:].data_ptr() if need_b else None, M, V, K, x16.stride(0), v0, vc,
                                             ignore_index, s), "cx_linear_xent_grad")
            vp = _up(vc, _TILE)   # the kernel wrote (M, vp) and (vp, Mp) with these leading dimensions; padding is zero
            if need_x:   # dX (M, K) += G (M, vp) . (W[chunk]^T (K, vp))^T
                _C.check(lib.cx_transpose_bf16(w16[v0:].data_ptr(), wt.data_ptr(), vc, K, K, vp, vp, s), "transpose w")
                _C.check(lib.cx_gemm_bf16_nt_accum(g.data_ptr(), wt.data_ptr(), dx32.data_ptr(), gws.data_ptr(), gws.numel(),
                                                   M, K, vp, vp, vp, s), "gemm dx")
            if need_w:   # dW[chunk] (vp, K) = G^T (vp, Mp) . (X^T (K, Mp))^T
                dwc.zero_()
                _C.check(lib.cx_gemm_bf16_nt_accum(gt.data_ptr(), xt.data_ptr(), dwc.data_ptr(), gws.data_ptr(), gws.numel(),
                                                   vp, K, Mp, Mp, Mp, s), "gemm dw")
                dw[v0:v0 + vc].copy_(dwc[:vc])
        dx = dx32.to(xdtype) if need_x else None
        if need_b:
            db = db.to(bdtype)
        return dx, dw, db, None, None, None


def linear_cross_entropy(x, weight, bias, labels, ignore_index: int = -100, reduction: str = "mean", chunk_cols: int = 8192):
    """loss of `CrossEntropyLoss(ignore_index, reduction)(x @ weight.T + bias, labels)`, fp32, without the logits.

    x: (M, K) bf16 / fp32 (computed in bf16), weight: (V, K) (cast to bf16 once if it is not), bias: (V) or None, labels: (M) int64.
    K % 64 == 0, 64 <= K <= 1024.  Differentiable in x, weight and bias; under `torch.no_grad()` only the forward kernel runs.
    `chunk_cols` (rounded up to a multiple of 128) is the vocabulary chunk of the backward: it bounds the working set and does
    not change the forward."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"x must be (M, K) and weight (V, K); got {tuple(x.shape)} and {tuple(weight.shape)}")
    M, K = x.shape
    V = weight.shape[0]
    if K % 64 or not 64 <= K <= 1024:
        raise ValueError(f"K = {K}: the kernel covers K % 64 == 0, 64 <= K <= 1024")
    if M < 1 or V < 1:
        raise ValueError("empty x or weight")
    if labels.dim() != 1 or labels.shape[0] != M:
        raise ValueError(f"labels must be ({M},), got {tuple(labels.shape)}")
    if labels.dtype != torch.int64:
        raise ValueError(f"labels must be int64, got {labels.dtype}")
    if bias is not None and tuple(bias.shape) != (V,):
        raise ValueError(f"bias must be ({V},), got {tuple(bias.shape)}")
    for t in (x, weight) + (() if bias is None else (bias,)):
        if t.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"dtype {t.dtype}: bf16 or fp32 only")
    if int(chunk_cols) < 1:
        raise ValueError("chunk_cols must be positive")
    if not (x.is_cuda and weight.is_cuda and labels.is_cuda and (bias is None or bias.is_cuda)):
        raise RuntimeError("linear_cross_entropy runs on the HIP kernels only (no CPU path)")
    labels = labels.contiguous()
    loss = _LinearXent.apply(x, weight, bias, labels, int(ignore_index), int(chunk_cols))
    if reduction == "mean":
        return loss.sum() / (labels != ignore_index).sum()
    if reduction == "sum":
        return loss.sum()
    return loss
