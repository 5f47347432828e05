"""Yardsticks for the variable-length self-attention kernels: a float64 reference, an fp32 model with the kernels'
documented bf16 rounding points, a per-row error metric, seeded input families and the acceptance rule built on them.
Plain torch, runs on CPU or GPU, calls no kernel.

Layouts are the C-ABI's: qkv (T, 3, H, 64) packed over the sequences of `lens`, dout / out (T, H, 64), lse (H, T) natural
log, dq / dk / dv (T, H, 64) with dq / dk un-rotated.  `cos` / `sin` are the (>= max(lens), 32) fp32 tables of the full
non-interleaved rotary, or None.  `keep` / `p_drop` describe attention dropout: keep (B, H, S, S) in {0, 1}, S >= max(lens).
"""
from __future__ import annotations

import math

import torch

OUTPUTS = ("out", "dq", "dk", "dv")
FAMILIES = ("gauss", "peaked", "shift_pos", "shift_neg", "max_first", "max_last", "sentinel", "uniform")
FACTOR = 3.0             # the project's "3 x bf16-eager" rule, with bf16_model in the place of bf16-eager
BF16_HALF_ULP = 2.0 ** -9  # stands in for a model error of exactly 0 (the uniform family): one rounding of a stored bf16 value


def _rot(u, c, s):
    """Full non-interleaved rotation of (l, H, 64) rows by the (l, 1, 32) tables; (c, -s) is the inverse."""
    u1, u2 = u[..., :32], u[..., 32:]
    return torch.cat([u1 * c - u2 * s, u2 * c + u1 * s], -1)


def _round_bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def rotate_bf16(u, cos, sin):
    """Rotated q / k rows as every kernel forms them (csrc/cx_common.h, rotary_pair): fp32, the second product rounded by
    itself, the first fused into the sum, then one rounding to bf16.  u: (l, H, 64) holding bf16 values, cos / sin (>= l, 32)
    fp32.  The FMA is taken in float64 (a bf16 x fp32 product is exact there).  Returns float32 holding bf16 values."""
    l = u.shape[0]
    u = u.to(torch.float32)
    x1, x2 = u[..., :32], u[..., 32:]
    c, s = cos[:l, None, :].to(torch.float32), sin[:l, None, :].to(torch.float32)
    o1 = (x1.double() * c.double() - (x2 * s).double()).float()
    o2 = (x2.double() * c.double() + (x1 * s).double()).float()
    return _round_bf16(torch.cat([o1, o2], -1))


def _tables(cos, sin, l, dtype):
    return cos[:l, None, :].to(dtype), sin[:l, None, :].to(dtype)


def _drop_scale(keep, b, l, p_drop, dtype):
    return None if keep is None else keep[b, :, :l, :l].to(dtype) / (1.0 - p_drop)


def reference(qkv, lens, cos, sin, scale, dout, keep=None, p_drop=0.0):
    """Float64, one sequence at a time, all heads at once.  The only modelled rounding: rotated q / k are bf16 before the
    products (the fused kernels and the in-place rotary op both store them so), formed by rotate_bf16 -- the rotation's fp32
    operation order decides which way a value on a bf16 tie goes, so it is part of that rounding point; the gradient passes
    the rounding as the identity."""
    T, _, H, D = qkv.shape
    f64 = torch.float64
    res = {k: torch.zeros(T, H, D, dtype=f64, device=qkv.device) for k in OUTPUTS}
    res["lse"] = torch.zeros(H, T, dtype=f64, device=qkv.device)
    t0 = 0
    for b, l in enumerate(lens):
        if l == 0:
            continue
        x = qkv[t0:t0 + l].to(f64)
        q, k, v, do = x[:, 0], x[:, 1], x[:, 2], dout[t0:t0 + l].to(f64)
        if cos is not None:
            c, s = _tables(cos, sin, l, f64)
            q, k = rotate_bf16(q, cos, sin).to(f64), rotate_bf16(k, cos, sin).to(f64)
        sc = torch.einsum("qhd,khd->hqk", q, k) * scale
        lse = torch.logsumexp(sc, -1)                                   # (H, l)
        P = torch.exp(sc - lse[..., None])
        w = _drop_scale(keep, b, l, p_drop, f64)
        Pd = P if w is None else P * w
        out = torch.einsum("hqk,khd->qhd", Pd, v)
        dP = torch.einsum("qhd,khd->hqk", do, v)
        if w is not None:
            dP = dP * w
        delta = (do * out).sum(-1).transpose(0, 1)                      # (H, l)
        dS = P * (dP - delta[..., None])
        dq = torch.einsum("hqk,khd->qhd", dS, k) * scale
        dk = torch.einsum("hqk,qhd->khd", dS, q) * scale
        if cos is not None:
            dq, dk = _rot(dq, c, -s), _rot(dk, c, -s)
        res["out"][t0:t0 + l], res["lse"][:, t0:t0 + l] = out, lse
        res["dq"][t0:t0 + l], res["dk"][t0:t0 + l] = dq, dk
        res["dv"][t0:t0 + l] = torch.einsum("hqk,qhd->khd", Pd, do)
        t0 += l
    return res


def bf16_model(qkv, lens, cos, sin, scale, dout, keep=None, p_drop=0.0, key_window=None):
    """The same operation in fp32 with the rounding points the kernel sources document and nothing else: rotated q / k in
    bf16; P rounded to bf16 for P V, the row sum from the unrounded fp32 P; out stored bf16; the backward recomputes
    P = exp(s * scale - lse) from the stored fp32 lse; delta = rowsum(dO * O) from the stored bf16 out; dS rounded to bf16
    for the dQ / dK products; dq / dk / dv stored bf16.  No tiling, no online softmax, no exp2.

    key_window (tests of the metric only): {sequence index: (a, b)} makes that sequence's queries see the packed key rows
    [t0 + a, t0 + l + b) in the place of their own [t0, t0 + l) -- a planted masking error, no rotary."""
    T, _, H, D = qkv.shape
    f32 = torch.float32
    res = {k: torch.zeros(T, H, D, dtype=f32, device=qkv.device) for k in OUTPUTS}
    res["lse"] = torch.zeros(H, T, dtype=f32, device=qkv.device)
    t0 = 0
    for b, l in enumerate(lens):
        if l == 0:
            continue
        k0, k1 = t0, t0 + l
        if key_window and b in key_window:
            assert cos is None and keep is None
            k0, k1 = max(0, t0 + key_window[b][0]), min(T, t0 + l + key_window[b][1])
        q, do = qkv[t0:t0 + l, 0].to(f32), dout[t0:t0 + l].to(f32)
        k, v = qkv[k0:k1, 1].to(f32), qkv[k0:k1, 2].to(f32)
        if cos is not None:
            c, s = _tables(cos, sin, l, f32)
            q, k = rotate_bf16(q, cos, sin), rotate_bf16(k, cos, sin)
        sc = torch.einsum("qhd,khd->hqk", q, k) * scale
        m = sc.amax(-1, keepdim=True)
        E = torch.exp(sc - m)
        rowsum = E.sum(-1, keepdim=True)
        lse = (m + torch.log(rowsum))[..., 0]                           # (H, l) stored fp32
        w = _drop_scale(keep, b, l, p_drop, f32)
        out = torch.einsum("hqk,khd->qhd", _round_bf16(E if w is None else E * w), v) / rowsum[..., 0].transpose(0, 1)[..., None]
        out = _round_bf16(out)
        P = torch.exp(sc - lse[..., None])
        dP = torch.einsum("qhd,khd->hqk", do, v)
        if w is not None:
            dP = dP * w
        delta = (do * out).sum(-1).transpose(0, 1)
        dS = _round_bf16(P * (dP - delta[..., None]))
        dq = torch.einsum("hqk,khd->qhd", dS, k) * scale
        dk = torch.einsum("hqk,qhd->khd", dS, q) * scale
        if cos is not None:
            dq, dk = _rot(dq, c, -s), _rot(dk, c, -s)
        res["out"][t0:t0 + l], res["lse"][:, t0:t0 + l] = out, lse
        res["dq"][t0:t0 + l] = _round_bf16(dq)
        res["dk"][k0:k1] += _round_bf16(dk)
        res["dv"][k0:k1] += _round_bf16(torch.einsum("hqk,qhd->khd", _round_bf16(P if w is None else P * w), do))
        t0 += l
    return res


def row_errors(got, ref, lens):
    """(T, H) tensor: ||got - ref||_2 of each (token, head) row over max(||ref row||_2, rms), rms = the root mean square of the
    reference row norms of that sequence and head (rows that are ~0 by cancellation have no meaningful relative error)."""
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    diff, norm = (got - ref).norm(dim=-1), ref.norm(dim=-1)            # (T, H)
    err = torch.zeros_like(diff)
    t0 = 0
    for l in lens:
        if l:
            n = norm[t0:t0 + l]
            rms = n.pow(2).mean(0, keepdim=True).sqrt()
            err[t0:t0 + l] = diff[t0:t0 + l] / torch.maximum(n, rms).clamp_min(1e-300)
        t0 += l
    return err


def frobenius(got, ref):
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def locate(err, lens):
    """Where the worst row of a (T, H) error tensor sits: sequence, row, head and the kernels' tile units."""
    flat = int(err.argmax())
    t, h = divmod(flat, err.shape[1])
    t0 = 0
    for b, l in enumerate(lens):
        if t < t0 + l:
            r = t - t0
            return {"seq": b, "len": l, "row": r, "head": h, "from_end": l - 1 - r, "mod32": r % 32, "mod64": r % 64,
                    "mod128": r % 128, "mod256": r % 256}
        t0 += l
    return {"token": t, "head": h}


def ulp_fp32(x):
    """Spacing of fp32 at magnitude x."""
    return 2.0 ** (math.floor(math.log2(max(float(x), 2.0 ** -126))) - 23)


def judge(got, model, ref, lens, outputs=OUTPUTS, check_lse=True, zero_bounds=None):
    """The acceptance rule.  For each output: worst row error and whole-tensor Frobenius error of `got` against `ref` at most
    FACTOR x those of `model` against `ref`; for lse: max |got - ref| <= FACTOR x the model's + 4 ulp_fp32(max |ref|) (the
    kernels form lse through exp2 / log2 with the scale folded in, the model does not).  A model error of exactly 0 counts
    as one bf16 rounding.  Rows whose exact value is 0 (zero_bounds, see zero_grad_bounds) have no relative error: their norm is
    held to the bound given and they are left out of the two relative figures.  Returns (figures, failures): figures for the
    report, failures as readable strings."""
    fig, fails = {}, []
    got, model = dict(got), dict(model)
    for name, bound in (zero_bounds or {}).items():
        rows = torch.isfinite(bound)
        if name not in outputs or not rows.any():
            continue
        n = got[name].to(torch.float64).norm(dim=-1)
        bad = rows & ~(n <= bound)
        if bad.any():
            where = locate(torch.where(bad, n / bound.clamp_min(1e-300), torch.zeros_like(n)), lens)
            fails.append(f"{name}: {int(bad.sum())} rows whose exact value is 0 exceed their rounding bound, worst at {where}")
        got[name] = torch.where(rows[..., None], ref[name].to(got[name].dtype), got[name])
        model[name] = torch.where(rows[..., None], ref[name].to(model[name].dtype), model[name])
    for name in outputs:
        eg, em = row_errors(got[name], ref[name], lens), row_errors(model[name], ref[name], lens)
        fg, fm = frobenius(got[name], ref[name]), frobenius(model[name], ref[name])
        wg, wm = float(eg.max()), float(em.max())
        where = locate(eg, lens)
        fig[name] = {"row": wg, "model_row": wm, "fro": fg, "model_fro": fm, "where": where}
        if not torch.isfinite(got[name].float()).all():
            fails.append(f"{name}: not finite")
        if not wg <= FACTOR * (wm if wm > 0 else BF16_HALF_ULP):
            fails.append(f"{name}: worst row error {wg:.3e} > {FACTOR:g} x model {wm:.3e} at {where}")
        if not fg <= FACTOR * (fm if fm > 0 else BF16_HALF_ULP):
            fails.append(f"{name}: Frobenius error {fg:.3e} > {FACTOR:g} x model {fm:.3e}")
    if check_lse:
        r = ref["lse"].to(torch.float64)
        dg, dm = (got["lse"].to(torch.float64) - r).abs(), (model["lse"].to(torch.float64) - r).abs()
        wg, wm = float(dg.max()) if dg.numel() else 0.0, float(dm.max()) if dm.numel() else 0.0
        bound = FACTOR * wm + 4 * ulp_fp32(float(r.abs().max()) if r.numel() else 0.0)
        where = locate(dg.transpose(0, 1), lens) if dg.numel() else {}
        fig["lse"] = {"abs": wg, "model_abs": wm, "bound": bound, "where": where}
        if not wg <= bound:      # (a NaN fails here too)
            fails.append(f"lse: max |error| {wg:.3e} > bound {bound:.3e} (model {wm:.3e}) at {where}")
    return fig, fails


# ------------------------------------------------------------------------------------------------------ input families
def _orthonormal(H, n, g):
    """(H, n, 64): n orthonormal directions per head."""
    return torch.linalg.qr(torch.randn(H, 64, n, generator=g, dtype=torch.float64))[0].transpose(1, 2).float()


def make_inputs(family, lens, H, seed, cos=None, sin=None):
    """Seeded (qkv (T, 3, H, 64), dout (T, H, 64)) in bf16 on the CPU, all finite.  With tables the family is designed in
    the rotated frame and q / k are rotated back, so that the scores the kernels form after their rotation are the designed
    ones (up to one bf16 rounding).

    gauss      N(0, 1) everywhere: diffuse softmax (scores of unit variance at scale 1/8).
    peaked     q x 3, k x 2.5: near one-hot softmax.
    shift_pos / shift_neg
               a common unit direction u: q += 20 u, k += +-20 u -- every scaled score of a row moves by about +-50.
    max_first / max_last
               every q += 4 d; the first / last key of each sequence is 18 d: it dominates every row (scaled score 9 +- 2.25
               against O(1): about 0.98 of a row at 100 keys, 0.7 at 2049 -- strong, yet dq / dk are not all cancellation),
               and for max_last the running maximum arrives in the last, ragged key tile.
    sentinel   three orthonormal directions e0, e1, e2 per head.  First, middle and last query of sequence b are
               8 e2 + 8 e[(b + 1) % 2]; the last key of every sequence is 16 e2 (scaled score 16 for the chosen queries, v row
               +1); the first key of sequence b is 24 e[b % 2] (v row -1): invisible to the chosen queries of its own sequence,
               scaled score 24 for those of the sequence before it.  A key mask that is one too long lets it in and turns the
               row over; one that is one too short drops the last key and turns it as well; one that starts a row early lets
               in the previous sequence's last key at equal score.
    uniform    one k row and one v row per (sequence, head): P = 1 / len, out = v, lse = scale q . k + log(len), dq = dk = 0.
               Without tables only: keys rotated by position are not identical and the closed form is gone.
    """
    assert family in FAMILIES, family
    assert not (family == "uniform" and cos is not None)
    g = torch.Generator(device="cpu").manual_seed(seed)
    T = sum(lens)
    qkv = torch.randn(T, 3, H, 64, generator=g)
    dout = torch.randn(T, H, 64, generator=g)
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
    dirs = _orthonormal(H, 3, g)
    starts = [sum(lens[:b]) for b in range(len(lens))]
    if family == "peaked":
        q *= 3.0
        k *= 2.5
    elif family in ("shift_pos", "shift_neg"):
        q += 20.0 * dirs[:, 0]
        k += (20.0 if family == "shift_pos" else -20.0) * dirs[:, 0]
    elif family in ("max_first", "max_last"):
        q += 4.0 * dirs[:, 0]
        for t0, l in zip(starts, lens):
            if l:
                k[t0 if family == "max_first" else t0 + l - 1] = 18.0 * dirs[:, 0]
    elif family == "sentinel":
        for b, (t0, l) in enumerate(zip(starts, lens)):
            if not l:
                continue
            for r in {0, l // 2, l - 1}:
                q[t0 + r] = 8.0 * dirs[:, 2] + 8.0 * dirs[:, (b + 1) % 2] + 0.1 * q[t0 + r]
            k[t0 + l - 1] = 16.0 * dirs[:, 2]
            v[t0 + l - 1] = 1.0
            k[t0] = 24.0 * dirs[:, b % 2] + (16.0 * dirs[:, 2] if l == 1 else 0.0)
            v[t0] = -1.0 if l > 1 else 1.0
    elif family == "uniform":
        for t0, l in zip(starts, lens):
            if l:
                k[t0:t0 + l] = k[t0].clone()
                v[t0:t0 + l] = v[t0].clone()
    if cos is not None:
        t0 = 0
        for l in lens:
            if l:
                c, s = cos[:l, None, :].cpu().float(), sin[:l, None, :].cpu().float()
                q[t0:t0 + l], k[t0:t0 + l] = _rot(q[t0:t0 + l], c, -s), _rot(k[t0:t0 + l], c, -s)
            t0 += l
    return qkv.to(torch.bfloat16), dout.to(torch.bfloat16)


def rotary_tables(n, D=64, base=1000.0):
    inv = 1.0 / (base ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(n).float(), inv)
    return torch.cos(fr).contiguous(), torch.sin(fr).contiguous()


def uniform_closed_form(qkv, lens, scale):
    """The uniform family without tables, in float64: out = v and lse = scale q . k + log(len)."""
    T, _, H, D = qkv.shape
    x = qkv.to(torch.float64)
    out = torch.zeros(T, H, D, dtype=torch.float64, device=qkv.device)
    lse = torch.zeros(H, T, dtype=torch.float64, device=qkv.device)
    t0 = 0
    for l in lens:
        if l:
            out[t0:t0 + l] = x[t0, 2]
            lse[:, t0:t0 + l] = ((x[t0:t0 + l, 0] * x[t0, 1]).sum(-1) * scale + math.log(l)).transpose(0, 1)
        t0 += l
    return out, lse


def zero_grad_bounds(qkv, lens, scale, dout, uniform=False, p_drop=0.0):
    """dq and dk are exactly 0 where every visible key carries the same v row: sequences of length 1, and every sequence of
    the uniform family.  There dP_qk = dO_q . v and delta_q = dO_q . out_q are the same number, so dS = P (dP - delta) is pure
    rounding and no relative error exists.  Returns {"dq", "dk"}: (T, H) bounds on the row norms there, +inf elsewhere.

    The bounds follow from the arithmetic, not from a measurement.  dP (MFMA: bf16 operands, fp32 accumulation over 64 products)
    and delta = rowsum(dO * O) with O = v exactly are one sum in two orders, each within 64 x 2^-24 of it relative to
    A_q = sum_i |dO_qi v_i|.  Under dropout the stored O = bf16(v / (1 - p)) adds one bf16 rounding (2^-9) to delta, and both
    carry the factor 1 / (1 - p).  So |dS_qk| <= P_qk x g x A_q with g = (2 x 64 x 2^-24 [+ 2^-9]) / (1 - p), sum_k P_qk = 1,
    P_qk = 1 / len where the keys are identical, and ||dq_q|| <= scale g A_q ||k||, ||dk_k|| <= scale g mean_q(A_q ||q_q||)
    (rotation preserves the norms).  A further 1.02 covers the bf16 roundings of dS and of the stored result and that of P."""
    T, _, H, D = qkv.shape
    x, do = qkv.to(torch.float64), dout.to(torch.float64)
    inf = torch.full((T, H), float("inf"), dtype=torch.float64, device=qkv.device)
    dq_b, dk_b = inf.clone(), inf.clone()
    g = (2 * 64 * 2.0 ** -24 + (2.0 ** -9 if p_drop > 0 else 0.0)) / (1.0 - p_drop) * 1.02
    t0 = 0
    for l in lens:
        if l == 1 or (uniform and l):
            q, k, v = x[t0:t0 + l, 0], x[t0, 1], x[t0, 2]               # k, v: (H, 64)
            A = (do[t0:t0 + l].abs() * v.abs()).sum(-1)                 # (l, H)
            dq_b[t0:t0 + l] = scale * g * A * k.norm(dim=-1)
            dk_b[t0:t0 + l] = scale * g * (A * q.norm(dim=-1)).mean(0, keepdim=True)
        t0 += l
    return {"dq": dq_b, "dk": dk_b}
