"""Sequence classification on the device: the typed embedding kernels and the fused head through the C ABI against the fp64
references of tests/seqcls_ref.py, the model against the reference's golden and its fp32 twin, and GlueTrainer.

Tolerances (none invented here):
  typed embedding   per row, the criterion of tests/ln_ref.py for the untyped embedding kernels (half a bf16 ulp + C 2^-24 S per
                    element, C = 4 x the fp32 emulation's worst ratio on the test's inputs; the type rows under "scatter", like
                    dtype0 there), with the constants measured on THESE inputs: tests/seqcls_ref.py TYPED_C_MEAS
  head              rel_err against fp64 <= max(3 x the error of the same restatement in fp32 eager torch, floor), floors 1e-5
                    (values) / 1e-4 (gradients): the rule of tests/test_distill_gpu.py
  model             tests/test_engine_gpu.py: |logit - golden| <= 5e-3 and <= 3 x bf16 eager + 1e-4; gradients
                    rel_err <= 3 x (bf16 eager + 1e-4) against the fp32 twin
"""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from contrastors_amd import _C
from contrastors_amd.config import Config, DataArgs, ModelArgs, TrainArgs
from contrastors_amd.glue import GlueTrainer, ShardedBatches
from contrastors_amd.nomic_bert import NomicBertConfig, NomicBertEngine, VarlenBatch
from contrastors_amd.seqcls import NomicBertForSequenceClassification
from contrastors_amd.trainers import TRAINER_REGISTRY
from oracle import encoder_ref
from oracle.make_golden import TINY_BERT
from tests import ln_ref as R
from tests import seqcls_ref as SR
from tests.gpu_util import L, S, max_err, rel_err, report
from tests.ln_ref import EPS24
from tests.seqcls_ref import TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
ERR_SHAPE, ERR_ARG = -1, -3
ROW_FLOOR, GRAD_FLOOR = 1e-5, 1e-4
NAN = float("nan")


def P(t):
    return None if t is None else t.data_ptr()


def dev(e, *keys):
    return {k: e[k].to(DEV) for k in keys}


def nan_like(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ================================================================================================== typed embedding
def embed_operands(e, use_pos=True):
    s = dev(e, "word", "type", "gamma", "beta", "ids", "tts", "indices", "da", "db")
    s["pos"] = e["pos"].to(DEV) if use_pos else None
    s["z"], s["tid"], s["p"], s["tt"] = SR.typed_embed_z(s["word"], s["type"], s["pos"], s["ids"], s["tts"], s["indices"], e["seq"])
    return s


def embed_fwd(s, e, d, typed=True, tts="own"):
    T = e["T"]
    out, mean, rstd = nan_like(T, d, dtype=BF), nan_like(T), nan_like(T)
    if typed:
        t = s["tts"] if isinstance(tts, str) else tts
        _C.check(L().cx_embed_ln_fwd_typed(s["ids"].data_ptr(), P(t), s["indices"].data_ptr(), s["word"].data_ptr(), s["type"].data_ptr(),
                                           2, P(s["pos"]), s["gamma"].data_ptr(), s["beta"].data_ptr(), out.data_ptr(), mean.data_ptr(),
                                           rstd.data_ptr(), T, e["seq"], d, 1e-12, S()), "embed_ln_fwd_typed")
    else:
        _C.check(L().cx_embed_ln_fwd(s["ids"].data_ptr(), s["indices"].data_ptr(), s["word"].data_ptr(), s["type"].data_ptr(),
                                     P(s["pos"]), s["gamma"].data_ptr(), s["beta"].data_ptr(), out.data_ptr(), mean.data_ptr(),
                                     rstd.data_ptr(), T, e["seq"], d, 1e-12, S()), "embed_ln_fwd")
    return out, mean, rstd


# ln_grid: one block per 4 tokens, at most 2048 blocks -> 8192 tokens is the last grid without a second token per wave
@pytest.mark.parametrize("d,T", SR.TYPED_FWD_SHAPES)
def test_typed_embed_fwd(d, T):
    """Sequences of 1, 5 and 128 tokens (S = 128) with padding-id tokens; segment ids all 0, all 1, and switching inside the
    sequences: per row against fp64.  All-zero types and NULL types are the untyped entry point bit for bit."""
    figures = {}
    for types in SR.TYPED_TYPES:
        e = SR.typed_embed_inputs(T, d, SR.TYPED_FWD_VOCAB, types=types)
        s = embed_operands(e)
        assert int((s["tid"] == e["pad_id"]).sum()) >= 3 and (types != "switch" or 0 < int(s["tt"].sum()) < T)
        out, mean, rstd = embed_fwd(s, e, d)
        f = R.ln_fwd_ref(s["z"], None, s["gamma"], s["beta"], 1e-12)
        figures[types] = dict(out=SR.check_typed_out(f"typed_embed[{types}].out", out, f),
                              mean=R.check_mean(f"typed_embed[{types}].mean", mean, f, TC("embed_fwd", "mean")),
                              rstd=R.check_rstd(f"typed_embed[{types}].rstd", rstd, f, TC("embed_fwd", "rstd")))
        if types == "zeros":
            plain = embed_fwd(s, e, d, typed=False)
            for a, b in zip((out, mean, rstd), plain):
                assert torch.equal(R.bits(a), R.bits(b)), "all-zero segment ids = the untyped kernel, bit for bit"
            for a, b in zip(embed_fwd(s, e, d, tts=None), plain):
                assert torch.equal(R.bits(a), R.bits(b)), "NULL segment ids = the untyped entry point, bit for bit"
        if types == "ones":      # row 1 is really read: the untyped kernel (row 0) gives another result
            assert not torch.equal(R.bits(out), R.bits(embed_fwd(s, e, d, typed=False)[0]))
    report("seqcls.cx_embed_ln_fwd_typed", d=d, T=T, **{f"{t}_{k}": v for t, r in figures.items() for k, v in r.items()})


def embed_bwd(s, e, d, form, typed=True, tts="own", ws_blocks=1024, two=True):
    """-> dict of the accumulators after one backward (all start at 0) and the fp64 reference."""
    T, V = e["T"], e["vocab"]
    st = R.ln_fwd_ref(s["z"], None, s["gamma"], None, 1e-12)
    mean, rstd = st.mean.float(), st.rstd.float()
    o = dict(dword=torch.zeros(V, d, device=DEV), dtype=torch.zeros(2, d, device=DEV), dpos=torch.zeros(e["seq"], d, device=DEV),
             dgamma=torch.zeros(d, device=DEV), dbeta=torch.zeros(d, device=DEV))
    db = s["db"] if two else None
    o["ref"] = R.ln_bwd_ref(s["da"], db, s["z"], s["gamma"], mean, rstd, None)
    ws = torch.empty(ws_blocks * 4 * d, device=DEV)       # per block [2][d] for the type rows + [2][d] for dgamma / dbeta
    head = (s["da"].data_ptr(), P(db), s["ids"].data_ptr())
    t = s["tts"] if isinstance(tts, str) else tts
    mid = (s["indices"].data_ptr(), s["word"].data_ptr(), s["type"].data_ptr())
    rest = (P(s["pos"]), s["gamma"].data_ptr(), mean.data_ptr(), rstd.data_ptr(), o["dword"].data_ptr(), o["dtype"].data_ptr(),
            o["dpos"].data_ptr(), o["dgamma"].data_ptr(), o["dbeta"].data_ptr())
    tail = (T, e["seq"], d, e["pad_id"])
    if form == "sorted":
        sids, perm = torch.sort(s["tid"].to(torch.int32), stable=True)
        o["scratch"] = nan_like(T, d)
        srt = (V, sids.data_ptr(), perm.to(torch.int32).data_ptr(), o["scratch"].data_ptr())
        if typed:
            _C.check(L().cx_embed_ln_bwd_sorted_typed(*head, P(t), *mid, 2, *rest, ws.data_ptr(), ws.numel(), *tail, *srt, S()),
                     "embed_ln_bwd_sorted_typed")
        else:
            _C.check(L().cx_embed_ln_bwd_sorted(*head, *mid, *rest, *tail, *srt, S()), "embed_ln_bwd_sorted")
    elif typed:
        _C.check(L().cx_embed_ln_bwd_typed(*head, P(t), *mid, 2, *rest, ws.data_ptr(), ws.numel(), *tail, S()), "embed_ln_bwd_typed")
    else:
        _C.check(L().cx_embed_ln_bwd(*head, *mid, *rest, *tail, S()), "embed_ln_bwd")
    torch.cuda.synchronize()
    return o


def check_typed_bwd(e, s, o, tag):
    ref, fam = o["ref"], "embed_bwd"
    bound = lambda what, scale: TC(fam, what) * EPS24 * scale   # noqa: E731
    r = dict(dgamma=R.check_rows(f"{tag}.dgamma", o["dgamma"], ref.dgamma, bound("dgamma", ref.dgamma_abs)),
             dbeta=R.check_rows(f"{tag}.dbeta", o["dbeta"], ref.dbeta, bound("dbeta", ref.dbeta_abs)))
    # both type rows: the scatter of the fp64 dz rows by segment id against 2^-24 x the sum of the rows' S, as dtype0 in the untyped tests
    r["dtype"] = R.check_rows(f"{tag}.dtype", o["dtype"], R.scatter_rows(ref.dz, s["tt"], 2), bound("dtype", R.scatter_rows(ref.scale, s["tt"], 2)))
    for row in (0, 1):       # a type row receives a gradient exactly when a token carries that type
        has, nonzero = bool((s["tt"] == row).any()), bool((o["dtype"][row] != 0).any())
        assert has == nonzero, f"{tag}: type row {row}: tokens {has}, gradient {nonzero}"
        if not has:
            assert bool((R.bits(o["dtype"][row]) == 0).all())
    r["dpos"] = R.check_rows(f"{tag}.dpos", o["dpos"], R.scatter_rows(ref.dz, s["p"], e["seq"]),
                             bound("scatter", R.scatter_rows(ref.scale, s["p"], e["seq"])))
    real = s["tid"] != e["pad_id"]
    assert int((~real).sum()) > 0
    r["dword"] = R.check_rows(f"{tag}.dword", o["dword"], R.scatter_rows(ref.dz[real], s["tid"][real], e["vocab"]),
                              bound("scatter", R.scatter_rows(ref.scale[real], s["tid"][real], e["vocab"])))
    assert bool((R.bits(o["dword"][e["pad_id"]]) == 0).all()), "nn.Embedding(padding_idx): that row gets no gradient"
    if "scratch" in o:
        r["dz"] = R.check_result(f"{tag}.dz_scratch", o["scratch"], ref.dz, ref.scale, TC(fam, "dz"))
    return r


# atomic form: ln_grid_bwd = at most 256 blocks x 4 waves -> 1024 tokens; sorted form: 1024 blocks -> 4096 tokens
@pytest.mark.parametrize("form,d,T", SR.TYPED_BWD_SHAPES)
def test_typed_embed_bwd(form, d, T):
    """One below, at and one above the token count that fills the launcher's grid; segment ids all 0, all 1, switching.  Both
    type rows, dgamma / dbeta, dpos and the word rows per element against fp64; the type rows and dgamma / dbeta -- folds of
    block partials in block order, no atomics -- are the same bits on a second run."""
    figures = {}
    for types in SR.TYPED_TYPES:
        e = SR.typed_embed_inputs(T, d, SR.TYPED_BWD_VOCAB, types=types)
        s = embed_operands(e)
        o = embed_bwd(s, e, d, form)
        figures[types] = check_typed_bwd(e, s, o, f"typed_{form}[{types}]")
        again = embed_bwd(s, e, d, form)
        for k in ("dtype", "dgamma", "dbeta"):
            assert torch.equal(R.bits(o[k]), R.bits(again[k])), f"{k} is reduced in a fixed order: the same bits on every run"
        if form == "sorted":
            assert torch.equal(R.bits(o["dword"]), R.bits(again["dword"])) and torch.equal(R.bits(o["scratch"]), R.bits(again["scratch"]))
            if types == "zeros":     # what the untyped form computes deterministically, it computes to the same bits
                plain = embed_bwd(s, e, d, form, typed=False)
                assert torch.equal(R.bits(o["dword"]), R.bits(plain["dword"])) and torch.equal(R.bits(o["scratch"]), R.bits(plain["scratch"]))
    report(f"seqcls.cx_embed_ln_bwd_{form}_typed", d=d, T=T, **{f"{t}_{k}": v for t, r in figures.items() for k, v in r.items()})


@pytest.mark.parametrize("form", ["atomic", "sorted"])
def test_typed_embed_bwd_null_types_and_small_workspace(form):
    """NULL segment ids are the untyped entry point: on one block of four distinct tokens (where its fp32 atomics have one
    possible order) every gradient has the same bits; on 1025 / 4097 tokens the deterministic results have, and the atomically
    reduced ones agree within the summation-order noise tests/test_checkpoint_gpu.py allows them (2e-5 of the largest entry).
    A workspace that holds 7 block partials caps the grid at 7 blocks, and dout_b may be NULL: the same bounds."""
    d = 768
    e = SR.typed_embed_inputs(4, d, 300, lens=(5,), types="zeros", n_pad=1)
    s = embed_operands(e)
    assert len(set(s["tid"].tolist())) == 4
    a, b = embed_bwd(s, e, d, form, tts=None), embed_bwd(s, e, d, form, typed=False)
    for k in ("dword", "dtype", "dpos", "dgamma", "dbeta"):
        assert torch.equal(R.bits(a[k]), R.bits(b[k])), k
    T = 1025 if form == "atomic" else 4097
    e = SR.typed_embed_inputs(T, d, SR.TYPED_BWD_VOCAB, types="switch")
    s = embed_operands(e)
    s0 = dict(s)                      # the untyped kernels add type row 0 to every token: the z of the statistics they are fed
    s0["z"] = SR.typed_embed_z(s["word"], s["type"], s["pos"], s["ids"], torch.zeros_like(s["tts"]), s["indices"], e["seq"])[0]
    a, b = embed_bwd(s0, e, d, form, tts=None), embed_bwd(s0, e, d, form, typed=False)
    assert bool((a["dtype"][1] == 0).all()) and bool((a["dtype"][0] != 0).any())
    for k in ("dword", "dtype", "dpos", "dgamma", "dbeta"):
        assert float((a[k] - b[k]).abs().max()) <= 2e-5 * float(b[k].abs().max()), k
    if form == "sorted":
        assert torch.equal(R.bits(a["dword"]), R.bits(b["dword"])) and torch.equal(R.bits(a["scratch"]), R.bits(b["scratch"]))
    small = embed_bwd(s, e, d, form, ws_blocks=SR.TYPED_SMALL_WS_BLOCKS)
    report(f"seqcls.typed_embed_small_ws_{form}", **check_typed_bwd(e, s, small, f"small_ws_{form}"))
    one = embed_bwd(s, e, d, form, two=False)          # dout_b NULL
    check_typed_bwd(e, s, one, f"one_branch_{form}")


# ============================================================================================================ the head
def head_inputs(B, d, Cn, mode, seed, ldx=None, ignore=0):
    g = torch.Generator().manual_seed(seed)
    ldx = ldx or d
    buf = torch.full((B, ldx), 7.0)            # (what lies past the width must not be read)
    buf[:, :d] = torch.randn(B, d, generator=g)     # a LayerNorm output: unit scale
    X = buf.to(DEV)[:, :d]
    Wp, bp = (torch.randn(d, d, generator=g) * 0.05).to(DEV), (torch.randn(d, generator=g) * 0.05).to(DEV)
    Wc, bc = (torch.randn(Cn, d, generator=g) * 0.05).to(DEV), (torch.randn(Cn, generator=g) * 0.05).to(DEV)
    if mode == 0:
        labels = torch.randint(0, Cn, (B,), generator=g)
        labels[torch.randperm(B, generator=g)[:ignore]] = -100
    else:
        labels = torch.randn(B, Cn, generator=g)
    return X, Wp, bp, Wc, bc, labels.to(DEV)


def head_fwd(X, Wp, bp, Wc, bc, labels, mode, drop=(0.0, 0, 0)):
    B, d, Cn = X.shape[0], X.shape[1], Wc.shape[0]
    pooled, logits, rows = nan_like(B, d), nan_like(B, Cn), nan_like(B)
    _C.check(L().cx_seqcls_head_fwd(X.data_ptr(), X.stride(0), Wp.data_ptr(), bp.data_ptr(), Wc.data_ptr(), bc.data_ptr(), P(labels),
                                    mode, drop[0], drop[1], drop[2], pooled.data_ptr(), logits.data_ptr(), rows.data_ptr(), B, d, Cn, S()),
             "cx_seqcls_head_fwd")
    return pooled, logits, rows


def head_bwd(X, Wp, Wc, pooled, logits, labels, mode, coef, drop=(0.0, 0, 0)):
    B, d, Cn = X.shape[0], X.shape[1], Wc.shape[0]
    ws = torch.empty(L().cx_seqcls_ws_floats(B, d, Cn), device=DEV)
    g = dict(dWp=nan_like(d, d), dbp=nan_like(d), dWc=nan_like(Cn, d), dbc=nan_like(Cn), dX=nan_like(B, d))
    _C.check(L().cx_seqcls_head_bwd(X.data_ptr(), X.stride(0), Wp.data_ptr(), Wc.data_ptr(), pooled.data_ptr(), logits.data_ptr(),
                                    labels.data_ptr(), mode, coef, drop[0], drop[1], drop[2], ws.data_ptr(), ws.numel(),
                                    g["dWp"].data_ptr(), g["dbp"].data_ptr(), g["dWc"].data_ptr(), g["dbc"].data_ptr(), g["dX"].data_ptr(),
                                    B, d, Cn, S()), "cx_seqcls_head_bwd")
    return g


def head_run(inp, mode, coef, drop=(0.0, 0, 0)):
    X, Wp, bp, Wc, bc, labels = inp
    pooled, logits, rows = head_fwd(X, Wp, bp, Wc, bc, labels, mode, drop)
    g = head_bwd(X, Wp, Wc, pooled, logits, labels, mode, coef, drop)
    return dict(pooled=pooled, logits=logits, loss_rows=rows, **g)


NAMES = ("pooled", "logits", "loss_rows", "dWp", "dbp", "dWc", "dbc", "dX")


def judge(name, got, inp, mode, coef, keep=None):
    X, Wp, bp, Wc, bc, labels = inp
    r64 = SR.head_ref(X, Wp, bp, Wc, bc, labels, mode, coef, keep, torch.float64)
    r32 = SR.head_ref(X, Wp, bp, Wc, bc, labels, mode, coef, keep, torch.float32)
    errs = {n: rel_err(got[n], r64[n]) for n in NAMES}
    eager = {n: rel_err(r32[n], r64[n]) for n in NAMES}
    print(f"seqcls head {name}: kernel {errs}  fp32 eager {eager}")
    report("seqcls.head", case=name, **{f"e_{k}": v for k, v in errs.items()}, **{f"eager_{k}": v for k, v in eager.items()})
    for n in NAMES:
        assert torch.isfinite(got[n]).all(), n
        floor = GRAD_FLOOR if n.startswith("d") else ROW_FLOOR
        assert errs[n] <= max(3 * eager[n], floor), f"{name}/{n}: kernel {errs[n]:.3e}, fp32 eager {eager[n]:.3e}"
    return r64


HEAD_CASES = {
    # name: (B, d, C, mode, ldx, rows labelled -100)
    "one_row": (1, 768, 2, 0, None, 0),
    "glue_16": (16, 768, 2, 0, None, 2),
    "33_rows_c3": (33, 768, 3, 0, 1024, 3),          # a third, ragged chunk of 16 rows; X inside a wider buffer
    "32_rows_c8": (32, 768, 8, 0, None, 0),
    "65_rows_mse_d256": (65, 256, 1, 1, 512, 0),     # past 64 rows: the 16-column forward tile; the backward's second 64-row pass
    "130_rows_mse_d1024": (130, 1024, 1, 1, None, 0),
    "4096_rows_c3": (4096, 768, 3, 0, None, 40),
}


@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_head_matches_float64_by_the_fp32_eager_rule(name):
    B, d, Cn, mode, ldx, ignore = HEAD_CASES[name]
    inp = head_inputs(B, d, Cn, mode, 40 + B, ldx, ignore)
    count = B - ignore
    got = head_run(inp, mode, 1.0 / count)
    r64 = judge(name, got, inp, mode, 1.0 / count)
    if ignore:
        dead = inp[5] == -100
        assert int(dead.sum()) == ignore and bool((got["loss_rows"][dead] == 0).all()) and bool((got["dX"][dead] == 0).all())
        assert bool((r64["dX"][dead] == 0).all())
    # no atomics anywhere: a second call gives the same bits
    again = head_run(inp, mode, 1.0 / count)
    for n in NAMES:
        assert torch.equal(R.bits(got[n]), R.bits(again[n])), n


def test_head_with_every_row_ignored_is_exactly_zero():
    inp = list(head_inputs(16, 768, 2, 0, 5))
    inp[5] = torch.full((16,), -100, device=DEV)
    got = head_run(inp, 0, 1.0)
    for n in ("loss_rows", "dWp", "dbp", "dWc", "dbc", "dX"):
        assert torch.equal(got[n], torch.zeros_like(got[n])), n      # 0, not NaN: nothing divides by the (zero) count
    assert torch.isfinite(got["logits"]).all() and torch.isfinite(got["pooled"]).all()


@pytest.mark.parametrize("name,B,d,Cn,mode", [("drop_33_c3", 33, 768, 3, 0), ("drop_65_mse", 65, 256, 1, 1)])
def test_head_dropout_matches_float64_under_the_host_philox_mask(name, B, d, Cn, mode):
    """p = 0.1: the kernels' mask is dropout_keep4 of (seed, offset, b * d + j), which tests/seqcls_ref.py evaluates on the host;
    forward and backward under THAT mask against fp64 -- one element kept on one side and dropped on the other would show as an
    error of the size of one pooled activation, four orders above the tolerance."""
    p, seed, offset = 0.1, 0x1234_5678_9ABC, 16
    inp = head_inputs(B, d, Cn, mode, 60 + B, None, 2 if mode == 0 else 0)
    count = B - (2 if mode == 0 else 0)
    keep = SR.head_keep(seed, offset, B, d, p).to(DEV)
    got = head_run(inp, mode, 1.0 / count, (p, seed, offset))
    judge(name, got, inp, mode, 1.0 / count, keep)
    again = head_run(inp, mode, 1.0 / count, (p, seed, offset))
    for n in NAMES:
        assert torch.equal(R.bits(got[n]), R.bits(again[n])), n
    other = head_run(inp, mode, 1.0 / count, (p, seed, offset + 4))           # another offset: another mask
    assert not torch.equal(got["logits"], other["logits"]) and torch.equal(got["pooled"], other["pooled"])


def test_head_dropout_mask_seen_through_one_row():
    """B = 1 makes the mask visible: dWc[c] = dl[c] * keep * pooled and dbp = dh * keep * (1 - pooled^2) are zero exactly where the
    backward dropped, and the logits rebuilt in fp64 from the mask read off dWc are the forward's -- so the regenerated mask is
    the forward's; it is the host Philox mask; survivors carry 1 / (1 - p); the kept count is inside the binomial 6 sigma band."""
    p, seed, offset, d = 0.1, 99, 4, 768
    X, Wp, bp, Wc, bc, labels = head_inputs(1, d, 2, 0, 71)
    got = head_run((X, Wp, bp, Wc, bc, labels), 0, 1.0, (p, seed, offset))
    r0 = SR.head_ref(X, Wp, bp, Wc, bc, labels, 0, 1.0, None)             # for d(loss)/d(logits) we need the logits: below
    pooled = got["pooled"].double()[0]
    assert rel_err(got["pooled"], r0["pooled"]) < 1e-5                     # the mask does not touch `pooled`
    z = got["logits"].double()[0]
    dl = torch.softmax(z, -1) - torch.nn.functional.one_hot(labels[0], 2).double()
    mask_bwd = got["dWc"].double()[0] / (dl[0] * pooled)                   # keep factor per column, read off the backward
    kept = mask_bwd != 0
    assert torch.equal(kept, got["dbp"] != 0) and torch.equal(kept, got["dWc"][1] != 0), "one mask for every backward product"
    inv = 1.0 / (1.0 - p)
    assert float((mask_bwd[kept] - inv).abs().max()) < 1e-4 * inv, "survivors are scaled by 1 / (1 - p)"
    logits_from_bwd_mask = (pooled * torch.where(kept, inv, 0.0)) @ Wc.double().T + bc.double()
    assert float((logits_from_bwd_mask - z).abs().max()) < 1e-5, "the backward regenerated the forward's mask"
    host = SR.head_keep(seed, offset, 1, d, p).to(DEV)[0]
    assert torch.equal(kept, host > 0), "dropout_keep4 keyed by (seed, offset + site, element / 4)"
    n_kept = int(kept.sum())
    assert abs(n_kept - (1 - p) * d) <= 6 * (d * p * (1 - p)) ** 0.5, n_kept
    big = SR.head_keep(seed, offset, 64, d, p)
    assert abs(int((big > 0).sum()) - (1 - p) * big.numel()) <= 6 * (big.numel() * p * (1 - p)) ** 0.5


def test_head_error_codes_leave_the_outputs_untouched():
    X, Wp, bp, Wc, bc, labels = head_inputs(16, 768, 2, 0, 81)
    pooled, logits, rows = nan_like(16, 768), nan_like(16, 2), nan_like(16)
    ws = torch.empty(16 * 768, device=DEV)
    g = [nan_like(768, 768), nan_like(768), nan_like(2, 768), nan_like(2), nan_like(16, 768)]

    def fwd(**kw):
        a = dict(X=X.data_ptr(), ldx=768, Wp=Wp.data_ptr(), bp=bp.data_ptr(), Wc=Wc.data_ptr(), bc=bc.data_ptr(), labels=labels.data_ptr(),
                 mode=0, p=0.0, B=16, d=768, C=2)
        a.update(kw)
        return L().cx_seqcls_head_fwd(a["X"], a["ldx"], a["Wp"], a["bp"], a["Wc"], a["bc"], a["labels"], a["mode"], a["p"], 0, 0,
                                      pooled.data_ptr(), logits.data_ptr(), rows.data_ptr(), a["B"], a["d"], a["C"], S())

    def bwd(**kw):
        a = dict(X=X.data_ptr(), Wp=Wp.data_ptr(), labels=labels.data_ptr(), mode=0, p=0.0, ws=ws.data_ptr(), ws_floats=ws.numel(), B=16,
                 d=768, C=2)
        a.update(kw)
        return L().cx_seqcls_head_bwd(a["X"], 768, a["Wp"], Wc.data_ptr(), pooled.data_ptr(), logits.data_ptr(), a["labels"], a["mode"],
                                      1.0, a["p"], 0, 0, a["ws"], a["ws_floats"], *[t.data_ptr() for t in g], a["B"], a["d"], a["C"], S())

    for kw in (dict(d=384), dict(d=2048), dict(C=0), dict(C=9), dict(B=0), dict(B=4097), dict(ldx=512)):
        assert fwd(**kw) == ERR_SHAPE, kw
    for kw in (dict(X=None), dict(Wp=None), dict(bp=None), dict(Wc=None), dict(bc=None), dict(mode=2), dict(p=1.0), dict(p=-0.5)):
        assert fwd(**kw) == ERR_ARG, kw
    for kw in (dict(d=384), dict(C=9), dict(B=4097), dict(B=0)):
        assert bwd(**kw) == ERR_SHAPE, kw
    for kw in (dict(X=None), dict(Wp=None), dict(labels=None), dict(ws=None), dict(ws_floats=16 * 768 - 1), dict(mode=3), dict(p=1.0)):
        assert bwd(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    for t in (pooled, logits, rows, *g):
        assert bool(torch.isnan(t).all()), "an error return launches nothing"
    # typed embedding: another type-table height launches nothing either
    e = SR.typed_embed_inputs(16, 256, 300, lens=(16,))
    s = embed_operands(e)
    out, mean, rstd = nan_like(16, 256, dtype=BF), nan_like(16), nan_like(16)
    for tv in (1, 3):
        assert L().cx_embed_ln_fwd_typed(s["ids"].data_ptr(), s["tts"].data_ptr(), s["indices"].data_ptr(), s["word"].data_ptr(),
                                         s["type"].data_ptr(), tv, P(s["pos"]), s["gamma"].data_ptr(), s["beta"].data_ptr(), out.data_ptr(),
                                         mean.data_ptr(), rstd.data_ptr(), 16, e["seq"], 256, 1e-12, S()) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(mean).all()) and bool(torch.isnan(rstd).all())


# =========================================================================================================== the model
TINY = NomicBertConfig(**{k: v for k, v in TINY_BERT.items() if k in NomicBertConfig.__dataclass_fields__})
TINY_NS = SimpleNamespace(**TINY_BERT)


def golden_model(gold, case, Cn, problem):
    g = gold("seqcls_tiny")
    trunk = encoder_ref.random_state_dict(TINY_NS, int(g["seed"]))
    sd = {f"bert.{k}": v for k, v in trunk.items()}
    sd.update({k: torch.from_numpy(g[f"{case}/head/{k}"]) for k in ("bert.pooler.dense.weight", "bert.pooler.dense.bias",
                                                                     "classifier.weight", "classifier.bias")})
    model = NomicBertForSequenceClassification(TINY, Cn, problem, device=DEV, seed=0)
    rep = model.load_reference_state_dict(sd)
    assert rep == {"fresh": [], "mismatched": [], "skipped": []}
    model.bert.sync_shadows()
    batch = {k: torch.from_numpy(g[k]).to(DEV) for k in ("input_ids", "attention_mask", "token_type_ids")}
    batch["labels"] = torch.from_numpy(g[f"{case}/labels"]).to(DEV)
    return g, sd, model, batch


def twin(sd, batch, mode, bf16=False, dtype=torch.float32):
    sdd = {k: v.detach().to(DEV, dtype).requires_grad_() for k, v in sd.items()}
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        loss, logits = SR.seqcls_twin(sdd, TINY_NS, batch["input_ids"], batch["attention_mask"], batch["token_type_ids"],
                                      batch["labels"].to(dtype) if mode else batch["labels"], mode)
    return loss.float(), logits.float(), sdd


@pytest.mark.parametrize("case,Cn,problem", [("c2", 2, "single_label_classification"), ("c3", 3, None), ("c1", 1, "regression")])
def test_model_matches_the_reference_golden_and_the_fp32_twin(gold, case, Cn, problem):
    g, sd, model, batch = golden_model(gold, case, Cn, problem)
    mode = 1 if Cn == 1 else 0
    model.train()                                            # (the tiny config has no dropout: training mode = the saving path)
    model.zero_grad()
    out = model(**batch)
    assert model.problem_type == ("regression" if Cn == 1 else "single_label_classification")     # None is inferred (:728-734)
    out.loss.backward()
    gold_logits, gold_loss = torch.from_numpy(g[f"{case}/logits"]).to(DEV), float(g[f"{case}/loss"])
    loss16, logits16, sd16 = twin(sd, batch, mode, bf16=True)
    loss32, logits32, sd32 = twin(sd, batch, mode)
    e_hip, e_b = max_err(out.logits, gold_logits), max_err(logits16, gold_logits)
    l_hip, l_b = abs(float(out.loss) - gold_loss), abs(float(loss16) - gold_loss)
    assert e_hip <= 5e-3 and e_hip <= 3 * e_b + 1e-4, (e_hip, e_b)
    assert l_hip <= 5e-3 and l_hip <= 3 * l_b + 1e-4, (l_hip, l_b)
    assert max_err(logits32, gold_logits) < 2e-5                      # the twin itself is the reference class
    loss32.backward()
    loss16.backward()
    grads = model.reference_grad_dict()
    word = "bert.embeddings.word_embeddings.weight"
    used = torch.unique(batch["input_ids"][batch["attention_mask"].bool()])
    figures = {}
    for n, gh in grads.items():
        r32, r16 = sd32[n].grad, sd16[n].grad
        if n == word:
            gh, r32, r16 = gh[used], r32[used], r16[used]
        elif n == "bert.embeddings.position_embeddings.weight":
            gh, r32, r16 = gh[:16], r32[:16], r16[:16]
        eh, eb = rel_err(gh, r32), rel_err(r16.float(), r32)
        figures[n] = (eh, eb)
        assert eh <= 3 * (eb + 1e-4), f"{n}: rel grad err {eh:.4f} vs bf16 eager {eb:.4f}"
    ty = grads["bert.embeddings.token_type_embeddings.weight"]
    assert bool((ty[0] != 0).any()) and bool((ty[1] != 0).any()), "both segment rows train"
    report("seqcls.model", case=case, e_logits=e_hip, e_logits_bf16=e_b, e_loss=l_hip, e_loss_bf16=l_b,
           worst=max(figures.items(), key=lambda kv: kv[1][0] / (kv[1][1] + 1e-4))[0],
           **{f"g_{k}": figures[k][0] for k in ("bert.pooler.dense.weight", "classifier.weight", "bert.embeddings.token_type_embeddings.weight",
                                                "bert.encoder.layers.0.attn.Wqkv.weight", word)})
    # forward_backward (the trainer's route: no autograd) accumulates the same gradients
    before = {k: v.clone() for k, v in grads.items()}
    out2 = model.forward_backward(**batch)
    assert torch.equal(out2.logits, out.logits) and torch.equal(out2.loss, out.loss.detach())
    for k, v in model.reference_grad_dict().items():
        assert rel_err(v, 2 * before[k]) < 1e-5, k


def test_segment_ids_reach_the_logits_and_none_is_all_zero(gold):
    g, sd, model, batch = golden_model(gold, "c2", 2, "single_label_classification")
    model.eval()
    with torch.no_grad():
        own = model(batch["input_ids"], batch["attention_mask"], batch["token_type_ids"]).logits
        swapped = model(batch["input_ids"], batch["attention_mask"], (1 - batch["token_type_ids"]) * batch["attention_mask"]).logits
        none = model(batch["input_ids"], batch["attention_mask"], None).logits
        zeros = model(batch["input_ids"], batch["attention_mask"], torch.zeros_like(batch["token_type_ids"])).logits
    moved = float(np.abs(g["c2/logits_swapped_types"] - g["c2/logits"]).max())           # how far the reference's logits move
    assert moved > 1e-3 and max_err(own, swapped) > 0.5 * moved
    assert max_err(swapped, torch.from_numpy(g["c2/logits_swapped_types"]).to(DEV)) <= 5e-3
    assert torch.equal(R.bits(none), R.bits(zeros)), "token_type_ids=None is all-zero segment ids, bit for bit"
    # ... and the engine's untyped path is untouched by the feature: the typed entry with zeros equals it
    vb = VarlenBatch.from_mask(batch["input_ids"], batch["attention_mask"])
    plain, _ = model.bert.forward_chunk(vb, False, normalize=False)
    typed, _ = model.bert.forward_chunk(vb.with_token_types(torch.zeros_like(batch["token_type_ids"])), False, normalize=False)
    assert torch.equal(R.bits(plain), R.bits(typed))
    with pytest.raises(ValueError):
        vb.with_token_types(batch["token_type_ids"][:, :8])
    with pytest.raises(NotImplementedError):
        NomicBertForSequenceClassification(TINY, 2, "multi_label_classification", device=DEV)
    one_type = NomicBertEngine(dataclasses.replace(TINY, type_vocab_size=1), device=DEV, pooling="cls", normalize=False)
    with pytest.raises(NotImplementedError):
        one_type.forward_chunk(vb.with_token_types(batch["token_type_ids"]), False)


def test_typed_path_under_gradient_checkpointing_gives_the_same_gradients(gold):
    """As tests/test_checkpoint_gpu.py has it for the untyped trunk: same logits, the blocks' matrices bit for bit, what fp32
    atomics reduce within summation-order noise -- and the type rows, which no atomic touches here, bit for bit."""
    res = {}
    for ck in (False, True):
        g, sd, model, batch = golden_model(gold, "c3", 3, "single_label_classification")
        model.train()
        model.gradient_checkpointing_enable(ck, keep_layers=0)
        model.zero_grad()
        out = model.forward_backward(**batch)
        torch.cuda.synchronize()
        res[ck] = (out.logits.clone(), out.loss.clone(), {k: v.clone() for k, v in model.reference_grad_dict().items()})
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    for name, a in res[False][2].items():
        b = res[True][2][name]
        if (".layers." in name and not name.endswith(".bias")) or "token_type" in name or name.startswith(("classifier", "bert.pooler")):
            assert torch.equal(a, b), (name, float((a - b).abs().max()))
        else:
            assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-30, name


def test_pretraining_checkpoint_loads_with_a_fresh_head(tmp_path):
    from contrastors_amd.mlm import NomicBertForPreTraining

    mlm = NomicBertForPreTraining(TINY, device=DEV, seed=3)
    mlm.save_pretrained(str(tmp_path / "mlm"))
    model = NomicBertForSequenceClassification(TINY, 3, "single_label_classification", device=DEV, seed=5)
    fresh = {k: v.clone() for k, v in model.head().items()}
    report_ = model.load_pretrained(str(tmp_path / "mlm"))
    assert report_["fresh"] == list(fresh) and report_["mismatched"] == [] and report_["skipped"]
    assert all(k.startswith("cls.") for k in report_["skipped"])
    assert torch.equal(model.bert.flat_param, mlm.bert.flat_param), "the trunk is the checkpoint's"
    for k, v in model.head().items():
        assert torch.equal(v, fresh[k])
    std = float(model.head()["bert.pooler.dense.weight"].std())
    assert abs(std - TINY.initializer_range) < 0.1 * TINY.initializer_range and float(model.head()["classifier.bias"].abs().max()) == 0.0
    # its own directory round-trips, head included; another label count keeps the pooler and a fresh classifier
    model.save_pretrained(str(tmp_path / "cls"))
    again = NomicBertForSequenceClassification(TINY, 3, "single_label_classification", device=DEV, seed=9)
    assert again.load_pretrained(str(tmp_path / "cls")) == {"fresh": [], "mismatched": [], "skipped": []}
    assert torch.equal(again._head_param, model._head_param) and torch.equal(again.bert.flat_param, model.bert.flat_param)
    two = NomicBertForSequenceClassification(TINY, 2, "single_label_classification", device=DEV, seed=9)
    assert two.load_pretrained(str(tmp_path / "cls"))["mismatched"] == ["classifier.weight", "classifier.bias"]
    assert torch.equal(two.head()["bert.pooler.dense.weight"], model.head()["bert.pooler.dense.weight"])


# ========================================================================================================= the trainer
def pair_trainer(tmp_path, regression=False, epochs=None, checkpoint=None, accum=1):
    r = SR.PAIR_RUN
    task = "stsb" if regression else "rte"
    cfg = Config(train_args=TrainArgs(num_epochs=epochs or r["epochs"], learning_rate=r["lr"], adam_beta1=0.9, adam_beta2=0.98,
                                      weight_decay=1e-6, eps=1e-6, max_grad_norm=0.0, schedule_type="linear", warmup_pct=r["warmup_pct"],
                                      eval_strategy="epochs", gradient_accumulation_steps=accum),
                 data_args=DataArgs(batch_size=r["batch"], seed=r["seed"], task_name=task),
                 model_args=ModelArgs(model_type="glue", seq_len=16, checkpoint=checkpoint))
    data = {"train": SR.pair_task(r["n_train"], r["seed"], regression), "validation": SR.pair_task(r["n_val"], r["seed"] + 1, regression)}
    tr = TRAINER_REGISTRY["glue"](cfg, torch.bfloat16, device=DEV, trunk_config=TINY, datasets=data)
    assert isinstance(tr, GlueTrainer)
    if checkpoint is None:
        tr.model["model"].load_reference_state_dict(SR.pair_initial_state(TINY_BERT, r["seed"], 1 if regression else 2))
        tr.model["model"].bert.sync_shadows()
    return tr


def test_glue_trainer_learns_a_task_only_segment_ids_solve(tmp_path):
    """The synthetic pair task of tests/seqcls_ref.py (the label is the token range of sentence B; sentence A draws from a random
    range), 256 train / 128 held-out rows, batch 16, 4 epochs = 64 steps, lr 1e-3, linear schedule, 6 % warm-up, seed 11.

    fp32 torch twin on the CPU (python -m tests.seqcls_ref), same data, seed and initial weights:
        loss every 8th step  0.718 0.712 0.711 0.097 0.007 0.004 0.003 0.003; mean of the first ten steps 0.699, of the last ten
        0.0032; held-out accuracy per epoch 0.445 0.953 0.961 0.977; majority-class rate 0.555
    this trainer on an MI355X (bf16 trunk; two runs, which differ by the summation order of the backward's fp32 atomics):
        loss every 8th step  0.718 0.712 0.711 0.097 0.007 0.004 0.003 0.003 / 0.718 0.712 0.711 0.096 0.007 0.004 0.003 0.003; mean of
        the first ten steps 0.699 / 0.699, of the last ten 0.0032 / 0.0032; held-out accuracy per epoch 0.445 0.953 0.938 0.938 /
        0.445 0.953 0.961 0.977
    Conditions: last-ten mean below half the first-ten mean; held-out accuracy above the majority-class rate."""
    tr = pair_trainer(tmp_path)
    assert tr.steps_per_epoch == 16 and tr.total_steps == 64 and tr.warmup_steps == int(64 * 0.06)
    losses = [float(x) for x in tr.train()]
    assert len(losses) == 64 and len(tr.history) == 4
    acc = [h["val_metric"]["accuracy"] for h in tr.history]
    refs = np.array([r["labels"] for r in tr.datasets["validation"]])
    majority = max(refs.mean(), 1 - refs.mean())
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print("glue trainer: loss every 8th step", [round(x, 3) for x in losses[::8]], "first ten", first, "last ten", last, "accuracy", acc,
          "majority", majority)
    report("seqcls.trainer", losses=[round(x, 4) for x in losses[::8]], first_ten=first, last_ten=last, accuracy=acc, majority=float(majority))
    assert last < 0.5 * first
    assert acc[-1] > majority
    assert tr.scheduler.get_last_lr()[0] == 0.0           # the linear schedule reached its horizon


def test_glue_trainer_resumes_to_the_same_next_step_loss(tmp_path):
    a = pair_trainer(tmp_path)
    batches = list(a.train_batches)
    a.train(iter(batches[:5]))
    a.save_state(str(tmp_path / "state"))
    next_a = float(a.training_step(batches[5]))
    b = pair_trainer(tmp_path)
    b.load_state(str(tmp_path / "state"))
    assert b.step == 5
    lr_b = b.scheduler.get_last_lr()
    next_b = float(b.training_step(batches[5]))
    assert next_a == next_b, (next_a, next_b)                 # the same weights and the same kernels: the same bits
    assert b.scheduler.get_last_lr() == a.scheduler.get_last_lr() and lr_b != b.scheduler.get_last_lr()
    # optimizer state came back too: the step after agrees (to the summation-order noise of the backward's fp32 atomics)
    after_a, after_b = float(a.training_step(batches[6])), float(b.training_step(batches[6]))
    assert after_a == pytest.approx(after_b, rel=1e-4)


def test_glue_trainer_regression_reports_finite_correlations(tmp_path):
    tr = pair_trainer(tmp_path, regression=True, epochs=1)
    losses = tr.train()
    assert len(losses) == 16 and all(np.isfinite(float(x)) for x in losses)
    m = tr.history[0]["val_metric"]
    assert set(m) == {"pearson", "spearmanr"} and np.isfinite(m["pearson"]) and np.isfinite(m["spearmanr"])
    report("seqcls.trainer_stsb", **m, last_loss=float(losses[-1]))


def test_glue_trainer_accumulates_and_shards(tmp_path):
    """gradient_accumulation_steps = 2: the optimizer fires every second micro-step and an epoch runs len(batches) // 2
    micro-steps (sc/trainers/base.py:465); the head's gradients of two micro-steps are summed like the trunk's."""
    tr = pair_trainer(tmp_path, accum=2, epochs=1)
    assert tr.steps_per_epoch == 8 and tr.total_steps == 8
    model = tr.model["model"]
    batches = list(tr.train_batches)
    w0 = model._head_param.clone()
    tr.training_step(batches[0])
    assert torch.equal(model._head_param, w0) and float(model._head_grad.abs().max()) > 0      # no step yet, gradients kept
    g1 = model._head_grad.clone()
    model2 = pair_trainer(tmp_path, accum=2, epochs=1).model["model"]
    model2.forward_backward(**batches[1])
    g2 = model2._head_grad.clone()
    tr.optimizer.step = lambda *a, **k: None                  # look at the summed gradient before the step consumes it
    tr.model["model"].zero_grad = lambda *a, **k: None
    tr.training_step(batches[1])
    assert rel_err(model._head_grad, g1 + g2) < 1e-6
    assert len(ShardedBatches(tr.datasets["train"], 16, 0, 2)) == 8


def test_glue_cli_trains_and_evaluates_from_local_files(tmp_path, monkeypatch, capsys):
    """python -m contrastors_amd.train --config glue.yaml --input_shards DIR --task_name rte: the reference's recipe file, a
    pre-training checkpoint directory, a saved local tokenizer and jsonl splits -- one epoch, then the task's metric."""
    import json

    import yaml
    from transformers import BertTokenizer

    from contrastors_amd import train as cli
    from contrastors_amd.mlm import NomicBertForPreTraining
    from tests.conftest import GOLD

    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(40)]
    (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n")
    BertTokenizer(str(tmp_path / "vocab.txt"), do_lower_case=True).save_pretrained(str(tmp_path / "tok"))
    NomicBertForPreTraining(TINY, device=DEV, seed=3).save_pretrained(str(tmp_path / "mlm"))
    data = tmp_path / "rte"
    data.mkdir()
    g = torch.Generator().manual_seed(5)
    for split, n in (("train", 48), ("validation", 24)):
        rows = []
        for _ in range(n):
            y = int(torch.randint(0, 2, (1,), generator=g))
            sent = lambda lo: " ".join(f"w{lo + int(i)}" for i in torch.randint(0, 20, (4,), generator=g))   # noqa: E731
            rows.append({"sentence1": sent(20 * int(torch.randint(0, 2, (1,), generator=g))), "sentence2": sent(20 * y),
                         "label": ["entailment", "not_entailment"][y]})
        (data / f"{split}.jsonl").write_text("".join(json.dumps(r) + "\n" for r in rows))
    recipe = json.loads((GOLD / "host_contracts.json").read_text())["recipes"]["glue.yaml"]
    recipe["train_args"].update(num_epochs=1, wandb=False, learning_rate=1e-3)
    recipe["model_args"].update(checkpoint=str(tmp_path / "mlm"), tokenizer_name=str(tmp_path / "tok"), seq_len=16)
    recipe["data_args"].update(batch_size=8)
    (tmp_path / "glue.yaml").write_text(yaml.safe_dump(recipe, sort_keys=False))
    monkeypatch.setattr("sys.argv", ["train", "--config", str(tmp_path / "glue.yaml"), "--input_shards", str(data), "--task_name", "rte"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main()
    out = capsys.readouterr().out
    assert "fresh initialisation ['bert.pooler.dense.weight'" in out and "cls.predictions.decoder.bias" in out
    assert "{'val_metric': {'accuracy':" in out and "'epoch': 0}" in out
