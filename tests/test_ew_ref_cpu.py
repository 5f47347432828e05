"""tests/ew_ref.py proven on the CPU before it meets a kernel: every reference against fp64 torch autograd (F.normalize of a mean /
cls pool, F.cross_entropy with ignore_index, torch.optim.AdamW with clip_grad_norm_), the bit-exact references against independent
restatements, the sharpness of the bit-exact inputs, the fp32 emulations inside their bounds, every planted error rejected with the
row and column named, and the measured constants of the table ew_ref.C_MEAS."""
import re

import pytest
import torch
import torch.nn.functional as F

from tests import ew_ref as E
from tests import gemm_ref as R
from tests.gemm_ref import BF, F32, F64, BitMismatch
from tests.ln_ref import RowMismatch, bits

WHERE = r"\(row (\d+), column (\d+)\)"


def rejected(exc, fn, row=None, col=None):
    """fn() must raise `exc` naming a (row, column); returns them (and compares with the expected ones)."""
    with pytest.raises(exc) as ei:
        fn()
    m = re.search(WHERE, str(ei.value))
    assert m, str(ei.value)
    r, c = int(m.group(1)), int(m.group(2))
    assert (row is None or r == row) and (col is None or c == col), (r, c, row, col, str(ei.value))
    return r, c


# ================================================================================================ bit-exact references
def test_cast_reference_equals_integer_rounding_and_inputs_are_sharp():
    x = E.cast_inputs(1027)
    ref = E.cast_ref(x)
    b = bits(x).to(torch.int64) & 0xFFFFFFFF
    rne = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF                   # round to nearest, ties to even, on the bit pattern
    nan = torch.isnan(x)
    got = (bits(ref).to(torch.int64) & 0xFFFF)
    assert bool((got[~nan] == rne[~nan]).all()) and bool(torch.isnan(ref[nan]).all()) and int(nan.sum()) == 1
    tie = E.is_tie(x) & torch.isfinite(x)
    assert float(tie.double().mean()) >= 0.05                                # at least 5 % exact ties ...
    par = (b[tie] >> 16) & 1
    assert int((par == 0).sum()) > 20 and int((par == 1).sum()) > 20         # ... of both parities
    up = got[tie] != ((b[tie] >> 16) & 0xFFFF)
    assert bool((up == (par == 1)).all())                                    # a tie goes up exactly when the value below is odd
    expo = (b >> 23) & 0xFF
    assert not bool(((expo == 0) & ((b & 0x7FFFFF) != 0)).any()), "no fp32 subnormals"
    assert bool(torch.isinf(ref[x.abs() == torch.finfo(F32).max]).all()) and int((x.abs() == torch.finfo(F32).max).sum()) == 2
    assert bits(ref[3:5]).tolist() == [0, -32768]                            # +0, -0
    for n in (1, 2, 3, 4, 5, 7):
        small = E.cast_inputs(n)                                             # the small sizes: a tie first, the specials from 3 on
        assert bool(E.is_tie(small)[0]) and (n < 7 or bits(small[3:7]).tolist() == bits(x[3:7]).tolist())


def test_transpose_reference_equals_index_arithmetic():
    rows, cols, pad = 13, 8, 16
    x = R.gauss_bf16(rows, cols, 3)
    ref = E.transpose_ref(x, pad)
    flat = x.reshape(-1)
    for c in range(cols):
        for r in range(pad):
            want = float(flat[r * cols + c]) if r < rows else 0.0
            assert float(ref[c, r]) == want
    x32 = E.cast_inputs(130 * 70, 5).reshape(130, 70)
    assert torch.equal(bits(E.transpose_ref(x32)).reshape(-1), bits(x32).reshape(-1)[(torch.arange(130)[None, :] * 70 + torch.arange(70)[:, None]).reshape(-1)])


def _rot_case(H=2, lens=(1, 33, 0, 7), seed=21):
    T = sum(lens)
    x = R.gauss_bf16(T, 3 * H * 64, seed)
    cos, sin = E.rotary_tables(max(lens))
    return x, lens, H, cos, sin


def test_rotary_reference_restated_and_sharp():
    x, lens, H, cos, sin = _rot_case()
    ref = E.rotary_ref(x, lens, H, 2, cos, sin, 1)
    t0, pre = 0, []
    for l in lens:
        for w in range(2):
            if l:
                u = x[t0:t0 + l, w * H * 64:(w + 1) * H * 64].reshape(l, H, 64)
                f = E.rotate_f32(u, cos, sin)
                pre.append(f.reshape(-1))
                assert R.check_bits("rotary", f.to(BF).reshape(l, H * 64), ref[t0:t0 + l, w * H * 64:(w + 1) * H * 64].contiguous()) == 0
        t0 += l
    assert torch.equal(bits(ref[:, 2 * H * 64:].contiguous()), bits(x[:, 2 * H * 64:].contiguous()))      # v untouched
    pre = torch.cat(pre)
    assert float((pre.to(BF).float() != pre).double().mean()) >= 0.5          # most results need the rounding
    back = E.rotary_ref(ref, lens, H, 2, cos, sin, -1)                         # the inverse rotation returns within 2 bf16 ulps
    assert float((back.double() - x.double()).abs().max()) <= 2 * float(R.bf16_ulp(x.double().abs().max()))


def test_planted_rotary_sign_and_truncating_cast_are_rejected():
    x, lens, H, cos, sin = _rot_case()
    ref = E.rotary_ref(x, lens, H, 2, cos, sin, 1)
    bad_sin = sin.clone()
    bad_sin[:, 8:16] = -bad_sin[:, 8:16]                                     # the sign flipped on one 8-column chunk
    r, c = rejected(BitMismatch, lambda: R.check_bits("rotary", E.rotary_ref(x, lens, H, 2, cos, bad_sin, 1), ref))
    assert c % 32 in range(8, 16) and r >= 2                                 # position 0 has sin = 0: the first rotated token is row 2
    x32 = E.cast_inputs(1027)
    trunc = (bits(x32) >> 16).to(torch.int16).view(BF)
    r, c = rejected(BitMismatch, lambda: E.check_bits_nan("cast", trunc[None], E.cast_ref(x32)[None]), row=0)
    first_up = int(torch.nonzero(bits(trunc) != bits(E.cast_ref(x32)))[0])
    assert c == first_up
    nan_lost = E.cast_ref(x32).clone()
    nan_lost[7] = 1.0
    rejected(BitMismatch, lambda: E.check_bits_nan("cast", nan_lost[None], E.cast_ref(x32)[None]), row=0, col=7)


# ====================================================================================================== ViT front end
def test_vit_patchify_reference_equals_index_arithmetic():
    B, C, H, W, p = E.VIT_PATCHIFY[0]
    pix = E.cast_inputs(B * C * H * W, 31).reshape(B, C, H, W)
    keep = E.vit_keep(B)
    wp, P = W // p, (H // p) * (W // p)
    assert P == E.VIT_P_ALL and all(sorted(k) != list(k) and E.VIT_P_ALL - 1 in k for k in E.VIT_KEEP)
    for kp in (None, keep):
        ref = E.patchify_ref(pix, p, kp)
        rows = P if kp is None else kp.shape[1]
        assert tuple(ref.shape) == (B * rows, C * p * p)
        want = torch.empty(B * rows, C * p * p, dtype=F32)
        for b in range(B):
            for j in range(rows):
                pi = j if kp is None else int(kp[b, j])
                ph, pw = divmod(pi, wp)
                for c in range(C):
                    for p1 in range(p):
                        for p2 in range(p):
                            want[b * rows + j, (c * p + p1) * p + p2] = pix[b, c, ph * p + p1, pw * p + p2]
        assert E.check_bits_nan("patchify", ref, E.cast_ref(want)) == 0
    bf = E.cast_ref(pix)                                                     # bf16 pixels: the rearrangement alone
    assert E.check_bits_nan("patchify bf16", E.patchify_ref(bf, p), E.patchify_ref(pix, p)) == 0
    r, c = rejected(BitMismatch, lambda: E.check_bits_nan("patchify", E.patchify_ref(pix, p, keep.flip(1)), E.patchify_ref(pix, p, keep)))
    assert r == 0


def test_vit_assemble_references_restated_and_planted_errors_are_rejected():
    B, P_all, d = 3, E.VIT_P_ALL, 24
    keep = E.vit_keep(B)
    K = keep.shape[1]
    inv = E.vit_inv(keep, P_all)
    assert sorted(int(inv[b, pi]) for b in range(B) for pi in keep[b].tolist()) == sorted(list(range(K)) * B)
    assert bool((inv[:, 4] < 0).all())                                        # patch 4: dropped by every image
    cls, pos = torch.randn(d, generator=E._gen(41)), torch.randn(P_all + 1, d, generator=E._gen(42))
    for kp, P in ((None, P_all), (keep, K)):
        proj = R.gauss_bf16(B * P, d, 43)
        ref = E.assemble_fwd_ref(proj, cls, pos, B, P, kp).reshape(B, P + 1, d)
        for b in range(B):
            assert torch.equal(ref[b, 0], (cls + pos[0]).to(BF))
            for s in range(1, P + 1):
                ps = s if kp is None else 1 + int(kp[b, s - 1])
                assert torch.equal(ref[b, s], (proj[b * P + s - 1].float() + pos[ps]).to(BF)), (b, s)
    # planted: the position row of the kept SLOT instead of the kept PATCH
    proj = R.gauss_bf16(B * K, d, 43)
    rejected(BitMismatch, lambda: R.check_bits("assemble_fwd", E.assemble_fwd_ref(proj, cls, pos, B, K, None), E.assemble_fwd_ref(proj, cls, pos, B, K, keep)), row=1)
    # backward: every dz row lands once; the sums in the images' order; an untouched row stays what it was
    gpos0, gcls0 = torch.randn(P_all + 1, d, generator=E._gen(44)), torch.randn(d, generator=E._gen(45))
    dz = E.vit_dz(B, K, d, 46)
    hole = inv.clone()
    hole[2, 1] = -1                                                          # image 2 loses its slot 3 (patch 1): dproj row 2 K + 3 is never written
    poison = torch.full((B * K, d), float("nan"), dtype=BF)
    dproj, gpos, gcls = E.assemble_bwd_ref(dz, B, K, gpos0, gcls0, poison, hole)
    z = dz.reshape(B, K + 1, d)
    assert bool(torch.isnan(dproj[2 * K + 3]).all()) and int(torch.isnan(dproj).any(1).sum()) == 1
    assert torch.equal(dproj.reshape(B, K, d)[:2], z[:2, 1:]) and torch.equal(dproj.reshape(B, K, d)[2, :3], z[2, 1:4])
    assert torch.equal(gpos[5], gpos0[5]) and torch.equal(gcls, gcls0 + ((z[0, 0].float() + z[1, 0].float()) + z[2, 0].float()))
    assert torch.equal(gpos[1], gpos0[1] + (z[0, 2].float() + z[1, 4].float()))             # patch 0: slot 1 of image 0, slot 3 of image 1
    dproj_p, gpos_p, _ = E.assemble_bwd_ref(dz[:B * (K + 1)], B, K, gpos0[:K + 1], gcls0, poison, None)
    assert torch.equal(dproj_p.reshape(B, K, d), z[:, 1:]) and torch.equal(gpos_p[2], gpos0[2] + ((z[0, 2].float() + z[1, 2].float()) + z[2, 2].float()))
    # planted: the batch summed in the reverse order (vit_dz makes the order visible)
    rev = gpos0[0] + ((z[2, 0].float() + z[1, 0].float()) + z[0, 0].float())
    rejected(BitMismatch, lambda: R.check_bits("gpos order", rev[None], gpos[0][None]), row=0)


# ======================================================================================================== activations
def _act_floors(inp, bias):
    """form -> the fp32 underflow term of its bound (ew_ref.act_floor)."""
    d, y, g, act = R.d64(inp["d"], inp["y"], inp["g"], inp["act"])
    v = E.pre_plus_bias(inp["pre"], bias, F64)
    return {form: E.act_floor(form, d=d, y=y, g=g, v=v, act=act) for form in E.C_MEAS["gauss"]}


def _act_forms(inp, family, bias):
    """Every activation form on one input set: name -> (emulation fp32, reference fp64, T)."""
    y, g, d, pre, act = (inp[k] for k in ("y", "g", "d", "pre", "act"))
    f32, f64 = (lambda *ts: [t.to(F32) for t in ts]), (lambda *ts: [t.to(F64) for t in ts])
    out = {}
    out["swiglu"] = (E.emu_swiglu(*f32(y, g)),) + R.f_swiglu(*f64(y, g))
    edy, edg = E.emu_swiglu_bwd(*f32(d, y, g))
    dy, tdy, dg, tdg = R.f_swiglu_bwd(*f64(d, y, g))
    out["swiglu_bwd.dy"], out["swiglu_bwd.dg"] = (edy, dy, tdy), (edg, dg, tdg)
    edy, edg = E.emu_swiglu_bwd_ag(*f32(d, act, g))
    dy, tdy, dg, tdg = E.f_swiglu_bwd_ag(*f64(d, act, g))
    out["swiglu_bwd_ag.dy"], out["swiglu_bwd_ag.dg"] = (edy, dy, tdy), (edg, dg, tdg)
    for a, form in E.ACT_FORM.items():
        v32, v64 = E.pre_plus_bias(pre, bias, F32), E.pre_plus_bias(pre, bias, F64)
        out[form] = (E.emu_act(v32, a),) + R.f_act(v64, a)
        out[form + "_bwd"] = (d.to(F32) * E.emu_act_grad(v32, a),) + R.f_act_bwd(d.to(F64), v64, a)
    return out


def _measure_act(family):
    worst = {}
    for T, I in E.ACT_SHAPES_CPU:
        inp = E.act_inputs(T, I, family)
        for bias in (None, inp["bias"]):
            floors = _act_floors(inp, bias)
            for form, (emu, ref, t) in _act_forms(inp, family, bias).items():
                worst[form] = max(worst.get(form, 0.0), E.meas_ratio(ref, t, emu, E.BF16_QUANTUM + floors[form]))
    return worst


def _pool_cases():
    for d in E.POOL_D:
        for zero_seq in (None, 3):
            h, demb = E.pool_inputs(E.POOL_LENS, d, zero_seq=zero_seq)
            for mode in (0, 1):
                for normalize in (0, 1):
                    yield d, zero_seq, mode, normalize, h, demb


def _live(lens):
    return torch.tensor([l > 0 for l in lens])


def _measure_pool():
    worst = {"emb": 0.0, "norm": 0.0, "dh": 0.0}
    lens = E.POOL_LENS
    for d, zero_seq, mode, normalize, h, demb in _pool_cases():
        emb, norm = E.emu_pool_fwd(h, lens, mode, normalize)
        remb, temb, rnorm, tnorm = E.pool_fwd_ref(h, lens, mode, normalize)
        ok = _live(lens) if mode == 0 else torch.ones(len(lens), dtype=torch.bool)
        worst["emb"] = max(worst["emb"], R.meas_ratio(remb[ok], temb[ok], emb[ok]))
        worst["norm"] = max(worst["norm"], R.meas_ratio(rnorm[ok], tnorm[ok], norm[ok]))
        emb = torch.nan_to_num(emb)                                          # the empty sequence's row is never read by the backward
        dh_ref, th = E.pool_bwd_ref(demb, emb, norm, lens, mode, normalize)
        g = demb.to(F32)
        # before the bf16 rounding: the emulation's own fp32 value
        e32 = _pool_bwd_f32(g, emb, norm, lens, mode, normalize)
        worst["dh"] = max(worst["dh"], R.meas_ratio(dh_ref, th, e32))
    return worst


def _pool_bwd_f32(demb, emb, norm, lens, mode, normalize):
    """emu_pool_bwd without its last rounding (the constant is measured before it)."""
    dh = torch.zeros(sum(lens), demb.shape[1], dtype=F32)
    one, t0 = torch.tensor(1.0, dtype=F32), 0
    for b, l in enumerate(lens):
        if l:
            g = demb[b]
            if normalize:
                g = (g - emb[b] * (demb[b] * emb[b]).sum()) * (one / torch.maximum(norm[b], torch.tensor(1e-12, dtype=F32)))
            if mode == 1:
                dh[t0] = g
            else:
                dh[t0:t0 + l] = g * (one / torch.tensor(float(l), dtype=F32))
        t0 += l
    return dh


def _xent_cases():
    for V in E.XENT_V:
        lab = E.xent_labels(V)
        for dtype in (BF, F32):
            for fam in E.XENT_FAMILIES:
                x = E.xent_inputs(V, fam, dtype)
                for scale in (1.0, 0.25):
                    for vec in sorted({1, E.xent_vec(V, V, dtype)}):
                        yield V, lab, dtype, fam, x, scale, vec
            if V >= 2048:
                x, lab2 = E.xent_neginf_inputs(V, dtype)
                for vec in sorted({1, E.xent_vec(V, V, dtype)}):
                    yield V, lab2, dtype, "neginf", x, 1.0, vec


def _dloss(N=E.XENT_N):
    return torch.tensor([1.0, -0.5, 2.0, 0.25, 3.0])[:N]


def _measure_xent():
    worst = {"lse": 0.0, "loss": 0.0, "dlogits": 0.0}
    for V, lab, dtype, fam, x, scale, vec in _xent_cases():
        loss, lse = E.emu_xent_fwd(x, lab, scale, vec)
        ref = E.xent_ref(x, lab, scale)
        worst["lse"] = max(worst["lse"], R.meas_ratio(ref["lse"], ref["t_lse"], lse))
        worst["loss"] = max(worst["loss"], R.meas_ratio(ref["loss"], ref["t_loss"], loss))
        z = x.to(F32) * torch.tensor(scale, dtype=F32)                       # the emulation before its last rounding
        live = ~E.ignored_rows(lab, V)
        hot = torch.zeros(x.shape, dtype=F32)
        hot[live, lab[live]] = 1.0
        e32 = (torch.exp(z - lse[:, None]) - hot) * (_dloss() * torch.tensor(scale, dtype=F32))[:, None] * live[:, None]
        dref, t, extra = E.xent_bwd_ref(x, lab, _dloss(), lse, scale, ref["lse"])
        worst["dlogits"] = max(worst["dlogits"], E.meas_ratio(dref, t, e32, E.xent_floor(_dloss(), scale)))
    return worst


OPT_CASES = E.OPT_CASES


def _measure_opt():
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "ema": 0.0}
    for n in (1027, 65539):
        p, g, m, v = E.opt_inputs(n)
        sq = g.double().pow(2).sum()
        for step, wd, kind, max_norm, LR in OPT_CASES:
            s = None if kind is None else sq
            rp, rm, rv, tp, tm, tv = E.adamw_step(p, g, m, v, LR, wd, step, s, max_norm)
            ep, em, ev = E.adamw_step(p, g, m, v, LR, wd, step, s, max_norm, dtype=F32)
            for k, (ref, t, emu) in {"p": (rp, tp, ep), "m": (rm, tm, em), "v": (rv, tv, ev)}.items():
                worst[k] = max(worst[k], R.meas_ratio(ref, t, emu))
        for decay in (0.0, 0.999, 1.0):
            ref, t = E.ema_step(m, p, decay)
            worst["ema"] = max(worst["ema"], R.meas_ratio(ref, t, E.ema_step(m, p, decay, dtype=F32)[0]))
    return worst


@pytest.fixture(scope="module")
def measured():
    return {"gauss": _measure_act("gauss"), "sat": _measure_act("sat"), "pool": _measure_pool(), "xent": _measure_xent(),
            "opt": _measure_opt()}


def test_measured_constants(measured):
    print({f: {k: round(v, 3) for k, v in d.items()} for f, d in measured.items()})
    for fam, table in E.C_MEAS.items():
        assert set(table) == set(measured[fam]), fam
        for form, c in table.items():
            w = measured[fam][form]
            assert 0.8 * c <= w <= c, f"{fam}.{form}: measured {w:.3f}, table {c}: re-measure and update ew_ref.C_MEAS"


# --------------------------------------------------------------------------------- activations: autograd, bounds, planted errors
def test_swiglu_bwd_ag_contract_at_zero_gate():
    inp = E.act_inputs(3, 96, "sat")
    d, act, g, y = (inp[k].double() for k in ("d", "act", "g", "y"))
    dy, _, dg, _ = E.f_swiglu_bwd_ag(d, act, g)
    zero = g == 0
    assert int(zero.sum()) > 0 and bool((act[zero] == 0).all()) and bool((dg[zero] == 0).all()) and bool((dy[zero] == 0).all())
    assert bool(torch.isfinite(dg).all())
    big = ((g.abs() >= 8) & (g != -100)) | (g.abs() == 2.0 ** -20)                          # where act lost nothing to a subnormal rounding: the two
    _, _, dg2, t2 = R.f_swiglu_bwd(d, y, g)                                   # forms are the same derivative up to act's bf16 rounding
    assert float(((dg - dg2).abs() / (t2 + 1e-300))[big & (t2 > 0)].max()) < 2.0 ** -7


def test_emulations_pass_and_planted_activation_errors_are_rejected():
    T, I = 3, 96
    for family in ("gauss", "sat"):
        inp = E.act_inputs(T, I, family)
        floors = _act_floors(inp, inp["bias"])
        for form, (emu, ref, t) in _act_forms(inp, family, inp["bias"]).items():
            assert E.check_bf16(form, emu.to(BF), ref, t, E.C(family, form), floors[form]) <= 1.0
    # a sigmoid that the hardware's reciprocal flushed to 0 below the smallest fp32 normal (quick-GELU at v <= -51.5) is inside the bound
    # by its underflow term alone; the same zero where the sigmoid is a normal number is not
    v = torch.tensor([[-51.5, -52.0, -60.0, -50.0]], dtype=F64)
    ref, t = R.f_act(v, 1)
    sig = ref / v
    assert bool((sig[0, :3] < E.F32_MIN_NORMAL).all()) and float(sig[0, 3]) > E.F32_MIN_NORMAL
    zero = torch.zeros(1, 4, dtype=BF)
    assert E.check_bf16("qgelu", zero[:, :3], ref[:, :3], t[:, :3], E.C("sat", "qgelu"), E.act_floor("qgelu", v=v[:, :3])) <= 1.0
    rejected(RowMismatch, lambda: E.check_bf16("qgelu", zero[:, :3], ref[:, :3], t[:, :3], E.C("sat", "qgelu")), row=0, col=0)
    rejected(RowMismatch, lambda: E.check_bf16("qgelu", zero, ref, t, E.C("sat", "qgelu"), E.act_floor("qgelu", v=v)), row=0, col=3)
    inp = E.act_inputs(T, I, "gauss")
    pre, bias, d, y, g = (inp[k] for k in ("pre", "bias", "d", "y", "g"))
    # 1. the bias skipped on the last 8 columns
    b_bad = bias.clone()
    b_bad[-8:] = 0
    for a, form in E.ACT_FORM.items():
        ref, t = R.f_act(E.pre_plus_bias(pre, bias, F64), a)
        bad = E.emu_act(E.pre_plus_bias(pre, b_bad, F32), a).to(BF)
        r, c = rejected(RowMismatch, lambda: E.check_bf16(form, bad, ref, t, E.C("gauss", form)))
        assert c >= I - 8
    # 2. a sigmoid derivative without the (1 - s) term
    s = E.k_sig(g.float())
    bad = ((s + g.float() * s) * d.float() * y.float()).to(BF)
    _, _, dg, tdg = R.f_swiglu_bwd(*R.d64(d, y, g))
    rejected(RowMismatch, lambda: E.check_bf16("dg", bad, dg, tdg, E.C("gauss", "swiglu_bwd.dg")))
    # the reciprocal of the gate clamped to +-1e30 (what rcp_clamped did before it clamped at FLT_MAX): d gate of a gate of +-2^-126
    # comes out as d * act * 1e30, eight orders too small; the saturation family holds such gates, the Gaussian one does not
    sat = E.act_inputs(T, I, "sat")
    d64, a64, g64 = R.d64(sat["d"], sat["act"], sat["g"])
    _, _, dg, tdg = E.f_swiglu_bwd_ag(d64, a64, g64)
    _, bad = E.emu_swiglu_bwd_ag(sat["d"].float(), sat["act"].float(), sat["g"].float(), rcp_clamp=1e30)
    r, c = rejected(RowMismatch, lambda: E.check_bf16("dg", bad.to(BF), dg, tdg, E.C("sat", "swiglu_bwd_ag.dg"), E.act_floor("swiglu_bwd_ag.dg", d=d64, act=a64, g=g64)))
    assert abs(float(sat["g"][r, c])) == 2.0 ** -126
    _, ok = E.emu_swiglu_bwd_ag(d.float(), inp["act"].float(), g.float(), rcp_clamp=1e30)
    _, _, dg, tdg = E.f_swiglu_bwd_ag(*R.d64(d, inp["act"], g))
    assert E.check_bf16("dg", ok.to(BF), dg, tdg, E.C("gauss", "swiglu_bwd_ag.dg")) <= 1.0


def test_colsum_bound_and_grid():
    assert [E.colsum_grid(T, 8) for T in (1, 256, 257, 1000, 131072, 131073)] == [1, 1, 2, 4, 512, 512]
    assert E.colsum_grid(1000, 768) == 4 and E.colsum_grid(1 << 20, 768) == 342             # the three clamps: T, 1024 / colblocks, 512
    x = R.gauss_bf16(1000, 264, 31)
    init = torch.randn(264, generator=torch.Generator().manual_seed(32))
    good = (init.double() + x.double().sum(0)).float()
    assert E.check_colsum("colsum", good, x, init) <= 0.1
    bad = (init.double() + x[:-1].double().sum(0)).float()                                   # the last row left out
    rejected(RowMismatch, lambda: E.check_colsum("colsum", bad, x, init), row=0)
    no_init = x.double().sum(0).float()                                                      # `=` where `+=` is meant
    rejected(RowMismatch, lambda: E.check_colsum("colsum", no_init, x, init), row=0)
    assert E.sq_norm_bound(5) == 8 * 2.0 ** -24 and E.sq_norm_bound((1 << 22) + 4099) == 12 * 2.0 ** -24


# ============================================================================================================ pooling
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("normalize", [0, 1])
def test_pool_reference_equals_fp64_autograd(mode, normalize):
    lens, d = (5, 1, 300, 2), 64
    h, demb = E.pool_inputs(lens, d)
    x = h.double().requires_grad_(True)
    cu = E.cu_of(lens).tolist()
    rows = [x[cu[b]] if mode == 1 else x[cu[b]:cu[b + 1]].mean(0) for b in range(len(lens))]
    pooled = torch.stack(rows)
    emb = F.normalize(pooled, dim=-1) if normalize else pooled
    (auto,) = torch.autograd.grad((emb * demb.double()).sum(), x)
    remb, _, rnorm, _ = E.pool_fwd_ref(h, lens, mode, normalize)
    assert float((remb - emb.detach()).abs().max()) < 1e-14
    assert float((rnorm - pooled.detach().norm(dim=-1)).abs().max()) < 1e-13
    dh, _ = E.pool_bwd_ref(demb, remb, rnorm, lens, mode, normalize)
    assert float((dh - auto).abs().max()) < 1e-13


def test_pool_empty_and_zero_sequences():
    lens, d = E.POOL_LENS, 64
    h, demb = E.pool_inputs(lens, d, zero_seq=3)
    for mode in (0, 1):
        emb, _, norm, _ = E.pool_fwd_ref(h, lens, mode, 1)
        e32, n32 = E.emu_pool_fwd(h, lens, mode, 1)
        for e, n in ((emb, norm), (e32, n32)):
            assert bool(torch.isnan(e[1]).all()) if mode == 0 else bool((e[1] == 0).all())      # the empty sequence
            assert bool((e[3] == 0).all()) and float(n[3]) == 0                                 # the all-zero one: the eps clamp
            assert bool(torch.isfinite(e[[0, 2, 4]]).all())
        dh, th = E.pool_bwd_ref(demb, torch.nan_to_num(emb), norm, lens, mode, 1)
        row = 6 if mode == 1 else 100                                                            # a row of sequence 3 (tokens 6 .. 305)
        assert torch.allclose(dh[6], demb[3].double() / E.EPS_NORM / (1 if mode == 1 else 300), rtol=1e-12)
        assert bool((dh[7] == 0).all()) == (mode == 1) and bool(torch.isfinite(dh).all()) and row


def test_pool_emulation_passes_and_planted_errors_are_rejected():
    lens, d = E.POOL_LENS, 64
    h, demb = E.pool_inputs(lens, d)
    ok = _live(lens)
    for mode in (0, 1):
        for normalize in (0, 1):
            emb, norm = E.emu_pool_fwd(h, lens, mode, normalize)
            remb, temb, rnorm, tnorm = E.pool_fwd_ref(h, lens, mode, normalize)
            sel = ok if mode == 0 else torch.ones_like(ok)
            assert E.check_f32("emb", emb[sel], remb[sel], temb[sel], E.C("pool", "emb")) <= 1.0
            assert E.check_f32("norm", norm[sel, None], rnorm[sel, None], tnorm[sel, None], E.C("pool", "norm")) <= 1.0
            emb = torch.nan_to_num(emb)
            dh, th = E.pool_bwd_ref(demb, emb, norm, lens, mode, normalize)
            assert E.check_bf16("dh", E.emu_pool_bwd(demb, emb, norm, lens, mode, normalize), dh, th, E.C("pool", "dh")) <= 1.0
    # 3. 1 / len replaced by 1 / (len + 1) on one sequence (the fourth: rows 3 of emb, tokens 6 .. 305 of dh)
    remb, temb, rnorm, tnorm = E.pool_fwd_ref(h, lens, 0, 0)
    bad, _ = E.emu_pool_fwd(h, lens, 0, 0, len_plus=3)
    rejected(RowMismatch, lambda: E.check_f32("emb", bad[ok], remb[ok], temb[ok], E.C("pool", "emb")), row=2)
    emb, norm = E.emu_pool_fwd(h, lens, 0, 1)
    emb = torch.nan_to_num(emb)
    dh, th = E.pool_bwd_ref(demb, emb, norm, lens, 0, 1)
    rejected(RowMismatch, lambda: E.check_bf16("dh", E.emu_pool_bwd(demb, emb, norm, lens, 0, 1, len_plus=3), dh, th, E.C("pool", "dh")), row=6)
    # 4. cls mode reading (forward) or writing (backward) row 1 of the sequence
    remb, temb, _, _ = E.pool_fwd_ref(h, lens, 1, 0)
    bad, _ = E.emu_pool_fwd(h, (5, 0, 1, 300, 2), 1, 0, cls_row=1)
    rejected(RowMismatch, lambda: E.check_f32("emb", bad, remb, temb, E.C("pool", "emb")), row=0)
    emb, norm = E.emu_pool_fwd(h, lens, 1, 1)
    dh, th = E.pool_bwd_ref(demb, emb, norm, lens, 1, 1)
    shifted = torch.roll(E.emu_pool_bwd(demb, emb, norm, lens, 1, 1), 1, 0)
    rejected(RowMismatch, lambda: E.check_bf16("dh", shifted, dh, th, E.C("pool", "dh")), row=0)


# =============================================================================================================== xent
@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_xent_reference_equals_fp64_autograd(scale):
    V = 2056
    lab = E.xent_labels(V)
    for fam in ("gauss1", "edge"):
        x = E.xent_inputs(V, fam, BF)
        z = (x.double() * scale).requires_grad_(True)
        ign = E.ignored_rows(lab, V)
        tgt = torch.where(ign, torch.full_like(lab, E.IGNORE), lab)
        loss = F.cross_entropy(z, tgt, ignore_index=E.IGNORE, reduction="none")
        (auto,) = torch.autograd.grad((loss * _dloss().double()).sum(), z)
        ref = E.xent_ref(x, lab, scale)
        assert float((ref["loss"] - loss.detach()).abs().max()) < 1e-12
        assert float((ref["lse"] - torch.logsumexp(z.detach(), -1)).abs().max()) < 1e-12
        d, t, extra = E.xent_bwd_ref(x, lab, _dloss(), ref["lse"], scale, ref["lse"])
        assert float((d - auto * scale).abs().max()) < 1e-13 and float(extra.max()) == 0
        assert bool((d[ign] == 0).all()) and bool((t >= d.abs() * (1 - 1e-12)).all())


def test_xent_neginf_row_is_finite_only_with_the_guard():
    """What xent_fwd_kernel did before its guard, on the CPU: a lane whose first loaded columns are all -inf forms exp(-inf - -inf)."""
    V = 2056
    for dtype in (BF, F32):
        x, lab = E.xent_neginf_inputs(V, dtype)
        ref = E.xent_ref(x, lab, 1.0)
        assert bool(torch.isfinite(ref["lse"]).all())
        want = F.cross_entropy(x.double(), torch.where(ref["ign"], torch.full_like(lab, E.IGNORE), lab), ignore_index=E.IGNORE, reduction="none")
        assert float((ref["loss"] - want).abs().max()) < 1e-12
        for vec in (1, E.xent_vec(V, V, dtype)):
            loss, lse = E.emu_xent_fwd(x, lab, 1.0, vec, guard=False)
            assert bool(torch.isnan(lse).all()) and bool(torch.isnan(loss[~ref["ign"]]).all())
            rejected(RowMismatch, lambda: E.check_xent_fwd("unguarded", loss, lse, x, lab, 1.0), row=0, col=0)
            loss, lse = E.emu_xent_fwd(x, lab, 1.0, vec)
            r1, r2, _ = E.check_xent_fwd("guarded", loss, lse, x, lab, 1.0)
            assert max(r1, r2) <= 1.0
            dl = E.emu_xent_bwd(x, lab, _dloss(), lse, 1.0)
            assert E.check_xent_bwd("guarded", dl, x, lab, _dloss(), lse, 1.0, ref["lse"]) <= 1.0
            assert bool((dl[:, :16] == 0).all()) and bool((dl[:, V - 1] == 0).all())


def test_xent_emulation_passes_and_planted_errors_are_rejected():
    for V, lab, dtype, fam, x, scale, vec in _xent_cases():
        if V not in (7, 2056) or fam not in ("gauss1", "edge"):
            continue
        loss, lse = E.emu_xent_fwd(x, lab, scale, vec)
        r1, r2, ref = E.check_xent_fwd(f"{V} {fam}", loss, lse, x, lab, scale)
        dl = E.emu_xent_bwd(x, lab, _dloss(), lse, scale)
        assert max(r1, r2, E.check_xent_bwd(f"{V} {fam}", dl, x, lab, _dloss(), lse, scale, ref["lse"])) <= 1.0
        # 5. the one-hot label off by one (row 0 has label 0 -> column 1; the loss reads the wrong logit)
        bad = E.emu_xent_bwd(x, lab, _dloss(), lse, scale, label_shift=1)
        r, c = rejected(RowMismatch, lambda: E.check_xent_bwd("shift", bad, x, lab, _dloss(), lse, scale, ref["lse"]), row=0)
        assert c in (0, 1)
        bad_loss, _ = E.emu_xent_fwd(x, lab, scale, vec, label_shift=1)
        rejected(RowMismatch, lambda: E.check_xent_fwd("shift", bad_loss, lse, x, lab, scale), col=0)
        # 6. lse from all but the last column: the edge family's odd rows keep their maximum there
        if fam == "edge":
            _, bad_lse = E.emu_xent_fwd(x, lab, scale, vec, drop_last=True)
            rejected(RowMismatch, lambda: E.check_xent_fwd("drop", loss, bad_lse, x, lab, scale), row=1, col=0)
    # an ignored row that is not exactly zero
    V = 8
    x, lab = E.xent_inputs(V, "gauss1", F32), E.xent_labels(V)
    loss, lse = E.emu_xent_fwd(x, lab, 1.0, 4)
    dl = E.emu_xent_bwd(x, lab, _dloss(), lse, 1.0)
    dl[2, 3] = 1e-30
    with pytest.raises(AssertionError, match="ignored row"):
        E.check_xent_bwd("ign", dl, x, lab, _dloss(), lse, 1.0, lse.double())


def test_xent_dispatch():
    assert [E.xent_vec(V, V, BF) for V in E.XENT_V] == [1, 1, 8, 8, 8, 1, 8]
    assert [E.xent_vec(V, V, F32) for V in E.XENT_V] == [1, 1, 4, 4, 4, 1, 4]
    assert E.xent_vec(2048, 2056, BF) == 8 and E.xent_vec(2048, 2051, BF) == 1 and E.xent_vec(2048, 2048, BF, aligned=False) == 1
    assert E.xent_vec(2048, 2048, F32, ld_d=2051) == 1 and E.xent_vec(2048, 2048, F32, ld_d=2052) == 4


# ========================================================================================================== optimizer
def test_adamw_reference_equals_torch_adamw_fp64():
    n = 1027
    p0, g0, m0, v0 = E.opt_inputs(n)
    f32 = lambda t: float(torch.tensor(t, dtype=F32))                          # noqa: E731
    for wd, max_norm in ((0.1, 0.05), (0.0, 1e6)):
        w = torch.nn.Parameter(p0.double().clone())
        opt = torch.optim.AdamW([w], lr=1.0, betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(wd))
        p, m, v = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        for step, lr in ((1, 2e-4), (2, 1e-4), (3, 5e-5)):                    # a changing lr
            g = g0.double() * step + 1e-3 * p
            for grp in opt.param_groups:
                grp["lr"] = f32(lr)
            w.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([w], f32(max_norm))
            opt.step()
            p, m, v, tp, tm, tv = E.adamw_step(p, g, m, v, lr, wd, step, g.pow(2).sum(), max_norm)
            # (the launcher rounds the bias corrections to fp32: 2^-24 relative on the update, which is <= lr)
            assert float((p - w.detach()).abs().max()) < 3e-4 * 2.0 ** -22
            st = opt.state[w]
            assert float((m - st["exp_avg"]).abs().max()) < 1e-15 and float((v - st["exp_avg_sq"]).abs().max()) < 1e-15
            assert bool((tp >= p.abs() * (1 - 1e-9)).all()) and bool((tm >= m.abs() * (1 - 1e-9)).all())


def test_optimizer_emulation_passes_and_planted_errors_are_rejected():
    n = 1027
    p, g, m, v = E.opt_inputs(n)
    sq = g.double().pow(2).sum()
    for step, wd, kind, max_norm, LR in OPT_CASES:
        s = None if kind is None else sq
        rp, rm, rv, tp, tm, tv = E.adamw_step(p, g, m, v, LR, wd, step, s, max_norm)
        ep, em, ev = E.adamw_step(p, g, m, v, LR, wd, step, s, max_norm, dtype=F32)
        for k, (ref, t, emu) in {"p": (rp, tp, ep), "m": (rm, tm, em), "v": (rv, tv, ev)}.items():
            assert E.check_f32(k, emu, ref, t, E.C("opt", k)) <= 1.0
    assert float(E.clip_coef(sq, 0.01)) < 1 and float(E.clip_coef(sq, 1e6)) == 1 and float(E.clip_coef(sq, -1.0)) == 1
    # 9. the weight decay applied after the update
    LR = 0.05                                                  # (at lr = 2e-4 the order of the two steps is below the fp32 rounding of p)
    rp, _, _, tp, _, _ = E.adamw_step(p, g, m, v, LR, 0.1, 1, sq, 0.01)
    bad, _, _ = E.adamw_step(p, g, m, v, LR, 0.1, 1, sq, 0.01, dtype=F32, wd_after=True)
    rejected(RowMismatch, lambda: E.check_f32("p", bad, rp, tp, E.C("opt", "p")), row=0)
    # the gradient not scaled by the clip coefficient
    noclip, _, _ = E.adamw_step(p, g, m, v, LR, 0.1, 1, None, 0.01, dtype=F32)
    rejected(RowMismatch, lambda: E.check_f32("p", noclip, rp, tp, E.C("opt", "p")), row=0)
    # 10. an EMA with decay and 1 - decay swapped
    ref, t = E.ema_step(m, p, 0.999)
    assert E.check_f32("ema", E.ema_step(m, p, 0.999, dtype=F32)[0], ref, t, E.C("opt", "ema")) <= 1.0
    rejected(RowMismatch, lambda: E.check_f32("ema", E.ema_step(m, p, 0.999, dtype=F32, swapped=True)[0], ref, t, E.C("opt", "ema")), row=0, col=0)
    assert torch.equal(E.ema_step(m, p, 0.0, dtype=F32)[0], p) and torch.equal(E.ema_step(m, p, 1.0, dtype=F32)[0], m)


def test_slab_guards():
    s = E.Slab(3, 8, 11, dtype=F32, data=torch.ones(3, 8), lead=1, name="s")
    assert s.intact() and s.ptr % 16 == 4 and bool((s.get() == 1).all())
    R.check_poison([s])
    s.t[1, 2] = 5.0                                     # the payload may change
    assert s.intact()
    s.full[s.guard + s.lead + 8] = 0.0                  # the first gap element of row 0
    assert not s.intact()
    with pytest.raises(AssertionError, match="'s'"):
        R.check_poison([s])
    e = E.Slab(1, 5, dtype=BF)
    assert bool(torch.isnan(e.get()).all()) and e.ptr % 16 == 0
