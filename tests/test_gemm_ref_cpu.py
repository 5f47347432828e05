"""tests/gemm_ref.py proven on the CPU before it meets a kernel: the exact restatements against a plain fp32 emulation (natural,
permuted and unevenly split K order), the activation derivatives against fp64 autograd, the sharpness of the inputs (most results
are not bf16 values, several per cent are exact ties, every sum stays below 2^24), every planted error rejected by the checker that
should catch it, and the measured constants of the nonlinear bounds."""
import pytest
import torch

from tests import gemm_ref as R
from tests.gemm_ref import BF, F32, F64
from tests.ln_ref import RowMismatch, bits


# ------------------------------------------------------------------------------------------------------ fp32 emulation
def emu_acc(x, w, order=None, slices=None, drop_product=None, drop_ktile=None):
    """X W^T accumulated in fp32, one product at a time in `order` (a permutation of k); `slices`: uneven K ranges, each summed
    by itself into an fp32 slab, the slabs then added in fixed order (the split-K scheme)."""
    K = x.shape[1]
    prods = x.float()[:, None, :] * w.float()[None, :, :]            # (M, N, K): a product of two bf16 values is exact in fp32
    if drop_product is not None:
        m, n, k = drop_product
        prods[m, n, k] = 0.0
    if drop_ktile is not None:
        m, kt = drop_ktile
        prods[m, :, kt * 64:(kt + 1) * 64] = 0.0
    order = list(range(K)) if order is None else order

    def chain(ks):
        a = torch.zeros(prods.shape[:2], dtype=F32)
        for k in ks:
            a = a + prods[:, :, k]
        return a

    if slices is None:
        return chain(order)
    out, lo = torch.zeros(prods.shape[:2], dtype=F32), 0
    for n in slices:
        out = out + chain(order[lo:lo + n])
        lo += n
    assert lo == K
    return out


def trunc_bf16(v32):
    return (bits(v32.contiguous()) >> 16).to(torch.int16).view(BF)


def emu_nt(x, w, bias=None, alpha=1.0, res=None, out_mode=0, acc=None, no_bias_cols=0, trunc=False, ignore_alpha=False, res_shift=0):
    """The entry point's epilogue as single fp32 torch operations on an emulated accumulator (with optional planted errors)."""
    v = emu_acc(x, w) if acc is None else acc
    if not ignore_alpha:
        v = v * torch.tensor(alpha, dtype=F32)
    if bias is not None:
        b = bias.clone()
        if no_bias_cols:
            b[-no_bias_cols:] = 0.0
        v = v + b
    if out_mode == 1:
        return v
    o = trunc_bf16(v) if trunc else v.to(BF)
    if res is not None:
        o = (o.float() + torch.roll(res, -res_shift, 0).float()).to(BF)
    return o


M0, N0, K0 = 130, 40, 192      # a partial last 128-row panel (rows 128, 129), three K-tiles


@pytest.fixture(scope="module")
def small():
    x, w = R.operands(M0, N0, K0, 11)
    return dict(x=x, w=w, bias=R.bias_vec(N0, 13), res=R.residual(M0, N0, 14), acc=emu_acc(x, w))


# ------------------------------------------------------------------------------------------- the restatements are right
def test_accumulator_is_order_independent(small):
    x, w = small["x"], small["w"]
    exact = R.acc_exact(x, w)
    perm = torch.randperm(K0, generator=torch.Generator().manual_seed(5)).tolist()
    for name, a in (("natural", small["acc"]), ("permuted", emu_acc(x, w, order=perm)),
                    ("uneven slices", emu_acc(x, w, slices=[7, 64, 1, 100, 20])),
                    ("permuted uneven slices", emu_acc(x, w, order=perm, slices=[50, 3, 139]))):
        assert R.check_bits(name, a, exact.to(F32)) == 0
        assert bool((a.double() == exact).all())


@pytest.mark.parametrize("alpha", [1.0, 0.5, -2.0])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("out_mode", [0, 1])
def test_nt_restatement_equals_fp32_emulation(small, alpha, with_bias, out_mode):
    b = small["bias"] if with_bias else None
    got = emu_nt(small["x"], small["w"], b, alpha, out_mode=out_mode, acc=small["acc"])
    assert R.check_bits("nt", got, R.nt_ref(small["x"], small["w"], b, alpha, out_mode)) == 0


@pytest.mark.parametrize("with_bias", [False, True])
def test_residual_and_splitk_restatement_equals_fp32_emulation(small, with_bias):
    b = small["bias"] if with_bias else None
    ref = R.nt_ref(small["x"], small["w"], b, res=small["res"])
    assert R.check_bits("residual", emu_nt(small["x"], small["w"], b, res=small["res"], acc=small["acc"]), ref) == 0
    split = emu_acc(small["x"], small["w"], slices=[64, 64, 64])     # bias and residual folded in after the fixed-order sum
    assert R.check_bits("splitk", emu_nt(small["x"], small["w"], b, res=small["res"], acc=split), ref) == 0


def test_accumulate_restatements_equal_fp32_emulation(small):
    out0 = torch.randint(-50, 50, (M0, N0), generator=torch.Generator().manual_seed(6)).float()
    emu = out0.clone()
    for _ in range(2):
        emu = emu + emu_acc(small["x"], small["w"], slices=[64, 128])
    assert R.check_bits("nt_accum", emu, R.accum_ref(out0, small["x"], small["w"], times=2)) == 0
    T, O, I = 65, 24, 16
    dy, a = R.ints(T, O, 21, 20), R.ints(T, I, 22, 20)
    g0 = torch.randint(-50, 50, (O, I), generator=torch.Generator().manual_seed(7)).float()
    emu = g0 + emu_acc(dy.T.contiguous(), a.T.contiguous())
    assert R.check_bits("tn_accum", emu, R.tn_ref(g0, dy, a)) == 0


def test_inexact_inputs_are_refused():
    x = torch.randn(8, 64).to(BF)
    with pytest.raises(R.NotExact):
        R.nt_ref(x, x)


def test_activation_derivatives_equal_fp64_autograd():
    g = torch.Generator().manual_seed(9)
    v = (torch.randn(4000, generator=g, dtype=F64) * 3).requires_grad_(True)
    for act in (0, 1):
        val, _ = R.f_act(v, act)
        (auto,) = torch.autograd.grad(val.sum(), v)
        gr, _ = R.f_act_grad(v.detach(), act)
        assert float((auto - gr).abs().max()) < 1e-14
    y = torch.randn(4000, generator=g, dtype=F64).requires_grad_(True)
    gate = (torch.randn(4000, generator=g, dtype=F64) * 2).requires_grad_(True)
    d = torch.randn(4000, generator=g, dtype=F64) * 3
    act, _ = R.f_swiglu(y, gate)
    ay, ag = torch.autograd.grad((act * d).sum(), (y, gate))
    dy, _, dg, _ = R.f_swiglu_bwd(d, y.detach(), gate.detach())
    assert float((ay - dy).abs().max()) < 1e-13 and float((ag - dg).abs().max()) < 1e-13
    # the (act, gate) form is the same derivative with y = act / silu(gate) (here on the unrounded act)
    dy2, _, dg2, tg2 = R.f_swiglu_bwd_ag(d, act.detach(), gate.detach())
    assert float((ay - dy2).abs().max()) < 1e-13 and float(((ag - dg2).abs() / tg2).max()) < 1e-13
    assert float((torch.nn.functional.silu(gate) * y - act).detach().abs().max()) < 1e-14
    assert float((torch.nn.functional.gelu(v) - R.f_act(v, 0)[0]).detach().abs().max()) < 1e-14


def test_layout_helpers_round_trip():
    y, g = R.ints(5, 96, 1), R.ints(5, 96, 2)
    yg = R.join_yg(y, g)
    assert torch.equal(yg[:, 32:64], g[:, :32]) and torch.equal(yg[:, 64:96], y[:, 32:64])
    y2, g2 = R.split_yg(yg)
    assert torch.equal(y2, y) and torch.equal(g2, g)
    wy, wg = R.ints(96, 64, 3), R.ints(96, 64, 4)
    wi = R.interleave32(wy, wg)
    x = R.ints(5, 64, 5)
    assert torch.equal(R.acc_exact(x, wi), R.join_yg(R.acc_exact(x, wy), R.acc_exact(x, wg)))


# ------------------------------------------------------------------------------------------------ the inputs are sharp
def _families(K):
    M, N = 64, 72                                   # 4608 outputs
    x, w = R.operands(M, N, K, 31)
    acc = R.acc_exact(x, w)
    b = R.bias_vec(N, 33).double()
    fam = {"plain": acc, "bias": acc + b}
    for al in R.ALPHAS:
        fam[f"alpha {al}"] = acc * al
        fam[f"alpha {al} + bias"] = acc * al + b
    fam["residual add"] = R.nt_ref(x, w, b.float()).double() + R.residual(M, N, 35).double()
    return acc, fam


def _scaled_families(K):
    M, N = 64, 72
    x, w = R.operands(M, N, K, 41, scaled=True)
    acc = R.acc_exact(x, w)
    return acc, {"saved linear (YG, G, d act)": acc, "Pre": acc + R.bias_vec(N, 43, kmax=8).double()}


@pytest.mark.parametrize("K", R.K_PLAIN + R.K_SPLITK)
def test_inputs_are_sharp(K):
    for unit, (acc, fam) in ((1.0, _families(K)),) + (((R.w_scale(K), _scaled_families(K)),) if K in R.K_FUSED else ()):
        assert acc.numel() >= 4096
        assert float((acc / unit).abs().max()) < 2 ** 24          # the largest |sum| in units of the operands' grid
        for name, v in fam.items():
            off, ties = R.sharpness(v)
            assert off >= 0.5, (K, name, off)
            assert ties >= 0.01, (K, name, ties)
    x, w = R.operands(64, 72, K, 31)
    assert float(R.acc_exact(x, w).abs().max()) < 2 ** 24 and R.amp(K) <= 32
    if K in R.K_FUSED:
        sd = float(R.acc_exact(*R.operands(64, 72, K, 41, scaled=True)).std())
        assert 1.0 <= sd <= 4.0


# --------------------------------------------------------------------------------------------- planted errors are caught
def _ref_and_args(small, **kw):
    return R.nt_ref(small["x"], small["w"], **kw)


def test_planted_dropped_product_in_partial_panel(small):
    acc = emu_acc(small["x"], small["w"], drop_product=(129, 17, 77))
    with pytest.raises(R.BitMismatch, match=r"row 129, column 17"):
        R.check_bits("nt", emu_nt(small["x"], small["w"], acc=acc), _ref_and_args(small))
    with pytest.raises(R.BitMismatch):
        R.check_bits("nt f32", emu_nt(small["x"], small["w"], acc=acc, out_mode=1), _ref_and_args(small, out_mode=1))


def test_planted_dropped_ktile_in_one_row(small):
    acc = emu_acc(small["x"], small["w"], drop_ktile=(64, 1))
    with pytest.raises(R.BitMismatch, match=r"in 1 rows; first at \(row 64"):
        R.check_bits("nt", emu_nt(small["x"], small["w"], small["bias"], acc=acc), _ref_and_args(small, bias=small["bias"]))


def test_planted_last_panel_shifted_by_one_row(small):
    out = emu_nt(small["x"], small["w"], acc=small["acc"]).clone()
    out[128:] = torch.roll(out[128:], 1, 0)
    with pytest.raises(R.BitMismatch, match=r"first at \(row 128"):
        R.check_bits("nt", out, _ref_and_args(small))


def test_planted_bias_missing_on_last_8_columns(small):
    out = emu_nt(small["x"], small["w"], small["bias"], acc=small["acc"], no_bias_cols=8)
    with pytest.raises(R.BitMismatch, match=r"in 130 rows; first at \(row 0, column 3[2-9]\)"):
        R.check_bits("nt", out, _ref_and_args(small, bias=small["bias"]))
    one_row = emu_nt(small["x"][:1], small["w"], small["bias"], no_bias_cols=8)       # M = 1 is enough to see it
    with pytest.raises(R.BitMismatch):
        R.check_bits("nt", one_row, R.nt_ref(small["x"][:1], small["w"], small["bias"]))


def test_planted_truncation_instead_of_rne(small):
    for kw in (dict(), dict(bias=small["bias"]), dict(alpha=-2.0)):
        out = emu_nt(small["x"], small["w"], acc=small["acc"], trunc=True, **kw)
        with pytest.raises(R.BitMismatch):
            R.check_bits("nt", out, _ref_and_args(small, **kw))
    trunc_second = (emu_nt(small["x"], small["w"], acc=small["acc"]).float() + small["res"].float())
    with pytest.raises(R.BitMismatch):
        R.check_bits("residual", trunc_bf16(trunc_second), _ref_and_args(small, res=small["res"]))


@pytest.mark.parametrize("alpha", R.ALPHAS)
def test_planted_alpha_ignored(small, alpha):
    out = emu_nt(small["x"], small["w"], small["bias"], alpha, acc=small["acc"], ignore_alpha=True)
    with pytest.raises(R.BitMismatch):
        R.check_bits("nt", out, _ref_and_args(small, bias=small["bias"], alpha=alpha))


def test_planted_residual_from_the_next_row(small):
    out = emu_nt(small["x"], small["w"], acc=small["acc"], res=small["res"], res_shift=1)
    with pytest.raises(R.BitMismatch, match=r"first at \(row 0"):
        R.check_bits("residual", out, _ref_and_args(small, res=small["res"]))


def test_planted_y_and_gate_swapped_in_one_group():
    M, I, K = 33, 96, 128
    x, wi, wy, wg = R.swiglu_case(M, I, K)
    yg = R.linear_bf16(x, wi)
    y, g = R.split_yg(yg)
    assert R.check_bits("y", y, R.linear_bf16(x, wy)) == 0 and R.check_bits("g", g, R.linear_bf16(x, wg)) == 0
    ref, t = R.f_swiglu(*R.d64(y, g))
    good = (g.float() * y.float() * torch.sigmoid(g.float())).to(BF)
    assert R.check_nonlinear("act", good, ref, t, "swiglu") <= 1.0
    bad_yg = yg.clone()
    bad_yg[:, 64:96], bad_yg[:, 96:128] = yg[:, 96:128], yg[:, 64:96]
    with pytest.raises(R.BitMismatch, match="column 64"):
        R.check_bits("YG", bad_yg, yg)
    by, bg = R.split_yg(bad_yg)
    bad_act = (bg.float() * by.float() * torch.sigmoid(bg.float())).to(BF)
    with pytest.raises(RowMismatch, match=r"column 3[2-9]|column [45]\d|column 6[0-3]"):
        R.check_nonlinear("act", bad_act, ref, t, "swiglu")


def test_planted_writes_outside_the_payload(small):
    ref = _ref_and_args(small)
    out = R.Buf(M0, N0, N0 + 24, data=ref, name="out")
    R.check_poison([out, None])
    assert R.check_bits("out", out.get(), ref) == 0
    out.full.view(-1, N0 + 24)[R.GUARD + M0, 3] = 1.0            # one element written past M
    with pytest.raises(AssertionError, match="out"):
        R.check_poison([out])
    pad = R.Buf(M0, N0, N0 + 24, data=ref, name="pad")
    pad.full.view(-1, N0 + 24)[R.GUARD + 5, N0 + 2] = 0.0        # one poisoned pad column overwritten
    with pytest.raises(AssertionError, match="pad"):
        R.check_poison([pad])
    ws = R.Buf(1, 100, 164, dtype=F32, name="ws")
    assert ws.intact() and bool(torch.isnan(ws.t).all())
    ws.full[R.GUARD * 164 + 100] = 0.0                           # the float just past ws_floats
    assert not ws.intact()
    before = R.Buf(4, 8, 8, dtype=F32, name="before")
    before.full[R.GUARD * 8 - 1] = 0.0
    assert not before.intact()


def test_planted_nan_reaches_the_result_and_the_checkers(small):
    ref = _ref_and_args(small)
    out = ref.clone()
    bits(out)[7, 7] = R.POISON[2]
    with pytest.raises(R.BitMismatch, match=r"row 7, column 7"):
        R.check_bits("nt", out, ref)
    r64 = ref.double()
    with pytest.raises(RowMismatch):
        R.check_nonlinear("nan", out, r64, r64.abs(), "swiglu")


def test_dbias_and_gauss_bounds_reject_a_lost_row():
    M, N, K = 129, 136, 128
    dy, w, pre = R.act_bwd_case(M, N, K)
    d = R.linear_bf16(dy, w)
    ref, t = R.f_act_bwd(*R.d64(d, pre), 0)
    dpre = ref.to(BF)
    init = torch.full((N,), 3.0)
    good = (init.double() + dpre.double().sum(0)).float()
    assert R.check_dbias("dbias", good, init, dpre, M) <= 1.0
    lost = (init.double() + dpre[:128].double().sum(0)).float()       # the partial block's row never summed
    with pytest.raises(RowMismatch):
        R.check_dbias("dbias", lost, init, dpre, M)
    x, wg = torch.randn(M, K).to(BF), (torch.randn(N, K) * 0.05).to(BF)
    out = x.float() @ wg.float().T
    assert R.check_gauss_f32("gauss", out, x, wg, None) <= 1.0
    out[128, 5] -= x[128, 64:].float() @ wg[5, 64:].float()          # one K-tile lost in one element
    with pytest.raises(RowMismatch, match="row 128, column 5"):
        R.check_gauss_f32("gauss", out, x, wg, None)


# ------------------------------------------------------------------------------------------------ measured constants
def _measure():
    """Worst |fp32 torch evaluation - fp64| / (2^-24 T) of every nonlinear formula on the inputs of the GPU cases."""
    worst = {k: 0.0 for k in R.C_MEAS}

    def upd(form, ref, t, emu):
        worst[form] = max(worst[form], R.meas_ratio(ref, t, emu))

    K = R.K_FUSED[0]
    for M in R.NONLINEAR_M:             # every case of the GPU file (a smaller M is not exactly a prefix of a larger Gaussian draw)
        for I in R.SWIGLU_I:
            x, wi, _, _ = R.swiglu_case(M, I, K)
            y, g = R.split_yg(R.linear_bf16(x, wi))
            upd("swiglu", *R.f_swiglu(*R.d64(y, g)), R.f_swiglu(y.float(), g.float())[0])
        for N in R.ACT_N:
            x, w, b = R.act_case(M, N, K)
            pre = R.linear_bf16(x, w, b)
            for act, form in ((0, "gelu"), (1, "qgelu")):
                upd(form, *R.f_act(pre.double(), act), R.f_act(pre.float(), act)[0])
        for I in R.BWD_I:
            dy, w, y, g, act = R.swiglu_bwd_case(M, I, K)
            d = R.acc_exact(dy, w)
            ry, ty, rg, tg = R.f_swiglu_bwd(d, *R.d64(y, g))
            ey, _, eg, _ = R.f_swiglu_bwd(d.float(), y.float(), g.float())
            upd("swiglu_bwd.dy", ry, ty, ey)
            upd("swiglu_bwd.dg", rg, tg, eg)
            ry, ty, rg, tg = R.f_swiglu_bwd_ag(d, *R.d64(act, g))
            _, _, eg, _ = R.f_swiglu_bwd_ag(d.float(), act.float(), g.float())
            upd("swiglu_bwd_ag.dg", rg, tg, eg)
    for M in R.ACT_BWD_M:
        for N in R.ACT_N:
            dy, w2, pre2 = R.act_bwd_case(M, N, K)
            d = R.linear_bf16(dy, w2)
            for act, form in ((0, "gelu_bwd"), (1, "qgelu_bwd")):
                upd(form, *R.f_act_bwd(*R.d64(d, pre2), act), R.f_act_bwd(d.float(), pre2.float(), act)[0])
    return worst


def test_measured_constants():
    worst = _measure()
    print({k: round(v, 3) for k, v in worst.items()})
    for form, c in R.C_MEAS.items():
        assert 0.4 * c <= worst[form] <= c, f"{form}: measured {worst[form]:.3f}, table {c}: re-measure and update C_MEAS and the GPU file's docstring"


def test_fp32_emulation_passes_the_nonlinear_bounds():
    """The checker accepts what it should: an fp32 evaluation rounded once to bf16 stays inside 1 ulp + C 2^-24 T."""
    M, N, K = 129, 136, 128
    x, w, b = R.act_case(M, N, K)
    pre = R.linear_bf16(x, w, b)
    for act, form in ((0, "gelu"), (1, "qgelu")):
        ref, t = R.f_act(pre.double(), act)
        assert R.check_nonlinear(form, R.f_act(pre.float(), act)[0].to(BF), ref, t, form) <= 1.0
        off_by_two = (ref + 2.5 * R.bf16_ulp(ref) * (ref != 0)).to(BF)
        with pytest.raises(RowMismatch):
            R.check_nonlinear(form, off_by_two, ref, t, form)
