"""cx_xent_fwd / cx_xent_bwd (contrastors_amd/csrc/xent.hip) and cx_grad_sq_norm / cx_adamw_clip_step / cx_ema_update
(optimizer.hip) through the C ABI against tests/ew_ref.py, per element, at every branch of their launchers.

xent: lse and loss per row, dlogits per element, against fp64 on the rounded inputs under C 2^-24 T (fp32) or 1 ulp_bf16 + C 2^-24 T
(bf16 gradients), T including the argument-dependent error of __expf (ew_ref's docstring derives it); the backward reference is
formed from the lse the forward STORED.  Ignored rows (ignore_index, label < 0, label >= V) are exactly zero in loss and gradient.
Optimizer: p, m, v per element against one fp64 AdamW step in the operation order of adam_one, the clip coefficient from an fp64 sum
of squares handed to the kernel as its device double; cx_grad_sq_norm by itself under its derived relative bound (4 k + 4) 2^-24.
C = 4 C_meas, C_meas measured by tests/test_ew_ref_cpu.py on fp32 emulations (never against a kernel).

Every operand and result is an ew_ref.Slab (NaN guard elements either side, NaN in the gap between V and the leading dimension,
results start as NaN); the guards are checked when each test ends.  Worst err / bound per entry point goes through gpu_util.report.

Which test reaches what (by reading the launchers):
    xent_fwd / bwd <bf16, 8> and <float, 4>: V % 8 (4) == 0, ld = V and ld = V + 8 .............. test_xent[V 8, 2048, 2056, 30528]
    xent_fwd / bwd <*, 1> by V (1, 7, 30522), by ld (V + 3), by a base pointer one element off,
       by ld_d alone (backward: ld_d = ld + 3 under a vector-capable ld) ........................ test_xent (every V), test_xent_bwd_ld_d_alone
    lanes without a column (V < 256 VEC), one step, several steps, a partial last step .......... test_xent[V 1 .. 30528]
    labels 0 and V - 1, ignore_index, label = V, label = -1; logit_scale 1 and 0.25 ............. test_xent
    backward out of place with ld_d != ld, and in place ......................................... test_xent
    the in-lane update while every logit seen so far is -inf (guarded; it formed NaN before) .... test_xent_neginf
    CX_ERR_SHAPE (ld < V), CX_ERR_ARG (NULL) .................................................... test_xent_rejections
    grad_sq_norm / adamw / ema kernels: n < 4 (tail lanes only), n % 4 = 0, 1, 3, one block, the
       4096-block cap wrapped (2^22 + 4099: 1 049 600 float4 on 1 048 576 lanes, tail 3) ......... test_grad_sq_norm, test_adamw, test_ema
    coef: sq_norm NULL, max_norm <= 0, clipping, not clipping; step 1 and 1000; decay 0 and 0.1 .. test_adamw
    CX_ERR_SHAPE (a pointer 4 bytes off), CX_ERR_ARG (step 0, decay > 1, NULL) .................. test_optimizer_rejections
"""
import functools

import pytest
import torch

from contrastors_amd import _C
from tests import ew_ref as E
from tests import gemm_ref as R
from tests.gemm_ref import BF, F32, F64
from tests.gpu_util import L, S, report
from tests.test_elementwise_edges_gpu import ERR_ARG, ERR_SHAPE, Worst, _BUFS, _poison, slab  # noqa: F401  (_poison: the autouse guard check)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DLOSS = torch.tensor([1.0, -0.5, 2.0, 0.25, 3.0])


# =============================================================================================================== xent
def run_xent(tag, x, lab, scale, ld, lead, w, neginf_cols=None):
    """Forward, backward out of place (ld_d = ld + 8: keeps a vector route, differs from ld) and in place, all checked."""
    N, V = x.shape
    dtype, is_bf = x.dtype, int(x.dtype == BF)
    labels = lab.to(DEV)
    X = slab(N, V, ld, dtype=dtype, data=x, lead=lead, name="logits")
    LOSS, LSE = slab(1, N, dtype=F32, name="loss"), slab(1, N, dtype=F32, name="lse")
    _C.check(L().cx_xent_fwd(X.ptr, is_bf, labels.data_ptr(), LOSS.ptr, LSE.ptr, N, V, ld, scale, E.IGNORE, S()), f"xent_fwd {tag}")
    loss, lse = LOSS.get()[0], LSE.get()[0]
    r1, r2, ref = E.check_xent_fwd(tag, loss, lse, x, lab, scale)
    w.add("cx_xent_fwd.lse", r1)
    w.add("cx_xent_fwd.loss", r2)
    DL = slab(1, N, dtype=F32, data=DLOSS, name="dloss")
    ldd = ld + 8
    DX = slab(N, V, ldd, dtype=dtype, lead=lead, name="dlogits")
    _C.check(L().cx_xent_bwd(DL.ptr, X.ptr, is_bf, LSE.ptr, labels.data_ptr(), DX.ptr, N, V, ld, ldd, scale, E.IGNORE, S()), f"xent_bwd {tag}")
    out = DX.get()
    w.add("cx_xent_bwd", E.check_xent_bwd(f"{tag} out of place", out, x, lab, DLOSS, lse, scale, ref["lse"]))
    assert R.check_bits(f"{tag}: the logits of an out-of-place backward", X.get(), x) == 0
    _C.check(L().cx_xent_bwd(DL.ptr, X.ptr, is_bf, LSE.ptr, labels.data_ptr(), X.ptr, N, V, ld, ld, scale, E.IGNORE, S()), f"xent_bwd in place {tag}")
    inpl = X.get()
    w.add("cx_xent_bwd", E.check_xent_bwd(f"{tag} in place", inpl, x, lab, DLOSS, lse, scale, ref["lse"]))
    if neginf_cols is not None:
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss).all()), f"{tag}: lse / loss of a row with -inf logits"
        for g in (out, inpl):
            assert bool((g[:, neginf_cols] == 0).all()), f"{tag}: the gradient of a -inf logit is exactly 0"


def _routes(V, dtype):
    """(ld, lead, elements per lane the launcher picks)."""
    return [(ld, lead, E.xent_vec(V, ld, dtype, aligned=lead == 0, ld_d=ld + 8 if lead == 0 else None))
            for ld, lead in ((V, 0), (V + 8, 0), (V + 3, 0), (V, 1))]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", E.XENT_V)
def test_xent(V, dtype):
    lab = E.xent_labels(V)
    w = Worst()
    routes = _routes(V, dtype)
    if V % 8 == 0:
        assert [r[2] for r in routes] == [8 if dtype == BF else 4] * 2 + [1, 1]
    else:
        assert [r[2] for r in routes] == [1, 1, 1, 1]
    for fam in E.XENT_FAMILIES:
        x = E.xent_inputs(V, fam, dtype)
        for scale in (1.0, 0.25):
            for ld, lead, vec in routes:
                run_xent(f"xent V={V} {fam} scale={scale} ld={ld} lead={lead} vec={vec}", x, lab, scale, ld, lead, w)
    w.flush(f"xent V={V} {dtype}")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_xent_bwd_ld_d_alone(dtype):
    """The backward's scalar route chosen by ld_d alone (ld and both pointers allow vectors)."""
    V, scale = 2048, 1.0
    x, lab = E.xent_inputs(V, "gauss1", dtype), E.xent_labels(V)
    ref = E.xent_ref(x, lab, scale)
    lse = ref["lse"].float()
    X, LSE = slab(E.XENT_N, V, dtype=dtype, data=x, name="logits"), slab(1, E.XENT_N, dtype=F32, data=lse, name="lse")
    DL, DX = slab(1, E.XENT_N, dtype=F32, data=DLOSS, name="dloss"), slab(E.XENT_N, V, V + 3, dtype=dtype, name="dlogits")
    labels = lab.to(DEV)
    assert E.xent_vec(V, V, dtype, ld_d=V + 3) == 1
    _C.check(L().cx_xent_bwd(DL.ptr, X.ptr, int(dtype == BF), LSE.ptr, labels.data_ptr(), DX.ptr, E.XENT_N, V, V, V + 3, scale, E.IGNORE, S()))
    r = E.check_xent_bwd("xent_bwd ld_d = V + 3", DX.get(), x, lab, DLOSS, lse, scale, ref["lse"])
    report("cx_xent_bwd", test=f"ld_d alone {dtype}", worst_err_over_bound=r)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [v for v in E.XENT_V if v >= 2048])
def test_xent_neginf(V, dtype):
    """Rows with -inf at columns 0-15 and at the last column, a finite maximum and an unmasked label: lse and loss finite and within
    bound, the gradient exactly 0 at the masked columns.  Before the guard in xent_fwd_kernel's in-lane update, lane 0 (vector
    routes: lanes 0 and 1; scalar routes: lanes 0-15) formed exp(-inf - -inf) = NaN in its first step and lse, loss were NaN."""
    x, lab = E.xent_neginf_inputs(V, dtype)
    w = Worst()
    cols = list(range(16)) + [V - 1]
    for ld, lead, vec in _routes(V, dtype):
        run_xent(f"xent -inf V={V} ld={ld} lead={lead} vec={vec}", x, lab, 1.0, ld, lead, w, neginf_cols=cols)
    w.flush(f"xent -inf V={V} {dtype}")


def test_xent_rejections():
    X, O = slab(2, 16, dtype=F32, name="x"), slab(1, 2, dtype=F32, name="o")
    lab = torch.zeros(2, dtype=torch.int64, device=DEV)
    lib = L()
    assert lib.cx_xent_fwd(X.ptr, 0, lab.data_ptr(), O.ptr, O.ptr, 2, 16, 12, 1.0, E.IGNORE, S()) == ERR_SHAPE
    assert lib.cx_xent_fwd(X.ptr, 0, lab.data_ptr(), O.ptr, O.ptr, 2, 0, 16, 1.0, E.IGNORE, S()) == ERR_SHAPE
    assert lib.cx_xent_fwd(X.ptr, 0, None, O.ptr, O.ptr, 2, 16, 16, 1.0, E.IGNORE, S()) == ERR_ARG
    assert lib.cx_xent_bwd(O.ptr, X.ptr, 0, O.ptr, lab.data_ptr(), X.ptr, 2, 16, 16, 12, 1.0, E.IGNORE, S()) == ERR_SHAPE
    assert lib.cx_xent_bwd(O.ptr, X.ptr, 0, None, lab.data_ptr(), X.ptr, 2, 16, 16, 16, 1.0, E.IGNORE, S()) == ERR_ARG


# ========================================================================================================== optimizer
@functools.lru_cache(maxsize=2)
def opt_case(n):
    p, g, m, v = E.opt_inputs(n)
    return p, g, m, v, g.double().pow(2).sum()


@pytest.mark.parametrize("n", E.OPT_N)
def test_grad_sq_norm(n):
    _, g, _, _, sq = opt_case(n)
    G = slab(1, n, dtype=F32, data=g, name="grad")
    for init in (0.0, 1.5):                                          # the kernel accumulates into the double
        acc = torch.tensor([7.0, init, 7.0], dtype=F64, device=DEV)
        _C.check(L().cx_grad_sq_norm(G.ptr, n, acc.data_ptr() + 8, S()), "grad_sq_norm")
        got = acc.cpu()
        assert got[0] == 7.0 and got[2] == 7.0
        err, bound = abs(float(got[1]) - init - float(sq)), E.sq_norm_bound(n) * float(sq) + (E.sq_norm_blocks(n) + 8) * 2.0 ** -53 * (init + float(sq))
        assert err <= bound, f"grad_sq_norm n={n}: got {float(got[1]) - init!r}, fp64 {float(sq)!r}, |err| {err:.3e} > bound {bound:.3e}"
    assert R.check_bits("the gradient of grad_sq_norm", G.get(), g[None]) == 0
    report("cx_grad_sq_norm", test=f"n={n}", worst_err_over_bound=err / bound if bound else 0.0)


@pytest.mark.parametrize("case", range(len(E.OPT_CASES)))
@pytest.mark.parametrize("n", E.OPT_N)
def test_adamw(n, case):
    step, wd, kind, max_norm, lr = E.OPT_CASES[case]
    p, g, m, v, sq = opt_case(n)
    Ps, G, M, V = (slab(1, n, dtype=F32, data=t, name=nm) for t, nm in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")))
    SQ = None if kind is None else torch.tensor([sq], dtype=F64, device=DEV)       # the fp64 sum of squares, as cx_grad_sq_norm's double
    _C.check(L().cx_adamw_clip_step(Ps.ptr, G.ptr, M.ptr, V.ptr, n, lr, E.HP["beta1"], E.HP["beta2"], E.HP["eps"], wd, step,
                                    None if SQ is None else SQ.data_ptr(), max_norm, S()), "adamw")
    rp, rm, rv, tp, tm, tv = E.adamw_step(p, g, m, v, lr, wd, step, None if kind is None else sq, max_norm)
    if kind == "clip" and n >= 1027:
        assert float(E.clip_coef(sq, max_norm)) < 1.0
    w = Worst()
    for nm, got, ref, t in (("p", Ps, rp, tp), ("m", M, rm, tm), ("v", V, rv, tv)):
        w.add(f"cx_adamw_clip_step.{nm}", E.check_f32(f"adamw n={n} case={case} {nm}", got.get(), ref[None], t[None], E.C("opt", nm)))
    assert R.check_bits("the gradient of adamw", G.get(), g[None]) == 0
    w.flush(f"adamw n={n} case={case}")


@pytest.mark.parametrize("decay", [0.0, 0.999, 1.0])
@pytest.mark.parametrize("n", E.OPT_N)
def test_ema(n, decay):
    p, _, m, _, _ = opt_case(n)
    Es, Ps = slab(1, n, dtype=F32, data=m, name="ema"), slab(1, n, dtype=F32, data=p, name="param")
    _C.check(L().cx_ema_update(Es.ptr, Ps.ptr, n, decay, S()), "ema")
    ref, t = E.ema_step(m, p, decay)
    r = E.check_f32(f"ema n={n} decay={decay}", Es.get(), ref[None], t[None], E.C("opt", "ema"))
    if decay in (0.0, 1.0):
        assert R.check_bits(f"ema decay={decay}", Es.get(), (p if decay == 0.0 else m)[None]) == 0
    assert R.check_bits("the parameters of ema", Ps.get(), p[None]) == 0
    report("cx_ema_update", test=f"n={n} decay={decay}", worst_err_over_bound=r)
    assert r <= 1.0


def test_optimizer_rejections():
    A, B, Cc, D = (slab(1, 16, dtype=F32, data=torch.ones(16), name=nm) for nm in "abcd")
    sq = torch.zeros(1, dtype=F64, device=DEV)
    lib, hp = L(), (2e-4, 0.9, 0.999, 1e-8, 0.1)
    assert lib.cx_adamw_clip_step(A.ptr + 4, B.ptr, Cc.ptr, D.ptr, 8, *hp, 1, None, 0.0, S()) == ERR_SHAPE
    assert lib.cx_adamw_clip_step(A.ptr, B.ptr, Cc.ptr, D.ptr + 4, 8, *hp, 1, None, 0.0, S()) == ERR_SHAPE
    assert lib.cx_adamw_clip_step(A.ptr, B.ptr, Cc.ptr, D.ptr, 8, *hp, 0, None, 0.0, S()) == ERR_ARG
    assert lib.cx_adamw_clip_step(A.ptr, None, Cc.ptr, D.ptr, 8, *hp, 1, None, 0.0, S()) == ERR_ARG
    assert lib.cx_grad_sq_norm(A.ptr + 4, 8, sq.data_ptr(), S()) == ERR_SHAPE
    assert lib.cx_grad_sq_norm(A.ptr, 8, None, S()) == ERR_ARG
    assert lib.cx_ema_update(A.ptr + 4, B.ptr, 8, 0.5, S()) == ERR_SHAPE
    assert lib.cx_ema_update(A.ptr, B.ptr, 8, 1.5, S()) == ERR_ARG
    assert lib.cx_ema_update(A.ptr, B.ptr, 8, -0.1, S()) == ERR_ARG
    assert lib.cx_ema_update(A.ptr, B.ptr, 8, float("nan"), S()) == ERR_ARG
    torch.cuda.synchronize()
    assert float(sq.cpu()) == 0.0 and all(bool((t.get() == 1).all()) for t in (A, B, Cc, D))
