"""The glue kernels of contrastors_amd/csrc/elementwise.hip and the front end of vit.hip through the C ABI against tests/ew_ref.py, per
element, at the grid, tail, width and stride edges of their launchers.

Transposes, casts, both rotary entry points and the three ViT front-end kernels are compared BIT FOR BIT (the cast with torch's CPU conversion on inputs full of exact
ties, the rotary with attn_ref.rotate_bf16).  Activations, pooling and the fused activation backward are held per element to the fp64
formula on the exact rounded inputs under 1 ulp_bf16(ref) + C 2^-24 T (bf16 results) or C 2^-24 T (fp32 results), C = 4 C_meas with
C_meas measured by tests/test_ew_ref_cpu.py on an fp32 emulation of the kernels' formulas (never against a kernel), on Gaussian inputs
and on the saturation family (0, +-2^-126, +-2^-20, +-8, +-20, +-50, +-100 as gate or pre-activation); each activation bound also
carries the fp32 underflow term ew_ref.act_floor (2^-126 times the factor a flushed sigmoid multiplies: ~1e-36).  Column sums are held to the
derived bound (chain + 4) 2^-23 (sum|term| + |init|); the dbias of the fused backward to the fp64 sum of the bf16 dpre the kernel returned.

Every operand and result is an ew_ref.Slab: a payload inside a larger allocation whose guard elements either side and whose columns
between the width and the leading dimension hold a NaN bit pattern; results start as NaN, so a skipped element stays NaN and a read
outside an operand poisons the result.  The guards are checked when each test ends (`_poison`).  Each test reports its worst
err / bound (0 for the bit-exact ones) per entry point through gpu_util.report.

Which test reaches what (by reading the launchers):
    transpose_bf16_kernel: partial tiles in rows and cols, rows_pad = rows / > rows (zero fill) / a further
       tile of pure padding, ld_out > rows_pad, the five CX_ERR_ALIGN conditions ............ test_transpose_bf16
    transpose_f32_kernel, cast_transpose_f32_bf16_kernel: 1 x 8 .. 130 x 70, free strides .... test_transpose_f32_and_cast_transpose
    cast_transpose_batched_kernel: blocks past a job's tile count leave at once .............. test_cast_transpose_batched
    cast_f32_bf16_kernel: scalar tail n % 4 = 1, 2, 3 (alone and after vectors), grid_for's
       2048-block cap (2^21 + 3075: 524 288 float4 on 524 288 lanes + 768 wrapped + tail 3) ... test_cast_f32_to_bf16
    cast_bf16_f32_kernel: one lane, partial block, two blocks, the 2048-block cap wrapped .... test_cast_bf16_to_f32
    swiglu_fwd / swiglu_bwd (layouts 0, 1), swiglu_bwd_gate, bias_gelu_fwd<GELU / QUICK_GELU>
       (bias or NULL), bias_gelu_bwd (bias or NULL): one chunk, one row, several rows, more
       than one block, the 2048-block cap (537 600 chunks: the stride wraps over 51 rows) ..... test_activations
    CX_ERR_SHAPE (I % 8, layout 1 with I % 32), CX_ERR_ARG (act) ............................. test_activation_rejections
    colsum_kernel<false> (U = 4), ld = N + 8, dbias += on a non-zero vector; colsum_rows_grid:
       gy = 1 (T <= 256: one atomic, run twice bit-identical), the T / 256 clamp (257, 1000),
       the 1024 / colblocks clamp (N = 768: colblocks 3), the 512 cap (T = 131 073) ........... test_bias_grad
    colsum_kernel<true, GELU / QUICK_GELU> (U = 2), bias or NULL, dbias or NULL, the clamped
       over-read tc = T - 1 of the unrolled pass (T = 1, 7, 17, 33 around 8 U gy rows) ........ test_bias_act_bwd_colsum
    pool_normalize_fwd / bwd: ngroups = 256 (d = 8), 32, 2 (d = 768: 192 of 256 lanes), 1 with
       127 idle lanes (d = 1032), 1 at the cap (d = 2048); an empty sequence, a one-token one,
       an all-zero one (the eps clamp); CX_ERR_SHAPE at d = 4, 2056 ........................... test_pool, test_pool_rejections
    rotary_kernel nwhich = 2: gx = 1 .. the cap of 64 blocks (H = 12: 19 200 work items of the
       200-token sequence on 16 384 lanes), an empty and a one-token sequence, sign +-1 ....... test_rotary_qkv
    rotary_kernel nwhich = 1: tok_stride = H 64, 3 H 64, H 64 + 8; max_seqlen below the longest
       sequence (gx from max_seqlen, the stride loop covers the rest); CX_ERR_ALIGN / _ARG ..... test_rotary_apply
    patchify_kernel<float / bf16>: one partial block (144 lanes), 13.5 blocks; every patch, or
       4 of 6 gathered in unsorted order, the last patch among them ........................... test_vit_patchify
    vit_assemble_fwd_kernel: 9 and 65 lanes of the last block idle; position rows by sequence
       slot, or by kept patch .................................................................. test_vit_assemble_fwd
    vit_assemble_bwd_kernel: a block of 3 lanes (d = 24), two column blocks with 63 lanes of the
       second idle (d = 520); every position, or the original positions through `inv` (-1 entries,
       a patch no image kept, a slot nothing maps to); += on non-zero gpos / gcls; either NULL .. test_vit_assemble_bwd
"""
import numpy as np
import pytest
import torch

from contrastors_amd import _C
from tests import ew_ref as E
from tests import gemm_ref as R
from tests.gemm_ref import BF, F32, F64
from tests.gpu_util import L, S, report
from tests.ln_ref import bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -3
_BUFS = []


def slab(rows, cols, ld=None, dtype=BF, data=None, lead=0, name=""):
    b = E.Slab(rows, cols, ld, dtype=dtype, device=DEV, data=data, lead=lead, name=name)
    _BUFS.append(b)
    return b


def P(b):
    return None if b is None else b.ptr


@pytest.fixture(autouse=True)
def _poison():
    _BUFS.clear()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a GPU fault: nothing more is started on this device
        _BUFS.clear()
        pytest.exit(f"GPU error, stopping the session: {e}", returncode=3)
    try:
        R.check_poison(_BUFS)
    finally:
        _BUFS.clear()


class Worst(dict):
    """entry point -> worst err / bound of one test; flush() reports them."""

    def add(self, entry, ratio):
        self[entry] = max(self.get(entry, 0.0), float(ratio))

    def flush(self, test):
        for entry, w in self.items():
            report(entry, test=test, worst_err_over_bound=w)
            assert w <= 1.0


def up(v, m):
    return (v + m - 1) // m * m


# ================================================================================================ transposes and casts
SHAPES_BF = ((1, 8), (13, 8), (63, 64), (64, 72), (65, 136))


@pytest.mark.parametrize("rows,cols", SHAPES_BF)
def test_transpose_bf16(rows, cols):
    x = R.gauss_bf16(rows, cols, 40 + rows)
    X = slab(rows, cols, cols + 8, data=x, name="In")
    for rows_pad in sorted({up(rows, 8), up(rows, 64), up(rows, 64) + 64}):
        O = slab(cols, rows_pad, rows_pad + 8, name=f"Out[{rows_pad}]")
        _C.check(L().cx_transpose_bf16(X.ptr, O.ptr, rows, cols, cols + 8, rows_pad + 8, rows_pad, S()), "transpose_bf16")
        assert R.check_bits(f"transpose_bf16 {rows}x{cols} pad {rows_pad}", O.get(), E.transpose_ref(x, rows_pad)) == 0
    O = slab(16, 16, name="untouched")
    for args in ((8, 12, 16, 16, 8), (8, 8, 12, 16, 8), (8, 8, 16, 12, 8), (8, 8, 16, 16, 12), (16, 8, 16, 16, 8)):
        assert L().cx_transpose_bf16(X.ptr, O.ptr, *args, S()) == ERR_ALIGN, args       # cols, ld_in, ld_out, rows_pad % 8; rows_pad < rows
    report("cx_transpose_bf16", test=f"{rows}x{cols}", differing=0)


@pytest.mark.parametrize("rows,cols", SHAPES_BF + ((130, 70),))
def test_transpose_f32_and_cast_transpose(rows, cols):
    x = E.cast_inputs(rows * cols, 50 + rows).reshape(rows, cols)
    X = slab(rows, cols, cols + 3, dtype=F32, data=x, name="In")
    O = slab(cols, rows, rows + 5, dtype=F32, name="Out")
    _C.check(L().cx_transpose_f32(X.ptr, O.ptr, rows, cols, cols + 3, rows + 5, S()), "transpose_f32")
    assert R.check_bits(f"transpose_f32 {rows}x{cols}", O.get(), E.transpose_ref(x)) == 0      # NaN payload and -0 included
    Xc = slab(rows, cols, dtype=F32, data=x, name="In dense")
    Oc = slab(cols, rows, name="OutT")
    _C.check(L().cx_cast_transpose_f32_to_bf16(Xc.ptr, Oc.ptr, rows, cols, S()), "cast_transpose")
    assert E.check_bits_nan(f"cast_transpose {rows}x{cols}", Oc.get(), E.cast_ref(x).T.contiguous()) == 0
    report("cx_transpose_f32", test=f"{rows}x{cols}", differing=0)
    report("cx_cast_transpose_f32_to_bf16", test=f"{rows}x{cols}", differing=0)


def test_cast_transpose_batched():
    shapes = ((63, 64), (130, 70), (64, 72))                        # 1, 6 and 2 tiles of 64 x 64
    tiles = [((r + 63) // 64) * ((c + 63) // 64) for r, c in shapes]
    assert tiles == [1, 6, 2]
    xs = [E.cast_inputs(r * c, 60 + i).reshape(r, c) for i, (r, c) in enumerate(shapes)]
    ins = [slab(r, c, dtype=F32, data=x, name=f"In{i}") for i, ((r, c), x) in enumerate(zip(shapes, xs))]
    outs = [slab(c, r, name=f"OutT{i}") for i, (r, c) in enumerate(shapes)]
    tab = np.zeros(3, dtype=np.dtype([("in", "u8"), ("out", "u8"), ("rows", "i4"), ("cols", "i4")]))
    for i, (a, o, (r, c)) in enumerate(zip(ins, outs, shapes)):
        tab[i] = (a.ptr, o.ptr, r, c)
    dev_tab = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    _C.check(L().cx_cast_transpose_f32_to_bf16_batched(dev_tab.data_ptr(), 3, max(tiles), S()), "batched")
    for i, (o, x) in enumerate(zip(outs, xs)):
        assert E.check_bits_nan(f"batched job {i}", o.get(), E.cast_ref(x).T.contiguous()) == 0
    assert L().cx_cast_transpose_f32_to_bf16_batched(None, 3, 6, S()) == ERR_ARG
    report("cx_cast_transpose_f32_to_bf16_batched", test="3 jobs", differing=0)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1027, (1 << 21) + 3075])
def test_cast_f32_to_bf16(n):
    x = E.cast_inputs(n, 70)
    X, O = slab(1, n, dtype=F32, data=x, name="In"), slab(1, n, name="Out")
    _C.check(L().cx_cast_f32_to_bf16(X.ptr, O.ptr, n, S()), "cast_f32_to_bf16")
    assert E.check_bits_nan(f"cast_f32_to_bf16 n={n}", O.get(), E.cast_ref(x)[None]) == 0
    report("cx_cast_f32_to_bf16", test=f"n={n}", differing=0)


@pytest.mark.parametrize("n", [1, 255, 257, (1 << 19) + 771])
def test_cast_bf16_to_f32(n):
    x = E.cast_ref(E.cast_inputs(n, 80))
    X, O = slab(1, n, data=x, name="In"), slab(1, n, dtype=F32, name="Out")
    _C.check(L().cx_cast_bf16_to_f32(X.ptr, O.ptr, n, S()), "cast_bf16_to_f32")
    assert E.check_bits_nan(f"cast_bf16_to_f32 n={n}", O.get(), x.float()[None]) == 0
    report("cx_cast_bf16_to_f32", test=f"n={n}", differing=0)


# ======================================================================================================== activations
@pytest.mark.parametrize("family", ["gauss", "sat"])
@pytest.mark.parametrize("T,I", E.ACT_SHAPES)
def test_activations(T, I, family):
    inp = E.act_inputs(T, I, family)
    y, g, d, pre, bias, act = (inp[k] for k in ("y", "g", "d", "pre", "bias", "act"))
    y64, g64, d64, act64 = R.d64(y, g, d, act)
    w = Worst()
    c = lambda form: E.C(family, form)                                          # noqa: E731
    fl = lambda form, v=None: E.act_floor(form, d=d64, y=y64, g=g64, v=v, act=act64)     # noqa: E731  (the fp32 underflow term)
    D = slab(T, I, data=d, name="dact")
    fwd_ref = R.f_swiglu(y64, g64)
    dy, tdy, dg, tdg = R.f_swiglu_bwd(d64, y64, g64)
    for layout in (0, 1):
        if layout == 1 and I % 32:
            continue
        join, split = (R.join_yg, R.split_yg) if layout else ((lambda a, b: torch.cat([a, b], 1)), (lambda t: (t[:, :I], t[:, I:])))
        YG, A, DYG = slab(T, 2 * I, data=join(y, g), name="yg"), slab(T, I, name="act"), slab(T, 2 * I, name="dyg")
        _C.check(L().cx_swiglu_fwd(YG.ptr, A.ptr, T, I, layout, S()), "swiglu_fwd")
        _C.check(L().cx_swiglu_bwd(D.ptr, YG.ptr, DYG.ptr, T, I, layout, S()), "swiglu_bwd")
        w.add("cx_swiglu_fwd", E.check_bf16(f"swiglu_fwd layout {layout}", A.get(), *fwd_ref, c("swiglu"), fl("swiglu")))
        gy, gg = split(DYG.get())
        w.add("cx_swiglu_bwd", E.check_bf16(f"swiglu_bwd layout {layout} dy", gy, dy, tdy, c("swiglu_bwd.dy"), fl("swiglu_bwd.dy")))
        w.add("cx_swiglu_bwd", E.check_bf16(f"swiglu_bwd layout {layout} dg", gg, dg, tdg, c("swiglu_bwd.dg"), fl("swiglu_bwd.dg")))
    if I % 32 == 0:
        ACT, G, DYG = slab(T, I, data=act, name="act in"), slab(T, I, data=g, name="gate"), slab(T, 2 * I, name="dyg ag")
        _C.check(L().cx_swiglu_bwd_gate(D.ptr, ACT.ptr, G.ptr, DYG.ptr, T, I, S()), "swiglu_bwd_gate")
        dy2, tdy2, dg2, tdg2 = E.f_swiglu_bwd_ag(d64, act64, g64)
        gy, gg = R.split_yg(DYG.get())
        w.add("cx_swiglu_bwd_gate", E.check_bf16("swiglu_bwd_gate dy", gy, dy2, tdy2, c("swiglu_bwd_ag.dy"), fl("swiglu_bwd_ag.dy")))
        w.add("cx_swiglu_bwd_gate", E.check_bf16("swiglu_bwd_gate dg", gg, dg2, tdg2, c("swiglu_bwd_ag.dg"), fl("swiglu_bwd_ag.dg")))
    PRE, B = slab(T, I, data=pre, name="pre"), slab(1, I, dtype=F32, data=bias, name="bias")
    for b, Bs in ((None, None), (bias, B)):
        v64 = E.pre_plus_bias(pre, b, F64)
        for a, form in E.ACT_FORM.items():
            O = slab(T, I, name=f"act {form}")
            _C.check(L().cx_bias_act_fwd(PRE.ptr, P(Bs), O.ptr, T, I, a, S()), "bias_act_fwd")
            w.add("cx_bias_act_fwd", E.check_bf16(f"bias_act_fwd {form} bias {b is not None}", O.get(), *R.f_act(v64, a), c(form), fl(form, v64)))
        O = slab(T, I, name="dpre")
        _C.check(L().cx_bias_gelu_bwd(D.ptr, PRE.ptr, P(Bs), O.ptr, T, I, S()), "bias_gelu_bwd")
        w.add("cx_bias_gelu_bwd", E.check_bf16(f"bias_gelu_bwd bias {b is not None}", O.get(), *R.f_act_bwd(d64, v64, 0), c("gelu_bwd"), fl("gelu_bwd", v64)))
    w.flush(f"activations {T}x{I} {family}")


def test_activation_rejections():
    A, Bq, O = slab(8, 64, name="a"), slab(8, 64, name="b"), slab(8, 128, name="o")
    lib = L()
    assert lib.cx_swiglu_fwd(O.ptr, A.ptr, 8, 12, 0, S()) == ERR_SHAPE
    assert lib.cx_swiglu_fwd(O.ptr, A.ptr, 8, 40, 1, S()) == ERR_SHAPE
    assert lib.cx_swiglu_bwd(A.ptr, O.ptr, O.ptr, 8, 12, 0, S()) == ERR_SHAPE
    assert lib.cx_swiglu_bwd(A.ptr, O.ptr, O.ptr, 8, 40, 1, S()) == ERR_SHAPE
    assert lib.cx_swiglu_bwd_gate(A.ptr, A.ptr, Bq.ptr, O.ptr, 8, 40, S()) == ERR_SHAPE
    assert lib.cx_swiglu_bwd_gate(A.ptr, None, Bq.ptr, O.ptr, 8, 32, S()) == ERR_ARG
    assert lib.cx_bias_act_fwd(A.ptr, None, Bq.ptr, 8, 12, 0, S()) == ERR_SHAPE
    assert lib.cx_bias_act_fwd(A.ptr, None, Bq.ptr, 8, 16, 2, S()) == ERR_ARG
    assert lib.cx_bias_gelu_bwd(A.ptr, A.ptr, None, Bq.ptr, 8, 12, S()) == ERR_SHAPE
    assert lib.cx_bias_act_bwd_colsum(A.ptr, A.ptr, None, Bq.ptr, None, 8, 12, 0, S()) == ERR_SHAPE
    assert lib.cx_bias_act_bwd_colsum(A.ptr, A.ptr, None, Bq.ptr, None, 8, 16, 2, S()) == ERR_ARG
    assert lib.cx_bias_act_bwd_colsum(A.ptr, None, None, Bq.ptr, None, 8, 16, 0, S()) == ERR_ARG
    assert lib.cx_bias_grad(A.ptr, O.ptr, 8, 12, 16, S()) == ERR_ALIGN
    assert lib.cx_bias_grad(A.ptr, O.ptr, 8, 16, 20, S()) == ERR_ALIGN
    # (nothing was launched: the slabs are as they were, which `_poison` checks)


# ======================================================================================================== column sums
COLSUM_CASES = [(T, N) for T in (1, 7, 17, 33, 256, 257, 1000) for N in (8, 264, 768)] + [(131073, 8)]


def _init(N, seed):
    return torch.randn(N, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("T,N", COLSUM_CASES)
def test_bias_grad(T, N):
    x, init = R.gauss_bf16(T, N, 90 + T % 97), _init(N, 91)
    X = slab(T, N, N + 8, data=x, name="dY")
    outs = []
    for _ in range(2):
        DB = slab(1, N, dtype=F32, data=init, name="dbias")
        _C.check(L().cx_bias_grad(X.ptr, DB.ptr, T, N, N + 8, S()), "bias_grad")
        outs.append(DB.get()[0])
    w = E.check_colsum(f"bias_grad {T}x{N}", outs[0], x, init)
    if T <= 256:
        assert E.colsum_grid(T, N) == 1
        assert R.check_bits("bias_grad: run 2 against run 1", outs[1][None], outs[0][None]) == 0
    else:
        assert E.check_colsum(f"bias_grad {T}x{N} run 2", outs[1], x, init) <= 1.0
    report("cx_bias_grad", test=f"{T}x{N}", worst_err_over_bound=w)


@pytest.mark.parametrize("T,N", COLSUM_CASES)
def test_bias_act_bwd_colsum(T, N):
    family = "sat" if N == 264 else "gauss"
    inp = E.act_inputs(T, N, family, seed=950)
    d, pre, bias = inp["d"], inp["pre"], inp["bias"]
    init = _init(N, 92)
    D, PRE, B = slab(T, N, data=d, name="dact"), slab(T, N, data=pre, name="pre"), slab(1, N, dtype=F32, data=bias, name="bias")
    w = Worst()
    for a, form in E.ACT_FORM.items():
        for b, Bs in ((None, None), (bias, B)):
            v64 = E.pre_plus_bias(pre, b, F64)
            ref, t = R.f_act_bwd(d.to(F64), v64, a)
            runs = []
            for _ in range(2 if T <= 256 else 1):
                DP, DB = slab(T, N, name="dpre"), slab(1, N, dtype=F32, data=init, name="dbias")
                _C.check(L().cx_bias_act_bwd_colsum(D.ptr, PRE.ptr, P(Bs), DP.ptr, DB.ptr, T, N, a, S()), "act_bwd_colsum")
                runs.append((DP.get(), DB.get()[0]))
            dp, db = runs[0]
            tag = f"act_bwd_colsum {T}x{N} {form} bias {b is not None}"
            w.add("cx_bias_act_bwd_colsum.dpre", E.check_bf16(f"{tag} dpre", dp, ref, t, E.C(family, form + "_bwd"), E.act_floor(form + "_bwd", d=d.to(F64), v=v64)))
            w.add("cx_bias_act_bwd_colsum.dbias", E.check_colsum(f"{tag} dbias", db, dp, init))     # sums what the next kernels read
            if T <= 256:
                assert R.check_bits(f"{tag}: dpre run 2", runs[1][0], dp) == 0 and R.check_bits(f"{tag}: dbias run 2", runs[1][1][None], db[None]) == 0
        # dbias = NULL still writes dpre
        DP = slab(T, N, name="dpre only")
        _C.check(L().cx_bias_act_bwd_colsum(D.ptr, PRE.ptr, B.ptr, DP.ptr, None, T, N, a, S()), "act_bwd_colsum no dbias")
        assert R.check_bits(f"act_bwd_colsum {form} dbias NULL", DP.get(), dp) == 0                  # the same bits as with a dbias
    w.flush(f"act_bwd_colsum {T}x{N}")


# ============================================================================================================ pooling
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", E.POOL_D)
def test_pool(d, mode, normalize):
    lens = E.POOL_LENS
    B, T = len(lens), sum(lens)
    cu = E.cu_of(lens).to(DEV)
    live = torch.tensor([l > 0 for l in lens])
    w = Worst()
    for zero_seq in (None, 3):
        h, demb = E.pool_inputs(lens, d, zero_seq=zero_seq)
        Hs, EMB, NRM = slab(T, d, data=h, name="h"), slab(B, d, dtype=F32, name="emb"), slab(1, B, dtype=F32, name="norm")
        _C.check(L().cx_pool_normalize_fwd(Hs.ptr, cu.data_ptr(), EMB.ptr, NRM.ptr, B, d, mode, normalize, S()), "pool fwd")
        emb, norm = EMB.get(), NRM.get()[0]
        remb, temb, rnorm, tnorm = E.pool_fwd_ref(h, lens, mode, normalize)
        tag = f"pool d={d} mode={mode} normalize={normalize} zero_seq={zero_seq}"
        if mode == 0:
            assert bool(torch.isnan(emb[1]).all()), f"{tag}: the empty sequence's mean is 0 / 0"
        else:
            assert bool((emb[1] == 0).all()) and float(norm[1]) == 0, f"{tag}: the empty sequence's cls row is 0"
        sel = live if mode == 0 else torch.ones_like(live)
        w.add("cx_pool_normalize_fwd.emb", E.check_f32(f"{tag} emb", emb[sel], remb[sel], temb[sel], E.C("pool", "emb")))
        w.add("cx_pool_normalize_fwd.norm", E.check_f32(f"{tag} norm", norm[sel, None], rnorm[sel, None], tnorm[sel, None], E.C("pool", "norm")))
        if zero_seq is not None:
            assert bool((emb[zero_seq] == 0).all()) and float(norm[zero_seq]) == 0, f"{tag}: the all-zero sequence"
        DE, DH = slab(B, d, dtype=F32, data=demb, name="demb"), slab(T, d, name="dh")
        _C.check(L().cx_pool_normalize_bwd(DE.ptr, EMB.ptr, NRM.ptr, cu.data_ptr(), DH.ptr, B, d, mode, normalize, S()), "pool bwd")
        dh, th = E.pool_bwd_ref(demb, torch.nan_to_num(emb), norm, lens, mode, normalize)      # from the STORED emb / norm
        w.add("cx_pool_normalize_bwd", E.check_bf16(f"{tag} dh", DH.get(), dh, th, E.C("pool", "dh")))
    w.flush(f"pool d={d} mode={mode} normalize={normalize}")


def test_pool_rejections():
    X, O = slab(4, 64, name="h"), slab(4, 64, dtype=F32, name="emb")
    cu = E.cu_of((2, 2)).to(DEV)
    for d in (4, 2056):
        assert L().cx_pool_normalize_fwd(X.ptr, cu.data_ptr(), O.ptr, O.ptr, 2, d, 0, 1, S()) == ERR_SHAPE
    assert L().cx_pool_normalize_bwd(O.ptr, O.ptr, O.ptr, cu.data_ptr(), X.ptr, 2, 2056, 0, 1, S()) == ERR_SHAPE
    assert L().cx_pool_normalize_bwd(O.ptr, O.ptr, O.ptr, cu.data_ptr(), X.ptr, 2, 12, 0, 1, S()) == ERR_SHAPE


# ============================================================================================================= rotary
ROT_LENS = (1, 33, 200, 0, 7)


def _tables(n):
    cos, sin = E.rotary_tables(n)
    return cos, sin, slab(n, 32, dtype=F32, data=cos, name="cos"), slab(n, 32, dtype=F32, data=sin, name="sin")


@pytest.mark.parametrize("H", [1, 12])
def test_rotary_qkv(H):
    lens = ROT_LENS
    T, B = sum(lens), len(lens)
    cu = E.cu_of(lens).to(DEV)
    cos, sin, COS, SIN = _tables(max(lens))                      # sized to the longest sequence: a read past it is poison
    x = R.gauss_bf16(T, 3 * H * 64, 120 + H)
    X = slab(T, 3 * H * 64, data=x, name="qkv")
    ref = x
    for sign in (1, -1):
        _C.check(L().cx_rotary_qkv_inplace(X.ptr, cu.data_ptr(), COS.ptr, SIN.ptr, B, H, T, max(lens), sign, S()), "rotary_qkv")
        ref = E.rotary_ref(ref, lens, H, 2, cos, sin, sign)
        assert R.check_bits(f"rotary_qkv H={H} sign={sign}", X.get(), ref) == 0            # v (the last third) untouched included
    assert torch.equal(bits(X.get()[:, 2 * H * 64:].contiguous()), bits(x[:, 2 * H * 64:].contiguous()))
    report("cx_rotary_qkv_inplace", test=f"H={H}", differing=0)


@pytest.mark.parametrize("max_seqlen", [200, 16])
@pytest.mark.parametrize("stride", ["H64", "3H64", "H64+8"])
def test_rotary_apply(stride, max_seqlen):
    H, lens = 2, ROT_LENS
    T, B = sum(lens), len(lens)
    tok = {"H64": H * 64, "3H64": 3 * H * 64, "H64+8": H * 64 + 8}[stride]
    cu = E.cu_of(lens).to(DEV)
    cos, sin, COS, SIN = _tables(max(lens))
    x = R.gauss_bf16(T, H * 64, 130)
    X = slab(T, H * 64, tok, data=x, name="x")                   # the gap between H 64 and the token stride must stay poison
    ref = x
    for sign in (1, -1):
        _C.check(L().cx_rotary_apply(X.ptr, tok, cu.data_ptr(), COS.ptr, SIN.ptr, B, H, T, max_seqlen, sign, S()), "rotary_apply")
        ref = E.rotary_ref(ref, lens, H, 1, cos, sin, sign)
        assert R.check_bits(f"rotary_apply stride={stride} max_seqlen={max_seqlen} sign={sign}", X.get(), ref) == 0
    assert L().cx_rotary_apply(X.ptr, H * 64 + 4, cu.data_ptr(), COS.ptr, SIN.ptr, B, H, T, max_seqlen, 1, S()) == ERR_ALIGN
    assert L().cx_rotary_apply(X.ptr, tok, cu.data_ptr(), None, SIN.ptr, B, H, T, max_seqlen, 1, S()) == ERR_ARG
    assert L().cx_rotary_apply(X.ptr, tok, None, COS.ptr, SIN.ptr, B, H, T, max_seqlen, 1, S()) == ERR_ARG
    assert R.check_bits("rotary_apply: a rejected call writes nothing", X.get(), ref) == 0
    report("cx_rotary_apply", test=f"stride={stride} max_seqlen={max_seqlen}", differing=0)


# ====================================================================================================== ViT front end
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,C,H,W,p", E.VIT_PATCHIFY)
def test_vit_patchify(B, C, H, W, p, dtype, gather):
    pix = E.cast_inputs(B * C * H * W, 140 + B).reshape(B, C, H, W)           # exact ties, +-0, inf and a NaN among the pixels
    if dtype == BF:
        pix = E.cast_ref(pix)
    keep = E.vit_keep(B) if gather else None
    rows = B * (keep.shape[1] if gather else E.VIT_P_ALL)
    X, O = slab(B * C * H, W, dtype=dtype, data=pix, name="pixels"), slab(rows, C * p * p, name="patches")
    kd = keep.to(DEV) if gather else None
    if gather:
        rc = L().cx_vit_patchify_gather(X.ptr, int(dtype == BF), O.ptr, B, C, H, W, p, kd.data_ptr(), keep.shape[1], S())
    else:
        rc = L().cx_vit_patchify(X.ptr, int(dtype == BF), O.ptr, B, C, H, W, p, S())
    _C.check(rc, "vit_patchify")
    assert E.check_bits_nan(f"patchify {B}x{C}x{H}x{W} p={p} gather={gather}", O.get(), E.patchify_ref(pix, p, keep)) == 0
    report("cx_vit_patchify_gather" if gather else "cx_vit_patchify", test=f"{H}x{W} p={p} {dtype}", differing=0)


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("B,P_all,d", E.VIT_ASSEMBLE)
def test_vit_assemble_fwd(B, P_all, d, gather):
    keep = E.vit_keep(B) if gather else None
    P = keep.shape[1] if gather else P_all
    proj = R.gauss_bf16(B * P, d, 150 + d)
    cls, pos = torch.randn(d, generator=E._gen(151)), torch.randn(P_all + 1, d, generator=E._gen(152))
    X, CLS, POS = slab(B * P, d, data=proj, name="proj"), slab(1, d, dtype=F32, data=cls, name="cls"), slab(P_all + 1, d, dtype=F32, data=pos, name="pos")
    O = slab(B * (P + 1), d, name="out")
    kd = keep.to(DEV) if gather else None
    if gather:
        rc = L().cx_vit_assemble_fwd_gather(X.ptr, CLS.ptr, POS.ptr, O.ptr, B, P, d, kd.data_ptr(), S())
    else:
        rc = L().cx_vit_assemble_fwd(X.ptr, CLS.ptr, POS.ptr, O.ptr, B, P, d, S())
    _C.check(rc, "vit_assemble_fwd")
    assert R.check_bits(f"assemble_fwd B={B} P={P} d={d} gather={gather}", O.get(), E.assemble_fwd_ref(proj, cls, pos, B, P, keep)) == 0
    report("cx_vit_assemble_fwd_gather" if gather else "cx_vit_assemble_fwd", test=f"B={B} d={d}", differing=0)


@pytest.mark.parametrize("mode", ["plain", "inv", "no_gpos", "no_gcls"])
@pytest.mark.parametrize("d", [24, 520])
def test_vit_assemble_bwd(d, mode):
    B, P_all = 3, E.VIT_P_ALL
    inv = None
    if mode == "inv":
        inv = E.vit_inv(E.vit_keep(B), P_all)
        inv[2, 1] = -1                      # image 2 loses slot 3 (patch 1): dproj row 2 K + 3 is never written and stays poison
    Pk = 4 if mode == "inv" else P_all   # patches per image in dz / dproj
    dz = E.vit_dz(B, Pk, d, 160 + d)
    gpos0, gcls0 = torch.randn(P_all + 1, d, generator=E._gen(161)), torch.randn(d, generator=E._gen(162))
    Z, DP = slab(B * (Pk + 1), d, data=dz, name="dz"), slab(B * Pk, d, name="dproj")
    GP = None if mode == "no_gpos" else slab(P_all + 1, d, dtype=F32, data=gpos0, name="gpos")
    GC = None if mode == "no_gcls" else slab(1, d, dtype=F32, data=gcls0, name="gcls")
    if inv is not None:
        iv = inv.to(DEV)
        rc = L().cx_vit_assemble_bwd_gather(Z.ptr, DP.ptr, P(GC), P(GP), B, Pk, d, iv.data_ptr(), P_all, S())
    else:
        rc = L().cx_vit_assemble_bwd(Z.ptr, DP.ptr, P(GC), P(GP), B, Pk, d, S())
    _C.check(rc, "vit_assemble_bwd")
    dproj, gpos, gcls = E.assemble_bwd_ref(dz, B, Pk, gpos0, gcls0, torch.zeros(B * Pk, d, dtype=BF), inv)
    got = DP.get()
    if inv is not None:                     # the row nothing maps to: still the slab's poison
        hole = 2 * Pk + 3
        assert bool(torch.isnan(got[hole]).all())
        got[hole] = 0.0
    assert R.check_bits(f"assemble_bwd dproj d={d} {mode}", got, dproj) == 0
    if GP is not None:
        assert R.check_bits(f"assemble_bwd gpos d={d} {mode}", GP.get(), gpos) == 0
        if inv is not None:
            assert R.check_bits("gpos of the patch no image kept", GP.get()[5:6], gpos0[5:6]) == 0
    if GC is not None:
        assert R.check_bits(f"assemble_bwd gcls d={d} {mode}", GC.get(), gcls[None]) == 0
    report("cx_vit_assemble_bwd_gather" if inv is not None else "cx_vit_assemble_bwd", test=f"d={d} {mode}", differing=0)
