"""Exact references of the bf16 GEMM family (contrastors_amd/csrc/gemm_api.hip, gemm_bf16_v5/v6/v7.hip, gemm_splitk_small.inc), the
seeded inputs of its edge tests, the poisoned strided buffers they run in and the checkers they share.  Plain torch, any device:
tests/test_gemm_ref_cpu.py proves this file against an fp32 emulation and planted errors, tests/test_gemm_edges_gpu.py holds the
kernels to it.

The idea.  Operands are bf16 SMALL INTEGERS (times one power of two for the nonlinear forms): every product and every partial sum
is exactly representable in fp32 whatever the summation order, the K split or the MFMA's internal adder, so a linear form has ONE
correct answer -- an fp32 output equals the exact product bit for bit, a bf16 output equals its round-to-nearest-even rounding at
each rounding point of the entry point, bit for bit.  No tolerance.  Each fp32 step a kernel does once (one multiply by alpha, one
bias add, one residual add) is exact on these inputs as well (`_f32_exact` asserts it), so neither its order nor an FMA contraction
can change the result: the restatement below is the only value a correct kernel can produce.

Rounding points (gemm_api.hip and the epilogues):
    cx_gemm_bf16_nt            out_mode 0: bf16(acc * alpha + bias)        out_mode 1: fp32(acc * alpha + bias)
    cx_gemm_bf16_nt_residual   bf16(bf16(acc + bias) + residual)
    cx_gemm_bf16_nt_splitk     bf16(bf16(sum of the slabs + bias) + residual), bias and residual folded in after the fixed-order sum
    cx_gemm_bf16_nt_accum      Out += acc          cx_gemm_bf16_tn_accum   G += dY^T A          (fp32)
    cx_gemm_bf16_swiglu        YG = bf16(acc) interleaved by 32, Act = bf16(g * y * sigmoid(g)) on the ROUNDED y, g
    cx_gemm_bf16_swiglu_gate   G = bf16(acc_gate), Act as above
    cx_gemm_bf16_bias_act      Pre = bf16(acc + bias), Act = bf16(act(Pre)) on the ROUNDED Pre
    cx_gemm_bf16_act_bwd       dPre = bf16(bf16(acc) * act'(Pre)), dbias += column sums of the bf16 dPre
    cx_gemm_bf16_swiglu_bwd    d = acc (fp32, not rounded); dy = bf16(g s d), dg = bf16((s + g s (1 - s)) d y), s = sigmoid(g)
    cx_gemm_bf16_swiglu_bwd_gate   dy as above, dg = bf16(d act (1 / g + 1 - s))

Nonlinear results are checked per element against the fp64 formula on the exact rounded inputs under
    |got - ref| <= 1 ulp_bf16(ref) + C * 2^-24 * T,      T = sum of the absolute values of the formula's terms,
C = 4 * C_MEAS[form]; C_MEAS is the worst |fp32 torch evaluation - fp64| / (2^-24 T) of the same formula on the tests' own inputs
(test_gemm_ref_cpu.py measures and asserts it, never against a kernel); the factor 4 covers the GPU's approximate exp and reciprocal
(1 ulp each) and the A&S 7.1.26 erf (|error| <= 1.5e-7 = 2.5 * 2^-24).
"""
from __future__ import annotations

import math

import torch

from tests.ln_ref import RowMismatch, bf16_ulp, bits, check_rows

EPS24 = 2.0 ** -24
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
POISON = {2: 0x7FA5, 4: 0x7FA5A5A5}     # a NaN in bf16 and in fp32 (tests/test_layernorm_edges_gpu.py uses the same patterns)
GUARD = 8                               # poisoned rows before and after every buffer
ALPHAS = (0.5, -2.0)

# worst |fp32 evaluation - fp64| / (2^-24 T) per nonlinear form (test_gemm_ref_cpu.py::test_measured_constants), rounded up
C_MEAS = {
    "swiglu": 3.0, "swiglu_bwd.dy": 3.5, "swiglu_bwd.dg": 10.5, "swiglu_bwd_ag.dg": 3.0,
    "gelu": 1.7, "qgelu": 14.0, "gelu_bwd": 2.5, "qgelu_bwd": 12.0,
}
C_FACTOR = 4.0


def C(form: str) -> float:
    return C_FACTOR * C_MEAS[form]


# ----------------------------------------------------------------------------------------------------------- inputs
TARGET_SD = 2000.0


def amp(K: int) -> int:
    """Largest |integer| of the operands at this K: 27 at K = 64 down to 8 at K = 6144, never more than 32.  A deliberate departure
    from one fixed range [-32, 32] for every K: the standard deviation of a sum of K products, A (A + 1) / 3 * sqrt(K), is held near
    2000, so sums of 2^9 .. 2^13 need 10 .. 14 significant bits (most are not bf16 values) and 7 .. 16 % of them sit exactly
    half-way between two bf16 values (ulp 4 .. 64).  At amplitude 32 and K = 6144 the sums reach 2^15 (ulp 256) and fewer than 1 % are
    ties, which test_gemm_ref_cpu.py::test_inputs_are_sharp would refuse."""
    return max(2, min(32, int(math.sqrt(3.0 * TARGET_SD / math.sqrt(K)))))


def acc_sd(K: int) -> float:
    a = amp(K)
    return a * (a + 1) / 3.0 * math.sqrt(K)


def w_scale(K: int) -> float:
    """Power of two that brings the standard deviation of the pre-activations into [2, 4)."""
    return 2.0 ** -(math.floor(math.log2(acc_sd(K))) - 1)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(rows, cols, seed, a=32):
    """(rows, cols) bf16 integers, uniform in [-a, a]; on the CPU."""
    return torch.randint(-a, a + 1, (rows, cols), generator=_gen(seed)).to(BF)


def operands(M, N, K, seed, scaled=False):
    """x (M, K), w (N, K): bf16 integers in [-amp(K), amp(K)]; scaled: w times w_scale(K) (exact)."""
    a = amp(K)
    x, w = ints(M, K, seed, a), ints(N, K, seed + 1, a)
    if scaled:
        w = (w.float() * w_scale(K)).to(BF)
    return x, w


def bias_vec(N, seed, kmax=256):
    """fp32 [N], non-zero multiples of 0.25 up to kmax / 4 in magnitude: half of the columns whole numbers (they keep the exact
    ties of an integer sum), half with a fractional part."""
    g = _gen(seed)
    k = torch.randint(1, kmax + 1, (N,), generator=g)
    whole = torch.rand(N, generator=g) < 0.5
    k = torch.where(whole, (k + 3) // 4 * 4, k)
    sign = torch.randint(0, 2, (N,), generator=g) * 2 - 1
    return (k * sign).float() * 0.25


def residual(M, N, seed):
    return ints(M, N, seed, 32)


def gauss_bf16(rows, cols, seed, std=1.0, nonzero=False):
    t = (torch.randn(rows, cols, generator=_gen(seed)) * std).to(BF)
    if nonzero:
        t = torch.where(t == 0, torch.full_like(t, 0.5), t)
    return t


def interleave32(a, b):
    """Rows (or, for 2-D activations, columns via .T) of a and b interleaved in groups of 32: [a 0..31 | b 0..31 | a 32..63 | ...]."""
    n = a.shape[0]
    return torch.stack([a.reshape(n // 32, 32, -1), b.reshape(n // 32, 32, -1)], 1).reshape(2 * n, -1).contiguous()


def join_yg(y, g):
    """(M, I) y and gate -> (M, 2I) in the interleaved-by-32 column layout."""
    M = y.shape[0]
    return torch.stack([y.reshape(M, -1, 32), g.reshape(M, -1, 32)], 2).reshape(M, -1).contiguous()


def split_yg(t):
    M = t.shape[0]
    v = t.reshape(M, -1, 2, 32)
    return v[:, :, 0].reshape(M, -1), v[:, :, 1].reshape(M, -1)


# ------------------------------------------------------------------------------------------------- exact restatements
class NotExact(AssertionError):
    pass


def _f32_exact(v64, what):
    """fp64 -> fp32, asserting that nothing is rounded: the fp32 step it stands for has one possible result."""
    v32 = v64.to(F32)
    if not bool((v32.to(F64) == v64).all()):
        raise NotExact(f"{what}: not exactly representable in fp32 -- the inputs are not of the exact family")
    return v32


def acc_exact(x, w):
    """X W^T of bf16 integer (times power-of-two) operands: exact in fp64 (|sum| < 2^53) and asserted exact in fp32."""
    return x.to(F64) @ w.to(F64).T


def nt_ref(x, w, bias=None, alpha=1.0, out_mode=0, res=None, acc=None):
    """cx_gemm_bf16_nt / _nt_residual / _nt_splitk.  fp32 steps: acc * alpha, + bias (each exact), one bf16 rounding, then
    bf16(fp32(that) + fp32(residual))."""
    acc = acc_exact(x, w) if acc is None else acc
    _f32_exact(acc, "acc")
    v = _f32_exact(acc * float(alpha), "acc * alpha")
    if bias is not None:
        v = _f32_exact(v.to(F64) + bias.to(F64), "acc * alpha + bias")
    if out_mode == 1:
        return v
    o = v.to(BF)
    if res is not None:
        o = (o.float() + res.float()).to(BF)     # one fp32 add of two bf16 values: exact, then rounded once
    return o


def accum_ref(out0, x, w, times=1):
    """cx_gemm_bf16_nt_accum called `times` times on Out = out0."""
    acc = acc_exact(x, w)
    out = out0.to(F64)
    for _ in range(times):
        out = _f32_exact(out + acc, "Out + acc").to(F64)
    return out.to(F32)


def tn_ref(g0, dy, a, times=1):
    """cx_gemm_bf16_tn_accum: G += dY^T A."""
    acc = dy.to(F64).T @ a.to(F64)
    out = g0.to(F64)
    for _ in range(times):
        out = _f32_exact(out + acc, "G + acc").to(F64)
    return out.to(F32)


def linear_bf16(x, w, bias=None):
    """bf16(acc + bias): the saved linear tensors (YG, G, Pre) and the bf16 d(act) of cx_gemm_bf16_act_bwd."""
    return nt_ref(x, w, bias)


# ------------------------------------------------------------------------------- nonlinear formulas (dtype-generic)
def _sig(g):
    return 1.0 / (1.0 + torch.exp(-g))


def f_swiglu(y, g):
    r = g * y * _sig(g)
    return r, r.abs()


def f_swiglu_bwd(d, y, g):
    """-> (dy, T_dy, dg, T_dg) from the saved (y, gate) pair."""
    s = _sig(g)
    dy = g * s * d
    t1, t2 = s * d * y, g * s * (1.0 - s) * d * y
    return dy, dy.abs(), t1 + t2, t1.abs() + t2.abs()


def f_swiglu_bwd_ag(d, act, g):
    """-> (dy, T_dy, dg, T_dg) from the saved (act, gate) pair: dg = d act (1 / g + 1 - s)."""
    s = _sig(g)
    dy = g * s * d
    da = d * act
    t1, t2, t3 = da / g, da, da * s
    return dy, dy.abs(), t1 + t2 - t3, t1.abs() + t2.abs() + t3.abs()


def f_act(v, act):
    if act == 1:
        r = v * _sig(1.702 * v)
        return r, r.abs()
    e = torch.erf(v * 0.7071067811865476)
    t1, t2 = 0.5 * v, 0.5 * v * e
    return t1 + t2, t1.abs() + t2.abs()


def f_act_grad(v, act):
    if act == 1:
        s = _sig(1.702 * v)
        t1, t2 = s, 1.702 * v * s * (1.0 - s)
        return t1 + t2, t1.abs() + t2.abs()
    e = torch.erf(v * 0.7071067811865476)
    t3 = v * 0.3989422804014327 * torch.exp(-0.5 * v * v)
    return 0.5 + 0.5 * e + t3, 0.5 + 0.5 * e.abs() + t3.abs()


def f_act_bwd(d, pre, act):
    gr, t = f_act_grad(pre, act)
    return d * gr, d.abs() * t


def d64(*ts):
    return tuple(t.to(F64) for t in ts)


def meas_ratio(ref64, t64, emu32):
    """C_meas of one evaluation: worst |fp32 - fp64| / (2^-24 T) (0 where T is 0 and the two agree)."""
    err = (emu32.to(F64) - ref64).abs()
    r = torch.where(t64 > 0, err / (EPS24 * t64).clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------- checkers
class BitMismatch(AssertionError):
    pass


def check_bits(name, got, ref):
    """Bit-for-bit equality of two tensors of one dtype and shape.  Raises BitMismatch naming the first differing (row, column);
    returns the number of differing elements (0)."""
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, ref.dtype, tuple(got.shape), tuple(ref.shape))
    g2, r2 = got.reshape(got.shape[0], -1) if got.ndim > 1 else got.reshape(1, -1), ref.reshape(ref.shape[0], -1) if ref.ndim > 1 else ref.reshape(1, -1)
    bad = bits(g2.contiguous()) != bits(r2.contiguous())
    n = int(bad.sum())
    if n:
        flat = int(torch.nonzero(bad.reshape(-1))[0])
        r, c = divmod(flat, g2.shape[1])
        raise BitMismatch(f"{name}: {n} of {bad.numel()} elements differ in {int(bad.any(1).sum())} rows; first at (row {r}, column {c}): "
                          f"got {float(g2[r, c])!r}, exact {float(r2[r, c])!r}")
    return 0


def bound_nonlinear(ref64, t64, c):
    ulp = torch.where(ref64 == 0, torch.zeros_like(ref64), bf16_ulp(ref64))
    return ulp + c * EPS24 * t64


def check_nonlinear(name, got, ref64, t64, form):
    """bf16 result of a nonlinear epilogue, per element: |got - ref| <= 1 ulp_bf16(ref) + C 2^-24 T.  Returns the worst err / bound."""
    return check_rows(name, got, ref64, bound_nonlinear(ref64, t64, C(form)))


def check_dbias(name, got, init, dpre_stored, M):
    """fp32 [N] column sums against init + the fp64 sum of the STORED bf16 dPre, per column under
        (M + 4) 2^-23 (sum_rows |dPre| + |init|).
    Derivation: one rounding per addition, at the unit roundoff 2^-23 of a truncating adder, along a chain of at most M + 4 additions
    (up to 128 rows per partial, ceil(M / 128) partials folded four ways, the final dst += sum); each rounding is relative to a
    partial sum no larger than sum|dPre| -- except the LAST one, dst = init + sum, which rounds at the magnitude of the result and so
    at up to ulp(|init| + sum|dPre|).  The |init| term is therefore needed (and wider than (M + 4) 2^-23 sum|dPre| alone): at M = 1
    with |dPre| << |init| that narrower bound is below half an ulp of the stored result, which no fp32 kernel can meet."""
    s = dpre_stored.to(F64)
    ref = init.to(F64) + s.sum(0)
    return check_rows(name, got, ref, (M + 4) * 2.0 ** -23 * (s.abs().sum(0) + init.to(F64).abs()))


def check_gauss_f32(name, got, x, w, bias, alpha=1.0):
    """fp32 output on Gaussian operands, per element: |err| <= (K + 2) 2^-23 (sum_k |x_k w_k| |alpha| + |bias|) -- one rounding per
    addition at the unit roundoff of a truncating adder, plus the alpha and bias steps."""
    K = x.shape[1]
    ref = x.to(F64) @ w.to(F64).T * alpha
    mag = x.to(F64).abs() @ w.to(F64).abs().T * abs(alpha)
    if bias is not None:
        ref, mag = ref + bias.to(F64), mag + bias.to(F64).abs()
    return check_rows(name, got, ref, (K + 2) * 2.0 ** -23 * mag)


# --------------------------------------------------------------------------------------------------- poisoned buffers
class Buf:
    """A (rows, cols) operand, result or workspace with leading dimension `ld` inside a larger allocation: GUARD rows of `ld`
    elements before and after it and the columns cols .. ld of every row hold a NaN bit pattern.  `data` fills the payload;
    without it the payload is poison as well (results and workspaces start as NaN: an element the kernel skips stays NaN).
    intact(): every element outside the payload still holds the poison, bit for bit."""

    def __init__(self, rows, cols, ld=None, dtype=BF, device="cpu", data=None, name=""):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.name = rows, cols, ld, name
        self.full = torch.empty((rows + 2 * GUARD) * ld, dtype=dtype, device=device)
        self.poison = POISON[self.full.element_size()]
        bits(self.full).fill_(self.poison)
        self.t = self.full.view(rows + 2 * GUARD, ld)[GUARD:GUARD + rows, :cols]
        if data is not None:
            assert tuple(data.shape) in ((rows, cols), (cols,)), (name, tuple(data.shape), rows, cols)
            self.t.copy_(data.to(device=device, dtype=dtype).reshape(-1, cols))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        """The payload as a contiguous tensor."""
        return self.t.contiguous()

    def intact(self):
        b = bits(self.full).view(self.rows + 2 * GUARD, self.ld).clone()
        b[GUARD:GUARD + self.rows, :self.cols] = self.poison
        return bool((b == self.poison).all())


def check_poison(bufs):
    """Every buffer's guard rows and pad columns still hold the poison.  Raises naming the buffers that do not."""
    bad = [b.name for b in bufs if b is not None and not b.intact()]
    assert not bad, f"memory outside [0:M, 0:N] of {bad} was written"


# ---------------------------------------------------------------------------------------------- sharpness of the inputs
def sharpness(v64):
    """Of the exact values about to be rounded to bf16: (share that is not a bf16 value, share that is an exact tie)."""
    q = bf16_ulp(v64)
    f = v64 / q                                  # exact: q is a power of two
    frac = f - torch.floor(f)
    return float((frac != 0).double().mean()), float((frac == 0.5).double().mean())


# K values the GPU cases use, per bf16-output family (tests/test_gemm_edges_gpu.py draws its operands through operands() above)
K_PLAIN = (64, 128, 192, 256, 320, 384, 448)
K_SPLITK = (1536, 1600, 6144)
K_FUSED = (128,)

# the shapes of the nonlinear cases (section f of the GPU file): (M, width, K); C_MEAS is measured on exactly these
NONLINEAR_M = (1, 127, 128, 129, 255, 257)
SWIGLU_I = (32, 96, 160, 256)
ACT_N = (8, 136, 264)
BWD_I = (256, 512)
ACT_BWD_M = (1, 127, 129, 257)


def swiglu_case(M, I, K, seed=500):
    """x, the interleaved fc1 weight (scaled), and the exact rounded y, gate (M, I) it produces."""
    a = amp(K)
    x = ints(M, K, seed + I, a)
    wy = (ints(I, K, seed + I + 1, a).float() * w_scale(K)).to(BF)
    wg = (ints(I, K, seed + I + 2, a).float() * w_scale(K)).to(BF)
    return x, interleave32(wy, wg), wy, wg


def act_case(M, N, K, seed=600):
    x, w = operands(M, N, K, seed + N, scaled=True)
    return x, w, bias_vec(N, seed + N + 2, kmax=8)


def act_bwd_case(M, N, K, seed=700):
    dy, w = operands(M, N, K, seed + N, scaled=True)
    return dy, w, gauss_bf16(M, N, seed + N + 2, std=2.0)


def swiglu_bwd_case(M, I, K, seed=800):
    """dY, W (scaled), and the saved tensors: y, gate (no gate exactly 0), act = bf16(y silu(gate))."""
    dy, w = operands(M, I, K, seed + I, scaled=True)
    y, g = gauss_bf16(M, I, seed + I + 2), gauss_bf16(M, I, seed + I + 3, std=2.0, nonzero=True)
    act = (g.float() * y.float() * torch.sigmoid(g.float())).to(BF)
    return dy, w, y, g, act
