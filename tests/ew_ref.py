"""fp64 and bit-exact references of the HBM-bound glue kernels (contrastors_amd/csrc/elementwise.hip, xent.hip, optimizer.hip, the
front end of vit.hip), the seeded inputs of their edge tests, fp32 emulations of the kernels' own formulas, poisoned slabs and the checkers they share.
Plain torch, any device: tests/test_ew_ref_cpu.py proves this file against fp64 autograd, measures the constants below and plants
errors; tests/test_elementwise_edges_gpu.py and tests/test_xent_optimizer_edges_gpu.py hold the kernels to it.  What exists is reused:
bf16_ulp / bf16_round / bits / check_rows (tests/ln_ref.py), the activation formulas, layouts, check_bits, check_poison and meas_ratio
(tests/gemm_ref.py), rotate_bf16 / rotary_tables (tests/attn_ref.py).

Bit-exact operations (no tolerance): cx_transpose_bf16, cx_transpose_f32, cx_cast_bf16_to_f32, cx_cast_f32_to_bf16,
cx_cast_transpose_f32_to_bf16 and its batched form, cx_rotary_qkv_inplace and cx_rotary_apply, and the three front-end kernels of
vit.hip (they move data, do at most one fp32 add per element or a short fp32 sum in a fixed order, and round to bf16 once).  The cast reference is torch's CPU
`.to(torch.bfloat16)` (round to nearest, ties to even); cast_inputs() holds exact ties of both parities, the two fp32 neighbours of a
tie, +-0, +-inf, NaN (compared with isnan, not by payload) and +-float32 max (rounds to inf).  It holds NO fp32 subnormals: the
denormal mode of the hardware conversion is not a contract of this project.

Bounds of everything else, per element against the fp64 value `ref` and its magnitude scale T (the sum of the absolute values of the
terms the element is built from, returned by every reference next to the value):
    bf16 result:  |got - ref| <= 1 ulp_bf16(ref) + C 2^-24 T          fp32 result:  |got - ref| <= C 2^-24 T
C = 4 C_MEAS[family][form].  C_MEAS is the worst |emulation - ref| / (2^-24 T) of an fp32 torch emulation of the kernel's own formula
(the emu_* functions below: exp2 of the argument times log2 e, the reciprocal, the A&S 7.1.26 erf polynomial, the kernels' summation
order where it is long) on exactly the inputs the tests use, measured and asserted by test_ew_ref_cpu.py::test_measured_constants,
never against a kernel.  The factor 4 is the project's stated margin: the two 1-ulp hardware approximations v_exp_f32 and v_rcp_f32
(cx_common.h: sigmoid_fast), the erf polynomial's 1.5e-7 and FMA contraction.  The saturation family (exact 0, +- the smallest bf16
normal, +-2^-20, +-8, +-20, +-50, +-100 as gate or pre-activation) has its own row: its constants are larger than the Gaussian ones
because T holds no term for the fp32 rounding of the exponent's argument log2(e) g, which reaches sigmoid(g) times |g| where the
exponential dominates (g = -50: about 50 2^-24 relative); at +-100 exp2 over- and underflows, the reciprocal sees inf, and the result
is 0 or the identity.

Underflow.  Both bounds are relative to T and so presuppose fp32 NORMAL intermediates.  Where a sigmoid, Gaussian or exponential is
below 2^-126 the hardware instructions return 0 (and gradual underflow would leave a few bits): the bound then also carries the
absolute term 2^-126 times the factor that value multiplies -- act_floor() for the activations (~1e-36), xent_floor() for dlogits -- and
ag_floor() for the subnormal product d * act at a gate of +-2^-126.  None of them is visible next to a result in the normal range.

xent uses __expf / __logf.  exp(a) is evaluated as exp2(a log2 e): the argument a = z - m carries one fp32 rounding of the subtraction
and one of the product, 2 |a| 2^-24 absolute in the exponent together, i.e. 2 |a| 2^-24 RELATIVE in exp(a), before the instruction's own
ulp.  With p_j = exp(z_j - lse) that is sum_j p_j |z_j - m| 2^-24-units of relative error in the sum of exponentials (the arguments
of the online rescalings of one element are all <= 0 and add up to z_j - m), and the same absolute error in lse = m + log S.  The
term is part of T (xent_ref: `targ`), C is not widened for it:
    T_lse = |m| + |log S| + 1 + sum_j p_j |z_j - m|        T_loss = T_lse + |z_label|
    T_dlogit_j = |g| (p_j (1 + |z_j - lse|) + [j = label]),   g = dloss * logit_scale.
The bound of dlogits also carries |g| 2^-126 (xent_floor): an exponential below the smallest fp32 normal has no relative accuracy.
The backward reference is formed from the STORED fp32 lse the kernel is fed; the bound carries the extra term
|d dlogit_j / d lse| |lse_stored - lse_ref| = |g| p_j |lse_stored - lse_ref| that storing lse in fp32 introduces.

Derived bounds (nothing measured):
    column sums (cx_bias_grad, the dbias of cx_bias_act_bwd_colsum): (chain + 4) 2^-23 (sum_rows |term| + |init|), the derivation of
        gemm_ref.check_dbias with the chain of colsum_kernel: ceil(T / (8 gy)) additions per lane, 8 across the row lanes, gy atomics.
        The dbias of the fused kernel is held to the fp64 sum of the bf16 dpre THE KERNEL RETURNED ("sums what the next kernels read").
    cx_grad_sq_norm: relative error <= (4 k + 4) 2^-24, k = ceil(ceil(n / 4) / (blocks 256)) float4 per lane (four squares and four
        additions each, every term >= 0); from there on the accumulation is in double.
"""
from __future__ import annotations

import math

import torch

from tests import gemm_ref as R
from tests.attn_ref import rotary_tables, rotate_bf16  # noqa: F401  (re-exported: the rotary reference and its tables)
from tests.gemm_ref import BF, EPS24, F32, F64
from tests.ln_ref import bf16_ulp, bits, check_rows

LOG2E = 1.4426950408889634
I64 = torch.int64

# worst |fp32 emulation - fp64| / (2^-24 T) per family and form (test_ew_ref_cpu.py::test_measured_constants), rounded up
C_MEAS = {
    "gauss": {"swiglu": 8.5, "swiglu_bwd.dy": 8.5, "swiglu_bwd.dg": 8.0, "swiglu_bwd_ag.dy": 8.5, "swiglu_bwd_ag.dg": 2.4,
              "gelu": 9.5, "qgelu": 19.0, "gelu_bwd": 9.5, "qgelu_bwd": 16.0},
    "sat": {"swiglu": 22.0, "swiglu_bwd.dy": 22.0, "swiglu_bwd.dg": 22.0, "swiglu_bwd_ag.dy": 22.0, "swiglu_bwd_ag.dg": 1.3,
            "gelu": 9.5, "qgelu": 54.0, "gelu_bwd": 10.0, "qgelu_bwd": 51.0},
    "pool": {"emb": 1.2, "norm": 0.75, "dh": 3.0},
    "xent": {"lse": 1.1, "loss": 1.1, "dlogits": 1.2},
    "opt": {"p": 2.4, "m": 2.1, "v": 3.0, "ema": 1.9},
}
C_FACTOR = 4.0


def C(family: str, form: str) -> float:
    return C_FACTOR * C_MEAS[family][form]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32c(v):
    """A Python number as the fp32 value a kernel receives it as."""
    return torch.tensor(v, dtype=F32)


# ====================================================================================================== poisoned slabs
class Slab:
    """A (rows, cols) payload with leading dimension `ld`, `lead` elements into an allocation whose every other element -- `guard`
    elements before and after, the lead, the columns cols .. ld of every row -- holds a NaN bit pattern (gemm_ref.POISON).  Without
    `data` the payload is poison too: an element a kernel skips stays NaN.  rows = 1 is a flat buffer; lead = 1 a misaligned base
    pointer.  The guard is 8 rows' worth, at most 65536 elements (a flat 16 MB buffer does not need 128 MB either side)."""

    def __init__(self, rows, cols, ld=None, dtype=BF, device="cpu", data=None, lead=0, name=""):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.lead, self.name = rows, cols, ld, lead, name
        self.guard = (min(R.GUARD * ld, 1 << 16) + 63) // 64 * 64          # a multiple of 64 elements: the payload stays 16-B aligned
        self.full = torch.empty(2 * self.guard + lead + rows * ld, dtype=dtype, device=device)
        self.poison = R.POISON[self.full.element_size()]
        bits(self.full).fill_(self.poison)
        self.t = self.full.as_strided((rows, cols), (ld, 1), self.guard + lead)
        if data is not None:
            assert data.numel() == rows * cols, (name, tuple(data.shape), rows, cols)
            self.t.copy_(data.to(device=device, dtype=dtype).reshape(rows, cols))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        """The payload as a contiguous CPU tensor."""
        return self.t.contiguous().cpu()

    def intact(self):
        b = bits(self.full).clone()
        b.as_strided((self.rows, self.cols), (self.ld, 1), self.guard + self.lead).fill_(self.poison)
        return bool((b == self.poison).all())


# ====================================================================================== bit-exact references and inputs
F32_MAX_BITS = 0x7F7FFFFF
_SPECIAL_BITS = (0x00000000, -0x80000000, 0x7F800000, -0x00800000, 0x7FC00000, F32_MAX_BITS, F32_MAX_BITS - (1 << 31))
_SPECIAL_AT = (3, 4, 5, 6, 7, 11, 12)     # +0, -0, +inf, -inf, NaN, +max, -max: positions that are none of the tie kinds below


def cast_inputs(n, seed=1):
    """fp32 [n] for the cast kernels: random sign, exponent field in [97, 157] (2^-30 .. 2^30: no subnormals, nothing near overflow)
    and mantissa; of every 8 elements the first is an EXACT bf16 tie (low 16 bits 0x8000, bit 16 -- the parity of the bf16 value below
    it -- random), the second and third its two fp32 neighbours (0x8001, 0x7fff); seven special values at fixed small positions."""
    g = _gen(seed)
    sign = torch.randint(0, 2, (n,), generator=g, dtype=I64) << 31
    expo = torch.randint(97, 158, (n,), generator=g, dtype=I64) << 23
    b = sign | expo | torch.randint(0, 1 << 23, (n,), generator=g, dtype=I64)
    kind = torch.arange(n) % 8
    for k, low in ((0, 0x8000), (1, 0x8001), (2, 0x7FFF)):
        b = torch.where(kind == k, (b & ~0xFFFF) | low, b)
    b = torch.where(b >= (1 << 31), b - (1 << 32), b)
    for pos, sb in zip(_SPECIAL_AT, _SPECIAL_BITS):
        if pos < n:
            b[pos] = sb
    return b.to(torch.int32).view(F32)


def cast_ref(x32):
    """The cast reference: torch's CPU conversion."""
    return x32.cpu().to(BF)


def is_tie(x32):
    return (bits(x32.contiguous()) & 0xFFFF) == 0x8000


def check_bits_nan(name, got, ref):
    """check_bits where a NaN of the reference asks for a NaN, whatever its payload."""
    gn, rn = torch.isnan(got), torch.isnan(ref)
    if not bool((gn == rn).all()):
        i = int(torch.nonzero((gn != rn).reshape(-1))[0])
        r, c = divmod(i, got.shape[-1]) if got.ndim > 1 else (0, i)
        raise R.BitMismatch(f"{name}: NaN expected and not found, or found and not expected, first at (row {r}, column {c})")
    z = torch.zeros((), dtype=got.dtype)
    return R.check_bits(name, torch.where(gn, z, got), torch.where(rn, z, ref))


def transpose_ref(x, rows_pad=None):
    """(rows, cols) -> (cols, rows_pad): the transpose, rows .. rows_pad zero-filled (cx_transpose_bf16's token padding)."""
    rows, cols = x.shape
    out = torch.zeros(cols, rows if rows_pad is None else rows_pad, dtype=x.dtype)
    out[:, :rows] = x.T
    return out


def rotate_f32(u, cos, sin):
    """rotary_pair before the bf16 rounding, restated independently of attn_ref.rotate_bf16: the second product rounded to fp32 by
    itself, the first fused into the sum (formed exactly in fp64: a 24-bit by 8-bit product and a 24-bit addend), one fp32 rounding."""
    l = u.shape[0]
    x1, x2 = u[..., :32].to(F64), u[..., 32:].to(F64)
    c, s = cos[:l, None, :].to(F32), sin[:l, None, :].to(F32)
    p2a, p2b = (x2.to(F32) * s).to(F64), (x1.to(F32) * s).to(F64)
    return torch.cat([(x1 * c.to(F64) - p2a).to(F32), (x2 * c.to(F64) + p2b).to(F32)], -1)


def rotary_ref(x, lens, H, nwhich, cos, sin, sign):
    """The in-place rotary of cx_rotary_qkv_inplace (nwhich = 2: q and k of (T, 3, H, 64)) / cx_rotary_apply (nwhich = 1) on the
    payload x (T, width >= nwhich H 64) holding bf16 values: position = index inside the sequence; columns past nwhich H 64 (v, or a
    stride gap's payload) untouched.  sign = -1 rotates back (sin negated: exact).  Returns bf16 (T, width)."""
    out = x.clone()
    t0 = 0
    sn = sin if sign >= 0 else -sin
    for l in lens:
        if l:
            for w in range(nwhich):
                u = x[t0:t0 + l, w * H * 64:(w + 1) * H * 64].reshape(l, H, 64)
                out[t0:t0 + l, w * H * 64:(w + 1) * H * 64] = rotate_bf16(u, cos, sn).reshape(l, H * 64).to(BF)
        t0 += l
    return out


# ======================================================================================================== activations
_SAT = (0.0, 2.0 ** -126, -2.0 ** -126, 2.0 ** -20, -2.0 ** -20, 8.0, -8.0, 20.0, -20.0, 50.0, -50.0, 100.0, -100.0)


def sat_bf16(rows, cols, seed):
    """(rows, cols) bf16 of the 13 saturation values, cycling with a stride coprime to 13, to 8 (a lane's chunk) and to 32 (the
    interleave): every value meets every lane position."""
    idx = (torch.arange(rows * cols) * 5 + seed) % len(_SAT)
    return torch.tensor(_SAT, dtype=F32)[idx].reshape(rows, cols).to(BF)


def act_inputs(T, I, family, seed=900):
    """y, gate, d (upstream gradient), pre-activation, bias [I] and act = bf16(f_swiglu(y, gate)) (so that gate = 0 <=> act = 0, as
    after the real forward).  family "gauss": gate and pre ~ N(0, 2^2); "sat": gate and pre of the saturation values."""
    y, d = R.gauss_bf16(T, I, seed + I), R.gauss_bf16(T, I, seed + I + 2)
    if family == "gauss":
        g, pre = R.gauss_bf16(T, I, seed + I + 1, std=2.0), R.gauss_bf16(T, I, seed + I + 3, std=2.0)
    else:
        g, pre = sat_bf16(T, I, seed), sat_bf16(T, I, seed + 1)
    bias = 0.5 * torch.randn(I, generator=_gen(seed + I + 4))
    act = R.f_swiglu(y.to(F64), g.to(F64))[0].to(F32).to(BF)
    return dict(y=y, g=g, d=d, pre=pre, bias=bias, act=act)


def f_swiglu_bwd_ag(d, act, g):
    """gemm_ref.f_swiglu_bwd_ag with the documented contract at an exactly-zero gate: act = 0 there and d gate comes out 0 (the
    kernel's clamped reciprocal times 0), where the plain formula divides 0 by 0."""
    zero = g == 0
    dy, tdy, dg, tdg = R.f_swiglu_bwd_ag(d, act, torch.where(zero, torch.ones_like(g), g))
    z = torch.zeros_like(dg)
    return torch.where(zero, z, dy), torch.where(zero, z, tdy), torch.where(zero & (act == 0), z, dg), torch.where(zero & (act == 0), z, tdg)


def k_sig(x, c=None):
    """The kernels' sigmoid in fp32: 1 / (1 + exp2(-log2(e) x)), or with the quick-GELU slope folded into the constant."""
    k = _f32c(-LOG2E) if c is None else _f32c(-c) * _f32c(LOG2E)
    return 1.0 / (1.0 + torch.exp2(k * x))


def k_gelu_cdf(v):
    """cx_common.h gelu_cdf in fp32: A&S 7.1.26 on v / sqrt 2; -> (cdf, gauss = exp(-v^2 / 2))."""
    f = _f32c
    t = 1.0 / (1.0 + (f(0.3275911) * f(0.70710678118654752)) * v.abs())
    poly = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) + t * (f(-1.453152027) + t * f(1.061405429)))))
    gauss = torch.exp2(f(-0.72134752044448170) * v * v)
    return 0.5 * (1.0 + torch.copysign(1.0 - poly * gauss, v)), gauss


def emu_swiglu(y, g):
    return g * k_sig(g) * y


def emu_swiglu_bwd(d, y, g):
    s = k_sig(g)
    gs = g * s
    return gs * d, (s + gs * (1.0 - s)) * d * y


F32_MAX = 3.4028234663852886e38


def emu_swiglu_bwd_ag(d, act, g, rcp_clamp=F32_MAX):
    """rcp_clamp: the bound of the clamped reciprocal (cx_common.h rcp_clamped): +-FLT_MAX, which no normal gate's reciprocal reaches."""
    s = k_sig(g)
    return g * s * d, (d * act) * ((1.0 / g).clamp(-rcp_clamp, rcp_clamp) + 1.0 - s)


def emu_act(v, act):
    return v * k_sig(v, 1.702) if act == 1 else v * k_gelu_cdf(v)[0]


def emu_act_grad(v, act):
    if act == 1:
        s = k_sig(v, 1.702)
        return s * (1.0 + _f32c(1.702) * v * (1.0 - s))
    cdf, gauss = k_gelu_cdf(v)
    return cdf + v * _f32c(0.3989422804014327) * gauss


ACT_FORM = {0: "gelu", 1: "qgelu"}
ACT_SHAPES = ((1, 8), (1, 32), (3, 96), (257, 160), (2100, 2048))     # (1, 8): layout 0 and the plain activations only
ACT_SHAPES_CPU = ACT_SHAPES[:4] + ((41, 2048),)                       # what C_MEAS is measured on: the values cycle with period 13


def pre_plus_bias(pre, bias, dtype):
    return pre.to(dtype) if bias is None else pre.to(dtype) + bias.to(dtype)


def check_bf16(name, got, ref64, t64, c, floor=0.0):
    """bf16 result per element under 1 ulp_bf16(ref) + c 2^-24 T (gemm_ref.bound_nonlinear) (+ an absolute underflow term where the
    form has one: ag_floor).  Returns the worst err / bound."""
    return check_rows(name, got, ref64, R.bound_nonlinear(ref64, t64, c) + floor)


def ag_floor(g64):
    """The fp32 underflow term of d gate = (d act) (1 / g + 1 - s): at a gate of +-2^-126 the saved act = bf16(g y / 2) and the
    product d act are SUBNORMAL in fp32 -- d act is rounded to a multiple of 2^-149 whatever its size, an absolute error of up to one
    quantum that 1 / g = 2^126 then multiplies (2^-23 absolute in d gate, where T = |d y| / 2 can be far smaller).  No multiple of
    2^-24 T covers it and no fp32 evaluation of this form avoids it, so the bound carries 2^-149 |1 / g + 1 - s| next to C 2^-24 T;
    for |g| >= 2^-20 that is below 2^-129 and plays no part."""
    g = torch.where(g64 == 0, torch.ones_like(g64), g64)
    return torch.where(g64 == 0, torch.zeros_like(g64), 2.0 ** -149 * (1.0 / g + 1.0 - R._sig(g)).abs())


def act_floor(form, d=None, y=None, g=None, v=None, act=None):
    """The fp32 underflow term of an activation form: 2^-126 times the form with its sigmoid (or Gaussian) replaced by 1.
    v_exp_f32 and v_rcp_f32 return 0 where the exact result is below the smallest fp32 normal (quick-GELU at v = -50 + bias:
    sigmoid(1.702 v) = 1e-38, the kernel returns -0 where fp64 has -4.9e-37), and gradual underflow would leave it a few bits: a
    sigmoid or exponential below 2^-126 has no relative accuracy in fp32, so its absolute error of up to 2^-126 reaches the result
    times the factor it multiplies.  At most ~1e-35 on these inputs: no part of any result in the normal range.  (d, y, g, v, act
    in fp64; the d gate of the (act, gate) form adds ag_floor.)"""
    a = lambda t: t.abs()                                                       # noqa: E731
    k = {"swiglu": lambda: a(g * y), "swiglu_bwd.dy": lambda: a(g * d), "swiglu_bwd.dg": lambda: a(d * y) * (1.0 + a(g)),
         "swiglu_bwd_ag.dy": lambda: a(g * d), "swiglu_bwd_ag.dg": lambda: a(d * act),
         "gelu": lambda: a(v), "qgelu": lambda: a(v), "gelu_bwd": lambda: a(d) * (1.0 + a(v)),
         "qgelu_bwd": lambda: a(d) * (1.0 + 1.702 * a(v))}[form]()
    f = F32_MIN_NORMAL * k
    return f + ag_floor(g) if form == "swiglu_bwd_ag.dg" else f


def check_f32(name, got, ref64, t64, c, floor=0.0):
    return check_rows(name, got, ref64, c * EPS24 * t64 + floor)


BF16_QUANTUM = 2.0 ** -133      # the spacing of bf16 below its smallest normal: bf16_ulp() never returns less
F32_MIN_NORMAL = 2.0 ** -126


def meas_ratio(ref64, t64, emu32, floor=0.0):
    """gemm_ref.meas_ratio on the part of the error that exceeds `floor`, the absolute term the checker grants next to C 2^-24 T:
    one bf16 quantum for a bf16 result (sigmoid(-100) = 3.7e-44 is not an fp32 normal: exp2 overflows, the kernel and the emulation
    return 0 where fp64 has 1e-41, an error no multiple of 2^-24 T = 2^-24 |ref| covers and the ulp term always does)."""
    err = ((emu32.to(F64) - ref64).abs() - floor).clamp(min=0)
    r = torch.where(t64 > 0, err / (EPS24 * t64).clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(r.max())


# ======================================================================================================== column sums
def colsum_grid(T, N):
    """colsum_rows_grid: row groups per 256-column block."""
    colblocks = (N + 255) // 256
    gy = min((1024 + colblocks - 1) // colblocks, (T + 255) // 256, 512)
    return max(gy, 1)


def colsum_chain(T, N):
    gy = colsum_grid(T, N)
    return -(-T // (8 * gy)) + 8 + gy


def colsum_ref(x, init):
    """-> (init + column sums of the bf16 matrix x, sum_rows |x| + |init|), fp64."""
    s = x.to(F64)
    return init.to(F64) + s.sum(0), s.abs().sum(0) + init.to(F64).abs()


def check_colsum(name, got, x, init):
    ref, mag = colsum_ref(x, init)
    T, N = x.shape
    return check_rows(name, got, ref, (colsum_chain(T, N) + 4) * 2.0 ** -23 * mag)


def sq_norm_blocks(n):
    return max(1, min((n // 4 + 255) // 256, 4096))


def sq_norm_bound(n):
    """Relative bound of cx_grad_sq_norm."""
    k = -(-(-(-n // 4)) // (sq_norm_blocks(n) * 256))
    return (4 * k + 4) * EPS24


# ============================================================================================================ pooling
EPS_NORM = float(_f32c(1e-12))          # the F.normalize clamp as the kernel holds it: 1e-12f
POOL_D = (8, 64, 768, 1032, 2048)
POOL_LENS = (5, 0, 1, 300, 2)


def cu_of(lens):
    return torch.tensor([0] + torch.tensor(list(lens)).cumsum(0).tolist(), dtype=torch.int32)


def pool_inputs(lens, d, seed=1100, zero_seq=None):
    """h (T, d) bf16 ~ N(0.25, 1) (a mean that does not cancel to nothing), demb (B, d) fp32; sequence `zero_seq` all zero."""
    T = sum(lens)
    h = (0.25 + torch.randn(T, d, generator=_gen(seed + d))).to(BF)
    if zero_seq is not None:
        t0 = sum(lens[:zero_seq])
        h[t0:t0 + lens[zero_seq]] = 0
    return h, torch.randn(len(lens), d, generator=_gen(seed + d + 1))


def pool_fwd_ref(h, lens, mode, normalize):
    """-> emb, T_emb (B, d), norm, T_norm (B,), fp64.  pooled = mean of the sequence's rows (mode 0; an empty sequence is 0 / 0 = NaN,
    as in the model this follows) or its first row (mode 1; empty: 0); norm = |pooled|; emb = pooled / max(norm, 1e-12f) under
    `normalize`.  T_pooled = sum |h| / len;  T_norm = |T_pooled| + norm (d norm = <pooled, d pooled> / norm <= |d pooled|);
    T_emb = (T_pooled + |emb| T_norm) / max(norm, 1e-12f), or T_pooled."""
    x = h.to(F64)
    B, d = len(lens), h.shape[1]
    pooled, tp = torch.zeros(B, d, dtype=F64), torch.zeros(B, d, dtype=F64)
    t0 = 0
    for b, l in enumerate(lens):
        if mode == 1:
            if l:
                pooled[b], tp[b] = x[t0], x[t0].abs()
        elif l:
            pooled[b], tp[b] = x[t0:t0 + l].sum(0) / l, x[t0:t0 + l].abs().sum(0) / l
        else:
            pooled[b], tp[b] = float("nan"), float("nan")
        t0 += l
    norm = pooled.pow(2).sum(-1).sqrt()
    tnorm = tp.pow(2).sum(-1).sqrt() + norm
    if not normalize:
        return pooled, tp, norm, tnorm
    den = norm.clamp(min=EPS_NORM)[:, None]
    emb = pooled / den
    return emb, (tp + emb.abs() * tnorm[:, None]) / den, norm, tnorm


def pool_bwd_ref(demb, emb, norm, lens, mode, normalize):
    """dh (T, d) and its T from the STORED fp32 emb / norm: g = demb, or (demb - emb <demb, emb>) / max(norm, 1e-12f); every row of
    a sequence receives g / len (mode 0), its first row g and the others 0 (mode 1).
    T = (|demb| + |emb| sum |demb emb|) / max(norm, 1e-12f) / len."""
    demb, emb, norm = demb.to(F64), emb.to(F64), norm.to(F64)
    d = demb.shape[1]
    dh, th = torch.zeros(sum(lens), d, dtype=F64), torch.zeros(sum(lens), d, dtype=F64)
    t0 = 0
    for b, l in enumerate(lens):
        if l:
            g, tg = demb[b], demb[b].abs()
            if normalize:
                inv = 1.0 / max(float(norm[b]), EPS_NORM)
                g = (g - emb[b] * (demb[b] * emb[b]).sum()) * inv
                tg = (tg + emb[b].abs() * (demb[b] * emb[b]).abs().sum()) * inv
            if mode == 1:
                dh[t0], th[t0] = g, tg
            else:
                dh[t0:t0 + l], th[t0:t0 + l] = g / l, tg / l
        t0 += l
    return dh, th


def emu_pool_fwd(h, lens, mode, normalize, len_plus=None, cls_row=0):
    """pool_normalize_fwd_kernel in fp32 with its summation order: 256 / (d / 8) row groups (at least one) each summing every
    ngroups-th row in turn, the groups added in order, one multiply by 1 / len; the squares summed per thread over c = tid, tid + 256,
    ... and then by torch.  Planted errors: len_plus = sequence whose 1 / len becomes 1 / (len + 1); cls_row = row read in cls mode."""
    x = h.to(F32)
    B, d = len(lens), h.shape[1]
    ng = max(256 // (d // 8), 1)
    emb, norm = torch.zeros(B, d, dtype=F32), torch.zeros(B, dtype=F32)
    t0 = 0
    for b, l in enumerate(lens):
        rows = x[t0 + cls_row:t0 + cls_row + 1] if (mode == 1 and l) else x[t0:t0 + (0 if mode == 1 else l)]
        part = torch.zeros(ng, d, dtype=F32)
        for k in range(-(-rows.shape[0] // ng)):
            blk = rows[k * ng:(k + 1) * ng]
            part[:blk.shape[0]] += blk
        v = torch.zeros(d, dtype=F32)
        for gi in range(ng):
            v = v + part[gi]
        if mode == 0:
            v = v * (_f32c(1.0) / _f32c(float(l + (1 if len_plus == b else 0))))
        sq = torch.zeros(256, dtype=F32)
        for c0 in range(0, d, 256):
            seg = v[c0:c0 + 256]
            sq[:seg.shape[0]] += seg * seg
        nrm = sq.sum().sqrt()
        norm[b] = nrm
        emb[b] = v / torch.maximum(nrm, _f32c(1e-12)) if normalize else v
        t0 += l
    return emb, norm


def emu_pool_bwd(demb, emb, norm, lens, mode, normalize, len_plus=None):
    """pool_normalize_bwd_kernel in fp32, one rounding to bf16."""
    demb, emb, norm = demb.to(F32), emb.to(F32), norm.to(F32)
    dh = torch.zeros(sum(lens), demb.shape[1], dtype=F32)
    t0 = 0
    for b, l in enumerate(lens):
        if l:
            g = demb[b]
            if normalize:
                g = (g - emb[b] * (demb[b] * emb[b]).sum()) * (_f32c(1.0) / torch.maximum(norm[b], _f32c(1e-12)))
            if mode == 1:
                dh[t0] = g
            else:
                dh[t0:t0 + l] = g * (_f32c(1.0) / _f32c(float(l + (1 if len_plus == b else 0))))
        t0 += l
    return dh.to(BF)


# =============================================================================================================== xent
XENT_V = (1, 7, 8, 2048, 2056, 30522, 30528)
XENT_N = 5
XENT_FAMILIES = ("gauss1", "gauss2", "gauss3", "edge")
IGNORE = -100


def xent_labels(V):
    """The five rows' labels: first and last class, the ignore index, and two out-of-range values (treated as ignored)."""
    return torch.tensor([0, V - 1, IGNORE, V, -1], dtype=I64)


def xent_inputs(V, family, dtype, seed=1300):
    """(5, V) logits of `dtype`.  gauss1..3: N(0, 3^2) of three seeds.  edge: N(0, 1) with the row maximum +80 planted at column 0
    (even rows) or V - 1 (odd rows) and -80 at every 5th column of the others."""
    if family.startswith("gauss"):
        return (3.0 * torch.randn(XENT_N, V, generator=_gen(seed + V + int(family[-1])))).to(dtype)
    x = torch.randn(XENT_N, V, generator=_gen(seed + V + 7))
    x[:, 2::5] = -80.0
    for r in range(XENT_N):
        x[r, 0 if r % 2 == 0 else V - 1] = 80.0
    return x.to(dtype)


def xent_neginf_inputs(V, dtype, seed=1400):
    """The -inf case: columns 0-15 and the last column of every row are -inf; the maximum is finite, the labels (16 and V - 2 on
    the live rows) are not masked."""
    x = (3.0 * torch.randn(XENT_N, V, generator=_gen(seed + V))).to(dtype)
    x[:, :16] = float("-inf")
    x[:, V - 1] = float("-inf")
    lab = torch.tensor([16, V - 2, IGNORE, V, 17], dtype=I64)
    return x, lab


def ignored_rows(labels, V, ignore_index=IGNORE):
    return (labels == ignore_index) | (labels < 0) | (labels >= V)


def xent_ref(x, labels, scale, ignore_index=IGNORE):
    """Forward from the rounded inputs, fp64 -> dict(lse, t_lse, loss, t_loss, ign).  scale is taken as its fp32 value."""
    sc = float(_f32c(scale))
    z = x.to(F64) * sc
    N, V = z.shape
    m = z.max(-1).values
    a = z - m[:, None]
    e = torch.exp(a)
    S = e.sum(-1)
    p = e / S[:, None]
    targ = torch.where(p > 0, p * a.abs(), torch.zeros_like(p)).sum(-1)          # the argument-dependent error of __expf, see above
    lse = m + torch.log(S)
    t_lse = m.abs() + torch.log(S).abs() + 1.0 + targ
    ign = ignored_rows(labels, V, ignore_index)
    zl = z.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    zero = torch.zeros_like(lse)
    return dict(lse=lse, t_lse=t_lse, loss=torch.where(ign, zero, lse - zl), t_loss=torch.where(ign, zero, t_lse + zl.abs()), ign=ign)


def xent_bwd_ref(x, labels, dloss, lse_stored, scale, lse_ref, ignore_index=IGNORE):
    """dlogits from the STORED fp32 lse -> (ref, T, extra): extra = |g| p |lse_stored - lse_ref|, added to the bound as it is."""
    sc = float(_f32c(scale))
    z = x.to(F64) * sc
    N, V = z.shape
    ign = ignored_rows(labels, V, ignore_index)
    g = torch.where(ign, torch.zeros(N, dtype=F64), dloss.to(F64) * sc)[:, None]
    a = z - lse_stored.to(F64)[:, None]
    p = torch.exp(a)
    hot = torch.zeros(N, V, dtype=F64)
    hot[~ign, labels[~ign]] = 1.0
    t = g.abs() * (torch.where(p > 0, p * (1.0 + a.abs()), torch.zeros_like(p)) + hot)
    extra = g.abs() * p * (lse_stored.to(F64) - lse_ref)[:, None].abs()
    ref = g * (p - hot)
    live = (~ign)[:, None]
    return torch.where(live, ref, torch.zeros_like(ref)), torch.where(live, t, torch.zeros_like(t)), torch.where(live, extra, torch.zeros_like(extra))


def xent_vec(V, ld, dtype, aligned=True, ld_d=None):
    """The launcher's dispatch: elements per lane (8 bf16 / 4 fp32 when V, every stride and the base pointers allow 16-B access)."""
    w = 8 if dtype == BF else 4
    ok = aligned and V % w == 0 and ld % w == 0 and (ld_d is None or ld_d % w == 0)
    return w if ok else 1


def _merge(m, s, m2, s2):
    mm = torch.maximum(m, m2)
    out = s * torch.exp(m - mm) + s2 * torch.exp(m2 - mm)
    return mm, torch.where(mm == float("-inf"), torch.zeros_like(s), out)


def emu_xent_fwd(x, labels, scale, vec, ignore_index=IGNORE, guard=True, drop_last=False, label_shift=0):
    """xent_fwd_kernel in fp32 with its structure: 256 lanes, lane i takes the `vec` columns from (256 k + i) vec in step k with an
    online (max, sum) update, a 64-lane xor butterfly of online merges, the four waves merged in order, lse = M + log S.
    guard: the in-lane update is skipped while the running maximum is still -inf (without it a lane whose first loaded columns are
    all -inf forms 0 * exp(-inf - -inf) = NaN).  Planted errors: drop_last (lse from all but the last column), label_shift."""
    NEG = float("-inf")
    z = x.to(F32) * _f32c(scale)
    N, V = z.shape
    Vs = V - 1 if drop_last else V
    steps = -(-V // (256 * vec))
    zp = torch.full((N, steps * 256 * vec), NEG, dtype=F32)
    zp[:, :Vs] = z[:, :Vs]
    zp = zp.view(N, steps, 256, vec)
    valid = (torch.arange(steps * 256) * vec < V).view(steps, 256)
    m, s = torch.full((N, 256), NEG, dtype=F32), torch.zeros(N, 256, dtype=F32)
    for k in range(steps):
        v = zp[:, k]
        mm = torch.maximum(m, v.max(-1).values)
        acc = s * torch.exp(m - mm)
        for e in range(vec):
            acc = acc + torch.exp(v[..., e] - mm)
        if guard:
            acc = torch.where(mm == NEG, s, acc)
        s, m = torch.where(valid[k], acc, s), torch.where(valid[k], mm, m)
    lane = torch.arange(64)
    m, s = m.view(N, 4, 64), s.view(N, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        m, s = _merge(m, s, m[..., lane ^ o], s[..., lane ^ o])
    M, S = m[:, 0, 0], s[:, 0, 0]
    for w in range(1, 4):
        M, S = _merge(M, S, m[:, w, 0], s[:, w, 0])
    lse = M + torch.log(S)
    lab = labels + label_shift
    ign = ignored_rows(labels, V, ignore_index)
    zl = z.gather(1, lab.clamp(0, V - 1)[:, None])[:, 0]
    return torch.where(ign, torch.zeros_like(lse), lse - zl), lse


def emu_xent_bwd(x, labels, dloss, lse, scale, ignore_index=IGNORE, label_shift=0):
    """xent_bwd_kernel in fp32, rounded once to the logits' dtype."""
    z = x.to(F32) * _f32c(scale)
    N, V = z.shape
    ign = ignored_rows(labels, V, ignore_index)
    v = torch.exp(z - lse.to(F32)[:, None])
    hot = torch.zeros(N, V, dtype=F32)
    live = ~ign
    hot[live, (labels[live] + label_shift).clamp(0, V - 1)] = 1.0
    out = (v - hot) * (dloss.to(F32) * _f32c(scale))[:, None]
    return torch.where(live[:, None], out, torch.zeros_like(out)).to(x.dtype)


def check_xent_fwd(tag, loss, lse, x, labels, scale):
    """-> (worst ratio lse, worst ratio loss, the fp64 reference)."""
    ref = xent_ref(x, labels, scale)
    r1 = check_f32(f"{tag} lse", lse[:, None], ref["lse"][:, None], ref["t_lse"][:, None], C("xent", "lse"))
    assert bool((loss[ref["ign"]] == 0).all()), f"{tag}: the loss of an ignored row is not exactly 0"
    r2 = check_f32(f"{tag} loss", loss[:, None], ref["loss"][:, None], ref["t_loss"][:, None], C("xent", "loss"))
    return r1, r2, ref


def check_xent_bwd(tag, dlogits, x, labels, dloss, lse_stored, scale, lse_ref):
    ref, t, extra = xent_bwd_ref(x, labels, dloss, lse_stored, scale, lse_ref)
    ign = ignored_rows(labels, x.shape[1])
    assert bool((dlogits[ign] == 0).all()), f"{tag}: the gradient of an ignored row is not exactly 0"
    fmt = torch.where(ref == 0, torch.zeros_like(ref), bf16_ulp(ref)) if dlogits.dtype == BF else 0.0
    return check_rows(f"{tag} dlogits", dlogits, ref, fmt + C("xent", "dlogits") * EPS24 * t + extra + xent_floor(dloss, scale))


def xent_floor(dloss, scale):
    """|g| 2^-126 per row: exp(z - lse) below the smallest fp32 normal (z - lse < -87.3) has no relative accuracy in fp32 -- gradual
    underflow quantises it to 2^-149, a flushing exponential returns 0 -- so the relative bound C 2^-24 T cannot hold there for any
    fp32 evaluation; the absolute term it needs is the smallest normal times |g|."""
    return (dloss.to(F64).abs() * float(_f32c(scale)) * F32_MIN_NORMAL)[:, None]


# ========================================================================================================== optimizer
OPT_N = (1, 3, 4, 5, 1027, (1 << 22) + 4099)
HP = dict(beta1=0.9, beta2=0.999, eps=1e-8)
# (step, weight_decay, clip kind, max_norm, lr): sq_norm NULL / clipping / not clipping / max_norm <= 0; lr = 0.05 with decay makes the
# order of decay and update visible in fp32 (at lr = 2e-4 the two orders differ by lr^2 wd = 4e-9, below the rounding of p)
OPT_CASES = ((1, 0.0, None, 0.0, 2e-4), (1, 0.1, "clip", 0.01, 0.05), (1000, 0.1, "noclip", 1e6, 2e-4), (1000, 0.0, "off", -1.0, 2e-4),
             (1000, 0.1, "clip", 0.01, 0.05))


def opt_inputs(n, seed=1500):
    """p, g, m, v (v >= 0) fp32 [n]: magnitudes of a trained model's state; every 7th gradient (from index 3) exactly 0."""
    gn = _gen(seed + n % 9973)
    p = 0.05 * torch.randn(n, generator=gn)
    g = 1e-2 * torch.randn(n, generator=gn)
    g[3::7] = 0.0
    m = 3e-3 * torch.randn(n, generator=gn)
    v = (1e-2 * torch.randn(n, generator=gn)).pow(2)
    return p, g, m, v


def bias_corrections(beta1, beta2, step):
    """(bias_c1, bias_c2_sqrt) as the launcher forms them: in double from the fp32 betas, rounded to fp32."""
    b1, b2 = float(_f32c(beta1)), float(_f32c(beta2))
    return float(_f32c(1.0 - b1 ** step)), float(_f32c(math.sqrt(1.0 - b2 ** step)))


def clip_coef(sq, max_norm, dtype=F64):
    """torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)); 1 without a sum of squares or max_norm <= 0."""
    if sq is None or not max_norm > 0:
        return torch.ones((), dtype=dtype)
    norm = torch.as_tensor(sq, dtype=F64).sqrt().to(dtype)
    one = torch.ones((), dtype=dtype)
    return torch.minimum(one, torch.tensor(float(_f32c(max_norm)), dtype=dtype) / (norm + torch.tensor(float(_f32c(1e-6)), dtype=dtype)))


def adamw_step(p, g, m, v, lr, wd, step, sq, max_norm, dtype=F64, wd_after=False, beta1=HP["beta1"], beta2=HP["beta2"], eps=HP["eps"]):
    """One AdamW step per element in the operation order of adam_one, in `dtype`: fp64 = the reference (hyperparameters at their
    fp32 values, the clip coefficient from the fp64 sum of squares `sq`), fp32 = the emulation of the kernel.
    -> p, m, v and (fp64 only) their scales
        T_m = |m| + (1 - beta1) |g c - m|,   T_v = beta2 v + (1 - beta2) (g c)^2,   T_p = |p| + (lr / bc1) (T_m + |m'|) / denom
    (the error of m' reaches p through the update).  wd_after: the planted error -- decay applied after the update."""
    f = lambda t: torch.tensor(float(_f32c(t)), dtype=dtype)          # noqa: E731
    lr_, b1, b2, eps_, wd_ = f(lr), f(beta1), f(beta2), f(eps), f(wd)
    bc1, bc2 = (torch.tensor(t, dtype=dtype) for t in bias_corrections(beta1, beta2, step))
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    g = g * clip_coef(sq, max_norm, dtype)
    decay = 1.0 - lr_ * wd_
    if not wd_after:
        p = p * decay
    tm = m.abs() + (g - m).abs() * (1.0 - b1)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    denom = v.sqrt() / bc2 + eps_
    tp = p.abs() + (lr_ / bc1) * (tm + m.abs()) / denom
    p = p - (lr_ / bc1) * (m / denom)
    if wd_after:
        p = p * decay
    return (p, m, v, tp, tm, v.clone()) if dtype == F64 else (p, m, v)


def ema_step(ema, p, decay, dtype=F64, swapped=False):
    """ema = decay ema + (1 - decay) p -> (value, T = |decay ema| + |(1 - decay) p|).  swapped: the planted error."""
    dk = torch.tensor(float(_f32c(decay)), dtype=dtype)
    w = 1.0 - dk
    if swapped:
        dk, w = w, dk
    a, b = dk * ema.to(dtype), w * p.to(dtype)
    return a + b, a.abs() + b.abs()


# ====================================================================================== ViT front end (vit.hip): bit-exact
VIT_PATCHIFY = ((2, 3, 8, 12, 4), (3, 3, 32, 48, 16))     # (B, C, H, W, patch): 144 lanes = one partial block; 3456 = 13.5 blocks
VIT_ASSEMBLE = ((3, 6, 24), (2, 6, 520))                 # (B, P, d)
# K = 4 of 6 patches per image, unsorted, the last patch in each; patch 4 is dropped by every image
VIT_P_ALL, VIT_KEEP = 6, ((5, 0, 3, 2), (1, 5, 2, 0), (2, 3, 5, 1))


def vit_keep(B):
    return torch.tensor(VIT_KEEP[:B], dtype=torch.int32)


def vit_inv(keep, P_all):
    """inv[b][patch] = position of `patch` among image b's kept ones, or -1 (what cx_vit_assemble_bwd_gather reads)."""
    inv = torch.full((keep.shape[0], P_all), -1, dtype=torch.int32)
    for b, row in enumerate(keep.tolist()):
        for j, pi in enumerate(row):
            inv[b, pi] = j
    return inv


def vit_dz(B, P, d, seed):
    """dz (B (P + 1), d) bf16 for the assembly backward: Gaussian, image b scaled by 2^20, 1, 1/2, ... so that the fp32 sum over the
    images rounds after each addition and their ORDER shows in the result (three bf16 values of one magnitude add exactly)."""
    z = R.gauss_bf16(B * (P + 1), d, seed).reshape(B, P + 1, d).float()
    scale = torch.tensor([2.0 ** 20] + [2.0 ** -i for i in range(B - 1)])
    return (z * scale[:, None, None]).to(BF).reshape(B * (P + 1), d)


def patchify_ref(pix, patch, keep=None):
    """pixels (B, C, H, W) -> (B * hp * wp, C * patch * patch) bf16: "b c (h p1) (w p2) -> b h w (c p1 p2)", then round to nearest even.
    keep (B, K): row b * K + j is patch keep[b][j]."""
    B, C, H, W = pix.shape
    hp, wp = H // patch, W // patch
    x = pix.reshape(B, C, hp, patch, wp, patch).permute(0, 2, 4, 1, 3, 5).reshape(B, hp * wp, C * patch * patch)
    if keep is not None:
        x = torch.stack([x[b, keep[b].long()] for b in range(B)])
    return x.reshape(-1, C * patch * patch).float().to(BF)


def assemble_fwd_ref(proj, cls, pos, B, P, keep=None):
    """out[b, 0] = bf16(cls + pos[0]); out[b, s] = bf16(float(proj[b P + s - 1]) + pos[s]) -- pos[1 + keep[b][s - 1]] with keep; one fp32
    add per element.  -> (B (P + 1), d) bf16."""
    d = proj.shape[1]
    out = torch.empty(B, P + 1, d, dtype=F32)
    out[:, 0] = cls + pos[0]
    for b in range(B):
        rows = torch.arange(1, P + 1) if keep is None else 1 + keep[b].long()
        out[b, 1:] = proj[b * P:(b + 1) * P].float() + pos[rows]
    return out.reshape(B * (P + 1), d).to(BF)


def assemble_bwd_ref(dz, B, P, gpos0, gcls0, dproj0, inv=None):
    """dproj[b P + sk - 1] = dz[b, sk] (a copy) and gpos[s] = gpos0[s] + (((0 + dz[0, .]) + dz[1, .]) + ...) in fp32, images in order, the
    kernel's order; gcls likewise from position 0.  With inv (B, P_all) the sum of original position s >= 1 takes image b's row
    sk = 1 + inv[b][s - 1] and skips the images that dropped the patch; rows of dproj0 that nothing maps to come back as they were.
    -> dproj, gpos, gcls"""
    d = dz.shape[1]
    z = dz.reshape(B, P + 1, d)
    n_pos = gpos0.shape[0]
    dproj, acc = dproj0.clone().reshape(B, P, d), torch.zeros(n_pos, d, dtype=F32)
    for b in range(B):
        for s in range(n_pos):
            sk = s
            if inv is not None and s > 0:
                if int(inv[b, s - 1]) < 0:
                    continue
                sk = 1 + int(inv[b, s - 1])
            if s > 0:
                dproj[b, sk - 1] = z[b, sk]
            acc[s] = acc[s] + z[b, sk].float()
    return dproj.reshape(B * P, d), gpos0 + acc, gcls0 + acc[0]
