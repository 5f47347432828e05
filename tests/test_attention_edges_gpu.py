"""Self-attention, every kernel route, at the edges of its tiles: each case runs forward then backward through the C-ABI and
compares every element of out, lse, dq, dk, dv with the float64 reference of tests/attn_ref.py, per (token, head) row.

Acceptance (attn_ref.judge): worst row error and whole-tensor Frobenius error of each output at most 3 x those of the fp32
model with the kernels' documented bf16 rounding points on the same inputs; max |lse error| at most 3 x the model's + 4 fp32
ulp.  No constant of this file enters a bound.  dq / dk rows that are exactly 0 (sequences of length 1, the uniform family)
are held to the rounding bound derived in attn_ref.zero_grad_bounds.

Every call runs with guard margins: qkv, dout, out, lse and dqkv are interior views of larger allocations, 64 rows in front
and behind.  Input margins hold NaN (a kernel that reads outside the packed tensor and masks by multiplication shows a NaN),
output margins a fixed bit pattern that must survive, output interiors NaN before the call (every element must be written).
The kernels clamp ragged loads to the last row of the sequence by design; this only verifies that they do.

Routes (the dispatch of cx_attn_varlen_fwd / _bwd / _bwd_prerotated selects the kernels by max_seqlen and tables):
  s128             product, with and without tables, max <= 128     attn_fwd_s128v, attn_bwd_fused2_s128
  s256             product, no tables, 129 .. 256                   attn_fwd_s256, attn_bwd_dq_long + _dkv_long
  s256-rot         product, tables                                  attn_fwd_s256, delta + general dq / dkv
  long             product, no tables, > 256                        attn_fwd_long, long dq / dkv
  long-rot-onload  product, tables, > 256                           general forward, delta + general dq / dkv
  long-prerot      product, q / k rotated in place, forward without tables, cx_attn_varlen_bwd_prerotated, > 128
  general-all      dev library with every switch at 0, with and without tables: the round-1 kernels at every length

Measured on an MI355X when this module was written, worst kernel / model ratio over all cases of a route (the rule allows 3;
lse as a fraction of its bound); every case appends its own figures to kernel_report.jsonl ("attention_edges"):
  route             out    dq    dk    dv   lse
  s128             1.00  1.00  1.01  1.01  0.22
  s256             1.00  1.05  1.08  1.00  0.27
  s256-rot         1.00  1.00  1.02  1.00  0.28
  long             1.06  1.05  1.07  1.00  0.23
  long-rot-onload  1.00  1.25  1.09  1.00  0.22
  long-prerot      1.02  1.25  1.09  1.00  0.28
  general-all      1.06  1.25  1.09  1.01  0.24
"""
import math
import time

import numpy as np
import pytest
import torch

from contrastors_amd import _C
from tests import attn_ref as ar
from tests.gpu_util import LD, L, S, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 64
SCALE = 1 / math.sqrt(D)
MARGIN = 64          # guard rows in front of and behind every buffer
PATTERN16, PATTERN32 = 0x5A5A, 0x5A5A5A5A

BATCHES = {
    "s128": [1, 128, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127],
    "s256": [129, 1, 159, 160, 161, 191, 192, 193, 64, 223, 224, 225, 255, 256],
    "longA": [257, 1, 288, 289, 319, 320, 321, 130, 383, 384, 385],
    "longB": [511, 512, 513, 33, 1023, 1025, 2047, 2049],
}
# route -> (tables, batches it runs on)
ROUTES = {
    "s128": (False, ["s128"]),
    "s128-rot": (True, ["s128"]),
    "s256": (False, ["s256"]),
    "s256-rot": (True, ["s256"]),
    "long": (False, ["longA", "longB"]),
    "long-rot-onload": (True, ["longA", "longB"]),
    "long-prerot": (True, ["s256", "longA", "longB"]),
    "general-all": (False, ["s128", "s256", "longA", "longB"]),
    "general-all-rot": (True, ["s128", "s256", "longA", "longB"]),
}
PRODUCT_ROUTES = [r for r in ROUTES if not r.startswith("general")]
_TABLES = {}


def _tables():
    if not _TABLES:
        cos, sin = ar.rotary_tables(2176)
        _TABLES["t"] = (cos.to(DEV), sin.to(DEV))
    return _TABLES["t"]


def _cases():
    """Every (route, batch) sees gauss (H = 1, 3, 12), sentinel and max_last (H = 1, 12); the other families run on the first
    batch of each route, H alternating between 1 and 12 (uniform without tables only: it has no closed form under rotation)."""
    out = []
    for route, (tables, batches) in ROUTES.items():
        for i, batch in enumerate(batches):
            fams = [("gauss", 1), ("gauss", 3), ("gauss", 12), ("sentinel", 1), ("sentinel", 12), ("max_last", 1), ("max_last", 12)]
            if i == 0:
                fams += [("peaked", 12), ("shift_pos", 1), ("shift_neg", 12), ("max_first", 1)]
                if not tables:
                    fams.append(("uniform", 12))
            out += [pytest.param(route, batch, f, H, id=f"{route}-{batch}-{f}-H{H}") for f, H in fams]
    return out


@pytest.fixture
def general_kernels():
    """The dev library with every attention switch at 0 (round 1's streaming kernels at every length); the switches are
    process-global, so the defaults (2, 3, 1, 1) come back whatever the test did."""
    d = LD()
    try:
        d.cx_attn_set_fwd_s128(0)
        d.cx_attn_set_bwd_s128(0)
        d.cx_attn_set_fwd_long(0)
        d.cx_attn_set_bwd_long(0)
        yield d
    finally:
        d.cx_attn_set_fwd_s128(2)
        d.cx_attn_set_bwd_s128(3)
        d.cx_attn_set_fwd_long(1)
        d.cx_attn_set_bwd_long(1)


# ------------------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """A flat allocation [margin | interior | margin]; `view` is the interior with the shape asked for."""

    def __init__(self, shape, dtype, row_elems, data=None):
        n, m = int(np.prod(shape)), MARGIN * row_elems
        self.m, self.n = m, n
        self.buf = torch.full((n + 2 * m,), float("nan"), dtype=dtype, device=DEV)
        self.bits = self.buf.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
        self.pattern = PATTERN16 if dtype == torch.bfloat16 else PATTERN32
        self.view = self.buf[m:m + n].view(shape)
        if data is None:          # an output: NaN interior, patterned margins
            self.bits[:m] = self.pattern
            self.bits[m + n:] = self.pattern
        else:                     # an input: NaN margins
            self.view.copy_(data)

    def margins_intact(self):
        return bool((self.bits[:self.m] == self.pattern).all() and (self.bits[self.m + self.n:] == self.pattern).all())


def _run(lib, mode, qkv, dout, lens, tables, H, max_seqlen=None, drop=None):
    """Forward then backward on guarded buffers.  lens may hold zeros.  mode: "onload" (tables, if any, go to the kernels) or
    "prerot" (q / k rotated in place first, forward without tables, cx_attn_varlen_bwd_prerotated).  drop = (p, seed, offset)
    selects the dropout entry points.  Returns float copies of out (T, H, 64), lse (H, T), dq, dk, dv."""
    T, B = sum(lens), len(lens)
    mx = max_seqlen or max(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    cos, sin = _tables() if tables else (None, None)
    x = Guarded((T, 3, H, D), torch.bfloat16, 3 * H * D, qkv)
    do = Guarded((T, H, D), torch.bfloat16, H * D, dout)
    out = Guarded((T, H, D), torch.bfloat16, H * D)
    lse = Guarded((H, T), torch.float32, H * D)
    dqkv = Guarded((T, 3, H, D), torch.bfloat16, 3 * H * D)
    delta = torch.empty(H, T, device=DEV)
    p = [x.view.data_ptr(), cu.data_ptr()]
    tail = [B, H, T, mx, SCALE]
    if mode == "prerot":
        assert tables and drop is None
        _C.check(lib.cx_rotary_qkv_inplace(*p, cos.data_ptr(), sin.data_ptr(), B, H, T, mx, 1, S()), "rotary")
        _C.check(lib.cx_attn_varlen_fwd(*p, None, None, out.view.data_ptr(), lse.view.data_ptr(), *tail, S()), "fwd")
        _C.check(lib.cx_attn_varlen_bwd_prerotated(do.view.data_ptr(), x.view.data_ptr(), out.view.data_ptr(), lse.view.data_ptr(),
                                                   cu.data_ptr(), cos.data_ptr(), sin.data_ptr(), delta.data_ptr(),
                                                   dqkv.view.data_ptr(), *tail, S()), "bwd_prerotated")
    else:
        fwd, bwd, extra = lib.cx_attn_varlen_fwd, lib.cx_attn_varlen_bwd, []
        if drop is not None:
            fwd, bwd, extra = lib.cx_attn_varlen_dropout_fwd, lib.cx_attn_varlen_dropout_bwd, [drop[0], drop[1], drop[2], 0]
        _C.check(fwd(*p, _C.ptr(cos), _C.ptr(sin), out.view.data_ptr(), lse.view.data_ptr(), *tail, *extra, S()), "fwd")
        _C.check(bwd(do.view.data_ptr(), x.view.data_ptr(), out.view.data_ptr(), lse.view.data_ptr(), cu.data_ptr(), _C.ptr(cos),
                     _C.ptr(sin), delta.data_ptr(), dqkv.view.data_ptr(), *tail, *extra, S()), "bwd")
    torch.cuda.synchronize()
    for name, g in (("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert g.margins_intact(), f"{name}: the kernel wrote outside the buffer"
        assert not torch.isnan(g.view).any(), f"{name}: NaN (an element not written, or a read outside the packed tensor)"
    g = dqkv.view.float()
    return {"out": out.view.float(), "lse": lse.view.clone(), "dq": g[:, 0].contiguous(), "dk": g[:, 1].contiguous(),
            "dv": g[:, 2].contiguous()}


def _lib_and_mode(route, dev):
    if route.startswith("general"):
        return dev, "onload"
    return L(), "prerot" if route == "long-prerot" else "onload"


def _inputs(family, lens, H, tables, seed):
    cos, sin = _tables() if tables else (None, None)
    qkv, dout = ar.make_inputs(family, lens, H, seed, None if cos is None else cos.cpu(), None if sin is None else sin.cpu())
    return qkv.to(DEV), dout.to(DEV), cos, sin


def _judge(got, qkv, dout, lens, cos, sin, family, keep=None, p_drop=0.0):
    ref = ar.reference(qkv, lens, cos, sin, SCALE, dout, keep, p_drop)
    model = ar.bf16_model(qkv, lens, cos, sin, SCALE, dout, keep, p_drop)
    zb = ar.zero_grad_bounds(qkv, lens, SCALE, dout, uniform=family == "uniform", p_drop=p_drop)
    fig, fails = ar.judge(got, model, ref, lens, zero_bounds=zb)
    return fig, fails, ref


def _record(kind, route, batch, family, H, fig, fails, **more):
    rec = {}
    for name in ar.OUTPUTS:
        f = fig[name]
        rec[f"{name}_row"], rec[f"{name}_model_row"] = f["row"], f["model_row"]
        rec[f"{name}_fro"], rec[f"{name}_model_fro"] = f["fro"], f["model_fro"]
        rec[f"{name}_where"] = f["where"]
    rec["lse_abs"], rec["lse_model_abs"], rec["lse_bound"] = fig["lse"]["abs"], fig["lse"]["model_abs"], fig["lse"]["bound"]
    rec["lse_where"] = fig["lse"]["where"]
    report("attention_edges", kind=kind, route=route.replace("-rot", "") if route.startswith(("s128", "general")) else route,
           tables=ROUTES[route][0], batch=batch, family=family, H=H, passed=not fails, **rec, **more)


# -------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("route,batch,family,H", _cases())
def test_attention_rows(route, batch, family, H, request):
    tables, _ = ROUTES[route]
    lens = BATCHES[batch]
    lib, mode = _lib_and_mode(route, request.getfixturevalue("general_kernels") if route.startswith("general") else None)
    t_start = time.time()
    qkv, dout, cos, sin = _inputs(family, lens, H, tables, seed=1000 + 7 * len(family) + H)
    got = _run(lib, mode, qkv, dout, lens, tables, H)
    fig, fails, ref = _judge(got, qkv, dout, lens, cos, sin, family)
    if family == "uniform":
        out_cf, lse_cf = ar.uniform_closed_form(qkv, lens, SCALE)
        # closed form: out = v exactly representable, one bf16 rounding at most; lse within the rule's own 4-ulp term + fp32 dot
        e_out = float(ar.row_errors(got["out"], out_cf, lens).max())
        e_lse = float((got["lse"].double() - lse_cf).abs().max())
        lse_bound = fig["lse"]["bound"]
        if not e_out <= ar.FACTOR * ar.BF16_HALF_ULP:
            fails.append(f"out against the closed form v: {e_out:.3e}")
        if not e_lse <= lse_bound:
            fails.append(f"lse against scale q.k + log(len): {e_lse:.3e} > {lse_bound:.3e}")
    _record("rows", route, batch, family, H, fig, fails, seconds=time.time() - t_start)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("batch,family,H", [("s128", "shift_neg", 12), ("longA", "gauss", 3), ("s256", "peaked", 1)])
def test_rotation_is_the_reference_rotation_bit_for_bit(batch, family, H):
    """cx_rotary_qkv_inplace against attn_ref.rotate_bf16, every bit of q and k, v untouched.  The rotated value is rounded to
    bf16 next, so the fp32 operation order of the rotation decides the elements that sit on a bf16 tie; every kernel takes it from
    one place (rotary_pair, csrc/cx_common.h) and the reference states the same order.  Before that, the fused S <= 128 backward
    rotated such a q element to the other neighbour than the forward had (s128-rot / shift_neg / H12 above: one dv row at 3.2 x
    the model, a whole P row off by 1.9 %)."""
    lens = BATCHES[batch]
    T, B = sum(lens), len(lens)
    qkv, _, cos, sin = _inputs(family, lens, H, True, seed=80)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    x = Guarded((T, 3, H, D), torch.bfloat16, 3 * H * D, qkv)
    _C.check(L().cx_rotary_qkv_inplace(x.view.data_ptr(), cu.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, H, T, max(lens), 1, S()))
    torch.cuda.synchronize()
    want = qkv.clone()
    t0 = 0
    for l in lens:
        want[t0:t0 + l, 0] = ar.rotate_bf16(qkv[t0:t0 + l, 0], cos, sin).to(torch.bfloat16)
        want[t0:t0 + l, 1] = ar.rotate_bf16(qkv[t0:t0 + l, 1], cos, sin).to(torch.bfloat16)
        t0 += l
    differ = (x.view.view(torch.int16) != want.view(torch.int16))
    assert not differ.any(), f"{int(differ.sum())} of {differ.numel()} elements differ, first at {differ.nonzero()[0].tolist()}"
    assert torch.isnan(x.buf[:x.m]).all() and torch.isnan(x.buf[x.m + x.n:]).all()


def _with_empties(lens):
    """Empty sequences first, in the middle (two in a row) and last."""
    mid = len(lens) // 2
    return [0] + lens[:mid] + [0, 0] + lens[mid:] + [0]


@pytest.mark.parametrize("route", PRODUCT_ROUTES)
def test_zero_length_sequences_change_nothing(route):
    """cu_seqlens with repeated entries: the other sequences' results are bit-identical to the batch without the empty ones
    (every kernel clamps ragged rows with `r < len ? r : len - 1`, row -1 for len == 0, and must return before using it; the
    empty first entry sits at t0 == 0, where row -1 is the NaN margin)."""
    tables, batches = ROUTES[route]
    lens, H = BATCHES[batches[0]], 3
    lib, mode = _lib_and_mode(route, None)
    qkv, dout, cos, sin = _inputs("gauss", lens, H, tables, seed=77)
    a = _run(lib, mode, qkv, dout, lens, tables, H)
    b = _run(lib, mode, qkv, dout, _with_empties(lens), tables, H)
    same = {k: torch.equal(a[k], b[k]) for k in a}
    fig, fails, _ = _judge(b, qkv, dout, lens, cos, sin, "gauss")
    _record("empties", route, batches[0], "gauss", H, fig, fails, identical=all(same.values()))
    assert all(same.values()), same
    assert not fails, "\n".join(fails)


def _kernel_class(mx):
    return (mx <= 128, mx <= 256)


@pytest.mark.parametrize("how", ["next64", "plus1"])
@pytest.mark.parametrize("route", PRODUCT_ROUTES)
def test_max_seqlen_larger_than_the_longest_sequence(route, how):
    """max_seqlen is an upper bound, not max(lens): a larger one gives bit-identical results where it selects the same kernels,
    and results inside the acceptance rule where it crosses 128 or 256 and selects others."""
    tables, batches = ROUTES[route]
    batch = batches[-1] if route != "long-prerot" else "longA"
    lens, H = BATCHES[batch], 3
    mx = max(lens)
    bigger = mx + 1 if how == "plus1" else (mx // 64 + 1) * 64
    lib, mode = _lib_and_mode(route, None)
    qkv, dout, cos, sin = _inputs("gauss", lens, H, tables, seed=78)
    a = _run(lib, mode, qkv, dout, lens, tables, H)
    b = _run(lib, mode, qkv, dout, lens, tables, H, max_seqlen=bigger)
    fig, fails, _ = _judge(b, qkv, dout, lens, cos, sin, "gauss")
    same_kernels = _kernel_class(mx) == _kernel_class(bigger)
    same = {k: torch.equal(a[k], b[k]) for k in a}
    _record("max_seqlen", route, batch, "gauss", H, fig, fails, max_seqlen=bigger, same_kernels=same_kernels,
            identical=all(same.values()))
    assert not fails, "\n".join(fails)
    if same_kernels:
        assert all(same.values()), same


@pytest.mark.parametrize("batch", ["s128", "s256", "longA", "longB"])
def test_dropout_instantiations(batch):
    """cx_attn_varlen_dropout_fwd / _bwd at p = 0.1 (the <DROP> instantiations of the same masking code, with their own
    register budgets) on sentinel inputs; the mask is read back with cx_attn_dropout_keep_mask as in
    tests/test_dropout_gpu.py and handed to the reference and to the model; same per-row rule."""
    lens, H, p, seed, off = BATCHES[batch], 2, 0.1, 4242, 8
    B, S_ = len(lens), (max(lens) + 3) // 4 * 4
    qkv, dout, cos, sin = _inputs("sentinel", lens, H, False, seed=79)
    got = _run(L(), "onload", qkv, dout, lens, False, H, drop=(p, seed, off))
    keep = torch.empty(B, H, S_, S_, dtype=torch.uint8, device=DEV)
    _C.check(LD().cx_attn_dropout_keep_mask(keep.data_ptr(), B, H, S_, p, seed, off, 0, S()))
    rate = keep[1, :, :lens[1], :lens[1]].float().mean().item() if lens[1] > 64 else keep.float().mean().item()
    assert abs(rate - (1 - p)) < 0.01, rate
    fig, fails, _ = _judge(got, qkv, dout, lens, None, None, "sentinel", keep, p)
    _record("dropout", {"s128": "s128", "s256": "s256"}.get(batch, "long"), batch, "sentinel", H, fig, fails, keep_rate=rate)
    assert not fails, "\n".join(fails)
