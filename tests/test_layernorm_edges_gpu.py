"""The LayerNorm family of contrastors_amd/csrc/layernorm.hip against the fp64 reference of tests/ln_ref.py, per row, at the
row counts where a wave takes a second and a third row, where each grid cap of the launchers binds, at all four widths, with
every optional pointer NULL on its own, and through the C ABI for the mixed-dtype kernels; the embedding kernels (gather +
LayerNorm, its backward with the atomic and the sorted word-row reduction) at their grid caps.

Every operand and result is a slice of a larger allocation whose 8 rows (8 elements for vectors) either side hold a NaN bit
pattern: a read outside the slice poisons the result, a write outside it is found when the test ends (`_guards`).

Bounds (tests/ln_ref.py): bf16 results 0.5 ulp_bf16(ref) + C 2^-24 S per element, fp32 results C 2^-24 S, mean
C 2^-24 mean|z_r|, rstd C 2^-24 relative, dgamma / dbeta / column sums C 2^-24 sum_rows|term| per column, with C = 4 C_meas
and C_meas measured by tests/test_ln_ref_cpu.py on an fp32 emulation against the fp64 reference (never against a kernel):

    family     out      out_tight  mean  rstd | family     dz    dx0   dgamma  dbeta  colsum
    fwd        3.0e6    4.5        3.6   4.2  | bwd        160   -     4.0     3.0    1.1
    fwd_f32    3.7e6    5.0        3.9   5.5  | bwd_rms    820   -     3.8     3.0    -
    fwd_rms    5.6      -          -     3.2  | bwd_drop   115   115   3.6     0.5    1.0
    fwd_drop   9600     4.8        3.5   3.7  | pooled     300   -     6.2     12.0   4.3
    embed_fwd  1.8e4    3.6        3.6   2.9  | embed_bwd  102   -     0.77    0.44   -      scatter 102

(embed_bwd "scatter": dtype0, dpos and dword are sums of fp32 dz rows; each against the same sum of the fp64 dz rows under
C 2^-24 sum|S_t| over the rows t it receives, S_t the scale of dz.)

(`out` on S = |xhat g| + |b| alone is so large because S lacks the rounding of the row mean times rstd; ln_ref.check_out applies
it together with `out_tight` on S + mean|z| rstd |g|, whichever is smaller.)  Each test reports its worst err / bound per entry
point and width through gpu_util.report.

Which test reaches what (grid caps and branches of the launchers):
    ln_grid cap 2048 blocks, second / third row per wave, prefetch ... test_fwd[rows 8193, 16389], test_mixed_uniform (8197),
                                                                       test_dropout_fwd (8197)
    ln_grid_bwd cap 256, second / third row per wave, nmean / nrstd .. test_bwd_atomics[rows 1025, 2053], test_mixed_uniform
                                                                       (1029), test_dropout_bwd (1029, no workspace)
    workspace route, ceil(rows / 32) blocks .......................... test_bwd_workspace, test_dropout_bwd (1029, workspace)
    workspace route, 768 cap ......................................... test_bwd_768_block_cap (24581 rows)
    workspace route, ws_floats / per_block cap ....................... test_bwd_workspace_size_cap_and_threshold[exact]
    ws_floats < per_block * 256 -> atomics / CX_ERR_ARG .............. test_bwd_workspace_size_cap_and_threshold[one_short]
    pooled: B blocks / 256 cap, sequence loop wraps .................. test_pooled[...], test_pooled_sequence_loop_wraps[300]
    pooled: workspace, 768 cap, sequence loop wraps .................. test_pooled_sequence_loop_wraps[800]
    CX_LN_DISPATCH default ........................................... test_unsupported_width
    embedding forward: ln_grid cap 2048, second row per wave ......... test_embed_fwd[8197-768]
    embedding backward: ln_grid_bwd cap 256, every wave's second row . test_embed_bwd (1029 tokens)
    sorted embedding backward: 1024-block cap; scatter: 8192-block cap,
        no token / one token (no fold) / fold, += , padding row ...... test_embed_bwd_sorted (4101 tokens, 8200 rows)
"""
import pytest
import torch

from contrastors_amd import _C
from tests import ln_ref as R
from tests.gpu_util import L, S, report
from tests.ln_ref import EPS24, WIDTHS, C

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
POISON = {2: 0x7FA5, 4: 0x7FA5A5A5}         # NaN in bf16 and in fp32
ERR_SHAPE, ERR_ARG = -1, -3
X0_F32, RES_F32, OUT_F32, Z_F32, RMS = 1, 2, 4, 8, 16
_SLABS = []


class Slab:
    """An operand or result: `t` is a slice of a larger allocation with poison either side (16-byte aligned offsets)."""

    def __init__(self, data=None, shape=None, dtype=None, fill=None, name=""):
        if data is not None:
            shape, dtype = tuple(data.shape), data.dtype
        n = 1
        for s in shape:
            n *= s
        self.pad = 8 * (shape[-1] if len(shape) == 2 else 1)
        self.full = torch.empty(n + 2 * self.pad, dtype=dtype, device=DEV)
        self.poison = POISON[self.full.element_size()]
        R.bits(self.full).fill_(self.poison)
        self.t = self.full[self.pad:self.pad + n].view(shape)
        assert self.t.data_ptr() % 16 == 0
        if data is not None:
            self.t.copy_(data)
        elif fill is not None:
            self.t.fill_(fill)
        self.name = name
        _SLABS.append(self)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        b = R.bits(self.full)
        return bool((b[:self.pad] == self.poison).all()) and bool((b[-self.pad:] == self.poison).all())

    def untouched(self):
        return bool((R.bits(self.full) == self.poison).all())


def P(s):
    return None if s is None else s.ptr


def out_slab(shape, dtype, name):
    return Slab(shape=shape, dtype=dtype, name=name)       # poison throughout: an element the kernel skips stays NaN


@pytest.fixture(autouse=True)
def _guards():
    _SLABS.clear()
    yield
    torch.cuda.synchronize()
    bad = [s.name for s in _SLABS if not s.guards_intact()]
    _SLABS.clear()
    assert not bad, f"memory outside the operand slices was written: {bad}"


def guards_ok():
    torch.cuda.synchronize()
    bad = [s.name for s in _SLABS if not s.guards_intact()]
    assert not bad, f"memory outside the operand slices was written: {bad}"


def cols_bound(fam, what, abs_sum):
    return C(fam, what) * EPS24 * abs_sum


# ------------------------------------------------------------------------------------------------------------ forward
def run_fwd(x0, res, g, b, eps, with_z=True):
    rows, d = x0.shape
    s = dict(x0=Slab(x0, name="x0"), res=None if res is None else Slab(res, name="res"), g=Slab(g, name="gamma"),
             b=Slab(b, name="beta"), out=out_slab((rows, d), BF, "out"), z=out_slab((rows, d), BF, "z_out") if with_z else None,
             mean=out_slab((rows,), F32, "mean"), rstd=out_slab((rows,), F32, "rstd"))
    _C.check(L().cx_layernorm_fwd(s["x0"].ptr, P(s["res"]), s["g"].ptr, s["b"].ptr, s["out"].ptr, P(s["z"]), s["mean"].ptr,
                                  s["rstd"].ptr, rows, d, eps, S()), "layernorm_fwd")
    return s


def check_fwd(s, eps, fam="fwd", rms=False, tag="fwd"):
    res = None if s["res"] is None else s["res"].t
    f = R.ln_fwd_ref(s["x0"].t, res, s["g"].t, None if s["b"] is None else s["b"].t, eps, rms=rms)
    r = dict(out=R.check_out(f"{tag}.out", s["out"].t, f, fam), rstd=R.check_rstd(f"{tag}.rstd", s["rstd"].t, f, C(fam, "rstd")))
    if rms:
        assert bool((R.bits(s["mean"].t) == 0).all()), "RMS stores mean = +0 exactly"
    else:
        r["mean"] = R.check_mean(f"{tag}.mean", s["mean"].t, f, C(fam, "mean"))
    if s["z"] is not None:
        z32 = s["x0"].t.float() if res is None else s["x0"].t.float() + res.float()
        assert torch.equal(R.bits(s["z"].t), R.bits(z32.to(s["z"].t.dtype))), "z_out = fp32(x0) + fp32(res), rounded once"
    return r


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("rows", [1, 5, 8193, 16389])
def test_fwd(d, rows):
    """One row; a partial last block; the first row of the second pass (2048 blocks x 4 waves = 8192 rows per pass: the
    prefetch guard is true for exactly one wave); the start of the third pass with a partial block."""
    x0, res, g, b = R.fwd_inputs(rows, d)
    r = check_fwd(run_fwd(x0, res, g, b, 1e-12), 1e-12)
    report("ln_edges.cx_layernorm_fwd", d=d, rows=rows, **r)


@pytest.mark.parametrize("null", ["residual", "z_out"])
def test_fwd_optional_pointers(null):
    rows, d = 8193, 768
    x0, res, g, b = R.fwd_inputs(rows, d)
    s = run_fwd(x0, None if null == "residual" else res, g, b, 1e-12, with_z=null != "z_out")
    report("ln_edges.cx_layernorm_fwd", d=d, rows=rows, null=null, **check_fwd(s, 1e-12))


def test_fwd_constant_rows_at_eps_1e5():
    """Constant rows: var = 0, rstd = rsqrt(eps), xhat ~ 0 and out ~ beta.  (Not at eps = 1e-12: rstd = 1e6 would amplify the
    legitimate fp32 error of the mean beyond any useful bound.)"""
    rows, d, eps = 9, 768, 1e-5
    x0, res, g, b = R.fwd_inputs(rows, d)
    for r_, v in ((2, -4.0), (5, 0.5), (6, 3.0)):
        x0[r_], res[r_] = v, 0.0
    s = run_fwd(x0, res, g, b, eps)
    r = check_fwd(s, eps)
    const = [2, 5, 6]
    f = R.ln_fwd_ref(s["x0"].t, s["res"].t, s["g"].t, s["b"].t, eps)
    assert torch.equal(f.out[const], s["b"].t.double().expand(3, d)), "the reference of a constant row is beta: check_fwd held out to it"
    assert float((s["rstd"].t[const].double() * eps ** 0.5 - 1).abs().max()) < 1e-6
    report("ln_edges.cx_layernorm_fwd", d=d, rows=rows, eps=eps, **r)


# ----------------------------------------------------------------------------------------------------------- backward
def run_bwd(w, *, colsum=False, ws_floats=0, db=True, ex=True, dgamma=True, dbeta=True, prefill=0.0, want_rc=0):
    rows, d = w["z"].shape
    s = dict(da=Slab(w["da"], name="dout_a"), db=Slab(w["db"], name="dout_b") if db else None, z=Slab(w["z"], name="z"),
             g=Slab(w["gamma"], name="gamma"), mean=Slab(w["mean"], name="mean"), rstd=Slab(w["rstd"], name="rstd"),
             ex=Slab(w["ex"], name="dz_extra") if ex else None, dz=out_slab((rows, d), BF, "dz"),
             dgamma=Slab(shape=(d,), dtype=F32, fill=prefill, name="dgamma") if dgamma else None,
             dbeta=Slab(shape=(d,), dtype=F32, fill=prefill, name="dbeta") if dbeta else None,
             cs=Slab(shape=(d,), dtype=F32, fill=prefill, name="colsum") if colsum else None,
             ws=out_slab((ws_floats,), F32, "ws") if ws_floats else None)
    common = (s["da"].ptr, P(s["db"]), s["z"].ptr, s["g"].ptr, s["mean"].ptr, s["rstd"].ptr, P(s["ex"]), s["dz"].ptr, P(s["dgamma"]),
              P(s["dbeta"]))
    if colsum:
        rc = L().cx_layernorm_bwd_colsum(*common, s["cs"].ptr, P(s["ws"]), ws_floats, rows, d, S())
    else:
        rc = L().cx_layernorm_bwd(*common, P(s["ws"]), ws_floats, rows, d, S())
    assert rc == want_rc, rc
    return s


def bwd_ref_of(s, rms=False):
    return R.ln_bwd_ref(s["da"].t, None if s["db"] is None else s["db"].t, s["z"].t, s["g"].t, s["mean"].t, s["rstd"].t,
                        None if s["ex"] is None else s["ex"].t, rms=rms)


def check_bwd(s, ref=None, fam="bwd", prefill=0.0, tag="bwd", dz_key="dz"):
    ref = ref or bwd_ref_of(s)
    r = dict(dz=R.check_result(f"{tag}.dz", s[dz_key].t, ref.dz, ref.scale, C(fam, "dz")))
    if s.get("dgamma") is not None:
        r["dgamma"] = R.check_rows(f"{tag}.dgamma", s["dgamma"].t, ref.dgamma + prefill, cols_bound(fam, "dgamma", ref.dgamma_abs + prefill))
    if s.get("dbeta") is not None:
        r["dbeta"] = R.check_rows(f"{tag}.dbeta", s["dbeta"].t, ref.dbeta + prefill, cols_bound(fam, "dbeta", ref.dbeta_abs + prefill))
    if s.get("cs") is not None:
        st = s[dz_key].t.double()
        r["colsum"] = R.check_rows(f"{tag}.colsum", s["cs"].t, st.sum(0) + prefill, cols_bound(fam, "colsum", st.abs().sum(0) + prefill))
    return r


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("rows", [1, 5, 1023, 1025, 2053])
def test_bwd_atomics(d, rows):
    """No workspace: 256 blocks at most, 1024 rows per pass.  1025 rows: one wave takes a second row and the prefetch carries
    that row's mean / rstd; 2053: a third pass with a partial block."""
    s = run_bwd(R.bwd_inputs(rows, d))
    report("ln_edges.cx_layernorm_bwd", d=d, rows=rows, route="atomics", **check_bwd(s))


@pytest.mark.parametrize("d", WIDTHS)
def test_bwd_workspace(d):
    """Workspace route at 1025 rows (33 blocks of 4 waves: every wave takes 8 or 9 rows), both forms, and the exact relations."""
    rows = 1025
    w = R.bwd_inputs(rows, d)
    ws2, ws3 = 2 * d * 256 + 5, 3 * d * 256 + 5
    at = run_bwd(w)
    a = run_bwd(w, ws_floats=ws2)
    ref = bwd_ref_of(a)
    report("ln_edges.cx_layernorm_bwd", d=d, rows=rows, route="workspace", **check_bwd(a, ref))
    c = run_bwd(w, colsum=True, ws_floats=ws3)
    report("ln_edges.cx_layernorm_bwd_colsum", d=d, rows=rows, **check_bwd(c, ref))
    assert not a["ws"].untouched() and not c["ws"].untouched()
    assert torch.equal(R.bits(at["dz"].t), R.bits(a["dz"].t)), "dz: atomics route == workspace route"
    assert torch.equal(R.bits(a["dz"].t), R.bits(c["dz"].t)), "dz: CS kernel == non-CS kernel"
    a2, c2 = run_bwd(w, ws_floats=ws2), run_bwd(w, colsum=True, ws_floats=ws3)
    for k in ("dgamma", "dbeta"):
        assert torch.equal(a[k].t, a2[k].t) and torch.equal(c[k].t, c2[k].t) and torch.equal(a[k].t, c[k].t), k
    assert torch.equal(c["cs"].t, c2["cs"].t)
    # += : the reduction adds its total to what the target holds, in one fp32 add
    c1 = run_bwd(w, colsum=True, ws_floats=ws3, prefill=1.0)
    for k in ("dgamma", "dbeta", "cs"):
        assert torch.equal(c1[k].t, 1.0 + c[k].t), k
    at1 = run_bwd(w, prefill=1.0)
    check_bwd(at1, ref, prefill=1.0)


def test_bwd_768_block_cap():
    """24581 rows: ceil(rows / 32) = 769 > 768 blocks, so one wave takes a ninth row; d = 256 keeps it small."""
    rows, d = 24581, 256
    w = R.bwd_inputs(rows, d)
    a = run_bwd(w, ws_floats=2 * d * 768)            # exactly 768 partials fit: block 768 would write past the slice
    ref = bwd_ref_of(a)
    report("ln_edges.cx_layernorm_bwd", d=d, rows=rows, route="workspace768", **check_bwd(a, ref))
    c = run_bwd(w, colsum=True, ws_floats=3 * d * 768)
    report("ln_edges.cx_layernorm_bwd_colsum", d=d, rows=rows, **check_bwd(c, ref))
    assert torch.equal(R.bits(a["dz"].t), R.bits(c["dz"].t))


@pytest.mark.parametrize("d", [256, 768])
@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one_short"])
def test_bwd_workspace_size_cap_and_threshold(d, short):
    """9600 rows ask for 300 blocks.  ws_floats = per_block * 256 caps the grid at 256 (a 257th block would write past the
    workspace slice); one float less is below the threshold: cx_layernorm_bwd takes the atomics route and leaves the workspace
    alone, the colsum form returns CX_ERR_ARG with every output untouched."""
    rows = 9600
    w = R.bwd_inputs(rows, d)
    a = run_bwd(w, ws_floats=2 * d * 256 - short)
    ref = bwd_ref_of(a)
    report("ln_edges.cx_layernorm_bwd", d=d, rows=rows, route="ws_cap" if not short else "ws_one_short", **check_bwd(a, ref))
    assert a["ws"].untouched() == bool(short)
    c = run_bwd(w, colsum=True, ws_floats=3 * d * 256 - short, want_rc=ERR_ARG if short else 0)
    if short:
        assert c["dz"].untouched() and c["ws"].untouched()
        assert all(bool((c[k].t == 0).all()) for k in ("dgamma", "dbeta", "cs"))
    else:
        report("ln_edges.cx_layernorm_bwd_colsum", d=d, rows=rows, route="ws_cap", **check_bwd(c, ref))
        a2 = run_bwd(w, ws_floats=2 * d * 256)
        assert torch.equal(a["dgamma"].t, a2["dgamma"].t) and torch.equal(a["dbeta"].t, a2["dbeta"].t)
        assert torch.equal(R.bits(a["dz"].t), R.bits(c["dz"].t))


@pytest.mark.parametrize("null", ["db", "ex", "dgamma", "dbeta"])
def test_bwd_optional_pointers(null):
    rows, d = 1025, 512
    w = R.bwd_inputs(rows, d)
    full = run_bwd(w, colsum=True, ws_floats=3 * d * 256)
    for kw in (dict(), dict(ws_floats=2 * d * 256), dict(colsum=True, ws_floats=3 * d * 256)):
        s = run_bwd(w, **{null: False}, **kw)
        r = check_bwd(s)
        if null in ("dgamma", "dbeta") and kw.get("colsum"):
            other = "dbeta" if null == "dgamma" else "dgamma"
            assert torch.equal(s[other].t, full[other].t) and torch.equal(s["cs"].t, full["cs"].t)
            assert torch.equal(R.bits(s["dz"].t), R.bits(full["dz"].t))
        report("ln_edges.cx_layernorm_bwd" + ("_colsum" if kw.get("colsum") else ""), d=d, rows=rows, null=null, **r)
    if null in ("dgamma", "dbeta"):       # both NULL: no parameter reduction is launched at all
        s = run_bwd(w, dgamma=False, dbeta=False, ws_floats=2 * d * 256)
        check_bwd(s)


# ---------------------------------------------------------------------------------------------------- pooled backward
def run_pooled(pin, mode, normalize, *, colsum, ws_floats, extra_rows=3):
    d, T, B = pin["z"].shape[1], pin["T"], pin["B"]
    zpad = torch.cat([pin["z"], pin["z"][:extra_rows]])              # rows of no sequence after cu[-1]
    stat = lambda v: torch.cat([v, v[:extra_rows]])
    s = dict(demb=Slab(pin["demb"], name="demb"), emb=Slab(pin["emb"], name="emb"), norm=Slab(pin["norm"], name="norm"),
             cu=Slab(pin["cu"], name="cu_seqlens"), z=Slab(zpad, name="z"), g=Slab(pin["gamma"], name="gamma"),
             mean=Slab(stat(pin["mean"]), name="mean"), rstd=Slab(stat(pin["rstd"]), name="rstd"),
             dz=out_slab((T + extra_rows, d), BF, "dz"), dgamma=Slab(shape=(d,), dtype=F32, fill=0.0, name="dgamma"),
             dbeta=Slab(shape=(d,), dtype=F32, fill=0.0, name="dbeta"),
             cs=Slab(shape=(d,), dtype=F32, fill=0.0, name="colsum") if colsum else None,
             ws=out_slab((ws_floats,), F32, "ws") if ws_floats else None)
    _C.check(L().cx_layernorm_bwd_pooled(s["demb"].ptr, s["emb"].ptr, s["norm"].ptr, s["cu"].ptr, B, mode, normalize,
                                         s["z"].ptr, s["g"].ptr, s["mean"].ptr, s["rstd"].ptr, s["dz"].ptr, s["dgamma"].ptr,
                                         s["dbeta"].ptr, P(s["cs"]), P(s["ws"]), ws_floats, T + extra_rows, d, S()), "bwd_pooled")
    return s


def check_pooled(s, pin, mode, normalize, tag):
    T = pin["T"]
    dout = R.pooled_dout_ref(s["demb"].t, s["emb"].t, s["norm"].t, pin["cu"], mode, normalize)
    ref = R.ln_bwd_ref(dout, None, s["z"].t[:T], s["g"].t, s["mean"].t[:T], s["rstd"].t[:T], None)
    assert bool((R.bits(s["dz"].t[T:]) == s["dz"].poison).all()), "dz rows of no sequence stay as they were"
    if mode == 1:                                                      # cls pooling: rows r != 0 come back as exact zeros
        first = torch.zeros(T, dtype=torch.bool, device=DEV)
        first[pin["cu"][:-1][pin["cu"][1:] > pin["cu"][:-1]].long().to(DEV)] = True
        assert bool((R.bits(s["dz"].t[:T][~first]) == 0).all())
    view = dict(s, dz=type("V", (), {"t": s["dz"].t[:T]})())
    return check_bwd(view, ref, fam="pooled", tag=tag)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("normalize", [0, 1])
def test_pooled(d, mode, normalize):
    lens = [1, 2, 3, 4, 5, 0, 9, 130, 7]
    pin = R.pooled_inputs(lens, d)
    a = run_pooled(pin, mode, normalize, colsum=False, ws_floats=0)
    report("ln_edges.cx_layernorm_bwd_pooled", d=d, B=len(lens), mode=mode, normalize=normalize, route="atomics",
           **check_pooled(a, pin, mode, normalize, "pooled"))
    c = run_pooled(pin, mode, normalize, colsum=True, ws_floats=3 * d * 256)
    report("ln_edges.cx_layernorm_bwd_pooled", d=d, B=len(lens), mode=mode, normalize=normalize, route="workspace+colsum",
           **check_pooled(c, pin, mode, normalize, "pooled_cs"))
    assert torch.equal(R.bits(a["dz"].t), R.bits(c["dz"].t))
    c2 = run_pooled(pin, mode, normalize, colsum=True, ws_floats=3 * d * 256)
    assert all(torch.equal(c[k].t, c2[k].t) for k in ("dgamma", "dbeta", "cs"))


@pytest.mark.parametrize("B", [300, 800])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("normalize", [0, 1])
def test_pooled_sequence_loop_wraps(B, mode, normalize):
    """B = 300 without a workspace (256 blocks) and B = 800 with one (768 blocks): `b += gridDim.x` runs a second time for
    the first 44 / 32 blocks, and with lengths cycling through [1, 0, 5, 2, 9] empty sequences fall on wrapped iterations."""
    d = 256
    lens = [[1, 0, 5, 2, 9][i % 5] for i in range(B)]
    pin = R.pooled_inputs(lens, d)
    ws = 3 * d * 768 if B == 800 else 0
    s = run_pooled(pin, mode, normalize, colsum=B == 800, ws_floats=ws)
    report("ln_edges.cx_layernorm_bwd_pooled", d=d, B=B, mode=mode, normalize=normalize, **check_pooled(s, pin, mode, normalize, "pooled"))


# -------------------------------------------------------------------------------------------------------- mixed dtypes
def run_fwd_mixed(x0, res, g, b, eps, flags, with_z=True):
    rows, d = x0.shape
    s = dict(x0=Slab(x0, name="x0"), res=None if res is None else Slab(res, name="res"), g=Slab(g, name="gamma"),
             b=None if b is None else Slab(b, name="beta"), out=out_slab((rows, d), F32 if flags & OUT_F32 else BF, "out"),
             z=out_slab((rows, d), F32 if flags & Z_F32 else BF, "z_out") if with_z else None,
             mean=out_slab((rows,), F32, "mean"), rstd=out_slab((rows,), F32, "rstd"))
    _C.check(L().cx_layernorm_fwd_mixed(s["x0"].ptr, P(s["res"]), s["g"].ptr, P(s["b"]), s["out"].ptr, P(s["z"]), s["mean"].ptr,
                                        s["rstd"].ptr, rows, d, eps, flags, S()), "fwd_mixed")
    return s


def run_bwd_mixed(w, flags, *, ex=True, dres=True, dbeta=True):
    rows, d = w["z"].shape
    s = dict(da=Slab(w["da"], name="dout"), db=None, z=Slab(w["z"], name="z"), g=Slab(w["gamma"], name="gamma"),
             mean=Slab(w["mean"], name="mean"), rstd=Slab(w["rstd"], name="rstd"), ex=Slab(w["ex"], name="dz_extra") if ex else None,
             dx0=out_slab((rows, d), F32 if flags & X0_F32 else BF, "dx0"),
             dres=out_slab((rows, d), F32 if flags & RES_F32 else BF, "dres") if dres else None,
             dgamma=Slab(shape=(d,), dtype=F32, fill=0.0, name="dgamma"),
             dbeta=Slab(shape=(d,), dtype=F32, fill=0.0, name="dbeta") if dbeta else None)
    _C.check(L().cx_layernorm_bwd_mixed(s["da"].ptr, s["z"].ptr, s["g"].ptr, s["mean"].ptr, s["rstd"].ptr, P(s["ex"]), s["dx0"].ptr,
                                        P(s["dres"]), s["dgamma"].ptr, P(s["dbeta"]), rows, d, flags, S()), "bwd_mixed")
    return s


def mixed_case(rows, d, flags, *, small):
    """Forward and backward of one flag combination; `small` selects the optional-pointer variant: NULL residual-gradient and
    no dz_extra, against both present."""
    rms = bool(flags & RMS)
    dx, dr = (F32 if flags & X0_F32 else BF), (F32 if flags & RES_F32 else BF)
    x0, res, g, b = R.fwd_inputs(rows[0], d, dtype_x=dx, dtype_r=dr)
    fam = "fwd_rms" if rms else ("fwd_f32" if flags & (X0_F32 | RES_F32) else "fwd")
    s = run_fwd_mixed(x0, res, g, None if rms else b, 1e-12, flags)
    r = check_fwd(s, 1e-12, fam=fam, rms=rms, tag=f"fwd_mixed[{flags}]")
    report("ln_edges.cx_layernorm_fwd_mixed", d=d, rows=rows[0], flags=flags, **r)
    w = R.bwd_inputs(rows[1], d, dtype_dy=F32 if flags & OUT_F32 else BF, dtype_z=F32 if flags & Z_F32 else BF, rms=rms)
    t = run_bwd_mixed(w, flags, ex=not small, dres=not small, dbeta=not rms)
    bfam = "bwd_rms" if rms else "bwd"
    ref = bwd_ref_of(t, rms=rms)
    r = check_bwd(t, ref, fam=bfam, tag=f"bwd_mixed[{flags}].dx0", dz_key="dx0")
    if t["dres"] is not None:       # the same values, each rounded to its own dtype
        R.check_result(f"bwd_mixed[{flags}].dres", t["dres"].t, ref.dz, ref.scale, C(bfam, "dz"))
        lo, hi = (t["dx0"].t, t["dres"].t) if t["dx0"].t.dtype == BF else (t["dres"].t, t["dx0"].t)
        assert torch.equal(R.bits(lo), R.bits(hi.to(lo.dtype))), "dx0 and dres carry one value"
    report("ln_edges.cx_layernorm_bwd_mixed", d=d, rows=rows[1], flags=flags, **r)


@pytest.mark.parametrize("flags", range(32))
def test_mixed_every_flag_combination(flags):
    mixed_case((9, 9), 512, flags, small=bool(flags & 1) ^ bool(flags & 4))


UNIFORM = {"bf16_bf16": 0, "f32_bf16": X0_F32 | RES_F32, "bf16_f32": OUT_F32 | Z_F32, "f32_f32": X0_F32 | RES_F32 | OUT_F32 | Z_F32}


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("io", list(UNIFORM))
@pytest.mark.parametrize("rms", [0, RMS])
def test_mixed_uniform(d, io, rms):
    """Operands (x0, residual) and results (out, z) each uniformly bf16 or fp32: 5 rows, and 8197 / 1029 rows where a wave of
    the forward (2048 blocks) / backward (256 blocks) takes a second row and the last block is partial."""
    mixed_case((5, 5), d, UNIFORM[io] | rms, small=True)
    mixed_case((8197, 1029), d, UNIFORM[io] | rms, small=False)


# ------------------------------------------------------------------------------------------------------------ dropout
SEED, OFFSET, SITE = 1234567, 40, 3


def run_drop_fwd(x0, res, g, b, p):
    rows, d = x0.shape
    s = dict(x0=Slab(x0, name="x0"), res=Slab(res, name="res"), g=Slab(g, name="gamma"), b=Slab(b, name="beta"),
             out=out_slab((rows, d), BF, "out"), z=out_slab((rows, d), BF, "z_out"), mean=out_slab((rows,), F32, "mean"),
             rstd=out_slab((rows,), F32, "rstd"))
    _C.check(L().cx_dropout_add_layernorm_fwd(s["x0"].ptr, s["res"].ptr, s["g"].ptr, s["b"].ptr, s["out"].ptr, s["z"].ptr, s["mean"].ptr,
                                              s["rstd"].ptr, rows, d, 1e-12, p, SEED, OFFSET, SITE, S()), "drop_fwd")
    s["mask"] = R.recover_mask(s["z"].t, s["res"].t, s["x0"].t, p)
    return s


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_fwd(d, p):
    masks = {}
    for rows in (5, 8197):
        x0, res, g, b = R.drop_inputs(8197, d)
        x0, res = x0[:rows].contiguous(), res[:rows].contiguous()
        s = run_drop_fwd(x0, res, g, b, p)
        m = masks[rows] = s["mask"]
        zin = s["x0"].t.double() * m / (1 - p)
        f = R.ln_fwd_ref(zin, s["res"].t, s["g"].t, s["b"].t, 1e-12)
        # z = fma(x0, fl(1 / (1 - p)), res) rounded to bf16: fl(1 / (1 - p)) is within 2^-24 relative (two roundings), the fma adds
        # one rounding of z -- 3 * 2^-24 (|x0| / (1 - p) + |res|) bounds them with room
        R.check_rows("drop.z", s["z"].t, f.z, 0.5 * R.bf16_ulp(f.z) + 3 * EPS24 * (zin.abs() + s["res"].t.double().abs()))
        r = dict(out=R.check_out("drop.out", s["out"].t, f, "fwd_drop"), mean=R.check_mean("drop.mean", s["mean"].t, f, C("fwd_drop", "mean")),
                 rstd=R.check_rstd("drop.rstd", s["rstd"].t, f, C("fwd_drop", "rstd")))
        if rows > 1000:
            assert abs(float(m.double().mean()) - (1 - p)) < 0.002
        report("ln_edges.cx_dropout_add_layernorm_fwd", d=d, rows=rows, p=p, **r)
    # the mask is indexed by element position: it cannot depend on the launch
    assert torch.equal(masks[8197][:5], masks[5])


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_bwd(d, p):
    for rows, ws_floats, colsum in ((5, 0, False), (1029, 0, False), (1029, 2 * d * 256, False), (1029, 3 * d * 256, True)):
        x0, res, g, b = R.drop_inputs(rows, d)
        mask = run_drop_fwd(x0, res, g, b, p)["mask"]
        w = R.bwd_inputs(rows, d)
        s = dict(da=Slab(w["da"], name="dout_a"), db=Slab(w["db"], name="dout_b"), z=Slab(w["z"], name="z"), g=Slab(w["gamma"], name="gamma"),
                 mean=Slab(w["mean"], name="mean"), rstd=Slab(w["rstd"], name="rstd"), ex=None, dz=out_slab((rows, d), BF, "dz"),
                 dx0=out_slab((rows, d), BF, "dx0"), dgamma=Slab(shape=(d,), dtype=F32, fill=0.0, name="dgamma"),
                 dbeta=Slab(shape=(d,), dtype=F32, fill=0.0, name="dbeta"),
                 cs=Slab(shape=(d,), dtype=F32, fill=0.0, name="colsum") if colsum else None,
                 ws=out_slab((ws_floats,), F32, "ws") if ws_floats else None)
        args = (s["da"].ptr, s["db"].ptr, s["z"].ptr, s["g"].ptr, s["mean"].ptr, s["rstd"].ptr, s["dz"].ptr, s["dx0"].ptr, s["dgamma"].ptr,
                s["dbeta"].ptr)
        tail = (P(s["ws"]), ws_floats, rows, d, p, SEED, OFFSET, SITE, S())
        if colsum:
            _C.check(L().cx_dropout_add_layernorm_bwd_colsum(*args, s["cs"].ptr, *tail), "drop_bwd_colsum")
        else:
            _C.check(L().cx_dropout_add_layernorm_bwd(*args, *tail), "drop_bwd")
        ref = bwd_ref_of(s)
        cs = s.pop("cs")
        r = check_bwd(s, ref, fam="bwd_drop", tag="drop_bwd")
        keep = mask.double() / (1 - p)
        r["dx0"] = R.check_result("drop_bwd.dx0", s["dx0"].t, ref.dz * keep, ref.scale * keep, C("bwd_drop", "dx0"))
        assert bool((s["dx0"].t[~mask] == 0).all()), "dx0 is exactly zero wherever the mask is"
        if cs is not None:
            r["colsum"] = R.check_colsum("drop_bwd.colsum", cs.t, s["dx0"].t, C("bwd_drop", "colsum"))
        report("ln_edges.cx_dropout_add_layernorm_bwd" + ("_colsum" if colsum else ""), d=d, rows=rows, p=p, ws=ws_floats, **r)
        guards_ok()


# ---------------------------------------------------------------------------------------------------------- embedding
def embed_slabs(e, use_pos=True):
    """The operands of the embedding kernels.  The integer operands are plain tensors, not slabs: a poisoned index would
    not poison a result, it would send a read anywhere."""
    s = dict(word=Slab(e["word"], name="word"), type=Slab(e["type"], name="type"), pos=Slab(e["pos"], name="pos") if use_pos else None,
             g=Slab(e["gamma"], name="gamma"), b=Slab(e["beta"], name="beta"), ids=e["ids"].to(DEV), indices=e["indices"].to(DEV))
    s["z"], s["tid"], s["p"] = R.embed_z(s["word"].t, s["type"].t, None if s["pos"] is None else s["pos"].t, s["ids"], s["indices"],
                                         e["seq"])
    return s


@pytest.mark.parametrize("use_pos", [1, 0], ids=["pos", "nopos"])
@pytest.mark.parametrize("T,d", R.EMBED_FWD_SHAPES)
def test_embed_fwd(T, d, use_pos):
    """77 tokens at every width, and 8197 tokens at d = 768: 2048 blocks x 4 waves take 8192, so a wave takes a second
    token; with and without position embeddings."""
    e = R.embed_fwd_inputs(T, d)
    s = embed_slabs(e, use_pos)
    out, mean, rstd = out_slab((T, d), BF, "out"), out_slab((T,), F32, "mean"), out_slab((T,), F32, "rstd")
    _C.check(L().cx_embed_ln_fwd(s["ids"].data_ptr(), s["indices"].data_ptr(), s["word"].ptr, s["type"].ptr, P(s["pos"]), s["g"].ptr,
                                 s["b"].ptr, out.ptr, mean.ptr, rstd.ptr, T, e["seq"], d, 1e-12, S()), "embed_ln_fwd")
    f = R.ln_fwd_ref(s["z"], None, s["g"].t, s["b"].t, 1e-12)
    report("ln_edges.cx_embed_ln_fwd", d=d, T=T, pos=use_pos, out=R.check_out("embed.out", out.t, f, "embed_fwd"),
           mean=R.check_mean("embed.mean", mean.t, f, C("embed_fwd", "mean")),
           rstd=R.check_rstd("embed.rstd", rstd.t, f, C("embed_fwd", "rstd")))


def embed_bwd_operands(e, s, d, *, two, dpos, dword_fill=0.0):
    """dout_a / dout_b, the statistics the forward would hand over (fp64 of the exact z, rounded to fp32), zeroed
    accumulators, and the fp64 reference of dz."""
    T = e["T"]
    st = R.ln_fwd_ref(s["z"], None, s["g"].t, None, 1e-12)
    o = dict(da=Slab(e["da"], name="dout_a"), db=Slab(e["db"], name="dout_b") if two else None,
             mean=Slab(st.mean.float(), name="mean"), rstd=Slab(st.rstd.float(), name="rstd"),
             dword=Slab(shape=(e["vocab"], d), dtype=F32, fill=dword_fill, name="dword"),
             dtype0=Slab(shape=(d,), dtype=F32, fill=0.0, name="dtype0"),
             dpos=Slab(shape=(e["seq"], d), dtype=F32, fill=0.0, name="dpos") if dpos else None,
             dgamma=Slab(shape=(d,), dtype=F32, fill=0.0, name="dgamma"), dbeta=Slab(shape=(d,), dtype=F32, fill=0.0, name="dbeta"))
    o["ref"] = R.ln_bwd_ref(o["da"].t, None if o["db"] is None else o["db"].t, s["z"], s["g"].t, o["mean"].t, o["rstd"].t, None)
    o["args"] = (o["da"].ptr, P(o["db"]), s["ids"].data_ptr(), s["indices"].data_ptr(), s["word"].ptr, s["type"].ptr, P(s["pos"]),
                 s["g"].ptr, o["mean"].ptr, o["rstd"].ptr, o["dword"].ptr, o["dtype0"].ptr, P(o["dpos"]), o["dgamma"].ptr,
                 o["dbeta"].ptr, T, e["seq"], d, R.EMBED_PAD)
    return o


def check_embed_bwd(e, s, o, tag, dword_fill=0.0):
    """dgamma / dbeta as everywhere; dtype0, dpos, dword against the scatter-added fp64 dz rows."""
    ref, fam = o["ref"], "embed_bwd"
    sc = lambda what, want, scale: R.check_rows(f"{tag}.{what}", o[what].t, want, cols_bound(fam, "scatter", scale))
    r = dict(dgamma=R.check_rows(f"{tag}.dgamma", o["dgamma"].t, ref.dgamma, cols_bound(fam, "dgamma", ref.dgamma_abs)),
             dbeta=R.check_rows(f"{tag}.dbeta", o["dbeta"].t, ref.dbeta, cols_bound(fam, "dbeta", ref.dbeta_abs)),
             dtype0=sc("dtype0", ref.dz.sum(0), ref.scale.sum(0)))
    if o["dpos"] is not None:
        r["dpos"] = sc("dpos", R.scatter_rows(ref.dz, s["p"], e["seq"]), R.scatter_rows(ref.scale, s["p"], e["seq"]))
    real = s["tid"] != R.EMBED_PAD
    assert int((~real).sum()) > 0, "the padding id occurs"
    want = R.scatter_rows(ref.dz[real], s["tid"][real], e["vocab"]) + dword_fill
    r["dword"] = sc("dword", want, R.scatter_rows(ref.scale[real], s["tid"][real], e["vocab"]) + abs(dword_fill))
    fill_bits = R.bits(torch.tensor([dword_fill], dtype=F32))[0].item()
    assert bool((R.bits(o["dword"].t[R.EMBED_PAD]) == fill_bits).all()), "nn.Embedding(padding_idx): that row gets no gradient"
    return r


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("null", ["none", "dout_b", "dpos", "pos_emb"])
def test_embed_bwd(d, null):
    """1029 tokens on 256 blocks x 4 waves: every wave takes a second token and five take a third; the word rows by fp32
    atomics (300 rows: they collide).  NULL one at a time: dout_b, dpos (with positions in z), pos_emb (and with it dpos)."""
    e = R.embed_bwd_inputs(d)
    s = embed_slabs(e, use_pos=null != "pos_emb")
    o = embed_bwd_operands(e, s, d, two=null != "dout_b", dpos=null not in ("dpos", "pos_emb"))
    _C.check(L().cx_embed_ln_bwd(*o["args"], S()), "embed_ln_bwd")
    report("ln_edges.cx_embed_ln_bwd", d=d, T=e["T"], null=null, **check_embed_bwd(e, s, o, "embed_bwd"))


def sorted_scatter_of(dz, tid, fill, vocab):
    """embed_scatter_sorted_kernel's sum on the host, in its order, from the fp32 rows it read: wave w adds the rows of its
    vocabulary row's tokens w, w + 4, ... (token order) to 0, the four sums fold as ((w0 + w1) + w2) + w3, and the row adds
    that once.  fp32 adds are correctly rounded everywhere: bit-exact."""
    dz, tid = dz.cpu(), tid.cpu()
    want = torch.full((vocab, dz.shape[1]), fill, dtype=F32)
    order = torch.sort(tid, stable=True).indices
    counts = torch.bincount(tid, minlength=vocab).tolist()
    at = 0
    for v, n in enumerate(counts):
        toks = order[at:at + n]
        at += n
        if n == 0 or v == R.EMBED_PAD:
            continue
        waves = []
        for w in range(4):
            acc = torch.zeros(dz.shape[1], dtype=F32)
            for t in toks[w::4].tolist():
                acc = acc + dz[t]
            waves.append(acc)
        want[v] += waves[0] if n <= 1 else ((waves[0] + waves[1]) + waves[2]) + waves[3]
    return want, counts


@pytest.mark.parametrize("d", [256, 768])
def test_embed_bwd_sorted(d):
    """4101 tokens on 1024 blocks x 4 waves (a wave's second token), 8200 vocabulary rows on the scatter's 8192 blocks (the
    first 8 take two rows, both with tokens), rows of 0 / 1 / 3 / 9 / 40 tokens, the padding id present, dword pre-filled:
    the fp32 row gradients in the scratch against fp64, dword against the fp64 scatter AND bit for bit against the
    kernel's own order of summation, and bit-identical from run to run."""
    e = R.embed_sorted_inputs(d)
    s = embed_slabs(e)
    T, V, fill = e["T"], e["vocab"], 1.0
    sids, perm = torch.sort(s["tid"].to(torch.int32), stable=True)
    perm = perm.to(torch.int32)
    runs = []
    for _ in range(2):
        o = embed_bwd_operands(e, s, d, two=True, dpos=True, dword_fill=fill)
        scratch = out_slab((T, d), F32, "dz_scratch")
        _C.check(L().cx_embed_ln_bwd_sorted(*o["args"], V, sids.data_ptr(), perm.data_ptr(), scratch.ptr, S()), "embed_ln_bwd_sorted")
        runs.append((o, scratch))
    o, scratch = runs[0]
    assert torch.equal(R.bits(o["dword"].t), R.bits(runs[1][0]["dword"].t)), "the sorted reduction is bit-reproducible"
    assert torch.equal(R.bits(scratch.t), R.bits(runs[1][1].t))
    r = check_embed_bwd(e, s, o, "embed_sorted", dword_fill=fill)
    r["dz"] = R.check_result("embed_sorted.dz_scratch", scratch.t, o["ref"].dz, o["ref"].scale, C("embed_bwd", "dz"))
    want, counts = sorted_scatter_of(scratch.t, s["tid"], fill, V)
    assert counts[5] >= 40 and counts[8195] >= 9 and 2 <= counts[7] <= 4 and 0 in counts and 1 in counts
    assert all(counts[v] > 0 for v in (0, 1, 2, 4, 5, 6, 7)) and all(c > 0 for c in counts[8192:]), "both rows of a two-row block"
    assert torch.equal(R.bits(o["dword"].t.cpu()), R.bits(want)), "dword += the rows in the kernel's order, one add per row"
    report("ln_edges.cx_embed_ln_bwd_sorted", d=d, T=T, vocab=V, **r)


# -------------------------------------------------------------------------------------------------- unsupported width
@pytest.mark.parametrize("d", [384, 1280])
def test_unsupported_width(d):
    """CX_LN_DISPATCH has no instance for d: CX_ERR_SHAPE from every entry point, nothing launched, outputs untouched."""
    rows = 9
    mk = lambda dt=BF: Slab(torch.ones(rows, d).to(dt), name="in")
    vec, stat = Slab(torch.ones(d), name="vec"), Slab(torch.ones(rows), name="stat")
    outs = [out_slab((rows, d), BF, "o0"), out_slab((rows, d), BF, "o1"), out_slab((rows,), F32, "o2"), out_slab((rows,), F32, "o3"),
            out_slab((d,), F32, "o4"), out_slab((d,), F32, "o5"), out_slab((d,), F32, "o6"), out_slab((3 * d * 256,), F32, "ws")]
    o0, o1, o2, o3, o4, o5, o6, ws = (o.ptr for o in outs)
    a, b_, c = mk(), mk(), mk()
    cu = Slab(torch.tensor([0, 4, 9], dtype=torch.int32), name="cu_seqlens")
    emb, nrm = Slab(torch.ones(2, d), name="emb"), Slab(torch.ones(2), name="norm")
    wsn = 3 * d * 256
    rcs = dict(
        fwd=L().cx_layernorm_fwd(a.ptr, b_.ptr, vec.ptr, vec.ptr, o0, o1, o2, o3, rows, d, 1e-12, S()),
        bwd=L().cx_layernorm_bwd(a.ptr, b_.ptr, c.ptr, vec.ptr, stat.ptr, stat.ptr, None, o0, o4, o5, None, 0, rows, d, S()),
        bwd_ws=L().cx_layernorm_bwd(a.ptr, b_.ptr, c.ptr, vec.ptr, stat.ptr, stat.ptr, None, o0, o4, o5, ws, wsn, rows, d, S()),
        bwd_colsum=L().cx_layernorm_bwd_colsum(a.ptr, b_.ptr, c.ptr, vec.ptr, stat.ptr, stat.ptr, None, o0, o4, o5, o6, ws, wsn, rows, d, S()),
        pooled=L().cx_layernorm_bwd_pooled(emb.ptr, emb.ptr, nrm.ptr, cu.ptr, 2, 0, 1, c.ptr, vec.ptr, stat.ptr, stat.ptr, o0, o4, o5,
                                           o6, ws, wsn, rows, d, S()),
        pooled_atomics=L().cx_layernorm_bwd_pooled(emb.ptr, emb.ptr, nrm.ptr, cu.ptr, 2, 1, 0, c.ptr, vec.ptr, stat.ptr, stat.ptr, o0,
                                                   o4, o5, None, None, 0, rows, d, S()),
        fwd_mixed=L().cx_layernorm_fwd_mixed(a.ptr, b_.ptr, vec.ptr, vec.ptr, o0, o1, o2, o3, rows, d, 1e-12, 0, S()),
        bwd_mixed=L().cx_layernorm_bwd_mixed(a.ptr, c.ptr, vec.ptr, stat.ptr, stat.ptr, None, o0, o1, o4, o5, rows, d, 0, S()),
        drop_fwd=L().cx_dropout_add_layernorm_fwd(a.ptr, b_.ptr, vec.ptr, vec.ptr, o0, o1, o2, o3, rows, d, 1e-12, 0.1, SEED, OFFSET, SITE, S()),
        drop_bwd=L().cx_dropout_add_layernorm_bwd(a.ptr, b_.ptr, c.ptr, vec.ptr, stat.ptr, stat.ptr, o0, o1, o4, o5, None, 0, rows, d, 0.1,
                                                  SEED, OFFSET, SITE, S()),
        drop_bwd_colsum=L().cx_dropout_add_layernorm_bwd_colsum(a.ptr, b_.ptr, c.ptr, vec.ptr, stat.ptr, stat.ptr, o0, o1, o4, o5, o6, ws, wsn,
                                                                rows, d, 0.1, SEED, OFFSET, SITE, S()),
    )
    assert all(rc == ERR_SHAPE for rc in rcs.values()), rcs
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), [o.name for o in outs if not o.untouched()]
