"""tests/ln_ref.py is itself checked here, on the CPU: the fp64 reference against torch's fp64 LayerNorm under autograd, the
row-wise checker against planted errors, and the constants C_MEAS of the GPU bounds against an fp32 emulation of the kernels'
arithmetic (fp32 statistics, the same formulas, one final bf16 rounding) -- measured against the reference, never a kernel."""
import pytest
import torch
import torch.nn.functional as F

from tests import ln_ref as R
from tests.ln_ref import EPS24, WIDTHS

# Row counts of the measurement.  The backward families: the small row counts of tests/test_layernorm_edges_gpu.py.  The
# forward families: also its largest ones, because err / (2^-24 S) of the forward has a heavy tail -- the row-wide error of the
# mean meets elements whose S = |xhat g| + |b| happens to be tiny, and the worst of N such elements grows like sqrt(N) -- so a
# maximum over fewer elements than the GPU test checks would not bound it.
MEASURE_ROWS = (5, 1025, 2053)
FWD_ROWS = {"fwd": (5, 16389), "fwd_f32": (5, 8197), "fwd_rms": (5, 8197), "fwd_drop": (5, 8197)}
POOL_LENS = ([1, 2, 3, 4, 5, 0, 9, 130, 7], [1, 0, 5, 2, 9] * 60)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


# ------------------------------------------------------------------------------------------- reference vs fp64 autograd
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("with_res,with_b,with_extra", [(True, True, True), (False, False, False), (True, False, True),
                                                        (False, True, False)])
def test_reference_matches_fp64_autograd(d, with_res, with_b, with_extra):
    rows = 37
    x0, res, gamma, beta = R.fwd_inputs(rows, d)
    bw = R.bwd_inputs(rows, d)
    eps = 1e-5                                         # (any eps: this compares two fp64 computations)
    zr = (x0.double() + (res.double() if with_res else 0)).requires_grad_()
    gr, br = gamma.double().requires_grad_(), beta.double().requires_grad_()
    out = F.layer_norm(zr, (d,), gr, br, eps)
    f = R.ln_fwd_ref(x0, res if with_res else None, gamma, beta, eps)
    assert torch.equal(f.z, zr.detach())
    assert _rel(f.out, out.detach()) < 1e-12
    assert _rel(f.mean, zr.detach().mean(-1)) < 1e-12
    assert _rel(f.rstd, 1 / torch.sqrt(zr.detach().var(-1, unbiased=False) + eps)) < 1e-12
    dy = bw["da"].double() + (bw["db"].double() if with_b else 0)
    out.backward(dy)
    b = R.ln_bwd_ref(bw["da"], bw["db"] if with_b else None, f.z, gamma, f.mean, f.rstd, bw["ex"] if with_extra else None)
    want_dz = zr.grad + (bw["ex"].double() if with_extra else 0)
    assert _rel(b.dz, want_dz) < 1e-12 and _rel(b.dgamma, gr.grad) < 1e-12 and _rel(b.dbeta, br.grad) < 1e-12
    assert bool((b.scale >= b.dz.abs() * (1 - 1e-12)).all()), "S bounds |dz| (triangle inequality)"


@pytest.mark.parametrize("d", WIDTHS)
def test_rms_reference_matches_the_definition_and_fp64_autograd(d):
    rows, eps = 29, 1e-6
    x0, res, gamma, beta = R.fwd_inputs(rows, d)
    bw = R.bwd_inputs(rows, d, rms=True)
    zr = (x0.double() + res.double()).requires_grad_()
    gr = gamma.double().requires_grad_()
    out = zr * torch.rsqrt((zr * zr).mean(-1, keepdim=True) + eps) * gr
    f = R.ln_fwd_ref(x0, res, gamma, None, eps, rms=True)
    assert _rel(f.out, out.detach()) < 1e-12 and bool((f.mean == 0).all())
    fb = R.ln_fwd_ref(x0, res, gamma, beta, eps, rms=True)
    assert _rel(fb.out, out.detach() + beta.double()) < 1e-12
    out.backward(bw["da"].double())
    b = R.ln_bwd_ref(bw["da"], None, f.z, gamma, f.mean, f.rstd, None, rms=True)
    assert _rel(b.dz, zr.grad) < 1e-12 and _rel(b.dgamma, gr.grad) < 1e-12 and _rel(b.dbeta, bw["da"].double().sum(0)) < 1e-12


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("normalize", [0, 1])
def test_pooled_dout_reference_matches_fp64_autograd(mode, normalize):
    lens, d = [3, 0, 1, 6], 256
    p = R.pooled_inputs(lens, d)
    h = torch.randn(p["T"], d, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).requires_grad_()
    keep = [i for i, ln in enumerate(lens) if ln > 0]
    cu = p["cu"].tolist()
    pooled = torch.stack([h[cu[i]] if mode == 1 else h[cu[i]:cu[i + 1]].mean(0) for i in keep])
    nrm = pooled.norm(dim=-1)
    emb = pooled / nrm[:, None] if normalize else pooled
    emb.backward(p["demb"].double()[keep])
    full_emb, full_nrm = torch.zeros(len(lens), d, dtype=torch.float64), torch.ones(len(lens), dtype=torch.float64)
    full_emb[keep], full_nrm[keep] = emb.detach(), nrm.detach()
    dout = R.pooled_dout_ref(p["demb"], full_emb, full_nrm, p["cu"], mode, normalize)
    assert _rel(dout, h.grad) < 1e-12


def test_bf16_helpers():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 255.0, 256.0, 1e-3, 0.0], dtype=torch.float64)
    assert R.bf16_ulp(x).tolist()[:7] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 1.0, 2.0]
    v = torch.randn(100000, dtype=torch.float32, generator=torch.Generator().manual_seed(0)) * 37
    assert torch.equal(R.bf16_round(v.double()), v.to(torch.bfloat16).double())      # fp32 -> bf16 is one rounding too
    tie = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert R.bf16_round(tie).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]         # ties to even; one rounding, not two


# ------------------------------------------------------------------------------------------------------ fp32 emulation
def emu_fwd(x0, res, gamma, beta, eps, rms=False, keep=None):
    """ln_fwd_kernel / ln_fwd_mixed_kernel / ln_fwd_drop_kernel in fp32 torch: returns z, mean, rstd, out (fp32, unrounded)."""
    z = x0.float()
    if keep is not None:
        z = z * keep
    if res is not None:
        z = z + res.float()
    d = z.shape[-1]
    mean = torch.zeros(z.shape[0]) if rms else z.sum(-1) / d
    c = z - mean[:, None]
    rstd = torch.rsqrt((c * c).sum(-1) / d + torch.tensor(eps, dtype=torch.float32))
    out = c * rstd[:, None] * gamma
    if beta is not None:
        out = out + beta
    return z, mean, rstd, out


def emu_bwd(dy, z, gamma, mean, rstd, ex, rms=False):
    """The shared arithmetic of the backward kernels on an fp32 dy: dz (fp32, unrounded), dgamma, dbeta."""
    d = z.shape[-1]
    xh = (z.float() - mean[:, None]) * rstd[:, None]
    w = gamma * dy
    s1 = (w * xh).sum(-1, keepdim=True) / d
    s2 = torch.zeros_like(s1) if rms else w.sum(-1, keepdim=True) / d
    o = (w - s1 * xh - s2) * rstd[:, None]
    if ex is not None:
        o = o + ex.float()
    return o, (dy * xh).sum(0), dy.sum(0)


def emu_pooled_dout(p, mode, normalize):
    """dout rows in fp32 as ln_bwd_pooled_kernel builds them."""
    demb, emb, norm, cu = p["demb"], p["emb"], p["norm"], p["cu"].tolist()
    dout = torch.zeros(p["T"], demb.shape[-1])
    for b in range(p["B"]):
        t0, ln = cu[b], cu[b + 1] - cu[b]
        if ln <= 0:
            continue
        g = demb[b]
        if normalize:
            g = (g - emb[b] * (demb[b] * emb[b]).sum()) * (1 / norm[b].clamp(min=1e-12))
        g = g * (torch.tensor(1.0) if mode == 1 else 1 / torch.tensor(float(ln)))
        if mode == 1:
            dout[t0] = g
        else:
            dout[t0:t0 + ln] = g
    return dout


def _ratio(err, scale):
    return torch.where(scale > 0, err / (EPS24 * scale).clamp(min=1e-300),
                       torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def ratio_result(got32, ref, scale, stored_dtype=torch.bfloat16):
    """Worst err / (2^-24 S) of an fp32 value before its rounding, and of its bf16 rounding beyond 0.5 ulp(ref)."""
    pre = _ratio((got32.double() - ref).abs(), scale).max()
    if stored_dtype != torch.bfloat16:
        return float(pre)
    post = _ratio(((got32.to(torch.bfloat16).double() - ref).abs() - 0.5 * R.bf16_ulp(ref)).clamp(min=0), scale).max()
    return float(max(pre, post))


def ratio_stats(mean32, rstd32, f):
    m = _ratio((mean32.double() - f.mean).abs(), f.z.abs().mean(-1)).max()
    r = _ratio((rstd32.double() - f.rstd).abs(), f.rstd.abs()).max()
    return float(m), float(r)


def ratio_cols(got32, ref, abs_sum):
    return float(_ratio((got32.double() - ref).abs(), abs_sum).max())


def measure():
    """C_meas of every family over MEASURE_ROWS x WIDTHS (and POOL_LENS; the embedding families: the shapes of their GPU
    tests), on the inputs of the GPU tests."""
    m = {k: dict.fromkeys(v, 0.0) for k, v in R.C_MEAS.items()}

    def up(fam, **kw):
        for k, v in kw.items():
            m[fam][k] = max(m[fam][k], v)

    for d in WIDTHS:
        # plain forward (bf16 operands), and the mixed kernel on fp32 operands (z = fp32 sum: one more rounding)
        for fam, dt in (("fwd", torch.bfloat16), ("fwd_f32", torch.float32)):
            for rows in FWD_ROWS[fam]:
                x0, res, g, b = R.fwd_inputs(rows, d, dtype_x=dt, dtype_r=dt)
                f = R.ln_fwd_ref(x0, res, g, b, 1e-12)
                _, mean, rstd, out = emu_fwd(x0, res, g, b, 1e-12)
                cm, cr = ratio_stats(mean, rstd, f)
                up(fam, out=ratio_result(out, f.out, f.scale, dt), out_tight=ratio_result(out, f.out, f.scale_tight, dt), mean=cm, rstd=cr)
        for dt in (torch.bfloat16, torch.float32):
            for rows in FWD_ROWS["fwd_rms"]:
                x0, res, g, b = R.fwd_inputs(rows, d, dtype_x=dt, dtype_r=dt)
                f = R.ln_fwd_ref(x0, res, g, None, 1e-12, rms=True)
                _, mean, rstd, out = emu_fwd(x0, res, g, None, 1e-12, rms=True)
                up("fwd_rms", out=ratio_result(out, f.out, f.scale, dt), rstd=ratio_stats(mean, rstd, f)[1])
        for p in (0.1, 0.5):
            for rows in FWD_ROWS["fwd_drop"]:
                x0, res, g, b = R.drop_inputs(rows, d)
                mask = torch.rand(rows, d, generator=torch.Generator().manual_seed(d + rows)) >= p
                keep32 = mask.float() * (1 / (1 - torch.tensor(p, dtype=torch.float32)))
                f = R.ln_fwd_ref(x0.double() * mask / (1 - p), res, g, b, 1e-12)
                _, mean, rstd, out = emu_fwd(x0, res, g, b, 1e-12, keep=keep32)
                cm, cr = ratio_stats(mean, rstd, f)
                up("fwd_drop", out=ratio_result(out, f.out, f.scale), out_tight=ratio_result(out, f.out, f.scale_tight), mean=cm, rstd=cr)
        for rows in MEASURE_ROWS:
            for dt in (torch.bfloat16, torch.float32):
                for rms, fam in ((False, "bwd"), (True, "bwd_rms")):
                    w = R.bwd_inputs(rows, d, dtype_dy=dt, dtype_z=dt, rms=rms)
                    for two in (True, False):
                        db_, ex = (w["db"], w["ex"]) if two else (None, None)
                        ref = R.ln_bwd_ref(w["da"], db_, w["z"], w["gamma"], w["mean"], w["rstd"], ex, rms=rms)
                        dy = w["da"].float() + w["db"].float() if two else w["da"].float()
                        o, dg, dbt = emu_bwd(dy, w["z"], w["gamma"], w["mean"], w["rstd"], ex, rms=rms)
                        up(fam, dz=ratio_result(o, ref.dz, ref.scale, dt), dgamma=ratio_cols(dg, ref.dgamma, ref.dgamma_abs),
                           dbeta=ratio_cols(dbt, ref.dbeta, ref.dbeta_abs))
                        if fam == "bwd" and dt == torch.bfloat16:
                            st = o.to(torch.bfloat16)
                            up(fam, colsum=ratio_cols(st.float().sum(0), st.double().sum(0), st.double().abs().sum(0)))
            for p in (0.1, 0.5):
                mask = torch.rand(rows, d, generator=torch.Generator().manual_seed(d + rows)) >= p
                keep32 = mask.float() * (1 / (1 - torch.tensor(p, dtype=torch.float32)))
                w = R.bwd_inputs(rows, d)
                ref = R.ln_bwd_ref(w["da"], w["db"], w["z"], w["gamma"], w["mean"], w["rstd"], None)
                o, dg, dbt = emu_bwd(w["da"].float() + w["db"].float(), w["z"], w["gamma"], w["mean"], w["rstd"], None)
                dx = (o * keep32).to(torch.bfloat16)
                up("bwd_drop", dz=ratio_result(o, ref.dz, ref.scale), dx0=ratio_result(o * keep32, ref.dz * mask / (1 - p), ref.scale * mask / (1 - p)),
                   dgamma=ratio_cols(dg, ref.dgamma, ref.dgamma_abs), dbeta=ratio_cols(dbt, ref.dbeta, ref.dbeta_abs),
                   colsum=ratio_cols(dx.float().sum(0), dx.double().sum(0), dx.double().abs().sum(0)))
        for lens in POOL_LENS:
            pin = R.pooled_inputs(lens, d)
            for mode in (0, 1):
                for normalize in (0, 1):
                    ref = R.ln_bwd_ref(R.pooled_dout_ref(pin["demb"], pin["emb"], pin["norm"], pin["cu"], mode, normalize), None,
                                       pin["z"], pin["gamma"], pin["mean"], pin["rstd"], None)
                    o, dg, dbt = emu_bwd(emu_pooled_dout(pin, mode, normalize), pin["z"], pin["gamma"], pin["mean"], pin["rstd"], None)
                    st = o.to(torch.bfloat16)
                    up("pooled", dz=ratio_result(o, ref.dz, ref.scale), dgamma=ratio_cols(dg, ref.dgamma, ref.dgamma_abs),
                       dbeta=ratio_cols(dbt, ref.dbeta, ref.dbeta_abs),
                       colsum=ratio_cols(st.float().sum(0), st.double().sum(0), st.double().abs().sum(0)))
    for T, d in R.EMBED_FWD_SHAPES:
        e = R.embed_fwd_inputs(T, d)
        for pos in (e["pos"], None):
            z, _, _ = R.embed_z(e["word"], e["type"], pos, e["ids"], e["indices"], e["seq"])
            f = R.ln_fwd_ref(z, None, e["gamma"], e["beta"], 1e-12)
            _, mean, rstd, out = emu_fwd(z, None, e["gamma"], e["beta"], 1e-12)
            cm, cr = ratio_stats(mean, rstd, f)
            up("embed_fwd", out=ratio_result(out, f.out, f.scale), out_tight=ratio_result(out, f.out, f.scale_tight), mean=cm, rstd=cr)
    for e in [R.embed_bwd_inputs(d) for d in WIDTHS] + [R.embed_sorted_inputs(768)]:
        for pos in (e["pos"], None):
            z, tid, p = R.embed_z(e["word"], e["type"], pos, e["ids"], e["indices"], e["seq"])
            st = R.ln_fwd_ref(z, None, e["gamma"], None, 1e-12)
            mean, rstd = st.mean.float(), st.rstd.float()
            for two in (True, False):
                ref = R.ln_bwd_ref(e["da"], e["db"] if two else None, z, e["gamma"], mean, rstd, None)
                dy = e["da"].float() + e["db"].float() if two else e["da"].float()
                o, dg, dbt = emu_bwd(dy, z, e["gamma"], mean, rstd, None)
                real = tid != R.EMBED_PAD
                sc = max(ratio_cols(o.sum(0), ref.dz.sum(0), ref.scale.sum(0)),
                         _ratio((R.scatter_rows(o, p, e["seq"]).double() - R.scatter_rows(ref.dz, p, e["seq"])).abs(),
                                R.scatter_rows(ref.scale, p, e["seq"])).max(),
                         _ratio((R.scatter_rows(o[real], tid[real], e["vocab"]).double() - R.scatter_rows(ref.dz[real], tid[real], e["vocab"])).abs(),
                                R.scatter_rows(ref.scale[real], tid[real], e["vocab"])).max())
                up("embed_bwd", dz=ratio_result(o, ref.dz, ref.scale, torch.float32), dgamma=ratio_cols(dg, ref.dgamma, ref.dgamma_abs),
                   dbeta=ratio_cols(dbt, ref.dbeta, ref.dbeta_abs), scatter=float(sc))
    return m


def test_measured_constants():
    """Every C_MEAS entry is the measured worst ratio rounded up: not below it, and not more than twice it (a constant that
    has drifted loose is re-measured, not kept)."""
    m = measure()
    print({f: {k: round(v, 3) for k, v in vals.items()} for f, vals in m.items()})
    for fam, vals in m.items():
        for k, v in vals.items():
            c = R.C_MEAS[fam][k]
            assert v <= c <= max(2 * v, 0.5), (fam, k, v, c)


# ------------------------------------------------------------------------------------------------------ planted errors
def _fwd_case(rows=41, d=512):
    x0, res, g, b = R.fwd_inputs(rows, d)
    f = R.ln_fwd_ref(x0, res, g, b, 1e-12)
    _, mean, rstd, out = emu_fwd(x0, res, g, b, 1e-12)
    return (x0, res, g, b), f, mean, rstd, out


def _bwd_case(rows=41, d=512):
    w = R.bwd_inputs(rows, d)
    ref = R.ln_bwd_ref(w["da"], w["db"], w["z"], w["gamma"], w["mean"], w["rstd"], w["ex"])
    o, dg, dbt = emu_bwd(w["da"].float() + w["db"].float(), w["z"], w["gamma"], w["mean"], w["rstd"], w["ex"])
    return w, ref, o, dg, dbt


def test_checker_accepts_the_emulation_and_names_the_first_failure():
    _, f, mean, rstd, out = _fwd_case()
    assert R.check_out("out", out.to(torch.bfloat16), f, "fwd") <= 1
    assert R.check_mean("mean", mean, f, R.C("fwd", "mean")) <= 1 and R.check_rstd("rstd", rstd, f, R.C("fwd", "rstd")) <= 1
    w, ref, o, dg, dbt = _bwd_case()
    assert R.check_result("dz", o.to(torch.bfloat16), ref.dz, ref.scale, R.C("bwd", "dz")) <= 1
    assert R.check_rows("dgamma", dg, ref.dgamma, R.C("bwd", "dgamma") * EPS24 * ref.dgamma_abs) <= 1
    bad = out.to(torch.bfloat16).clone()
    bad[17, 300] += 1.0
    bad[30, 2] = float("nan")
    with pytest.raises(R.RowMismatch, match=r"\(row 17, column 300\).*2 of"):
        R.check_out("out", bad, f, "fwd")


@pytest.mark.parametrize("lane_group", [0, 77, 127])
def test_planted_zeroed_column_group_is_rejected(lane_group):
    _, f, _, _, out = _fwd_case()
    bad = out.to(torch.bfloat16).clone()
    bad[23, lane_group * 4:lane_group * 4 + 4] = 0
    with pytest.raises(R.RowMismatch, match="row 23"):
        R.check_out("out", bad, f, "fwd")
    _, ref, o, _, _ = _bwd_case()
    bad = o.to(torch.bfloat16).clone()
    bad[23, lane_group * 4:lane_group * 4 + 4] = 0
    with pytest.raises(R.RowMismatch, match="row 23"):
        R.check_result("dz", bad, ref.dz, ref.scale, R.C("bwd", "dz"))


def test_planted_row_swap_is_rejected():
    _, f, mean, rstd, out = _fwd_case()
    perm = torch.arange(out.shape[0])
    perm[[11, 36]] = perm[[36, 11]]           # rows 25 apart share (mu, sigma): only the data tells them apart
    with pytest.raises(R.RowMismatch, match="row 11"):
        R.check_out("out", out.to(torch.bfloat16)[perm], f, "fwd")
    perm = torch.arange(out.shape[0])
    perm[[11, 12]] = perm[[12, 11]]
    with pytest.raises(R.RowMismatch, match="row 11"):
        R.check_mean("mean", mean[perm], f, R.C("fwd", "mean"))
    _, ref, o, _, _ = _bwd_case()
    with pytest.raises(R.RowMismatch, match="row 11"):
        R.check_result("dz", o.to(torch.bfloat16)[perm], ref.dz, ref.scale, R.C("bwd", "dz"))


def test_planted_stale_rstd_is_rejected():
    (x0, res, g, b), f, mean, rstd, out = _fwd_case()
    stale = rstd.clone()
    stale[20] = rstd[19]
    with pytest.raises(R.RowMismatch, match="row 20"):
        R.check_rstd("rstd", stale, f, R.C("fwd", "rstd"))
    z = x0.float() + res.float()
    bad = ((z - mean[:, None]) * stale[:, None] * g + b).to(torch.bfloat16)
    with pytest.raises(R.RowMismatch, match="row 20"):
        R.check_out("out", bad, f, "fwd")
    # the backward prefetch carrying the previous row's statistics
    w, ref, _, _, _ = _bwd_case()
    m2, r2 = w["mean"].clone(), w["rstd"].clone()
    m2[20], r2[20] = m2[16], r2[16]
    o, dg, _ = emu_bwd(w["da"].float() + w["db"].float(), w["z"], w["gamma"], m2, r2, w["ex"])
    with pytest.raises(R.RowMismatch, match="row 20"):
        R.check_result("dz", o.to(torch.bfloat16), ref.dz, ref.scale, R.C("bwd", "dz"))
    with pytest.raises(R.RowMismatch):
        R.check_rows("dgamma", dg, ref.dgamma, R.C("bwd", "dgamma") * EPS24 * ref.dgamma_abs)


def test_planted_double_rounding_is_rejected():
    _, ref, o, _, _ = _bwd_case()
    with pytest.raises(R.RowMismatch):
        R.check_result("dz", o.to(torch.float16).to(torch.bfloat16), ref.dz, ref.scale, R.C("bwd", "dz"))
    # ... also where fp16 neither overflows nor goes subnormal: rows of moderate size only
    rows = [r for r in range(o.shape[0]) if 1e-2 < float(ref.dz[r].abs().max()) < 1e3 and float(ref.dz[r].abs().min()) > 1e-4]
    assert len(rows) >= 8
    with pytest.raises(R.RowMismatch):
        R.check_result("dz", o[rows].to(torch.float16).to(torch.bfloat16), ref.dz[rows], ref.scale[rows], R.C("bwd", "dz"))


def test_planted_row_missing_from_dgamma_is_rejected():
    w, ref, _, _, _ = _bwd_case(rows=2053, d=256)
    keep = torch.ones(2053, dtype=torch.bool)
    keep[2052] = False                                        # e.g. the last row of the last pass
    dy = (w["da"].float() + w["db"].float())[keep]
    _, dg, dbt = emu_bwd(dy, w["z"][keep], w["gamma"], w["mean"][keep], w["rstd"][keep], None)
    with pytest.raises(R.RowMismatch):
        R.check_rows("dgamma", dg, ref.dgamma, R.C("bwd", "dgamma") * EPS24 * ref.dgamma_abs)
    with pytest.raises(R.RowMismatch):
        R.check_rows("dbeta", dbt, ref.dbeta, R.C("bwd", "dbeta") * EPS24 * ref.dbeta_abs)
    # a column sum that misses one stored row
    st = R.rows_like(2053, 256, 5, centred=True)
    with pytest.raises(R.RowMismatch):
        R.check_colsum("colsum", st[keep].float().sum(0), st, R.C("bwd", "colsum"))
