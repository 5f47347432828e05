"""The exact-fp32 loss kernels of contrastors_amd/csrc/infonce.hip -- cx_sgemm_nt, cx_infonce_fwd, cx_infonce_fwd_argmax,
cx_infonce_bwd, cx_simkl_fwd, cx_simkl_bwd -- through the C ABI against tests/loss_ref.py, per row and per element, at the tile,
slice, K-tail and leading-dimension edges of sgemm_tile and its epilogues.

Bit for bit, no tolerance: cx_sgemm_nt == loss_ref.sgemm_chain (the fmaf chain in the k order of sgemm_tile) on Gaussian operands
and on the integer family; GmatT == Gmat^T, QT == Q^T, DT == D^T; dQ == sgemm_chain(Gmat, DT) and dD == sgemm_chain(GmatT, QT) from
the Gmat the kernel wrote; every forward output and Gmat of a second call; cx_infonce_fwd_argmax's lse / loss_rows == cx_infonce_fwd's;
Gmat with dscale_accum = NULL; student == teacher gives kl_rows == 0 and Gmat == 0.  Under C 2^-24 T against fp64 on the fp32 inputs
(C = 4 C_meas, T derived in loss_ref's docstring, C_meas measured by tests/test_loss_ref_cpu.py on an fp32 emulation, never against a
kernel): lse, loss_rows, lse_s, lse_t, kl_rows per row, Gmat per element; dscale under its order-free bound, accumulated twice onto a
non-zero start.  The arg max equals the fp64 first-index arg max on EVERY row (the cases are built with the gap that allows it), the
planted exact ties report their first column, a maximum at G - 1 reports G - 1.

Every operand and result is an ew_ref.Slab: NaN guard elements either side, NaN between dim and ld, results, workspaces and all
backward scratch start as NaN; every result is finite inside its shape after the call and the guards are checked when each test ends
(`_poison`).  The worst err / bound per entry point goes through gpu_util.report.

Which test reaches what (by reading the launchers; the tile is 128 x 128, a wave covers 64 x 64, partials are per 64 columns):
    sgemm_tile K tail (K % 16 = 4, 12, 4, 4: dim 4, 12, 20, 36; sload zero-fills k >= K), one block exactly
       (16), eight blocks (128), ld = K and ld = K + 4 for either operand .................... every test: loss_ref.settings()
    EPI_STORE: partial tiles in M and N, `n + e < N` inside a quad (N = 1, 3, 63, 65, 127, 129),
       ldc = N and ldc = N + 3 ............................................................... test_sgemm_nt_bits
    EPI_LSE `n < p.N` mask inside a live slice (G = 1, 3, 63, 65, 127, 129, 260) ............. test_infonce_fwd[*-G]
    a slice wholly past G: partial (-inf, 0), skipped by lse_combine_kernel (G = 1, 3, 63, 64:
       slice 1; G = 129, 192: slice 3; G = 260: slice 5) ..................................... test_infonce_fwd, test_simkl_fwd[*-192]
    clamped rows (m >= M reads row M - 1 and its label; must write nothing): every N but 260's
       first two row tiles .................................................................. test_infonce_fwd[1 .. 260-*], test_infonce_bwd
    lab[m] ownership: labels 0, G - 1, 63, 64, 127, 128, col % 8 < 4 and >= 4, a shared label,
       the recipe's i (G // N); lab starts as NaN, loss_rows must be finite .................. test_infonce_fwd (loss_ref.labels_for)
    xcd_remap remainder (nwg = 9 = 8 + 1) with partial tiles on both axes .................... [260-260] of every test
    arg max: two columns of one lane (1, 2), the two lane halves (17, 21), the two slices of a
       tile (10, 70), two tiles (10, 138, the lse_combine_kernel min over slices) ............ test_infonce_fwd[*-G >= 3 / 22 / 71 / 139]
    arg max at G - 1 with G % 64 != 0 (never a padded column) ................................ test_infonce_fwd[*-3, 63, 65, 127, 129, 260]
    EPI_GRAD / simkl GRAD: float4 store of Gmat (n + 3 < N); with G % 4 == 0 the scalar tail
       only sees quads wholly past G and stores nothing (the guards after Gmat's rows hold);
       GmatT column stores, clamped rows, dscale wave_sum + atomic, dscale NULL ............... test_infonce_bwd, test_simkl_bwd
    the two output GEMMs: K = G and K = N with tails (G = 4, 60, 68, 132, 260; N = 4, 36, 132,
       260), ld = G / N, output width dim < 128 .............................................. test_infonce_bwd, test_simkl_bwd
    simkl_kernel: two K tails that differ (20, 36), (128, 64), (16, 16), four leading dimensions test_simkl_fwd, test_simkl_bwd
    CX_ERR_SHAPE / _ALIGN / _ARG, N = 0, G = 0, workspace sizes ............................... test_rejections, test_workspace_sizes
"""
import numpy as np
import pytest
import torch

from contrastors_amd import _C
from tests import gemm_ref as R
from tests import loss_ref as X
from tests.gemm_ref import F32
from tests.gpu_util import L, S, report
from tests.test_elementwise_edges_gpu import ERR_ALIGN, ERR_ARG, ERR_SHAPE, Worst, _BUFS, _poison, slab  # noqa: F401  (_poison: the autouse guard check)

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32


def T(a):
    return torch.from_numpy(np.array(a, order="C"))


def fs(a, pad=0, name=""):
    """An fp32 operand slab of a 2-D numpy array with ld = cols + pad."""
    return slab(a.shape[0], a.shape[1], a.shape[1] + pad, dtype=F32, data=T(a), name=name)


def out(rows, cols, ld=None, dtype=F32, name=""):
    return slab(rows, cols, ld, dtype=dtype, name=name)


def finite(tag, *slabs):
    """The payloads as numpy, every element finite (a float result) or not the poison (an int result)."""
    res = []
    for s in slabs:
        a = s.get().numpy()
        ok = np.isfinite(a).all() if a.dtype.kind == "f" else (a != s.poison).all()
        assert ok, f"{tag}: {s.name} holds an element the kernel did not write (or a NaN)"
        res.append(a)
    return res


def same_bits(tag, got, ref):
    assert R.check_bits(tag, T(got), T(ref)) == 0


def case_of(n, g, s):
    return X.make_case(n, g, s["dim"], s["family"], s["scale"], 0, s["tie_set"], s["rot"])


def tag_of(n, g, s):
    return f"N={n} G={g} dim={s['dim']} {s['family']} scale={s['scale']} pads={s['pads']}"


# ======================================================================================================== cx_sgemm_nt
@pytest.mark.parametrize("si", range(len(X.fwd_shapes())), ids=[f"{n}-{g}" for n, g in X.fwd_shapes()])
def test_sgemm_nt_bits(si):
    M, N = X.fwd_shapes()[si]
    for s in X.settings(si):
        K, (pa, pb) = s["dim"], s["pads"]
        for fam in (f for f in X.SGEMM_FAMILIES if f != "ints" or K <= 36):
            a, b = X.base_inputs(M, N, K, fam, 40)
            ref = X.sgemm_chain(a, b)
            for ldc in (N, N + 3):
                A, B, Cc = fs(a, pa, "A"), fs(b, pb, "B"), out(M, N, ldc, name="C")
                _C.check(L().cx_sgemm_nt(A.ptr, B.ptr, Cc.ptr, M, N, K, K + pa, K + pb, ldc, S()), "sgemm_nt")
                got, = finite("sgemm_nt", Cc)
                same_bits(f"cx_sgemm_nt {fam} M={M} N={N} K={K} lda={K + pa} ldb={K + pb} ldc={ldc}", got, ref)
    report("cx_sgemm_nt", test=f"M={M} N={N}", worst_err_over_bound=0.0)


# ============================================================================================================ forward
def infonce_fwd(c, s, argmax):
    """One call on fresh NaN slabs -> lse, loss_rows[, argmax] as numpy."""
    (N, dim), G, (pq, pd) = c.Q.shape, c.D.shape[0], s["pads"]
    Q, D = fs(c.Q, pq, "Q"), fs(c.D, pd, "D")
    lab = T(c.labels).to(DEV)
    LSE, LOSS = out(1, N, name="lse"), out(1, N, name="loss_rows")
    if argmax:
        WS, AM = out(1, L().cx_infonce_argmax_ws_floats(N, G), name="ws"), out(1, N, dtype=I32, name="argmax")
        rc = L().cx_infonce_fwd_argmax(Q.ptr, D.ptr, lab.data_ptr(), s["scale"], WS.ptr, LSE.ptr, LOSS.ptr, AM.ptr, N, G, dim, dim + pq, dim + pd, S())
    else:
        WS, AM = out(1, L().cx_infonce_ws_floats(N, G), name="ws"), None
        rc = L().cx_infonce_fwd(Q.ptr, D.ptr, lab.data_ptr(), s["scale"], WS.ptr, LSE.ptr, LOSS.ptr, N, G, dim, dim + pq, dim + pd, S())
    _C.check(rc, "infonce_fwd")
    return [a[0] for a in finite("infonce_fwd", LSE, LOSS, *([AM] if argmax else []))]


@pytest.mark.parametrize("si", range(len(X.fwd_shapes())), ids=[f"{n}-{g}" for n, g in X.fwd_shapes()])
def test_infonce_fwd(si):
    n, g = X.fwd_shapes()[si]
    w = Worst()
    for s in X.settings(si):
        c, tag = case_of(n, g, s), tag_of(n, g, s)
        ref = X.infonce_fwd_ref(c.Q, c.D, c.labels, s["scale"])
        lse, loss = infonce_fwd(c, s, False)
        w.add("cx_infonce_fwd.lse", X.check(f"{tag} lse", lse, ref.lse, ref.t_lse, X.C("lse")))
        w.add("cx_infonce_fwd.loss_rows", X.check(f"{tag} loss_rows", loss, ref.loss, ref.t_loss, X.C("loss")))
        lse2, loss2 = infonce_fwd(c, s, False)
        same_bits(f"{tag}: lse of a second call", lse2, lse)
        same_bits(f"{tag}: loss_rows of a second call", loss2, loss)
        lse3, loss3, am = infonce_fwd(c, s, True)
        same_bits(f"{tag}: lse of cx_infonce_fwd_argmax", lse3, lse)
        same_bits(f"{tag}: loss_rows of cx_infonce_fwd_argmax", loss3, loss)
        exp = X.argmax_ref(c.Q, c.D, s["scale"])
        bad = np.nonzero(am != exp)[0]
        assert bad.size == 0, f"{tag}: arg max of row {bad[0]} is {am[bad[0]]}, fp64 first index {exp[bad[0]]}; {bad.size} rows differ"
        for row, a, b in c.ties:
            assert am[row] == a, f"{tag}: the tie of columns {a} and {b} (row {row}) reported {am[row]}"
        if c.last_row is not None:
            assert am[c.last_row] == g - 1, f"{tag}: the maximum at G - 1 (row {c.last_row}) reported {am[c.last_row]}"
        same_bits(f"{tag}: arg max of a second call", infonce_fwd(c, s, True)[2], am)
        for r in c.zero_rows:
            assert abs(float(lse[r]) - np.log(g)) <= 4 * X.U * (np.log(g) + 1), f"{tag}: lse of a zero query is log G"
    w.flush(f"infonce_fwd N={n} G={g}")


# =========================================================================================================== backward
def check_out_gemms(tag, gm, gmT, q, d, QT, DT, dQ, dD):
    """The wiring after the epilogue, bit for bit: both transposes of the operands and of Gmat, both output GEMMs as fmaf chains."""
    same_bits(f"{tag}: GmatT == Gmat^T", gmT, gm.T)
    same_bits(f"{tag}: QT", QT, q.T)
    same_bits(f"{tag}: DT", DT, d.T)
    same_bits(f"{tag}: dQ == sgemm_chain(Gmat, DT)", dQ, X.sgemm_chain(gm, d.T))
    same_bits(f"{tag}: dD == sgemm_chain(GmatT, QT)", dD, X.sgemm_chain(gm.T, q.T))


def infonce_bwd(c, s, lse_fed, coef, ds_buf):
    (N, dim), G, (pq, pd) = c.Q.shape, c.D.shape[0], s["pads"]
    Q, D, LSE = fs(c.Q, pq, "Q"), fs(c.D, pd, "D"), fs(lse_fed[None], 0, "lse")
    lab = T(c.labels).to(DEV)
    o = [out(N, G, name="Gmat"), out(G, N, name="GmatT"), out(dim, N, name="QT"), out(dim, G, name="DT"), out(N, dim, name="dQ"), out(G, dim, name="dD")]
    _C.check(L().cx_infonce_bwd(Q.ptr, D.ptr, lab.data_ptr(), LSE.ptr, s["scale"], coef, *(b.ptr for b in o),
                                None if ds_buf is None else ds_buf.data_ptr() + 4, N, G, dim, dim + pq, dim + pd, S()), "infonce_bwd")
    return finite("infonce_bwd", *o)


BWD_BY_SHAPE = {}
for _n, _g, _s in X.bwd_cases():
    BWD_BY_SHAPE.setdefault((_n, _g), []).append(_s)


@pytest.mark.parametrize("n,g", list(BWD_BY_SHAPE), ids=[f"{n}-{g}" for n, g in BWD_BY_SHAPE])
def test_infonce_bwd(n, g):
    w = Worst()
    for s in BWD_BY_SHAPE[(n, g)]:
        c, tag, coef = case_of(n, g, s), tag_of(n, g, s), X.coef_for(n, s["coef_i"])
        lse_fed = X.infonce_fwd_ref(c.Q, c.D, c.labels, s["scale"]).lse.astype(np.float32)
        gm_ref, t, floor, ds_ref, ds_bound = X.infonce_bwd_ref(c.Q, c.D, c.labels, lse_fed, s["scale"], coef)
        init = 0.75
        ds = torch.tensor([7.0, init, 7.0], dtype=F32, device=DEV)
        gm, gmT, QT, DT, dQ, dD = infonce_bwd(c, s, lse_fed, coef, ds)
        one = float(ds.cpu()[1]) - init
        w.add("cx_infonce_bwd.Gmat", X.check(f"{tag} Gmat", gm, gm_ref, t, X.C("gm"), floor))
        check_out_gemms(tag, gm, gmT, c.Q, c.D, QT, DT, dQ, dD)
        gm2 = infonce_bwd(c, s, lse_fed, coef, ds)[0]
        same_bits(f"{tag}: Gmat of a second call", gm2, gm)
        got = ds.cpu()
        assert got[0] == 7.0 and got[2] == 7.0, f"{tag}: dscale_accum's neighbours were written"
        # the start value is rounded into every atomic of both calls: 2 * 4 waves * nwg roundings at the magnitude of the running total
        nwg = ((n + 127) // 128) * ((g + 127) // 128)
        acc = 8 * nwg * X.U * (init + 2 * abs(ds_ref) + 2 * ds_bound)
        two = float(got[1]) - init
        print(f"{tag}: dscale one call {one!r}, two calls {two!r}, fp64 {ds_ref!r}, bound {ds_bound:.3e}, err/bound {abs(one - ds_ref) / (ds_bound + acc / 2):.3f}")
        assert abs(one - ds_ref) <= ds_bound + acc / 2, f"{tag}: dscale {one!r}, fp64 {ds_ref!r}, |err| {abs(one - ds_ref):.3e} > bound {ds_bound + acc / 2:.3e}"
        assert abs(two - 2 * ds_ref) <= 2 * ds_bound + acc, f"{tag}: dscale after two calls {two!r}, fp64 {2 * ds_ref!r}, bound {2 * ds_bound + acc:.3e}"
        w.add("cx_infonce_bwd.dscale", max(abs(one - ds_ref) / (ds_bound + acc / 2), abs(two - 2 * ds_ref) / (2 * ds_bound + acc)))
        same_bits(f"{tag}: Gmat with dscale_accum = NULL", infonce_bwd(c, s, lse_fed, coef, None)[0], gm)
    w.flush(f"infonce_bwd N={n} G={g}")


# ============================================================================================================== simkl
def simkl_fwd(ops, it, pads, same=False):
    """same: the teacher pointers ARE the student pointers."""
    Qs, Ds, Qt, Dt = ops
    N, G = Qs.shape[0], Ds.shape[0]
    b = [fs(Qs, pads[0], "Qs"), fs(Ds, pads[1], "Ds")]
    b += b if same else [fs(Qt, pads[2], "Qt"), fs(Dt, pads[3], "Dt")]
    ld = [Qs.shape[1] + pads[0], Ds.shape[1] + pads[1]] + ([Qs.shape[1] + pads[0], Ds.shape[1] + pads[1]] if same else [Qt.shape[1] + pads[2], Dt.shape[1] + pads[3]])
    WS = out(1, L().cx_simkl_ws_floats(N, G), name="ws")
    o = [out(1, N, name=nm) for nm in ("lse_s", "lse_t", "kl_rows")]
    _C.check(L().cx_simkl_fwd(*(x.ptr for x in b), it, WS.ptr, *(x.ptr for x in o), N, G, Qs.shape[1], Qs.shape[1] if same else Qt.shape[1], *ld, S()), "simkl_fwd")
    return [a[0] for a in finite("simkl_fwd", *o)]


def simkl_bwd(ops, fs_, ft_, it, coef, pads, same=False):
    Qs, Ds, Qt, Dt = ops
    (N, dim), G = Qs.shape, Ds.shape[0]
    b = [fs(Qs, pads[0], "Qs"), fs(Ds, pads[1], "Ds")]
    b += b if same else [fs(Qt, pads[2], "Qt"), fs(Dt, pads[3], "Dt")]
    ld = [dim + pads[0], dim + pads[1]] + ([dim + pads[0], dim + pads[1]] if same else [Qt.shape[1] + pads[2], Dt.shape[1] + pads[3]])
    l = [fs(fs_[None], 0, "lse_s"), fs(ft_[None], 0, "lse_t")]
    o = [out(N, G, name="Gmat"), out(G, N, name="GmatT"), out(dim, N, name="QsT"), out(dim, G, name="DsT"), out(N, dim, name="dQs"), out(G, dim, name="dDs")]
    _C.check(L().cx_simkl_bwd(*(x.ptr for x in b), l[0].ptr, l[1].ptr, it, coef, *(x.ptr for x in o), N, G, dim, dim if same else Qt.shape[1], *ld, S()), "simkl_bwd")
    return finite("simkl_bwd", *o)


SIMKL_BY_SHAPE = {}
for _c in X.simkl_cases():
    SIMKL_BY_SHAPE.setdefault(_c[:2], []).append(_c)


@pytest.mark.parametrize("n,g", list(SIMKL_BY_SHAPE), ids=[f"{n}-{g}" for n, g in SIMKL_BY_SHAPE])
def test_simkl_fwd(n, g):
    w = Worst()
    for _, _, ds_, dt_, it, fam, pads, k in SIMKL_BY_SHAPE[(n, g)]:
        ops, tag = X.simkl_inputs(n, g, ds_, dt_, fam, k), f"simkl N={n} G={g} dims=({ds_}, {dt_}) {fam} inv_temp={it} pads={pads}"
        r = X.simkl_fwd_ref(*ops, it)
        ls, lt, kl = simkl_fwd(ops, it, pads)
        w.add("cx_simkl_fwd.lse_s", X.check(f"{tag} lse_s", ls, r.lse_s, r.t_lse_s, X.C("lse_s")))
        w.add("cx_simkl_fwd.lse_t", X.check(f"{tag} lse_t", lt, r.lse_t, r.t_lse_t, X.C("lse_t")))
        w.add("cx_simkl_fwd.kl_rows", X.check(f"{tag} kl_rows", kl, r.kl, r.t_kl, X.C("kl")))
        for nm, a, b in zip(("lse_s", "lse_t", "kl_rows"), simkl_fwd(ops, it, pads), (ls, lt, kl)):
            same_bits(f"{tag}: {nm} of a second call", a, b)
        ls0, lt0, kl0 = simkl_fwd(ops, it, pads, same=True)
        assert not kl0.any(), f"{tag}: student == teacher must give kl_rows == 0 exactly, row {np.nonzero(kl0)[0][0]} holds {kl0[np.nonzero(kl0)[0][0]]!r}"
        same_bits(f"{tag}: lse_s == lse_t for student == teacher", ls0, lt0)
        same_bits(f"{tag}: lse_s does not depend on the teacher", ls0, ls)
    w.flush(f"simkl_fwd N={n} G={g}")


@pytest.mark.parametrize("n,g", [k for k in SIMKL_BY_SHAPE if k[0] % 4 == 0 and k[1] % 4 == 0], ids=lambda v: str(v))
def test_simkl_bwd(n, g):
    w = Worst()
    for _, _, ds_, dt_, it, fam, pads, k in SIMKL_BY_SHAPE[(n, g)]:
        ops, tag, coef = X.simkl_inputs(n, g, ds_, dt_, fam, k), f"simkl N={n} G={g} dims=({ds_}, {dt_}) {fam} inv_temp={it} pads={pads}", X.coef_for(n, k)
        r = X.simkl_fwd_ref(*ops, it)
        fs_, ft_ = r.lse_s.astype(np.float32), r.lse_t.astype(np.float32)
        gm_ref, t, floor = X.simkl_bwd_ref(*ops, fs_, ft_, it, coef)
        gm, gmT, QT, DT, dQ, dD = simkl_bwd(ops, fs_, ft_, it, coef, pads)
        w.add("cx_simkl_bwd.Gmat", X.check(f"{tag} Gmat", gm, gm_ref, t, X.C("simkl_gm"), floor))
        check_out_gemms(tag, gm, gmT, ops[0], ops[1], QT, DT, dQ, dD)
        same_bits(f"{tag}: Gmat of a second call", simkl_bwd(ops, fs_, ft_, it, coef, pads)[0], gm)
        z = simkl_bwd(ops, fs_, fs_, it, coef, pads, same=True)
        assert not z[0].any() and not z[4].any() and not z[5].any(), f"{tag}: student == teacher must give Gmat, dQs, dDs == 0 exactly"
    w.flush(f"simkl_bwd N={n} G={g}")


# ========================================================================================================= rejections
def test_rejections():
    lib, N, G, dim = L(), 8, 12, 8
    rng = np.random.default_rng(0)
    q, d = rng.standard_normal((N, dim + 4)).astype(np.float32), rng.standard_normal((G, dim + 4)).astype(np.float32)
    Q, D, LSEIN = fs(q, 0, "Q"), fs(d, 0, "D"), fs(np.zeros((1, N), np.float32), 0, "lse")
    lab = torch.zeros(N, dtype=torch.int64, device=DEV)
    res = [out(1, 4096, name=f"o{i}") for i in range(8)]           # results, workspace and scratch: all stay NaN
    o = [r.ptr for r in res]
    ld, lp = dim + 4, lab.data_ptr()

    def fwd(Q_=Q.ptr, D_=D.ptr, lab_=lp, ws=o[0], lse=o[1], loss=o[2], n=N, g=G, k=dim, ldq=ld, ldd=ld):
        return lib.cx_infonce_fwd(Q_, D_, lab_, 20.0, ws, lse, loss, n, g, k, ldq, ldd, S())

    def fwda(am=o[3], **kw):
        a = dict(Q_=Q.ptr, D_=D.ptr, lab_=lp, ws=o[0], lse=o[1], loss=o[2], n=N, g=G, k=dim, ldq=ld, ldd=ld)
        a.update(kw)
        return lib.cx_infonce_fwd_argmax(a["Q_"], a["D_"], a["lab_"], 20.0, a["ws"], a["lse"], a["loss"], am, a["n"], a["g"], a["k"], a["ldq"], a["ldd"], S())

    def bwd(p=None, n=N, g=G, k=dim, ldq=ld, ldd=ld):
        a = [Q.ptr, D.ptr, lp, LSEIN.ptr] + o[:6]
        if p is not None:
            a[p] = None
        return lib.cx_infonce_bwd(*a[:4], 20.0, 0.5, *a[4:], o[6], n, g, k, ldq, ldd, S())

    def sk(p=None, n=N, g=G, ks=dim, kt=dim, lds=(ld, ld, ld, ld)):
        a = [Q.ptr, D.ptr, Q.ptr, D.ptr, o[0], o[1], o[2], o[3]]
        if p is not None:
            a[p] = None
        return lib.cx_simkl_fwd(*a[:4], 5.0, *a[4:], n, g, ks, kt, *lds, S())

    def skb(p=None, n=N, g=G, ks=dim, kt=dim, lds=(ld, ld, ld, ld)):
        a = [Q.ptr, D.ptr, Q.ptr, D.ptr, LSEIN.ptr, LSEIN.ptr] + o[:6]
        if p is not None:
            a[p] = None
        return lib.cx_simkl_bwd(*a[:6], 5.0, 0.5, *a[6:], n, g, ks, kt, *lds, S())

    for f in (fwd, fwda, bwd):
        assert f(k=6) == ERR_SHAPE and f(k=0) == ERR_SHAPE
        assert f(ldq=ld + 2) == ERR_ALIGN and f(ldd=ld + 1) == ERR_ALIGN
        assert f(n=0) == _C.CX_OK and f(g=0) == _C.CX_OK
    assert lib.cx_sgemm_nt(Q.ptr, D.ptr, o[0], N, G, 6, ld, ld, G, S()) == ERR_SHAPE
    assert lib.cx_sgemm_nt(Q.ptr, D.ptr, o[0], N, G, dim, ld + 2, ld, G, S()) == ERR_ALIGN
    assert lib.cx_sgemm_nt(Q.ptr, D.ptr, o[0], N, G, dim, ld, ld + 3, G, S()) == ERR_ALIGN
    assert lib.cx_sgemm_nt(Q.ptr, D.ptr, o[0], 0, G, dim, ld, ld, G, S()) == _C.CX_OK
    assert lib.cx_sgemm_nt(Q.ptr, D.ptr, o[0], N, 0, dim, ld, ld, G, S()) == _C.CX_OK
    for name in ("Q_", "D_", "lab_", "ws", "lse", "loss"):
        assert fwd(**{name: None}) == ERR_ARG and fwda(**{name: None}) == ERR_ARG, name
    for p in range(10):                                              # Q, D, labels, lse, Gmat, GmatT, QT, DT, dQ, dD
        assert bwd(p) == ERR_ARG, p
    assert bwd(n=6) == ERR_SHAPE and bwd(g=10) == ERR_SHAPE
    for f in (sk, skb):
        assert f(ks=6) == ERR_SHAPE and f(kt=10) == ERR_SHAPE
        for i in range(4):
            assert f(lds=tuple(ld + 2 * (j == i) for j in range(4))) == ERR_ALIGN, i
        assert f(n=0) == _C.CX_OK and f(g=0) == _C.CX_OK
    for p in range(8):
        assert sk(p) == ERR_ARG, p
    for p in range(12):
        assert skb(p) == ERR_ARG, p
    assert skb(n=6) == ERR_SHAPE and skb(g=10) == ERR_SHAPE
    torch.cuda.synchronize()
    for r in res:
        assert bool(torch.isnan(r.get()).all()), f"{r.name} was written by a rejected call"


def test_workspace_sizes():
    lib = L()
    for N, G in ((1, 1), (33, 128), (33, 129), (260, 260), (2048, 16384)):
        nparts = 2 * ((G + 127) // 128)
        assert lib.cx_infonce_ws_floats(N, G) == N * (2 * nparts + 1)
        assert lib.cx_infonce_argmax_ws_floats(N, G) == N * (3 * nparts + 1)
        assert lib.cx_simkl_ws_floats(N, G) == N * 5 * nparts
