"""tests/loss_ref.py proven on the CPU before it meets a kernel: the fp32 fma emulation against libm's fmaf (random triples and
triples built on, just below and just above fp32 rounding ties, where a fma evaluated in double and rounded again goes wrong),
sgemm_chain against a scalar libm chain, against fp64 and exactly on the integer family, the fp32 emulations of the kernels inside
their bounds with the measured constants of loss_ref.C_MEAS, the argmax-gap condition of every case the GPU tests run, the planted
ties and the label builder.  Nothing here touches a kernel."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from tests import loss_ref as X
from tests.loss_ref import F32, F64, U


def _libm_fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return m.fmaf


def _tie_triples():
    """(a, b, c) with a * b + c exactly on a fp32 tie (c + half an ulp of c), 2^-46 relative below it and 2^-22 above it, both
    signs, c of both parities."""
    rng = np.random.default_rng(5)
    e = F32(2.0 ** -23)
    out = []
    for _ in range(400):
        c = F32(rng.uniform(1.0, 2.0)) * F32(2.0 ** int(rng.integers(-20, 20)))
        h = float(np.spacing(c)) / 2                       # a power of two
        i = int(rng.integers(-10, 10))
        a0, b0 = F32(2.0 ** i), F32(h * 2.0 ** -i)
        sg = F32(rng.choice([-1.0, 1.0]))
        for fa, fb in ((F32(1), F32(1)), (F32(1) + e, F32(1) - e), (F32(1) + e, F32(1) + e)):
            out.append((a0 * fa * sg, b0 * fb, c * sg))      # the product has the sign of c: |sum| = |c| + h (1 + ...)
            out.append((a0 * fa * -sg, b0 * fb, c * sg))     # ... or the other: |c| - h (1 + ...)
    return np.array(out, dtype=F32)


def test_fmaf_equals_libm_one_scalar_at_a_time():
    fmaf = _libm_fmaf()
    rng = np.random.default_rng(1)
    rnd = (rng.standard_normal((3000, 3)) * 2.0 ** rng.integers(-12, 12, (3000, 3))).astype(F32)
    rnd[::7, 2] = -(rnd[::7, 0] * rnd[::7, 1]).astype(F32)           # massive cancellation: the low half of the product survives
    ties = _tie_triples()
    for name, tri in (("random", rnd), ("ties", ties)):
        got = X.fmaf(tri[:, 0], tri[:, 1], tri[:, 2])
        want = np.array([fmaf(float(a), float(b), float(c)) for a, b, c in tri], dtype=F32)
        assert got.dtype == F32 and np.array_equal(got.view(np.int32), want.view(np.int32)), (name, int((got != want).sum()))
    # the ties bite: a * b + c in double, rounded to fp32, is NOT fmaf on them
    naive = (ties[:, 0].astype(F64) * ties[:, 1].astype(F64) + ties[:, 2].astype(F64)).astype(F32)
    want = np.array([fmaf(float(a), float(b), float(c)) for a, b, c in ties], dtype=F32)
    assert int((naive != want).sum()) >= 50
    assert float(X.fmaf(F32(3), F32(4), F32(5))) == 17.0                # scalars pass through


def test_sgemm_chain_is_the_documented_chain():
    """Against a scalar libm chain in the k order written out by hand, zero-filled steps included: K = 20 (one full block and a
    tail of 4), and K = 4 / 16 on products that underflow to nothing from below (-0 survives a whole block, a K tail makes it +0)."""
    fmaf = _libm_fmaf()
    rng = np.random.default_rng(2)
    order = [0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15]
    assert tuple(order) == X.K_ORDER
    for K in (20, 4, 16):
        A, B = rng.standard_normal((3, K)).astype(F32), rng.standard_normal((2, K)).astype(F32)
        A[2] = -np.abs(A[2]) * F32(2.0 ** -100)
        B[1] = np.abs(B[1]) * F32(2.0 ** -100)
        got = X.sgemm_chain(A, B)
        for i in range(3):
            for j in range(2):
                acc = 0.0
                for k0 in range(0, K, 16):
                    for k in (k0 + o for o in order):
                        acc = fmaf(float(A[i, k]), float(B[j, k]), acc) if k < K else fmaf(0.0, 0.0, acc)
                assert got[i, j].view(np.int32) == F32(acc).view(np.int32), (K, i, j)
        assert got[2, 1] == 0 and bool(np.signbit(got[2, 1])) == (K == 16)


@pytest.mark.parametrize("K", [4, 12, 16, 20, 36, 128])
def test_sgemm_chain_against_fp64_and_exact_on_integers(K):
    swapped = tuple(k ^ 4 for k in X.K_ORDER)                          # the two k halves of every MFMA exchanged
    Q, D = X.base_inputs(33, 65, K, "gauss", 3)
    c = X.sgemm_chain(Q, D)
    ref, mag = Q.astype(F64) @ D.astype(F64).T, np.abs(Q.astype(F64)) @ np.abs(D.astype(F64)).T
    assert bool((np.abs(c - ref) <= K * U * mag).all())                # the standard bound of a K-term fma chain
    if K >= 16:
        assert int((X.sgemm_chain(Q, D, swapped) != c).sum()) > 0      # the order shows in the bits of Gaussian operands ...
    if K <= 36:
        Qi, Di = X.base_inputs(33, 65, K, "ints", 3)
        ci = X.sgemm_chain(Qi, Di)
        assert np.array_equal(ci.astype(F64), Qi.astype(F64) @ Di.astype(F64).T)
        assert np.array_equal(X.sgemm_chain(Qi, Di, swapped), ci)      # ... and not in those of the integer family


def _case(n, g, s):
    return X.make_case(n, g, s["dim"], s["family"], s["scale"], 0, s["tie_set"], s["rot"])


def test_measured_constants():
    """C_MEAS: the worst |fp32 emulation - fp64| / (2^-24 T) over every case the GPU tests run; the table holds it, rounded up."""
    w = dict.fromkeys(X.C_MEAS, 0.0)
    for n, g, s in X.fwd_cases():
        c = _case(n, g, s)
        ref = X.infonce_fwd_ref(c.Q, c.D, c.labels, s["scale"])
        lse, loss, _ = X.emu_infonce_fwd(c.Q, c.D, c.labels, s["scale"])
        w["lse"] = max(w["lse"], X.ratio(lse, ref.lse, ref.t_lse, 1.0))
        w["loss"] = max(w["loss"], X.ratio(loss, ref.loss, ref.t_loss, 1.0))
    for n, g, s in X.bwd_cases():
        c = _case(n, g, s)
        coef = X.coef_for(n, s["coef_i"])
        lse = X.infonce_fwd_ref(c.Q, c.D, c.labels, s["scale"]).lse.astype(F32)
        gm, t, floor, _, _ = X.infonce_bwd_ref(c.Q, c.D, c.labels, lse, s["scale"], coef)
        w["gm"] = max(w["gm"], X.ratio(X.emu_infonce_gm(c.Q, c.D, c.labels, lse, s["scale"], coef)[0], gm, t, 1.0, floor))
    for n, g, ds, dt, it, fam, _, k in X.simkl_cases():
        ops = X.simkl_inputs(n, g, ds, dt, fam, k)
        r = X.simkl_fwd_ref(*ops, it)
        ls, lt, kl = X.emu_simkl_fwd(*ops, it)
        w["lse_s"] = max(w["lse_s"], X.ratio(ls, r.lse_s, r.t_lse_s, 1.0))
        w["lse_t"] = max(w["lse_t"], X.ratio(lt, r.lse_t, r.t_lse_t, 1.0))
        w["kl"] = max(w["kl"], X.ratio(kl, r.kl, r.t_kl, 1.0))
        fs, ft = r.lse_s.astype(F32), r.lse_t.astype(F32)
        gm, t, floor = X.simkl_bwd_ref(*ops, fs, ft, it, X.coef_for(n, k))
        w["simkl_gm"] = max(w["simkl_gm"], X.ratio(X.emu_simkl_gm(*ops, fs, ft, it, X.coef_for(n, k)), gm, t, 1.0, floor))
    print({k: round(v, 4) for k, v in w.items()})
    for k, v in w.items():
        assert 0.5 * X.C_MEAS[k] <= v <= X.C_MEAS[k], (k, v, X.C_MEAS[k])


def test_emulation_catches_planted_errors():
    """The checker and the bounds reject what the GPU tests must reject: a padded column let into the sum, and a label one off."""
    n, g, s = 33, 65, dict(dim=16, family="gauss", scale=50.0, tie_set=0, rot=0)
    c = _case(n, g, s)
    ref = X.infonce_fwd_ref(c.Q, c.D, c.labels, 50.0)
    lse, loss, _ = X.emu_infonce_fwd(c.Q, c.D, c.labels, 50.0)
    assert X.check("lse", lse, ref.lse, ref.t_lse, X.C("lse")) <= 1.0
    Dpad = np.concatenate([c.D, c.D[-1:]])                             # the clamped row g - 1 read as a 66th column
    bad = X.emu_infonce_fwd(c.Q, Dpad, c.labels, 50.0)[0]
    with pytest.raises(X.Mismatch, match=r"index \(\d+,\)"):
        X.check("lse", bad, ref.lse, ref.t_lse, X.C("lse"))
    with pytest.raises(X.Mismatch):
        X.check("loss", X.emu_infonce_fwd(c.Q, c.D, (c.labels + 1) % g, 50.0)[1], ref.loss, ref.t_loss, X.C("loss"))


def test_argmax_gap_of_every_case():
    """Every column within 2 logit_bound of a row's maximum is an exact tie of it: the same document row bit for bit, any column of
    a zero query, or an equal exact sum of the integer family.  So argmax_ref is the fp64 first-index argmax with no row left out."""
    routes, last = set(), 0
    for n, g, s in X.fwd_cases():
        c = _case(n, g, s)
        x, near = X.near_max(c.Q, c.D, s["scale"])
        first = X.first_copy(c.D)
        best = x.argmax(1)
        for i in range(n):
            cols = np.nonzero(near[i])[0]
            if i in c.zero_rows:
                assert not c.Q[i].any() and len(cols) == g
            elif c.family == "ints":
                assert bool((x[i, cols] == x[i, best[i]]).all())
            else:
                assert bool((first[cols] == first[best[i]]).all()), (n, g, s, i, cols)
        exp = X.argmax_ref(c.Q, c.D, s["scale"])
        assert np.array_equal(X.emu_infonce_fwd(c.Q, c.D, c.labels, s["scale"])[2], exp)
        for row, a, b in c.ties:
            assert exp[row] == a and np.array_equal(c.D[a], c.D[b]) and near[row, b]
            routes.add((a, b))
        if c.last_row is not None:
            assert exp[c.last_row] == g - 1
            last += g % 64 != 0
    assert routes == {(1, 2), (17, 21), (10, 70), (10, 138)} and last >= 10
    assert (1 % 8 < 4) and (2 % 8 < 4) and (17 % 8 < 4) != (21 % 8 < 4) and 10 // 64 != 70 // 64 and 10 // 128 != 138 // 128


def test_label_builder():
    for n, g, _ in X.fwd_cases() + X.bwd_cases():
        for rot in range(8):
            lab = X.labels_for(n, g, rot)
            assert lab.dtype == np.int64 and lab.shape == (n,) and 0 <= lab.min() and lab.max() < g
    lab = X.labels_for(33, 260)
    assert lab[:8].tolist() == [0, 259, 63, 64, 127, 128, 2, 5] and lab[8] == lab[0]         # every special column; two rows share one
    assert {int(v) % 8 < 4 for v in lab[:8]} == {True, False}                               # both lane halves
    assert lab[9:].tolist() == [i * (260 // 33) for i in range(9, 33)]                      # the recipe
    assert X.labels_for(260, 65)[9:].tolist() == [i % 65 for i in range(9, 260)]
    assert X.labels_for(1, 260, 1).tolist() == [259] and X.labels_for(4, 3).tolist() == [0, 2, 0, 0]
    seen = {int(v) for n, g, s in X.fwd_cases() if g == 260 and n == 1 for v in X.labels_for(n, g, s["rot"])}
    assert len(seen) >= 4                                               # the rotation moves the one label of N = 1 over the specials


def test_case_lists_cover_the_issue():
    f, b, k = X.fwd_cases(), X.bwd_cases(), X.simkl_cases()
    assert {c[0] for c in f} == set(X.FWD_N) and {c[1] for c in f} == set(X.FWD_G) and {(260, 260), (1, 1), (1, 260), (260, 1)} <= {c[:2] for c in f}
    assert {(c[2]["dim"], c[2]["pads"]) for c in f} == {(d, p) for d in X.DIMS for p in X.LD_PADS}
    assert {(c[2]["family"], c[2]["scale"]) for c in f} >= set(X.FWD_SETTINGS)
    assert {c[:2] for c in b} == {(n, g) for n in X.BWD_N for g in X.BWD_G} and {c[2]["dim"] for c in b} == set(X.DIMS)
    assert {c[2]["family"] for c in b} == set(X.FAMILIES) and {c[2]["scale"] for c in b} == set(X.SCALES)
    assert {c[:2] for c in k} == {(n, g) for n in X.SIMKL_N for g in X.SIMKL_G} and {c[2:4] for c in k} == set(X.SIMKL_DIMS)
    assert {c[4] for c in k} == set(X.INV_TEMPS) and len({c[6] for c in k}) >= 8
