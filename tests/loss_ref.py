"""References, bounds, inputs and labels of the exact-fp32 loss kernels (contrastors_amd/csrc/infonce.hip): cx_sgemm_nt,
cx_infonce_fwd / _fwd_argmax / _bwd, cx_simkl_fwd / _bwd.  Plain numpy (fp64 and emulated fp32), no kernel: tests/test_loss_ref_cpu.py
proves this file and measures its constants, tests/test_loss_edges_gpu.py holds the kernels to it.

Bit-exact part.  fmaf() is a correctly rounded fp32 fused multiply-add: the product of two fp32 values is exact in fp64 (48 bits),
the addend is added with a TwoSum, a non-zero error term moves an even sum to its odd neighbour on the error's side (round to odd),
and the result is rounded to fp32 once.  53 >= 2 * 24 + 2, so the double rounding is innocuous.  sgemm_chain(A, B) is C = A B^T as
the chain of fmaf that sgemm_tile (infonce.hip) issues per accumulator: K in blocks of 16, inside a block g = 0, 1, then e = 0 .. 3,
each MFMA consuming k = 8 g + e (lane half 0) and then k = 8 g + 4 + e (lane half 1): K_ORDER = 0 4 1 5 2 6 3 7 8 12 9 13 10 14 11 15.
A zero-filled chunk at k >= K contributes fma(+0, +0, acc) = acc + +0: it keeps every bit pattern but -0, which it turns into +0
(a sum of products that all underflow to nothing from below is -0 after K % 16 == 0 and +0 after a K tail), so it is applied.

Bounded part.  All references are fp64 on the fp32 inputs; scale, inv_temp and coef are taken at their fp32 values.  A result is held
to |got - ref| <= C 2^-24 T, C = 4 C_MEAS[name].  With u = 2^-24, K the contraction length, x_j = scale <q, d_j> the natural-log logit
of column j, A_j = sum_k |q_k d_jk|, m = max_j x_j, S = sum_j exp(x_j - m), p_j = exp(x_j - lse):
    the K-term fma chain leaves s_j within K u A_j, hence x_j within K u |scale| A_j;
    sc2 = scale log2(e) is rounded once and so is its product with s_j: 2 u |x_j|; the argument x_j - m is rounded once: u |x_j - m|;
    exp2f is good to an ulp or two: 2 u relative.  Together the relative error of one term of S, in units of u, is
        E_j = K |scale| A_j + 2 |x_j| + |x_j - m| + 2
    the sum of a row runs over 32 terms in a lane, one addition across the lane halves, the rescaling exp2f(pm - mx) and its
    product per 64-column slice and the fold of the nparts slices across a wave: ADDS = 32 + 1 + 3 + 6 + nparts / 64 <= 48 roundings,
    each relative to a partial sum of positive terms <= S;
    lse = (mx + log2f(S)) ln 2: log2f, the addition and the product round at the magnitude of |m| + |log S| and |lse|.
        T_lse  = sum_j p_j E_j + ADDS + |m| + |log S| + |lse|
        T_loss = T_lse + K |scale| A_lab + 2 |x_lab| + |lse| + |x_lab|         (lab = scale s_lab is rounded twice; the difference once)
    T_loss is absolute in |lse| + |lab|: a row whose positive dominates has a loss near 0 and no relative accuracy in it.
    Gm_ij = coef scale (exp2f(s sc2 - lse2) - [j = label]), from the fp32 lse the kernel is FED (a_j = x_j - lse):
        T_g = |coef scale| (p_j (K |scale| A_j + 2 |x_j| + 2 |lse| + |a_j| + 2) + 3 |p_j - hot_j|)  (+ |coef scale| 2^-126: an
        exponential below the smallest normal has no relative accuracy).
    simkl, t = c <qt, dt_j> (teacher), s = c <qs, ds_j> (student), p = softmax t, q = softmax s, df_j = t_j - s_j:
        T_lse_s, T_lse_t as T_lse;   with R_x = sum_j p_j E_j + ADDS of either side,
        T_kl = sum_j p_j (c (K_t A^t_j + K_s A^s_j) + 2 |df_j|) + sum_j p_j |df_j| (E^t_j + ADDS) + |sum_j p_j df_j| R_t
               + R_s + R_t + 2 |m_s - m_t| + 2 |log(S_s / S_t)| + |kl|
        T_g  = |coef c| (q_j F^s_j + p_j F^t_j + 3 |q_j - p_j|),  F_j = K c A_j + 2 |x_j| + 2 |lse| + |x_j - lse| + 2  (+ the floor twice).
C_MEAS (test_loss_ref_cpu.py::test_measured_constants, rounded up) is the worst |emulation - fp64| / (2^-24 T) of emu_infonce_fwd,
emu_infonce_gm, emu_simkl_fwd and emu_simkl_gm below -- sgemm_chain, then per-slice maximum, sum and fold in fp32 numpy in the kernel's
order -- over every case of fwd_cases(), bwd_cases() and simkl_cases(): never measured against a kernel.
    C_MEAS = lse 0.40, loss 0.30, gm 0.55, lse_s 0.20, lse_t 0.25, kl 0.02, simkl_gm 0.28   (the table C_MEAS below; T is a worst-case
    first-order bound, so the measured figures are below 1)

dscale is reduced with wave_sum and one fp32 atomic per wave: its summation order is free, and so is its bound:
    |got - ref| <= 4 (N G + K) 2^-24 sum_ij |coef pr_ij s_ij|,   pr = p - hot  (reference and sum from the lse the kernel is fed).
It has no term for the error of the exponent's argument (2 |x| 2^-24 relative in p from rounding sc2 and its product alone), which
N G + K covers once there are a few hundred terms; at N = G = 4, dim 16, scale 100 (N G + K = 32) that error by itself is 1.03 of the
bound in the fp32 emulation.  The GPU test starts dscale at 0.75 and grants the roundings of that start in each of the 4 nwg atomics
of a call, 4 nwg 2^-24 (|start| + 2 |dscale| + 2 bound) per call; with it the kernel's worst case is that shape, at 0.93.

Argmax.  The first index of the row maximum is demanded on EVERY row, so every case is built (fix_gaps) such that the two best fp64
logits of a row differ by at least 2 logit_bound = 2 * 4 (K + 2) u |scale| max_j A_j, unless the runner-up is an exact tie: a
duplicated document row (make_case), a zero query row, or the integer family (entries k / 8, |k| <= 7, dim <= 36: every partial sum
is a multiple of 1 / 64 below 2^24 / 64, exact in fp32 and fp64 in any order).  argmax_ref() returns the first column within that
distance of the maximum; test_loss_ref_cpu.py asserts that each such column is one of those exact ties.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
LOG2E_F32 = F32(1.4426950408889634)
LN2_F32 = F32(0.6931471805599453)
F32_MIN_NORMAL = 2.0 ** -126
C_FACTOR = 4.0
# worst |fp32 emulation - fp64| / (2^-24 T) over every case the GPU tests run (test_loss_ref_cpu.py::test_measured_constants), rounded up
C_MEAS = {"lse": 0.40, "loss": 0.30, "gm": 0.55, "lse_s": 0.20, "lse_t": 0.25, "kl": 0.02, "simkl_gm": 0.28}
K_ORDER = (0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15)
ADDS = 48.0


def C(name: str) -> float:
    return C_FACTOR * C_MEAS[name]


def f32(v):
    """A Python number as the fp32 value a kernel receives it as, in fp64."""
    return float(F32(v))


# =================================================================================================== bit-exact fp32 fma
def fmaf(a, b, c):
    """Correctly rounded fp32 a * b + c of fp32 arrays (finite, no overflow): exact product, TwoSum, round to odd, one rounding."""
    a, b, c = (np.asarray(t, dtype=F32).astype(F64) for t in (a, b, c))
    p = a * b                                   # exact: 24 x 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)             # TwoSum: s + err = p + c exactly
    sb = np.atleast_1d(s).copy().view(np.int64)
    e1 = np.atleast_1d(err)
    fix = (e1 != 0) & ((sb & 1) == 0)
    # the odd neighbour on the side of the error: one step away from zero when err and s agree in sign, else one step towards it
    away = (e1 > 0) == (np.atleast_1d(s) > 0)
    sb += np.where(fix, np.where(away, 1, -1), 0)
    return sb.view(F64).reshape(np.shape(s)).astype(F32)


def sgemm_chain(A, B, order=K_ORDER):
    """C (M, N) fp32 = A (M, K) B (N, K)^T with the bits of sgemm_tile: one fmaf per k, in blocks of 16 walked in `order`."""
    A, B = np.ascontiguousarray(A, dtype=F32), np.ascontiguousarray(B, dtype=F32)
    (M, K), N = A.shape, B.shape[0]
    assert B.shape[1] == K and K % 4 == 0
    acc = np.zeros((M, N), dtype=F32)
    for k0 in range(0, K, 16):
        for j in order:
            k = k0 + j
            acc = fmaf(A[:, k:k + 1], B[None, :, k], acc) if k < K else acc + F32(0)      # the zero-filled chunk: -0 becomes +0
    return acc


# ======================================================================================================= fp64 references
Fwd = namedtuple("Fwd", "lse t_lse loss t_loss x absx m logS p e_rel")


def _rows(Q, D, scale, K=None):
    """x = scale Q D^T, |scale| |Q| |D|^T, and the per-term relative error E (see the docstring), fp64."""
    q, d = Q.astype(F64), D.astype(F64)
    sc = f32(scale)
    K = Q.shape[1] if K is None else K
    x, ax = sc * (q @ d.T), abs(sc) * (np.abs(q) @ np.abs(d).T)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    S = e.sum(1, keepdims=True)
    p = e / S
    e_rel = K * ax + 2 * np.abs(x) + np.abs(x - m) + 2
    return x, ax, m[:, 0], np.log(S[:, 0]), p, e_rel


def infonce_fwd_ref(Q, D, labels, scale):
    x, ax, m, logS, p, e_rel = _rows(Q, D, scale)
    K, rows = Q.shape[1], np.arange(Q.shape[0])
    lse = m + logS
    t_lse = (p * e_rel).sum(1) + ADDS + np.abs(m) + np.abs(logS) + np.abs(lse)
    xl = x[rows, labels]
    t_loss = t_lse + K * ax[rows, labels] + 3 * np.abs(xl) + np.abs(lse)
    return Fwd(lse, t_lse, lse - xl, t_loss, x, ax, m, logS, p, e_rel)


def _gm(Q, D, scale, lse_fed, k):
    """softmax from the fed lse, and F = K |scale| A + 2 |x| + 2 |lse| + |x - lse| + 2."""
    q, d = Q.astype(F64), D.astype(F64)
    sc = f32(scale)
    s = q @ d.T
    x, ax = sc * s, abs(sc) * (np.abs(q) @ np.abs(d).T)
    l = np.asarray(lse_fed, dtype=F64)[:, None]
    a = x - l
    p = np.exp(a)
    return s, p, Q.shape[1] * ax + 2 * np.abs(x) + 2 * np.abs(l) + np.abs(a) + 2


def infonce_bwd_ref(Q, D, labels, lse_fed, scale, coef):
    """-> Gm, T_g (+ floor inside), dscale increment, its bound (complete: margin included)."""
    N, G = Q.shape[0], D.shape[0]
    s, p, F = _gm(Q, D, scale, lse_fed, None)
    hot = np.zeros((N, G))
    hot[np.arange(N), labels] = 1.0
    k = f32(coef) * f32(scale)
    pr = p - hot
    gm = k * pr
    t = abs(k) * (p * F + 3 * np.abs(pr))
    terms = f32(coef) * pr * s
    ds_bound = C_FACTOR * (N * G + Q.shape[1]) * U * np.abs(terms).sum()
    return gm, t, abs(k) * F32_MIN_NORMAL, terms.sum(), ds_bound


Simkl = namedtuple("Simkl", "lse_s t_lse_s lse_t t_lse_t kl t_kl")


def simkl_fwd_ref(Qs, Ds, Qt, Dt, inv_temp):
    xs, axs, ms, logSs, q, es = _rows(Qs, Ds, inv_temp)
    xt, axt, mt, logSt, p, et = _rows(Qt, Dt, inv_temp)
    lse_s, lse_t = ms + logSs, mt + logSt
    r_s, r_t = (q * es).sum(1) + ADDS, (p * et).sum(1) + ADDS
    t_lse_s = r_s + np.abs(ms) + np.abs(logSs) + np.abs(lse_s)
    t_lse_t = r_t + np.abs(mt) + np.abs(logSt) + np.abs(lse_t)
    df = xt - xs
    pdf = (p * df).sum(1)
    kl = pdf - lse_t + lse_s
    t_kl = ((p * (Qt.shape[1] * axt + Qs.shape[1] * axs + 2 * np.abs(df))).sum(1) + (p * np.abs(df) * (et + ADDS)).sum(1) + np.abs(pdf) * r_t
            + r_s + r_t + 2 * np.abs(ms - mt) + 2 * np.abs(logSs - logSt) + np.abs(kl))
    return Simkl(lse_s, t_lse_s, lse_t, t_lse_t, kl, t_kl)


def simkl_bwd_ref(Qs, Ds, Qt, Dt, lse_s_fed, lse_t_fed, inv_temp, coef):
    _, q, Fs = _gm(Qs, Ds, inv_temp, lse_s_fed, None)
    _, p, Ft = _gm(Qt, Dt, inv_temp, lse_t_fed, None)
    k = f32(coef) * f32(inv_temp)
    return k * (q - p), abs(k) * (q * Fs + p * Ft + 3 * np.abs(q - p)), 2 * abs(k) * F32_MIN_NORMAL


def logit_bound(Q, D, scale):
    """Per row: 4 (K + 2) u |scale| max_j A_j, the derived bound of one fp32 logit (nothing measured)."""
    ax = abs(f32(scale)) * (np.abs(Q.astype(F64)) @ np.abs(D.astype(F64)).T)
    return C_FACTOR * (Q.shape[1] + 2) * U * ax.max(1)


def near_max(Q, D, scale):
    """(x, boolean (N, G): the columns within 2 logit_bound of the row maximum)."""
    x = f32(scale) * (Q.astype(F64) @ D.astype(F64).T)
    return x, x >= x.max(1, keepdims=True) - 2 * logit_bound(Q, D, scale)[:, None]


def argmax_ref(Q, D, scale):
    """The first column within 2 logit_bound of the row maximum (the CPU test proves each of them an exact tie of the maximum)."""
    return near_max(Q, D, scale)[1].argmax(1).astype(np.int32)


def ratio(got, ref, t, c, floor=0.0):
    """Worst |got - ref| / (c 2^-24 T + floor) (inf for a NaN)."""
    err = np.abs(np.asarray(got, dtype=F64) - ref)
    r = err / (c * U * t + floor)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


class Mismatch(AssertionError):
    pass


def check(name, got, ref, t, c, floor=0.0):
    """Every element: |got - ref| <= c 2^-24 T + floor (a NaN fails).  Raises Mismatch naming the first failing index; returns
    the worst err / bound."""
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bound = np.broadcast_to(c * U * np.asarray(t, dtype=F64) + floor, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise Mismatch(f"{name}: first mismatch at index {i}: got {got[i]!r}, reference {ref[i]!r}, |err| {err[i]:.3e} > bound "
                       f"{bound[i]:.3e}; {int(bad.sum())} of {bad.size} elements fail")
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    return float(r.max()) if r.size else 0.0


# ============================================================================================ fp32 emulations of the kernels
def _lane_sums(e):
    """e (N, parts, 64) fp32 -> (N, parts): lane half hi holds the columns with (col % 8) // 4 == hi and adds them in column order
    from 0; the two halves are added (hi 0 + hi 1)."""
    N, P, _ = e.shape
    v = e.reshape(N, P, 8, 2, 4).transpose(0, 1, 3, 2, 4).reshape(N, P, 2, 32)
    acc = np.zeros((N, P, 2), dtype=F32)
    for i in range(32):
        acc = acc + v[..., i]
    return acc[..., 0] + acc[..., 1]


def _pad_slices(z, fill):
    N, G = z.shape
    parts = 2 * ((G + 127) // 128)
    out = np.full((N, parts * 64), fill, dtype=F32)
    out[:, :G] = z
    return out.reshape(N, parts, 64)


def _wave_fold(v):
    """(N, parts <= 64) -> (N,): lane i holds slice i (0 beyond), xor butterfly 32 .. 1."""
    N, P = v.shape
    w = np.zeros((N, 64), dtype=F32)
    w[:, :P] = v
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    return w[:, 0]


def _emu_partials(acc, c2, extra=None):
    """acc (N, G) fp32 products -> per-slice (max, sum[, sum of et * extra]) in log2 units, as EPI_LSE / simkl_kernel<FWD> form them."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        z = _pad_slices(acc * c2, -np.inf)
        pm = z.max(2)
        live = np.isfinite(pm)
        e = np.where(live[..., None], np.exp2(z - np.where(live, pm, F32(0))[..., None]), F32(0)).astype(F32)
        ps = _lane_sums(e)
        pa = None if extra is None else _lane_sums((e * _pad_slices(extra, 0.0)).astype(F32))
    return pm, ps, pa, live


def _emu_fold(pm, ps, pa, live):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        mx = pm.max(1)
        w = np.where(live, np.exp2(pm - mx[:, None]), F32(0)).astype(F32)
        l = _wave_fold(np.where(live, ps * w, F32(0)).astype(F32))
        a = None if pa is None else _wave_fold(np.where(live, pa * w, F32(0)).astype(F32))
    return mx, l, a


def emu_infonce_fwd(Q, D, labels, scale, order=K_ORDER):
    """-> lse, loss_rows, argmax (first index) in fp32, in the kernels' operation order."""
    acc = sgemm_chain(Q, D, order)
    sc = F32(scale)
    pm, ps, _, live = _emu_partials(acc, F32(sc * LOG2E_F32))
    mx, l, _ = _emu_fold(pm, ps, None, live)
    lse = ((mx + np.log2(l)) * LN2_F32).astype(F32)
    lab = (acc[np.arange(Q.shape[0]), labels] * sc).astype(F32)
    v = (acc * F32(sc * LOG2E_F32)).astype(F32)
    return lse, (lse - lab).astype(F32), v.argmax(1).astype(np.int32)


def emu_infonce_gm(Q, D, labels, lse_fed, scale, coef, order=K_ORDER):
    """-> Gm fp32 and dscale (one fp32 summation order of many) as EPI_GRAD forms them."""
    acc = sgemm_chain(Q, D, order)
    sc, cf = F32(scale), F32(coef)
    lse2 = (np.asarray(lse_fed, dtype=F32) * LOG2E_F32).astype(F32)[:, None]
    hot = np.zeros(acc.shape, dtype=F32)
    hot[np.arange(acc.shape[0]), labels] = 1
    with np.errstate(under="ignore"):
        pr = (np.exp2(fmaf(acc, F32(sc * LOG2E_F32), -lse2)) - hot).astype(F32)
        gm = ((pr * cf).astype(F32) * sc).astype(F32)
        ds = np.float32(0)
        for row in ((pr * acc).astype(F32) * cf).astype(F32):
            ds = F32(ds + row.sum(dtype=F32))
    return gm, ds


def emu_simkl_fwd(Qs, Ds, Qt, Dt, inv_temp, order=K_ORDER):
    at, as_ = sgemm_chain(Qt, Dt, order), sgemm_chain(Qs, Ds, order)
    c = F32(inv_temp)
    c2 = F32(c * LOG2E_F32)
    df = ((at - as_).astype(F32) * c).astype(F32)
    pmt, plt, pat, live = _emu_partials(at, c2, df)
    pms, pls, _, _ = _emu_partials(as_, c2)
    mt, lt, a = _emu_fold(pmt, plt, pat, live)
    ms, ls, _ = _emu_fold(pms, pls, None, live)
    lse_t = ((mt + np.log2(lt)) * LN2_F32).astype(F32)
    lse_s = ((ms + np.log2(ls)) * LN2_F32).astype(F32)
    kl = (a / lt + ((ms - mt) + np.log2((ls / lt).astype(F32))) * LN2_F32).astype(F32)
    return lse_s, lse_t, kl


def emu_simkl_gm(Qs, Ds, Qt, Dt, lse_s_fed, lse_t_fed, inv_temp, coef, order=K_ORDER):
    at, as_ = sgemm_chain(Qt, Dt, order), sgemm_chain(Qs, Ds, order)
    c = F32(inv_temp)
    c2, k = F32(c * LOG2E_F32), F32(F32(coef) * c)
    ls2 = (np.asarray(lse_s_fed, dtype=F32) * LOG2E_F32).astype(F32)[:, None]
    lt2 = (np.asarray(lse_t_fed, dtype=F32) * LOG2E_F32).astype(F32)[:, None]
    with np.errstate(under="ignore"):
        qs, pt = np.exp2(fmaf(as_, c2, -ls2)), np.exp2(fmaf(at, c2, -lt2))
        return ((qs - pt).astype(F32) * k).astype(F32)


# ====================================================================================================== labels and inputs
LABEL_SPECIALS = (0, -1, 63, 64, 127, 128, 2, 5)      # -1: G - 1; 2 and 5: a column of each lane half (col % 8 < 4, >= 4)


def labels_for(N, G, rot=0):
    """int64 (N): the special columns that exist for this G -- 0, G - 1, 63, 64, 127, 128, one column of each lane half -- on the
    first rows (starting with special `rot`), the next row sharing the label of row 0, the recipe's i * (G // N) (i mod G where
    G < N) on the others."""
    sp = []
    for c in LABEL_SPECIALS:
        c = G - 1 if c < 0 else c
        if c < G and c not in sp:
            sp.append(c)
    lab = np.array([i * (G // N) if G >= N else i % G for i in range(N)], dtype=np.int64)
    for i in range(min(N, len(sp) + 1)):
        lab[i] = sp[(i + rot) % len(sp)]
    return lab


FAMILIES = ("gauss", "positive", "zero", "wide", "ints")
SGEMM_FAMILIES = ("gauss", "ints")      # cx_sgemm_nt: Gaussian (the k order shows in the bits) and integers (dim <= 36: exact in any order)
TIE_SETS = (((1, 2), (17, 21), (10, 70)), ((1, 2), (17, 21), (10, 138)))   # one lane; the two lane halves; two slices / two tiles
Case = namedtuple("Case", "Q D labels ties last_row zero_rows family")


def _unit(v):
    n = np.sqrt((v.astype(F64) ** 2).sum(-1, keepdims=True))
    return (v / np.where(n == 0, 1.0, n)).astype(F32)


def base_inputs(N, G, dim, family, seed):
    rng = np.random.default_rng(seed * 1000003 + N * 4099 + G * 17 + dim)
    if family == "ints":
        assert dim <= 36
        return (rng.integers(-7, 8, (N, dim)) / 8.0).astype(F32), (rng.integers(-7, 8, (G, dim)) / 8.0).astype(F32)
    Q, D = _unit(rng.standard_normal((N, dim))), _unit(rng.standard_normal((G, dim)))
    if family == "wide":
        D = (D * F32(8.0)).astype(F32)          # logits in +-8 scale: at scale 50 and 100 exp2f of most terms underflows
    return Q, D


def first_copy(D):
    """(G,): the index of the first row of D with the bits of row j (j itself where the row is not a duplicate)."""
    seen, out = {}, np.empty(D.shape[0], dtype=np.int64)
    for j, r in enumerate(np.ascontiguousarray(D)):
        out[j] = seen.setdefault(r.tobytes(), j)
    return out


def fix_gaps(Q, D, scale, exact_rows=(), rounds=60):
    """Nudge a query towards its best document until the two best fp64 logits differ by 2 logit_bound, leaving alone the rows
    whose runner-up is an exact tie of the maximum.  Deterministic; returns the new Q."""
    Q = Q.copy()
    rows = np.arange(Q.shape[0])
    for _ in range(rounds):
        x, near = near_max(Q, D, scale)
        best = x.argmax(1)
        bad = (near & (first_copy(D)[None, :] != first_copy(D)[best][:, None])).any(1) & ~np.isin(rows, list(exact_rows))
        if not bad.any():
            return Q
        for i in np.nonzero(bad)[0]:
            d = D[best[i]].astype(F64)
            qn = np.sqrt((Q[i].astype(F64) ** 2).sum())
            Q[i] = (Q[i].astype(F64) + 0.05 * qn * d / np.sqrt((d ** 2).sum())).astype(F32)
    raise AssertionError("fix_gaps did not converge")


@functools.lru_cache(maxsize=None)
def make_case(N, G, dim, family, scale, seed=0, tie_set=0, rot=0):
    """One seeded case.  Planted, from the last row upwards where N and G allow: a row whose maximum is column G - 1, then one row
    per pair of TIE_SETS[tie_set] whose two columns hold the SAME document row and whose query is that document (an exact tie of the
    maximum, first index expected).  "positive": every other query is its label's document (scale 100: loss near 0);
    "zero": query row 0 is all zero (lse = log G, every column ties, arg max 0)."""
    Q, D = base_inputs(N, G, dim, family, seed)
    Q, D = Q.copy(), D.copy()
    labels = labels_for(N, G, rot)
    pairs = [(a, b) for a, b in TIE_SETS[tie_set] if b < G]
    if family == "ints":      # a planted document of the integer family is a +-7/8 sign vector: no other row reaches its square
        for i, j in enumerate([a for a, _ in pairs] + [G - 1]):      # distinct patterns: the low bits of seed + G + i
            D[j] = (((seed + G + i) >> (np.arange(dim) % 4)) & 1) * F32(1.75) - F32(0.875)
    for a, b in pairs:
        D[b] = D[a]
    dup_cols = {c for pr in pairs for c in pr}
    if family == "positive":
        Q = _unit(D[labels])
    zero_rows = (0,) if family == "zero" else ()
    row, ties, last_row = N - 1, [], None
    free = lambda r: r >= 0 and r not in zero_rows          # noqa: E731
    unit = (lambda v: v.copy()) if family == "ints" else _unit
    if G - 1 not in dup_cols and free(row) and np.any(D[G - 1] != 0):
        Q[row], last_row = unit(D[G - 1]), row
        row -= 1
    for a, b in pairs:
        if free(row) and np.any(D[a] != 0):
            Q[row] = unit(D[a])
            ties.append((row, a, b))
            row -= 1
    for r in zero_rows:
        Q[r] = 0
    if family != "ints":
        Q = fix_gaps(Q, D, scale, exact_rows=[t[0] for t in ties] + list(zero_rows))
    for t in (Q, D, labels):
        t.setflags(write=False)
    return Case(Q, D, labels, tuple(ties), last_row, zero_rows, family)


# ================================================================================================================ shapes
FWD_N = (1, 31, 33, 64, 127, 129, 260)
FWD_G = (1, 3, 63, 64, 65, 127, 129, 192, 260)
DIMS = (4, 12, 16, 20, 36, 128)
BWD_N = (4, 36, 128, 132, 260)
BWD_G = (4, 60, 64, 68, 132, 192, 260)
SIMKL_N = (33, 132)
SIMKL_G = (65, 132, 192, 260)
SIMKL_DIMS = ((20, 36), (128, 64), (16, 16))
SCALES = (1.0, 50.0, 100.0)
INV_TEMPS = (5.0, 50.0)
LD_PADS = ((0, 0), (4, 0), (0, 4), (4, 4))
# (family, scale): every family, every scale; the dominant positive at 100; the wide family where exp2f underflows
FWD_SETTINGS = (("gauss", 1.0), ("gauss", 50.0), ("gauss", 100.0), ("positive", 100.0), ("zero", 50.0), ("wide", 100.0), ("wide", 50.0),
                ("ints", 1.0), ("ints", 100.0), ("zero", 1.0), ("positive", 50.0))


def fwd_shapes():
    s = [(n, g) for g in (65, 260) for n in FWD_N] + [(n, g) for n in (33, 129) for g in FWD_G] + [(1, 1), (260, 1)]
    return tuple(dict.fromkeys(s))


def bwd_shapes():
    return tuple((n, g) for n in BWD_N for g in BWD_G)


def simkl_shapes():
    return tuple((n, g) for n in SIMKL_N for g in SIMKL_G)


def coef_for(N, i):
    return 1.0 / N if i % 2 == 0 else 2.5


def settings(si):
    """The six runs of shape number si: one per dim, with (family, scale), the leading-dimension pads, the tie set and the label
    rotation cycling so that every value meets every dim over the shapes (11 settings and 6 dims are coprime)."""
    out = []
    for di, dim in enumerate(DIMS):
        fam, scale = FWD_SETTINGS[(si * len(DIMS) + di) % len(FWD_SETTINGS)]
        if fam == "ints" and dim > 36:
            fam = "gauss"
        out.append(dict(dim=dim, family=fam, scale=scale, pads=LD_PADS[(si + di) % 4], tie_set=(si + di) % 2, rot=(si + di) % 8,
                        coef_i=si + di))
    return out


def fwd_cases():
    """Every (N, G, setting) the forward GPU tests run."""
    return [(n, g, s) for si, (n, g) in enumerate(fwd_shapes()) for s in settings(si)]


def bwd_cases():
    """Three runs per backward shape (dims cycling in pairs so that all six appear at every other shape)."""
    out = []
    for si, (n, g) in enumerate(bwd_shapes()):
        ss = settings(si)
        out += [(n, g, s) for s in ss[si % 2::2]]
    return out


def simkl_cases():
    """(N, G, dim_s, dim_t, inv_temp, family, pads4, coef index): three runs per shape, one per width pair."""
    out = []
    for si, (n, g) in enumerate(simkl_shapes()):
        for wi, (ds_, dt_) in enumerate(SIMKL_DIMS):
            k = si * 3 + wi
            fam = ("gauss", "wide", "ints", "zero")[k % 4]
            if fam == "ints" and max(ds_, dt_) > 36:
                fam = "gauss"
            pads = tuple(4 * ((k >> b) & 1) for b in range(4))
            out.append((n, g, ds_, dt_, INV_TEMPS[k % 2], fam, pads, k))
    return out


@functools.lru_cache(maxsize=None)
def simkl_inputs(N, G, dim_s, dim_t, family, seed):
    Qs, Ds = base_inputs(N, G, dim_s, family, seed + 11)
    Qt, Dt = base_inputs(N, G, dim_t, family, seed + 12)
    if family == "zero":
        Qs, Qt = Qs.copy(), Qt.copy()
        Qs[0], Qt[N - 1] = 0, 0
    for t in (Qs, Ds, Qt, Dt):
        t.setflags(write=False)
    return Qs, Ds, Qt, Dt
