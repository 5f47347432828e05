"""fp64 reference of the LayerNorm family (contrastors_amd/csrc/layernorm.hip), the seeded inputs of its edge tests, and the
row-wise checker they share.  Plain torch, any device, no autograd: tests/test_ln_ref_cpu.py checks this file against
torch.nn.functional.layer_norm in fp64 and measures the constants below; tests/test_layernorm_edges_gpu.py holds the kernels
to it.

Bounds.  A kernel result is compared per element with the fp64 value `ref` under
    bf16 result:  |got - ref| <= 0.5 * bf16_ulp(ref) + C * 2^-24 * S
    fp32 result:  |got - ref| <=                       C * 2^-24 * S
where S is the magnitude scale of the terms the element is built from (returned by the reference next to the value: results
that cancel have |ref| << S and an fp32 kernel cannot do better than 2^-24 * S).  C = 4 * C_MEAS[...]: C_MEAS is the worst
ratio err / (2^-24 * S) of an fp32 emulation of the kernel's arithmetic (fp32 statistics, the same formula, one final bf16
rounding; torch on the CPU) against this reference, on these inputs; the factor 4 covers the reduction order of a 64-lane
butterfly versus torch's sum, the only arithmetic the emulation does not reproduce.  The constants are measured against the
fp64 reference, never against a kernel; test_ln_ref_cpu.py asserts them, so that changing the inputs re-measures them.
"""
from __future__ import annotations

from collections import namedtuple

import torch

EPS24 = 2.0 ** -24
WIDTHS = (256, 512, 768, 1024)

# worst err / (2^-24 * scale) of the fp32 emulation (tests/test_ln_ref_cpu.py::test_measured_constants), rounded up.
# "out" of the forward families is huge because S = |xhat g| + |b| does not contain the term that dominates the forward's fp32
# error on rows with |mean| >> sigma (mu = -4, sigma = 2^-6: mean|z| rstd ~ 250): the rounding of the row mean, 2^-24 mean|z|,
# reaches every element of the row times rstd |gamma|, also those whose S happens to be ~ 1e-4.  A bound of 4 * 3e6 * 2^-24 S
# = 0.7 S holds a kernel to nothing, so check_out() applies it TOGETHER with the bound on scale_tight = S + mean|z| rstd |gamma|
# ("out_tight": a few units, as an fp32 kernel should be), never a wider one than either.
C_MEAS = {
    "fwd": {"out": 3.0e6, "out_tight": 4.5, "mean": 3.6, "rstd": 4.2},
    "fwd_f32": {"out": 3.7e6, "out_tight": 5.0, "mean": 3.9, "rstd": 5.5},
    "fwd_rms": {"out": 5.6, "rstd": 3.2},
    "fwd_drop": {"out": 9600.0, "out_tight": 4.8, "mean": 3.5, "rstd": 3.7},
    "bwd": {"dz": 160.0, "dgamma": 4.0, "dbeta": 3.0, "colsum": 1.1},
    "bwd_rms": {"dz": 820.0, "dgamma": 3.8, "dbeta": 3.0},
    "bwd_drop": {"dz": 115.0, "dx0": 115.0, "dgamma": 3.6, "dbeta": 0.5, "colsum": 1.0},
    "pooled": {"dz": 300.0, "dgamma": 6.2, "dbeta": 12.0, "colsum": 4.3},
    # the embedding kernels: z = (word + pos) + type is an exact fp32 sum the host reproduces, so these are fwd_f32 / bwd on
    # the embedding inputs; "scatter" = dtype0 / dpos / dword, sums of fp32 dz rows, against 2^-24 * sum of the rows' S
    # (a vocabulary row with one token receives that token's dz row: "scatter" cannot be below "dz")
    "embed_fwd": {"out": 1.8e4, "out_tight": 3.6, "mean": 3.6, "rstd": 2.9},
    "embed_bwd": {"dz": 102.0, "dgamma": 0.77, "dbeta": 0.44, "scatter": 102.0},
}
C_FACTOR = 4.0


def C(family: str, what: str) -> float:
    return C_FACTOR * C_MEAS[family][what]


# ------------------------------------------------------------------------------------------------------ bf16 helpers
def bf16_ulp(x):
    """Spacing of bf16 (8 significant bits) at |x|, as fp64; the spacing of the smallest normal binade below it."""
    x = torch.as_tensor(x, dtype=torch.float64)
    _, e = torch.frexp(x.abs())                     # |x| = m * 2^e, m in [0.5, 1)
    e = e.clamp(min=-125).to(torch.int64)
    return ((e - 8 + 1023) << 52).view(torch.float64)      # 2^(e - 8) assembled from its exponent field: exact on any device


def bf16_round(x64):
    """fp64 -> nearest bf16 value (ties to even) in ONE rounding, returned as fp64."""
    x64 = torch.as_tensor(x64, dtype=torch.float64)
    q = bf16_ulp(x64)
    return torch.round(x64 / q) * q                 # torch.round is half-to-even; x / q is exact (q is a power of two)


def bits(t):
    """Integer view of a bf16 / fp32 tensor for bit-exact comparisons (NaN payloads included)."""
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------------- references
FwdRef = namedtuple("FwdRef", "z mean rstd out scale scale_tight")
BwdRef = namedtuple("BwdRef", "dz dgamma dbeta scale dgamma_abs dbeta_abs")


def _d(t):
    return None if t is None else t.to(torch.float64)


def ln_fwd_ref(x0, res, gamma, beta, eps, rms=False):
    """z = x0 + res (no rounding), mean / rstd of each row, out = (z - mean) * rstd * gamma + beta; all fp64.
    rms: mean = 0, rstd = rsqrt(mean(z^2) + eps).  scale = S = |xhat gamma| + |beta|;  scale_tight = S + mean|z| rstd |gamma|."""
    x0, res, gamma, beta = _d(x0), _d(res), _d(gamma), _d(beta)
    z = x0 if res is None else x0 + res
    d = z.shape[-1]
    mean = torch.zeros(z.shape[0], dtype=torch.float64, device=z.device) if rms else z.sum(-1) / d
    c = z - mean[:, None]
    rstd = 1.0 / torch.sqrt((c * c).sum(-1) / d + eps)
    xhat = c * rstd[:, None]
    out = xhat * gamma
    scale = out.abs()
    if beta is not None:
        out = out + beta
        scale = scale + beta.abs()
    # the term S lacks: the fp32 rounding of the row mean (2^-24 mean|z|) reaches every element of the row times rstd |gamma|
    tight = scale if rms else scale + (z.abs().mean(-1) * rstd)[:, None] * gamma.abs()
    return FwdRef(z, mean, rstd, out, scale, tight)


def ln_bwd_ref(dout_a, dout_b, z_stored, gamma, mean, rstd, dz_extra, rms=False):
    """Closed form of the LayerNorm backward from the STORED z / mean / rstd the kernel is fed:
        dy = dout_a + dout_b, xhat = (z - mean) rstd, w = gamma dy, s1 = mean_j(w xhat), s2 = mean_j(w)  (0 under rms)
        dz = (w - s1 xhat - s2) rstd + dz_extra,  dgamma = sum_rows dy xhat,  dbeta = sum_rows dy
    scale = (|w| + |s1 xhat| + |s2|) rstd + |dz_extra| per element; dgamma_abs / dbeta_abs = sum_rows |term| per column."""
    dy = _d(dout_a) if dout_b is None else _d(dout_a) + _d(dout_b)
    z, gamma, mean, rstd, ex = _d(z_stored), _d(gamma), _d(mean), _d(rstd), _d(dz_extra)
    d = z.shape[-1]
    xhat = (z - mean[:, None]) * rstd[:, None]
    w = gamma * dy
    s1 = (w * xhat).sum(-1, keepdim=True) / d
    s2 = torch.zeros_like(s1) if rms else w.sum(-1, keepdim=True) / d
    dz = (w - s1 * xhat - s2) * rstd[:, None]
    scale = (w.abs() + (s1 * xhat).abs() + s2.abs()) * rstd[:, None]
    if ex is not None:
        dz = dz + ex
        scale = scale + ex.abs()
    t = dy * xhat
    return BwdRef(dz, t.sum(0), dy.sum(0), scale, t.abs().sum(0), dy.abs().sum(0))


def pooled_dout_ref(demb, emb, norm, cu, mode, normalize, rows=None):
    """The fp64 dout rows cx_layernorm_bwd_pooled builds internally: g_b = d(pooled vector) = demb_b, or under `normalize`
    (demb_b - emb_b <demb_b, emb_b>) / max(norm_b, 1e-12); row t of sequence b receives g_b / len_b (mean pooling, mode 0)
    or g_b on the first token and 0 elsewhere (cls pooling, mode 1).  Rows of no sequence stay 0."""
    demb, emb, norm = _d(demb), _d(emb), _d(norm)
    cu = [int(v) for v in cu.tolist()]
    T = cu[-1] if rows is None else rows
    dout = torch.zeros(T, demb.shape[-1], dtype=torch.float64, device=demb.device)
    for b in range(len(cu) - 1):
        t0, ln = cu[b], cu[b + 1] - cu[b]
        if ln <= 0:
            continue
        g = demb[b]
        if normalize:
            g = (g - emb[b] * (demb[b] * emb[b]).sum()) / max(float(norm[b]), 1e-12)
        if mode == 1:
            dout[t0] = g
        else:
            dout[t0:t0 + ln] = g / ln
    return dout


# ----------------------------------------------------------------------------------------------------------- inputs
MU = (-4.0, -1.0, 0.0, 0.5, 3.0)
SIGMA = (2.0 ** -6, 2.0 ** -3, 1.0, 4.0, 16.0)


def row_profile(rows, shift=0):
    """Per-row mean and scale: mu cycles with period 5, sigma with period 25 -- coprime to 4 (waves per block) and to every
    grid size of the launchers (powers of two and 768), so no two rows one grid stride apart look alike."""
    r = torch.arange(rows) + shift
    return torch.tensor(MU, dtype=torch.float64)[r % 5], torch.tensor(SIGMA, dtype=torch.float64)[(r + r // 5) % 5]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rows_like(rows, d, seed, centred=False, shift=0, dtype=torch.bfloat16):
    """(rows, d) of mu_r + sigma_r * randn (mu_r = 0 if centred), seeded, on the CPU, rounded once to `dtype`."""
    mu, sg = row_profile(rows, shift)
    x = torch.randn(rows, d, generator=_gen(seed), dtype=torch.float32).double() * sg[:, None]
    if not centred:
        x = x + mu[:, None]
    return x.to(torch.float32).to(dtype)


def params(d, seed=7):
    g = _gen(seed)
    return 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)


def fwd_inputs(rows, d, seed=100, dtype_x=torch.bfloat16, dtype_r=torch.bfloat16):
    """x0, res, gamma, beta: z = x0 + res has row mean mu_r and per-element deviation ~ sigma_r * sqrt(1.25)."""
    mu, sg = row_profile(rows)
    x0 = rows_like(rows, d, seed + d, dtype=dtype_x)
    res = (0.5 * rows_like(rows, d, seed + d + 1, centred=True).double()).to(torch.float32).to(dtype_r)
    return (x0, res) + params(d)


def drop_inputs(rows, d, seed=300):
    """x0 = +-(3 + 0.3 randn) (bounded away from 0: the mask is recoverable from z), res as usual."""
    g = _gen(seed + d)
    x0 = 3.0 + 0.3 * torch.randn(rows, d, generator=g).clamp(-4, 4)
    x0 = x0 * (torch.randint(0, 2, (rows, d), generator=g) * 2 - 1)
    res = rows_like(rows, d, seed + d + 1)
    return (x0.to(torch.bfloat16), res) + params(d)


def recover_mask(z_out, res, x0, p):
    """keep[r, c] from the kernel's own z = x0 * keep / (1 - p) + res: |x0| / (1 - p) >= 1.8 / 0.9 = 2, while a bf16 z of
    magnitude < 128 is within 0.25 of the exact sum."""
    return (z_out.double() - res.double()).abs() > 1.0


def bwd_inputs(rows, d, seed=200, dtype_dy=torch.bfloat16, dtype_z=torch.bfloat16, rms=False, eps=1e-12):
    """dout_a, dout_b, dz_extra, the stored z, and mean / rstd = the fp64 statistics of the stored z rounded to fp32 (what a
    forward hands to the backward, without running one).  Returns a dict of CPU tensors."""
    x0, res, gamma, _ = fwd_inputs(rows, d, seed)
    z = (x0.float() + res.float()).to(dtype_z)
    st = ln_fwd_ref(z, None, gamma, None, eps, rms=rms)
    return dict(
        da=rows_like(rows, d, seed + d + 2, centred=True, shift=2, dtype=dtype_dy),
        db=rows_like(rows, d, seed + d + 3, centred=True, shift=3, dtype=dtype_dy),
        ex=torch.randn(rows, d, generator=_gen(seed + d + 4)).to(dtype_z),
        z=z, gamma=gamma, mean=st.mean.float(), rstd=st.rstd.float())


def pooled_inputs(lens, d, seed=400, eps=1e-12):
    """cu, demb, emb (unit rows), norm, z, gamma, mean, rstd for cx_layernorm_bwd_pooled."""
    T, B = sum(lens), len(lens)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32)
    g = _gen(seed + d)
    demb = torch.randn(B, d, generator=g)
    emb = torch.nn.functional.normalize(torch.randn(B, d, generator=g), dim=-1)
    norm = 0.5 + 4 * torch.rand(B, generator=g)
    x0, res, gamma, _ = fwd_inputs(T, d, seed)
    z = (x0.float() + res.float()).to(torch.bfloat16)
    st = ln_fwd_ref(z, None, gamma, None, eps)
    return dict(cu=cu, demb=demb, emb=emb, norm=norm, z=z, gamma=gamma, mean=st.mean.float(), rstd=st.rstd.float(), T=T, B=B)


def embed_inputs(T, d, vocab, seq=128, seed=500, planted=(), eps=1e-12):
    """The operands of cx_embed_ln_fwd / _bwd(_sorted) on the CPU: ids (Bq, seq) int64 and indices int32[T] = the flat
    positions of the unpadded tokens (sequence lengths 64 .. 128, so tokens of every position and a ragged batch), word
    (vocab, d) / type (2, d) / pos (seq, d) in fp32 with the row profile of the other inputs on the word rows, gamma, beta,
    dout_a / dout_b in bf16.  planted = ((id, count), ...): `count` tokens at seeded places carry `id`, the rest are
    uniform over the vocabulary."""
    lens, n = [], 0
    while n < T:
        lens.append(64 + (37 * len(lens)) % 65)
        n += lens[-1]
    indices = torch.cat([torch.arange(ln) + b * seq for b, ln in enumerate(lens)])[:T].to(torch.int32)
    g = _gen(seed + d)
    tok_ids = torch.randint(0, vocab, (T,), generator=g)
    place = torch.randperm(T, generator=g)
    at = 0
    for tid, count in planted:
        tok_ids[place[at:at + count]] = tid
        at += count
    assert at <= T
    ids = torch.randint(0, vocab, (len(lens), seq), generator=g)          # padded slots hold ids nobody reads
    ids.view(-1)[indices.long()] = tok_ids
    gamma, beta = params(d)
    e = dict(ids=ids, indices=indices, seq=seq, vocab=vocab, T=T, gamma=gamma, beta=beta,
             word=rows_like(vocab, d, seed + d + 1, dtype=torch.float32),
             pos=(0.5 * rows_like(seq, d, seed + d + 2, centred=True, dtype=torch.float32)),
             type=0.1 * torch.randn(2, d, generator=g),
             da=rows_like(T, d, seed + d + 3, centred=True, shift=2), db=rows_like(T, d, seed + d + 4, centred=True, shift=3))
    return e


# The shapes of the embedding edge tests (tests/test_layernorm_edges_gpu.py) and of the measurement of their constants.
EMBED_FWD_SHAPES = tuple((77, d) for d in WIDTHS) + ((8197, 768),)   # 8197 > 2048 blocks x 4 waves: a wave's second row
EMBED_PAD = 3


def embed_fwd_inputs(T, d):
    return embed_inputs(T, d, 512)


def embed_bwd_inputs(d):
    """T = 1029 > 256 blocks x 4 waves; 300 vocabulary rows, so the word-row atomics collide; the padding id occurs."""
    return embed_inputs(1029, d, 300, seed=600, planted=((EMBED_PAD, 5),))


def embed_sorted_inputs(d):
    """T = 4101 > 1024 blocks x 4 waves; 8200 vocabulary rows > the scatter's 8192 blocks, with tokens on both rows of the
    blocks that take two (v and v + 8192, v < 8); a row of 40 tokens and one of 9 (the fold, a wave summing several rows),
    one of 3 (the fold with an idle wave), rows of one token (no fold) and -- T < vocabulary -- rows of none; the padding id
    occurs."""
    planted = ((EMBED_PAD, 6), (5, 40), (8195, 9), (7, 3)) + tuple((v, 1) for v in (0, 1, 2, 4, 6, 8192, 8193, 8194, 8196,
                                                                                  8197, 8198, 8199))
    return embed_inputs(4101, d, 8200, seed=700, planted=planted)


def embed_z(word, type_e, pos_e, ids, indices, seq):
    """z = (word[id] + pos[p]) + type[0] in fp32, the kernels' order (pos_e None: word[id] + type[0]): sums of two and three
    fp32 values are correctly rounded on any device, so this IS the kernels' z.  Returns z, the token ids, the positions."""
    tok = indices.long()
    tid, p = ids.reshape(-1)[tok], tok % seq
    z = word[tid]
    if pos_e is not None:
        z = z + pos_e[p]
    return z + type_e[0], tid, p


def scatter_rows(rows, index, n):
    """out[index[t]] += rows[t] in the dtype of `rows` (fp64 for the references of dword / dpos)."""
    return torch.zeros(n, rows.shape[1], dtype=rows.dtype, device=rows.device).index_add_(0, index, rows)


# ---------------------------------------------------------------------------------------------------------- checker
class RowMismatch(AssertionError):
    pass


def check_rows(name, got, ref, bound, free=None):
    """The row-wise checker: every element of every row must satisfy |got - ref| <= bound (NaN fails).  `got`, `ref` and
    `bound` broadcast to (rows, cols); a 1-D result (dgamma, dbeta, column sums) is one row of per-column values, per-row
    values (mean, rstd) come as (rows, 1).  Raises RowMismatch naming the first failing (row, column); returns the worst
    err / bound (0 where both are 0).  `free` is the part of the bound that belongs to the result's format (half a bf16 ulp):
    with it the returned figure is the worst (err - free) / (bound - free), the share of the fp32 budget C 2^-24 S in use."""
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    bound = torch.as_tensor(bound, dtype=torch.float64, device=ref.device)
    if ref.ndim == 1:
        got, ref = got.reshape(1, -1), ref.reshape(1, -1)
        bound = bound.reshape(1, -1) if bound.ndim == 1 else bound
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    bound = bound.expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        flat = int(torch.nonzero(bad.reshape(-1))[0])
        r, c = divmod(flat, ref.shape[1])
        raise RowMismatch(f"{name}: first mismatch at (row {r}, column {c}): got {float(got[r, c])!r}, reference "
                          f"{float(ref[r, c])!r}, |err| {float(err[r, c]):.3e} > bound {float(bound[r, c]):.3e}; "
                          f"{int(bad.sum())} of {bad.numel()} elements in {int(bad.any(1).sum())} rows fail")
    if free is not None:
        free = torch.as_tensor(free, dtype=torch.float64, device=ref.device).expand_as(ref)
        err, bound = (err - free).clamp(min=0), bound - free
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def bound_bf16(ref, scale, c):
    return 0.5 * bf16_ulp(ref) + c * EPS24 * scale


def bound_f32(scale, c):
    return c * EPS24 * scale


def check_result(name, got, ref, scale, c):
    """A bf16 or fp32 kernel result against its fp64 reference under the bound of its dtype."""
    if got.dtype == torch.bfloat16:
        return check_rows(name, got, ref, bound_bf16(ref, scale, c), free=0.5 * bf16_ulp(ref))
    return check_rows(name, got, ref, bound_f32(scale, c))


def check_out(name, got, fwd: FwdRef, family):
    """Forward output: the bound on S, and -- never wider -- the bound on the scale that also holds the mean's rounding.
    On rows with |mean| >> sigma the measured constant on S alone is so large (see C_MEAS) that it bounds little; the
    second bound keeps those rows, and every other row, to a few 2^-24 of what an fp32 kernel can deliver."""
    half = 0.5 * bf16_ulp(fwd.out) if got.dtype == torch.bfloat16 else 0.0
    b = C(family, "out") * fwd.scale
    if "out_tight" in C_MEAS[family]:
        b = torch.minimum(b, C(family, "out_tight") * fwd.scale_tight)
    return check_rows(name, got, fwd.out, half + EPS24 * b, free=half)


def check_mean(name, got, fwd: FwdRef, c):
    return check_rows(name, got[:, None], fwd.mean[:, None], c * EPS24 * fwd.z.abs().mean(-1, keepdim=True))


def check_rstd(name, got, fwd: FwdRef, c):
    return check_rows(name, got[:, None], fwd.rstd[:, None], c * EPS24 * fwd.rstd.abs()[:, None])


def check_colsum(name, got, stored, c):
    """fp32[d] column sums against the fp64 sum of the STORED bf16 rows (they are defined on what is stored)."""
    s = stored.to(torch.float64)
    return check_rows(name, got, s.sum(0), c * EPS24 * s.abs().sum(0))
