"""The bf16 MFMA GEMM family (gemm_api.hip, gemm_bf16_v5 / v6 / v7.hip, gemm_splitk_small.inc) through the C ABI against the exact
references of tests/gemm_ref.py, at the tile, quadrant, K, ring-phase, XCD-grouping and leading-dimension edges.

Operands are bf16 small integers (tests/gemm_ref.py): every linear result has exactly one correct bit pattern, so the linear forms
are compared BIT FOR BIT (fp32 outputs with the exact product, bf16 outputs with its round-to-nearest-even rounding at the entry
point's rounding points) -- no tolerance.  Nonlinear epilogues: the saved linear tensors (Pre, YG, G) bit for bit, the activation or
its gradient per element under 1 ulp_bf16(ref) + C 2^-24 T against the fp64 formula on the exact rounded inputs, C = 4 C_meas with
C_meas measured by tests/test_gemm_ref_cpu.py on an fp32 torch evaluation against fp64 (never against a kernel):

    form      swiglu  swiglu_bwd.dy  swiglu_bwd.dg  swiglu_bwd_ag.dg  gelu  qgelu  gelu_bwd  qgelu_bwd
    C_meas    3.0     3.5            10.5           3.0               1.7   14.0   2.5       12.0

(qgelu and the dg of the (y, gate) form are large because T holds no term for the fp32 rounding of the exponent's argument, 1.702 v
or g, which reaches the result times |argument|; the bound stays three orders below a bf16 ulp.)  dbias: per column against the fp64
sum of the stored bf16 dPre on top of the initial value under (M + 4) 2^-23 (sum|dPre| + |init|) (the |init| term: the last addition
rounds at the magnitude of the result, see gemm_ref.check_dbias).  Two Gaussian-operand cases hold fp32 outputs to (K + 2) 2^-23 sum|x w|.

Every operand, result and workspace is a slice of a larger allocation (gemm_ref.Buf): 8 guard rows either side and every column
between the width and the leading dimension hold a NaN bit pattern, results and workspaces start as NaN.  A read outside an operand
poisons the result; a write outside [0:M, 0:N] of an output or past ws_floats is found when the test ends (`_poison`).  Every case
runs twice into fresh buffers and must be bit-identical.  Where a stride is named the leading dimension is width + 24 (width + 8 for
the second tensor of a pair that must differ, width + 4 for the 4-aligned fallbacks).  Each test reports its count of differing
elements (0) or its worst err / bound per entry point through gpu_util.report.

Which test reaches what (by reading the launchers; "dev" = the development library's switches cx_gemm_v7_mode and
cx_gemm_set_debug(gn << 8), restored in `finally`):
    v6 fast_tile (alpha 1, no bias, interior quadrant), +- residual ....... test_plain_quadrant_edges[M >= 128, N >= 136] (dev, v7 off)
    v6 store_tile<plain> (partial quadrant, alpha 1, no bias), +- residual . test_plain_quadrant_edges[M, N off 128]
    v6 store_tile<bias / alpha>, +- residual, n + 8 <= N predicate ......... test_plain_quadrant_edges (bias, alpha 0.5 / -2; N 8, 120, 136, 264)
    v6 M = 1: every X row clamped ......................................... test_plain_quadrant_edges[1-*], every fused test at M = 1
    v6 nk = 1 (ring of 3 X / 2 W slots never wraps) .. nk = 7 .............. test_v6_ring_phase_and_groups[nk]
    v6 ring phase carried across tiles, rounds past the first, cursors
       re-walking the first tile, XCDs without a tile, uneven gn ........... test_v6_ring_phase_and_groups (5 x 3 tiles; gn 0, 1, 2, 4, 8)
    v6 full grid, gn = 8 forced: 34 tiles per XCD of 32 workgroups ......... test_rounds_past_the_first[v6-gn8]
    v6 full grid, heuristic: tiles_m = 17 divides by no gm > 1, so gn = 1;
       M-panels split 2,2,2,2,2,2,2,3 -- one XCD with 48 tiles, seven with 32  test_rounds_past_the_first[v6-heuristic]
    v7 by policy (544 tiles on 512 workgroups) ............................. test_rounds_past_the_first[policy] (product library)
    v7 forced, no stagger: tile edges, bias, residual ...................... test_plain_quadrant_edges[*-384], test_v7_ring_phase_and_groups
    v7 forced, stagger (>= 1024 tiles) ..................................... test_v7_stagger_branch
    v7 SwiGLU (gate save) / SwiGLU backward (act, gate) .................... test_swiglu_gate[I 256, v7], test_swiglu_bwd_gate[v7, policy]
    v5 fp32 out (launch5<F32>), +- bias, alpha ............................. test_v5_routes, test_gauss_fp32_out
    v5 bf16 scalar epilogue (N % 8 = 4, or ldo % 8 = 4) ..................... test_v5_routes
    v5 SwiGLU (ld_yg or ld_act % 8 = 4) .................................... test_v5_swiglu
    v5 fp32 partial slabs + splitk_reduce_kernel ........................... test_nt_accum (one slab, nk 3; 16 slabs offered, nk 25)
    v5 fp32 partial slabs + splitk_reduce_bf16_kernel ...................... test_splitk, test_splitk_declines
    v6 TN form (gemm_bf16_v6tn_kernel) + splitk_reduce_kernel .............. test_tn_accum
    v6 SWIGLU / SWIGLU_G fast and predicated, save pointer NULL or not ..... test_swiglu, test_swiglu_gate
    v6 GELU / QGELU fast and predicated, Pre NULL or not ................... test_bias_act
    v6 SWIGLU_BWD (v7 declines the (y, gate) form) / SWIGLU_BWD_AG ......... test_swiglu_bwd, test_swiglu_bwd_gate[v6]
    v6 ACT_BWD / QACT_BWD fast_tile_actb and predicated, colsum partials +
       colsum_part_reduce_kernel (ceil(M / 128) blocks) ..................... test_act_bwd
Not reached: the dev-only generations (v1, v2, v5p: out of scope); tiles_n > 256 (N > 65536: hipErrorInvalidValue by inspection);
the ablation and trace instantiations (timing only, results are garbage by design).
"""
import functools
from contextlib import contextmanager

import pytest
import torch

from contrastors_amd import _C
from tests import gemm_ref as R
from tests.gemm_ref import BF, F32
from tests.gpu_util import L, LD, S, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_SHAPE = -1
_BUFS = []


def buf(rows, cols, ld=None, dtype=BF, data=None, name=""):
    b = R.Buf(rows, cols, ld, dtype=dtype, device=DEV, data=data, name=name)
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


@contextmanager
def route(name, gn=0):
    """"product": the product library (its own policy, no switches).  "v6" / "v7": the dev library with v7 off or with every covered
    launch on v7; gn: forced N-group count of the XCD grid (0 = heuristic)."""
    if name == "product":
        assert gn == 0
        yield L()
        return
    lib = LD()
    lib.cx_gemm_set_variant(6)
    try:
        lib.cx_gemm_v7_mode({"v6": 0, "v7": 1}[name])
        lib.cx_gemm_set_debug(gn << 8)
        yield lib
    finally:
        lib.cx_gemm_v7_mode(-1)
        lib.cx_gemm_set_debug(0)


@functools.lru_cache(maxsize=16)
def ops(M, N, K, seed, scaled=False):
    x, w = R.operands(M, N, K, seed, scaled)
    return x.to(DEV), w.to(DEV)


@functools.lru_cache(maxsize=4)
def acc_of(M, N, K, seed):
    return R.acc_exact(*ops(M, N, K, seed))


def same_twice(tag, a, b):
    for i, (u, v) in enumerate(zip(a, b)):
        if u is not None:
            R.check_bits(f"{tag}: run 2 against run 1 (output {i})", v.get(), u.get())


# ------------------------------------------------------------------------------------------------ the linear NT forms
def run_nt(lib, key, *, bias=None, alpha=1.0, res=None, out_mode=0, xpad=0, opad=0, rpad=0, entry="nt", tag=""):
    """One case of cx_gemm_bf16_nt / _nt_residual / _nt_splitk on the cached operands `key` = (M, N, K, seed): two runs into fresh
    poisoned outputs, bit-identical to each other and to the exact reference.  Returns the number of differing elements (0)."""
    M, N, K, _ = key
    x, w = ops(*key)
    ldx, ldw, ldo, ldr = K + xpad, K + xpad, N + opad, N + rpad
    X, W = buf(M, K, ldx, data=x, name="X"), buf(N, K, ldw, data=w, name="W")
    B = None if bias is None else buf(1, N, dtype=F32, data=bias, name="bias")
    Rs = None if res is None else buf(M, N, ldr, data=res, name="residual")
    outs = []
    for _ in range(2):
        O = buf(M, N, ldo, dtype=F32 if out_mode == 1 else BF, name="Out")
        if entry == "nt":
            assert res is None
            rc = lib.cx_gemm_bf16_nt(X.ptr, W.ptr, O.ptr, P(B), M, N, K, ldx, ldw, ldo, out_mode, 1, alpha, S())
        elif entry == "residual":
            rc = lib.cx_gemm_bf16_nt_residual(X.ptr, W.ptr, O.ptr, P(B), Rs.ptr, M, N, K, ldx, ldw, ldo, ldr, S())
        else:
            nws = min(16, K // 64 // 6) * M * N                      # exactly the slabs the route asks for
            WS = buf(1, nws, nws + 64, dtype=F32, name="ws")
            rc = lib.cx_gemm_bf16_nt_splitk(X.ptr, W.ptr, O.ptr, P(B), P(Rs), WS.ptr, nws, M, N, K, ldx, ldw, ldo, ldr, S())
        _C.check(rc, f"{entry} {tag}")
        outs.append(O)
    torch.cuda.synchronize()
    ref = R.nt_ref(x, w, bias, alpha, out_mode, res, acc=acc_of(*key))
    n = R.check_bits(f"{entry} {key} {tag}", outs[0].get(), ref)
    same_twice(f"{entry} {key} {tag}", outs[:1], outs[1:])
    return n


@pytest.mark.parametrize("N", [8, 120, 136, 264, 384])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 255, 257])
def test_plain_quadrant_edges(M, N):
    """a. M and N either side of the 128-row / 128-column wave quadrant and of the 256 tile: the four bias / residual combinations,
    alpha in {1, 0.5, -2} with and without bias, dense and strided (ldx, ldw, ldo = width + 24, ldr = N + 8 != ldo); on v6 and,
    where it covers the shape (N % 128 == 0, alpha == 1), on v7."""
    key = (M, N, 128, 100)
    bias, res = R.bias_vec(N, 103).to(DEV), R.residual(M, N, 104).to(DEV)
    n = cases = 0
    for r in ["v6"] + (["v7"] if N % 128 == 0 else []):
        with route(r) as lib:
            for pad in (0, 24):
                kw = dict(xpad=pad, opad=pad, rpad=8 if pad else 0)
                for b in (None, bias):
                    for rs in (None, res):
                        n += run_nt(lib, key, bias=b, res=rs, entry="nt" if rs is None else "residual", tag=f"{r} pad {pad}", **kw)
                        cases += 1
                    if r == "v6":
                        for alpha in R.ALPHAS:
                            n += run_nt(lib, key, bias=b, alpha=alpha, tag=f"{r} alpha {alpha} pad {pad}", **kw)
                            cases += 1
    report("gemm_edges.cx_gemm_bf16_nt+residual", M=M, N=N, K=128, cases=cases, differing=n)


def _walk(r, key, gns):
    bias, res = R.bias_vec(key[1], 113).to(DEV), R.residual(key[0], key[1], 114).to(DEV)
    n = 0
    for gn in gns:
        with route(r, gn) as lib:
            n += run_nt(lib, key, tag=f"{r} gn {gn}")
            n += run_nt(lib, key, bias=bias, res=res, entry="residual", xpad=24, opad=24, rpad=8, tag=f"{r} gn {gn} bias residual strided")
    return n


@pytest.mark.parametrize("nk", range(1, 8))
def test_v6_ring_phase_and_groups(nk):
    """b. 5 x 3 tiles of 256 x 256 (M = 1100, N = 712: a partial last panel both ways) on 16 workgroups: with gn forced to 8 or 1
    some XCDs own no tile and two workgroups walk up to five tiles in three rounds, with 2 and 4 the split is uneven; nk = 1 .. 7
    carries every phase of the ring of three X and two W slots from one tile into the next.  Heuristic and forced groupings are all
    bit-equal to the reference, therefore to each other."""
    n = _walk("v6", (1100, 712, 64 * nk, 110), (0, 1, 2, 4, 8))
    report("gemm_edges.v6_walk", nk=nk, differing=n)


@pytest.mark.parametrize("nk", range(2, 8))
def test_v7_ring_phase_and_groups(nk):
    """b. The same on v7 (forced): 5 x 5 tiles of 256 x 128."""
    n = _walk("v7", (1100, 640, 64 * nk, 120), (0, 1, 2, 4, 8))
    report("gemm_edges.v7_walk", nk=nk, differing=n)


@pytest.mark.parametrize("r", ["v6-gn8", "v6-heuristic", "policy"])
def test_rounds_past_the_first(r):
    """c. M = 4352 - 100, N = 4096, K = 128: 17 x 16 tiles of 256 x 256.  v6 with gn = 8 forced: every XCD owns 17 x 2 = 34 tiles on
    its 32 workgroups, two of which take a second tile, and W is sliced eight ways.  v6 with the heuristic grouping: 17 M-panels
    divide by no gm > 1, cx_gemm_v6_groups falls back to gn = 1 and the panels split 2,2,2,2,2,2,2,3 -- one XCD walks 48 tiles, half
    of its workgroups a second one.  Product policy: 272 tiles <= 400, so v7 with 544 tiles of 256 x 128 on 512 workgroups."""
    key = (4352 - 100, 4096, 128, 130)
    with route(*{"v6-gn8": ("v6", 8), "v6-heuristic": ("v6", 0), "policy": ("product", 0)}[r]) as lib:
        n = run_nt(lib, key, tag=r)
    report("gemm_edges.rounds", route=r, differing=n)


def test_v7_stagger_branch():
    """c. 32 x 32 = 1024 tiles of 256 x 128 on forced v7: the start stagger is on (v7_stagger_unit > 0), two tiles per workgroup."""
    key = (8192, 4096, 128, 140)
    bias, res = R.bias_vec(4096, 143).to(DEV), R.residual(8192, 4096, 144).to(DEV)
    with route("v7") as lib:
        n = run_nt(lib, key, tag="v7 stagger")
        n += run_nt(lib, key, bias=bias, res=res, entry="residual", tag="v7 stagger bias residual")
    report("gemm_edges.v7_stagger", differing=n)


# ------------------------------------------------------------------------------------------------------- v5 routes
@pytest.mark.parametrize("M", [1, 257])
def test_v5_routes(M):
    """d. What the product library sends to the one-tile-per-workgroup kernel: fp32 out with and without bias and alpha, bf16 out
    with N % 8 = 4 (N = 4, 132, 260) or ldo % 8 = 4."""
    n = cases = 0
    lib = L()
    for N in (4, 132, 260, 136):
        key = (M, N, 128, 150)
        bias = R.bias_vec(N, 153).to(DEV)
        for b in (None, bias):
            for alpha in (1.0,) + R.ALPHAS:
                for xpad, opad in ((0, 0), (24, 4)):
                    n += run_nt(lib, key, bias=b, alpha=alpha, out_mode=1, xpad=xpad, opad=opad, tag=f"fp32 alpha {alpha} opad {opad}")
                    if N % 8 == 4 or opad == 4:     # bf16 out off the 8-aligned path
                        n += run_nt(lib, key, bias=b, alpha=alpha, xpad=xpad, opad=opad, tag=f"bf16 alpha {alpha} opad {opad}")
                        cases += 1
                    cases += 1
    report("gemm_edges.v5", M=M, cases=cases, differing=n)


@pytest.mark.parametrize("M,N,K", [(257, 260, 128), (300, 768, 1536)])
def test_gauss_fp32_out(M, N, K):
    """Realistic mantissas: Gaussian operands, fp32 out, per element under (K + 2) 2^-23 (sum |x w| + |bias|)."""
    g = torch.Generator().manual_seed(160 + M)
    x, w = torch.randn(M, K, generator=g).to(BF).to(DEV), (torch.randn(N, K, generator=g) * 0.05).to(BF).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    X, W, B = buf(M, K, K + 24, data=x, name="X"), buf(N, K, K + 24, data=w, name="W"), buf(1, N, dtype=F32, data=bias, name="bias")
    outs = []
    for _ in range(2):
        O = buf(M, N, N + 4, dtype=F32, name="Out")
        _C.check(L().cx_gemm_bf16_nt(X.ptr, W.ptr, O.ptr, B.ptr, M, N, K, K + 24, K + 24, N + 4, 1, 1, 1.0, S()))
        outs.append(O)
    torch.cuda.synchronize()
    ratio = R.check_gauss_f32("gauss fp32", outs[0].get(), x, w, bias)
    same_twice("gauss fp32", outs[:1], outs[1:])
    report("gemm_edges.gauss_fp32", M=M, N=N, K=K, ratio=ratio)


# ---------------------------------------------------------------------------------------------------- split-K forms
@pytest.mark.parametrize("nk,slabs", [(3, 1), (25, 16)])
def test_nt_accum(nk, slabs):
    """e. Out += X W^T twice into a non-zero Out: ws_floats exactly one slab at nk = 3 (no split possible), room for 16 slabs at
    nk = 25 (the chosen split cuts 25 K-tiles into uneven slices)."""
    M, N, K = 300, 264, 64 * nk
    key = (M, N, K, 170)
    x, w = ops(*key)
    out0 = torch.randint(-99, 100, (M, N), generator=torch.Generator().manual_seed(171)).float().to(DEV) * 2 + 1
    X, W = buf(M, K, K + 24, data=x, name="X"), buf(N, K, K + 24, data=w, name="W")
    outs = []
    for _ in range(2):
        O = buf(M, N, dtype=F32, data=out0, name="Out")
        WS = buf(1, slabs * M * N, slabs * M * N + 64, dtype=F32, name="ws")
        for _ in range(2):
            _C.check(L().cx_gemm_bf16_nt_accum(X.ptr, W.ptr, O.ptr, WS.ptr, slabs * M * N, M, N, K, K + 24, K + 24, S()))
        outs.append(O)
    torch.cuda.synchronize()
    n = R.check_bits("nt_accum", outs[0].get(), R.accum_ref(out0, x, w, times=2))
    same_twice("nt_accum", outs[:1], outs[1:])
    report("gemm_edges.cx_gemm_bf16_nt_accum", nk=nk, slabs=slabs, differing=n)


@pytest.mark.parametrize("M", [1, 300])
@pytest.mark.parametrize("K", R.K_SPLITK)
def test_splitk(K, M):
    """e. The few-tile long-K route: K / 384 slices (4, 4 and 16), bias x residual, ldo = N + 24 and ldr = N + 8, ws_floats exactly
    the slabs (every float behind them stays poison)."""
    n = 0
    for N in (4, 264, 768):
        key = (M, N, K, 180)
        bias, res = R.bias_vec(N, 183).to(DEV), R.residual(M, N, 184).to(DEV)
        for b in (None, bias):
            for rs in (None, res):
                n += run_nt(L(), key, bias=b, res=rs, entry="splitk", xpad=24, opad=24, rpad=8, tag=f"bias {b is not None} res {rs is not None}")
    report("gemm_edges.cx_gemm_bf16_nt_splitk", M=M, K=K, differing=n)


def test_splitk_declines():
    """e. The documented declines still return CX_ERR_SHAPE and write nothing: more than 64 tiles, K < 1536, no room for the slabs."""
    def call(M, N, K, ws_floats):
        X, W = buf(M, K, data=torch.zeros(M, K), name="X"), buf(N, K, data=torch.zeros(N, K), name="W")
        O, WS = buf(M, N, name="Out"), buf(1, ws_floats, ws_floats + 64, dtype=F32, name="ws")
        rc = L().cx_gemm_bf16_nt_splitk(X.ptr, W.ptr, O.ptr, None, None, WS.ptr, ws_floats, M, N, K, K, K, N, N, S())
        torch.cuda.synchronize()
        assert bool(torch.isnan(O.t.float()).all()) and bool(torch.isnan(WS.t).all())
        return rc
    assert call(2304, 2048, 1536, 4 * 2304 * 2048) == ERR_SHAPE          # 9 x 8 = 72 tiles
    assert call(300, 264, 1472, 16 * 300 * 264) == ERR_SHAPE             # 23 K-tiles
    assert call(300, 264, 1536, 4 * 300 * 264 - 1) == ERR_SHAPE          # one float short of four slabs


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000])
def test_tn_accum(T):
    """e. G += dY^T A in the natural layout, twice into a non-zero G, O and I in {256, 512}, ld_dy = O + 24, ld_a = I + 24.  The
    kernel reads round_up(T, 64) rows by contract: those rows are zero, everything behind them (and every pad column) is poison."""
    Tp = (T + 63) // 64 * 64
    a_ = R.amp(max(T, 64))
    n = 0
    for O in (256, 512):
        for I in (256, 512):
            dy, a = R.ints(T, O, 190 + O, a_).to(DEV), R.ints(T, I, 191 + I, a_).to(DEV)
            g0 = torch.randint(-99, 100, (O, I), generator=torch.Generator().manual_seed(192)).float().to(DEV) * 2 + 1
            z = lambda t: torch.cat([t, torch.zeros(Tp - T, t.shape[1], dtype=BF, device=DEV)])
            DY, A = buf(Tp, O, O + 24, data=z(dy), name="dY"), buf(Tp, I, I + 24, data=z(a), name="A")
            slabs = 4 if T == 1000 else 1
            outs = []
            for _ in range(2):
                G = buf(O, I, dtype=F32, data=g0, name="G")
                WS = buf(1, slabs * O * I, slabs * O * I + 64, dtype=F32, name="ws")
                for _ in range(2):
                    _C.check(L().cx_gemm_bf16_tn_accum(DY.ptr, A.ptr, G.ptr, WS.ptr, slabs * O * I, T, O, I, O + 24, I + 24, S()))
                outs.append(G)
            torch.cuda.synchronize()
            n += R.check_bits(f"tn_accum T {T} O {O} I {I}", outs[0].get(), R.tn_ref(g0, dy, a, times=2))
            same_twice("tn_accum", outs[:1], outs[1:])
    report("gemm_edges.cx_gemm_bf16_tn_accum", T=T, differing=n)


# -------------------------------------------------------------------------------------------------- fused epilogues
KF = R.K_FUSED[0]
PAD = 24


def _swiglu_refs(x, wi):
    yg = R.linear_bf16(x, wi)
    y, g = R.split_yg(yg)
    ref, t = R.f_swiglu(*R.d64(y, g))
    return yg, g.contiguous(), ref, t


def _run_swiglu(lib, M, I, save, gate_form, pad_save=PAD, pad_act=PAD):
    x, wi, _, _ = (t.to(DEV) for t in R.swiglu_case(M, I, KF))
    yg, g, ref, t = _swiglu_refs(x, wi)
    X, W = buf(M, KF, KF + PAD, data=x, name="X"), buf(2 * I, KF, KF + PAD, data=wi, name="W")
    ws = I if gate_form else 2 * I
    outs = []
    for _ in range(2):
        Sv = buf(M, ws, ws + pad_save, name="G" if gate_form else "YG") if save else None
        Act = buf(M, I, I + pad_act, name="Act")
        fn = lib.cx_gemm_bf16_swiglu_gate if gate_form else lib.cx_gemm_bf16_swiglu
        _C.check(fn(X.ptr, W.ptr, P(Sv), Act.ptr, M, I, KF, KF + PAD, KF + PAD, ws + pad_save, I + pad_act, S()))
        outs.append((Sv, Act))
    torch.cuda.synchronize()
    n = R.check_bits("swiglu save", outs[0][0].get(), g if gate_form else yg) if save else 0
    ratio = R.check_nonlinear(f"swiglu act M {M} I {I}", outs[0][1].get(), ref, t, "swiglu")
    same_twice("swiglu", outs[0], outs[1])
    return n, ratio


@pytest.mark.parametrize("M", R.NONLINEAR_M)
def test_swiglu(M):
    """f. fc1 + SwiGLU with the (y, gate) save (v6 SWIGLU: fast and predicated path), save pointer NULL or not, every ld strided."""
    n, worst = 0, 0.0
    for I in R.SWIGLU_I:
        for save in (True, False):
            d, r = _run_swiglu(L(), M, I, save, gate_form=False)
            n, worst = n + d, max(worst, r)
    report("gemm_edges.cx_gemm_bf16_swiglu", M=M, differing=n, ratio=worst)
    assert worst <= 1.0


@pytest.mark.parametrize("M", R.NONLINEAR_M)
def test_swiglu_gate(M):
    """f. The same with the gate-only save: v6 by product policy, and v7 (forced) where it covers the width (2 I % 128 == 0)."""
    n, worst = 0, 0.0
    for I in R.SWIGLU_I:
        for r in ["product"] + (["v7"] if (2 * I) % 128 == 0 else []):
            with route(r) as lib:
                for save in (True, False):
                    d, rr = _run_swiglu(lib, M, I, save, gate_form=True)
                    n, worst = n + d, max(worst, rr)
    report("gemm_edges.cx_gemm_bf16_swiglu_gate", M=M, differing=n, ratio=worst)
    assert worst <= 1.0


@pytest.mark.parametrize("M", [1, 257])
def test_v5_swiglu(M):
    """d. ld_yg or ld_act with % 8 = 4 sends fc1 + SwiGLU to the v5 kernel."""
    n, worst = 0, 0.0
    for I in (32, 160):
        for ps, pa in ((4, PAD), (PAD, 4), (4, 4)):
            for save in (True, False):
                d, r = _run_swiglu(L(), M, I, save, gate_form=False, pad_save=ps, pad_act=pa)
                n, worst = n + d, max(worst, r)
    report("gemm_edges.cx_gemm_bf16_swiglu.v5", M=M, differing=n, ratio=worst)
    assert worst <= 1.0


@pytest.mark.parametrize("M", R.NONLINEAR_M)
def test_bias_act(M):
    """f. fc1 + bias + GELU / quick-GELU: Pre = bf16(acc + bias) bit for bit (NULL or not), Act per element on the rounded Pre."""
    n, worst = 0, {0: 0.0, 1: 0.0}
    for N in R.ACT_N:
        x, w, bias = (t.to(DEV) for t in R.act_case(M, N, KF))
        pre = R.linear_bf16(x, w, bias)
        X, W, B = buf(M, KF, KF + PAD, data=x, name="X"), buf(N, KF, KF + PAD, data=w, name="W"), buf(1, N, dtype=F32, data=bias, name="bias")
        for act in (0, 1):
            ref, t = R.f_act(pre.double(), act)
            for save in (True, False):
                outs = []
                for _ in range(2):
                    Pre = buf(M, N, N + PAD, name="Pre") if save else None
                    Act = buf(M, N, N + 8, name="Act")
                    _C.check(L().cx_gemm_bf16_bias_act(X.ptr, W.ptr, B.ptr, P(Pre), Act.ptr, M, N, KF, KF + PAD, KF + PAD, N + PAD, N + 8, act, S()))
                    outs.append((Pre, Act))
                torch.cuda.synchronize()
                if save:
                    n += R.check_bits(f"Pre M {M} N {N}", outs[0][0].get(), pre)
                worst[act] = max(worst[act], R.check_nonlinear(f"bias_act {act} M {M} N {N}", outs[0][1].get(), ref, t, "qgelu" if act else "gelu"))
                same_twice("bias_act", outs[0], outs[1])
    report("gemm_edges.cx_gemm_bf16_bias_act", M=M, differing=n, ratio_gelu=worst[0], ratio_qgelu=worst[1])
    assert max(worst.values()) <= 1.0


def _bwd_check(tag, got_dyg, ry, ty, rg, tg, form_g):
    dy, dg = R.split_yg(got_dyg)
    return (R.check_nonlinear(f"{tag} dy", dy, ry, ty, "swiglu_bwd.dy"), R.check_nonlinear(f"{tag} dg", dg, rg, tg, form_g))


@pytest.mark.parametrize("M", R.NONLINEAR_M)
def test_swiglu_bwd(M):
    """f. fc2 dgrad + SwiGLU backward from the (y, gate) pair, ld_yg = 2 I + 24.  One route only: cx_gemm_v7_covers declines
    GEMM_EPI_SWIGLU_BWD (v7 serves the (act, gate) form alone), so v7 mode 0, mode 1 and the product policy all run the v6 kernel."""
    wy = wg = 0.0
    for I in R.BWD_I:
        dy, w, y, g, _ = (t.to(DEV) for t in R.swiglu_bwd_case(M, I, KF))
        d = R.acc_exact(dy, w)
        refs = R.f_swiglu_bwd(d, *R.d64(y, g))
        X, W = buf(M, KF, KF + PAD, data=dy, name="dY"), buf(I, KF, KF + PAD, data=w, name="W")
        YG = buf(M, 2 * I, 2 * I + PAD, data=R.join_yg(y, g), name="YG")
        outs = []
        for _ in range(2):
            O = buf(M, 2 * I, 2 * I + PAD, name="dYG")
            _C.check(L().cx_gemm_bf16_swiglu_bwd(X.ptr, W.ptr, YG.ptr, O.ptr, M, I, KF, KF + PAD, KF + PAD, 2 * I + PAD, S()))
            outs.append(O)
        torch.cuda.synchronize()
        a, b = _bwd_check(f"swiglu_bwd M {M} I {I}", outs[0].get(), *refs, "swiglu_bwd.dg")
        wy, wg = max(wy, a), max(wg, b)
        same_twice("swiglu_bwd", outs[:1], outs[1:])
    report("gemm_edges.cx_gemm_bf16_swiglu_bwd", M=M, ratio_dy=wy, ratio_dg=wg)
    assert max(wy, wg) <= 1.0


@pytest.mark.parametrize("r", ["v6", "v7", "policy"])
@pytest.mark.parametrize("M", R.NONLINEAR_M)
def test_swiglu_bwd_gate(M, r):
    """f. The same from the (act, gate) pair: ld_ag = I + 24 != I, ld_dyg = 2 I + 8 != 2 I; on v6, on v7 and by product policy."""
    wy = wg = 0.0
    for I in R.BWD_I:
        dy, w, _, g, act = (t.to(DEV) for t in R.swiglu_bwd_case(M, I, KF))
        assert bool((g != 0).all())
        d = R.acc_exact(dy, w)
        refs = R.f_swiglu_bwd_ag(d, *R.d64(act, g))
        X, W = buf(M, KF, KF + PAD, data=dy, name="dY"), buf(I, KF, KF + PAD, data=w, name="W")
        A, G = buf(M, I, I + PAD, data=act, name="Act"), buf(M, I, I + PAD, data=g, name="G")
        outs = []
        with route("product" if r == "policy" else r) as lib:
            for _ in range(2):
                O = buf(M, 2 * I, 2 * I + 8, name="dYG")
                _C.check(lib.cx_gemm_bf16_swiglu_bwd_gate(X.ptr, W.ptr, A.ptr, G.ptr, O.ptr, M, I, KF, KF + PAD, KF + PAD, I + PAD, 2 * I + 8, S()))
                outs.append(O)
            torch.cuda.synchronize()
        a, b = _bwd_check(f"swiglu_bwd_gate {r} M {M} I {I}", outs[0].get(), *refs, "swiglu_bwd_ag.dg")
        wy, wg = max(wy, a), max(wg, b)
        same_twice("swiglu_bwd_gate", outs[:1], outs[1:])
    report("gemm_edges.cx_gemm_bf16_swiglu_bwd_gate", M=M, route=r, ratio_dy=wy, ratio_dg=wg)
    assert max(wy, wg) <= 1.0


@pytest.mark.parametrize("M", R.ACT_BWD_M)
def test_act_bwd(M):
    """f. fc2 dgrad + GELU / quick-GELU backward: dPre per element on the exact bf16 d(act), ld_pre = N + 24 != ld_dpre = N + 8, with
    and without dbias; dbias on top of a non-zero initial value through a workspace of exactly ceil(M / 128) * N floats."""
    worst, wdb = {0: 0.0, 1: 0.0}, 0.0
    nblocks = (M + 127) // 128
    for N in R.ACT_N:
        dy, w, pre = (t.to(DEV) for t in R.act_bwd_case(M, N, KF))
        d = R.linear_bf16(dy, w)
        init = torch.randint(1, 9, (N,), generator=torch.Generator().manual_seed(710)).float().to(DEV)
        X, W = buf(M, KF, KF + PAD, data=dy, name="dY"), buf(N, KF, KF + PAD, data=w, name="W")
        Pre = buf(M, N, N + PAD, data=pre, name="Pre")
        for act in (0, 1):
            ref, t = R.f_act_bwd(*R.d64(d, pre), act)
            for with_db in (True, False):
                outs = []
                for _ in range(2):
                    O = buf(M, N, N + 8, name="dPre")
                    DB = buf(1, N, dtype=F32, data=init, name="dbias") if with_db else None
                    WS = buf(1, nblocks * N, nblocks * N + 64, dtype=F32, name="ws") if with_db else None
                    _C.check(L().cx_gemm_bf16_act_bwd(X.ptr, W.ptr, Pre.ptr, O.ptr, P(DB), P(WS), nblocks * N if with_db else 0, M, N, KF,
                                                      KF + PAD, KF + PAD, N + PAD, N + 8, act, S()))
                    outs.append((O, DB))
                torch.cuda.synchronize()
                worst[act] = max(worst[act], R.check_nonlinear(f"act_bwd {act} M {M} N {N}", outs[0][0].get(), ref, t, "qgelu_bwd" if act else "gelu_bwd"))
                if with_db:
                    wdb = max(wdb, R.check_dbias(f"dbias {act} M {M} N {N}", outs[0][1].get().reshape(-1), init, outs[0][0].get(), M))
                same_twice("act_bwd", outs[0], outs[1])
    report("gemm_edges.cx_gemm_bf16_act_bwd", M=M, ratio_gelu=worst[0], ratio_qgelu=worst[1], ratio_dbias=wdb)
    assert max(worst.values()) <= 1.0 and wdb <= 1.0
