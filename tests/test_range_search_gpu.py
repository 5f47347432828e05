"""GPU checks of the range search (csrc/range.hip via FlatIPIndex.range_count / range_search and the C ABI): lims, ids and
scores equal to the float64 reference bit for bit on operands whose fp32 accumulation is exact (radii ON attained scores,
-inf, +inf, NaN; a tie-heavy variant), the dense case and random unit-norm embeddings against the search kernel's own bits
and against the reference's rounding band, min_id at the tile edges and the self-join, independence of split count / query
batching / run, the refusals (tests/range_ref.py)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import range_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MS, NS, DS = [1, 127, 129, 300], [1, 127, 129, 257, 1000], [64, 320, 1024]


def _grid_operands(M, N, d, levels, seed):
    """Entries from {-levels..levels}/levels: exact in bf16, products multiples of 1/levels^2, |score| <= d < 2^11 -- every
    partial sum is a multiple of 2^-6 below 2^11, so fp32 accumulation is exact in any order (as tests/test_rank_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randint(-levels, levels + 1, (M, d), generator=g).float() / levels).to(torch.bfloat16)
    D = (torch.randint(-levels, levels + 1, (N, d), generator=g).float() / levels).to(torch.bfloat16)
    return Q.to(DEV), D.to(DEV)


def _unit_operands(M, N, d):
    g = torch.Generator().manual_seed(1000 * M + N + d)
    Q = torch.nn.functional.normalize(torch.randn(M, d, generator=g), dim=1).to(torch.bfloat16).to(DEV)
    D = torch.nn.functional.normalize(torch.randn(N, d, generator=g), dim=1).to(torch.bfloat16).to(DEV)
    return Q, D


def _mixed_radii(S):
    """Per row, by m % 6: an ATTAINED score of the row (strictness: that column and its ties stay out) / the row's median /
    -inf / +inf / NaN / the row's maximum (attained: nothing is admitted)."""
    M, N = S.shape
    rad = torch.empty(M, dtype=torch.float32)
    Sc = S.cpu()
    for m in range(M):
        kind = m % 6
        rad[m] = (float(Sc[m, (7 * m + 3) % N]), float(Sc[m].median()), -math.inf, math.inf, math.nan, float(Sc[m].max()))[kind]
    return rad.to(DEV)


def _index(D, **kw):
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(D.shape[1], device=DEV, **kw)
    ix.add(D)
    return ix


@functools.lru_cache(maxsize=None)
def _case(kind, M, N, d):
    """Operands, radii, the index and the kernel's answer, computed once per case and shared (never modified)."""
    seed = 1000 * M + N + d
    if kind == "unit":
        Q, D = _unit_operands(M, N, d)
        rad = torch.full((M,), 2.0 / math.sqrt(d), dtype=torch.float32, device=DEV)
    else:
        Q, D = _grid_operands(M, N, d, 8 if kind == "grid8" else 2, seed)
        rad = _mixed_radii(R.scores64(Q, D))
    ix = _index(D)
    lims, scores, ids = ix.range_search(Q, rad)
    assert lims.dtype == torch.int64 and scores.dtype == torch.float32 and ids.dtype == torch.int64
    assert lims.device == scores.device == ids.device == torch.device(DEV)
    return dict(Q=Q, D=D, rad=rad, ix=ix, lims=lims, scores=scores, ids=ids)


def _same(a, b):
    """Two results equal bit for bit."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])


# ---- 1. exact operands: bit for bit, every row ------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_range_exact_grid(M, N, d):
    c = _case("grid8", M, N, d)
    R.check_against_ref(c["Q"], c["D"], c["rad"], None, c["lims"], c["scores"], c["ids"], exact=True)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_range_exact_grid_ties_at_the_threshold(M, N):
    c = _case("grid2", M, N, 64)
    R.check_against_ref(c["Q"], c["D"], c["rad"], None, c["lims"], c["scores"], c["ids"], exact=True)
    if M >= 127 and N >= 257:   # the variant is here for its ties: rows whose radius is attained see it attained many times
        S = R.scores64(c["Q"], c["D"])
        rows = torch.arange(M, device=DEV) % 6 == 0
        assert float((S[rows] == c["rad"][rows].double()[:, None]).sum(1).double().mean()) > 2


def test_range_dense_equals_search():
    """radius -inf: every row returns the whole corpus in id order, with the scores search(k = N) gives, bit for bit."""
    M, N = 129, 257
    for d, levels in ((64, 2), (320, 8)):
        Q, D = _grid_operands(M, N, d, levels, 17)
        ix = _index(D)
        lims, scores, ids = ix.range_search(Q, -math.inf)
        assert lims.tolist() == [N * m for m in range(M + 1)]
        assert torch.equal(ids.view(M, N), torch.arange(N, device=DEV).expand(M, N))
        s, i = ix.search(Q, N)
        by_id = torch.gather(s, 1, torch.argsort(i, dim=1))
        assert torch.equal(scores.view(M, N).view(torch.int32), by_id.view(torch.int32))
        assert ix.range_count(Q, -math.inf).tolist() == [N] * M


# ---- 2. random unit-norm embeddings --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
def test_range_unit_norm_embeddings(d):
    M, N = 300, 1000
    c = _case("unit", M, N, d)
    # against the search kernel: the same bits, so the same set -- no band
    s, i = c["ix"].search(c["Q"], N)
    keep = s > c["rad"][:, None]
    rows = torch.arange(M, device=DEV)[:, None].expand(M, N)[keep]
    key = rows * N + i[keep]
    order = torch.argsort(key)
    got_rows = torch.repeat_interleave(torch.arange(M, device=DEV), c["lims"][1:] - c["lims"][:-1])
    assert torch.equal(got_rows * N + c["ids"], key[order])
    assert torch.equal(c["scores"].view(torch.int32), s[keep][order].view(torch.int32))
    # against float64: classification outside the band, scores within it, few pairs inside it, enough admitted
    inband = R.check_against_ref(c["Q"], c["D"], c["rad"], None, c["lims"], c["scores"], c["ids"], exact=False)
    print(f"unit d={d}: {inband} in-band pairs of {M * N}, {c['ids'].numel()} admitted")
    assert inband <= M * N // 1000
    assert c["ids"].numel() >= 1000


# ---- 3. min_id -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,d", [("grid8", 257, 64), ("grid8", 1000, 320), ("grid2", 1000, 64), ("grid8", 129, 1024)])
def test_range_min_id_at_tile_edges(kind, N, d):
    M = 300
    c = _case(kind, M, N, d)
    vals = [-1, 0, 126, 127, 128, N - 2, N - 1, N, N + 500, 2 ** 40]
    mixed = torch.tensor([vals[m % len(vals)] for m in range(M)])          # every value inside every query tile
    for min_id in (mixed, *(torch.full((M,), v) for v in (-1, 127, 128, N - 1, N)),
                   torch.cat([torch.full((128,), 200), torch.full((M - 128,), 129)])):   # whole tiles skipped, per query tile
        got = c["ix"].range_search(c["Q"], c["rad"], min_id=min_id)
        R.check_against_ref(c["Q"], c["D"], c["rad"], min_id.clamp(max=N), *got, exact=True)
        assert torch.equal(c["ix"].range_count(c["Q"], c["rad"], min_id=min_id), got[0][1:] - got[0][:-1])
    assert _same(c["ix"].range_search(c["Q"], c["rad"], min_id=torch.full((M,), -1)), (c["lims"], c["scores"], c["ids"]))


@pytest.mark.parametrize("kind,N,d", [("unit", 1000, 64), ("grid2", 1000, 64), ("grid8", 300, 320)])
def test_range_self_join_is_the_strict_upper_triangle(kind, N, d):
    if kind == "unit":
        _, D = _unit_operands(1, N, d)
        D = torch.cat([D[: N // 2], D[: N // 2]]) if N % 2 == 0 else D       # every row has an exact copy: real pairs
        rad = 0.5
    else:
        _, D = _grid_operands(1, N, d, 8 if kind == "grid8" else 2, 23)
        rad = 1.0
    ix = _index(D)
    lims, scores, ids = ix.range_search(D, rad)
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), lims[1:] - lims[:-1])
    upper = ids > rows
    jl, js, ji = ix.range_search(D, rad, min_id=torch.arange(N))
    assert int(upper.sum()) >= N // 2
    assert torch.equal(ji, ids[upper]) and torch.equal(js.view(torch.int32), scores[upper].view(torch.int32))
    assert torch.equal(jl[1:] - jl[:-1], torch.bincount(rows[upper], minlength=N))


# ---- 4. independence of splits, batches and runs --------------------------------------------------------------------------------
def test_range_independent_of_splits_batches_and_runs():
    from contrastors_amd import _C

    for case in (_case("grid2", 300, 1000, 64), _case("unit", 300, 1000, 320)):
        want = (case["lims"], case["scores"], case["ids"])
        assert int(want[0][-1]) > 1000
        min_id = torch.arange(300) * 3 - 5
        want_mid = case["ix"].range_search(case["Q"], case["rad"], min_id=min_id)
        for nsplit in (1, 2, 3, 0):
            for _ in range(2):
                assert _same(case["ix"].range_search(case["Q"], case["rad"], nsplit=nsplit), want)
                assert _same(case["ix"].range_search(case["Q"], case["rad"], min_id=min_id, nsplit=nsplit), want_mid)
                assert torch.equal(case["ix"].range_count(case["Q"], case["rad"], nsplit=nsplit), want[0][1:] - want[0][:-1])
        small = _index(case["D"], workspace_bytes=1024)
        assert small.range_batch_rows(300) == 128                               # 300 rows: three query batches
        assert _C.lib().cx_range_ws_bytes(128, 1000, 0) > 1024
        assert _same(small.range_search(case["Q"], case["rad"]), want)
        assert _same(small.range_search(case["Q"], case["rad"], min_id=min_id), want_mid)
        assert torch.equal(small.range_count(case["Q"], case["rad"], min_id=min_id), want_mid[0][1:] - want_mid[0][:-1])


def test_range_numpy_round_trip_and_radius_forms():
    c = _case("grid8", 129, 257, 64)
    ix, Q = c["ix"], c["Q"]
    ln, sn, idn = ix.range_search(Q.float().cpu().numpy(), c["rad"].cpu().numpy())
    assert isinstance(ln, np.ndarray) and ln.dtype == np.int64 and sn.dtype == np.float32 and idn.dtype == np.int64
    assert ln.tolist() == c["lims"].tolist() and idn.tolist() == c["ids"].tolist() and sn.tolist() == c["scores"].tolist()
    cn = ix.range_count(Q.float().cpu().numpy(), c["rad"].cpu().tolist())
    assert isinstance(cn, np.ndarray) and cn.dtype == np.int64 and cn.tolist() == np.diff(ln).tolist()
    # a scalar radius is every row's radius
    assert _same(ix.range_search(Q, 2.5), ix.range_search(Q, torch.full((129,), 2.5)))
    assert _same(ix.range_search(Q, np.float32(2.5)), ix.range_search(Q, torch.full((129,), 2.5)))


# ---- 5. refusals and edges ---------------------------------------------------------------------------------------------------------
def test_range_refusals_and_edges():
    from contrastors_amd import _C
    from contrastors_amd.search import FlatIPIndex

    c = _case("grid8", 129, 257, 64)
    ix, Q, rad = c["ix"], c["Q"], c["rad"]
    total = int(c["lims"][-1])
    assert total > 100
    with pytest.raises(ValueError, match=rf"\b{total}\b.*max_results = {total - 1}\b"):
        ix.range_search(Q, rad, max_results=total - 1)
    assert _same(ix.range_search(Q, rad, max_results=total), (c["lims"], c["scores"], c["ids"]))
    # the running total over query batches is what is refused
    small = _index(c["D"], workspace_bytes=1024)
    first = int(c["lims"][128])
    with pytest.raises(ValueError, match=rf"\b{total}\b"):
        small.range_search(Q, rad, max_results=max(first, total - 1))
    with pytest.raises(ValueError, match="radius has 128 entries for 129"):
        ix.range_search(Q, rad[:128])
    with pytest.raises(ValueError, match="radius has 128 entries for 129"):
        ix.range_count(Q, rad[:128])
    with pytest.raises(ValueError, match="min_id has 130 entries for 129"):
        ix.range_search(Q, rad, min_id=torch.arange(130))
    with pytest.raises(ValueError, match="min_id has 1 entries for 129"):
        ix.range_count(Q, rad, min_id=[3])
    with pytest.raises(ValueError, match="integer"):
        ix.range_search(Q, rad, min_id=torch.zeros(129))
    with pytest.raises(ValueError):
        ix.range_search(Q[:, :32], rad)                                            # wrong width
    # an empty index, and no queries: zeros and empty arrays, nothing launched
    empty = FlatIPIndex(64, device=DEV)
    l0, s0, i0 = empty.range_search(Q, 0.0)
    assert l0.tolist() == [0] * 130 and s0.numel() == 0 and i0.numel() == 0
    assert s0.dtype == torch.float32 and i0.dtype == torch.int64
    assert empty.range_count(Q, 0.0).tolist() == [0] * 129
    l0, s0, i0 = ix.range_search(Q[:0], 0.0)
    assert l0.tolist() == [0] and s0.numel() == 0 and i0.numel() == 0
    assert ix.range_count(Q[:0], rad[:0]).numel() == 0
    l0, s0, i0 = ix.range_search(Q, math.inf)                                      # a zero total: no emit
    assert l0.tolist() == [0] * 130 and s0.numel() == 0 and i0.numel() == 0
    # the C ABI: errors are returned before any launch; M == 0 or N == 0 is a success that touches nothing
    h = _C.lib()
    D = c["D"]
    ws = torch.empty(h.cx_range_ws_bytes(129, 257, 0), dtype=torch.uint8, device=DEV)
    cnt = torch.empty(129, dtype=torch.int64, device=DEV)
    ok = (Q.data_ptr(), D.data_ptr(), 129, 257, 64, 64, 64, rad.data_ptr(), None, 0, ws.data_ptr())
    assert h.cx_range_count(*ok, cnt.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(cnt, c["lims"][1:] - c["lims"][:-1])

    def count_rc(**kw):
        a = dict(Q=Q.data_ptr(), D=D.data_ptr(), M=129, N=257, d=64, ldq=64, ldd=64, radius=rad.data_ptr(), min_id=None,
                 nsplit=0, ws=ws.data_ptr(), counts=cnt.data_ptr())
        a.update(kw)
        return h.cx_range_count(*a.values(), None)

    def emit_rc(**kw):
        a = dict(Q=Q.data_ptr(), D=D.data_ptr(), M=129, N=257, d=64, ldq=64, ldd=64, radius=rad.data_ptr(), min_id=None,
                 nsplit=0, ws=ws.data_ptr(), lims=c["lims"].data_ptr(), out_scores=c["scores"].data_ptr(),
                 out_ids=c["ids"].data_ptr())
        a.update(kw)
        return h.cx_range_emit(*a.values(), None)

    for rc in (count_rc, emit_rc):
        assert rc(Q=None) == -3 and rc(D=None) == -3 and rc(radius=None) == -3 and rc(ws=None) == -3      # CX_ERR_ARG
        assert rc(ldq=60) == -2 and rc(ldq=68) == -2 and rc(ldd=68) == -2                                  # CX_ERR_ALIGN
        assert rc(Q=Q.data_ptr() + 2) == -2 and rc(ws=ws.data_ptr() + 4) == -2
        assert rc(N=2 ** 31 - 128) == -1 and rc(d=96, ldq=96, ldd=96) == -1 and rc(d=2048, ldq=2048, ldd=2048) == -1
        assert rc(M=-1) == -1                                                                              # CX_ERR_SHAPE
        assert rc(M=0, Q=None, ws=None) == 0 and rc(N=0, D=None, ws=None) == 0
    assert count_rc(counts=None) == -3
    assert emit_rc(lims=None) == -3 and emit_rc(out_scores=None) == -3 and emit_rc(out_ids=None) == -3
    assert h.cx_range_ws_bytes(0, 257, 0) == 0 and h.cx_range_ws_bytes(129, 0, 0) == 0
