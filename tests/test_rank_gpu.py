"""GPU checks of the rank kernel (csrc/rank.hip via FlatIPIndex.rank and the C ABI): bit-exact ranks and scores on operands
whose fp32 accumulation is exact (tie-heavy variant included), a banded check on random unit-norm embeddings, agreement
with the search kernel position by position and bit by bit, determinism across split counts / runs / query batches, the
refusals, and the metrics of contrastors_amd.zeroshot end to end against dense float64 metrics (tests/rank_ref.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import rank_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PG = 8    # csrc/rank.hip PGMAX: targets per row and walk
MS, NS, DS = [1, 127, 129, 300], [1, 127, 129, 257, 1000], [64, 320, 1024]


def _grid_operands(M, N, d, levels, seed):
    """Entries from {-levels..levels}/levels: exact in bf16, products multiples of 1/levels^2, |score| <= d < 2^11 -- every
    partial sum is a multiple of 2^-6 below 2^11, so fp32 accumulation is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randint(-levels, levels + 1, (M, d), generator=g).float() / levels).to(torch.bfloat16)
    D = (torch.randint(-levels, levels + 1, (N, d), generator=g).float() / levels).to(torch.bfloat16)
    return Q.to(DEV), D.to(DEV)


def _mixed_targets(M, N, seed):
    """Per row, by m % 6: none / one / five / [0] / [N - 1] / a repeated id; row M // 2 gets PG + 1 targets, the last row 70
    (with id 0 and id N - 1 among them)."""
    rng = np.random.default_rng(seed)
    lists = []
    for m in range(M):
        kind = m % 6
        if kind == 0:
            t = []
        elif kind == 1:
            t = [int(rng.integers(N))]
        elif kind == 2:
            t = [int(x) for x in rng.integers(N, size=5)]
        elif kind == 3:
            t = [0]
        elif kind == 4:
            t = [N - 1]
        else:
            x = int(rng.integers(N))
            t = [x, int(rng.integers(N)), x]
        lists.append(t)
    lists[M // 2] = [int(x) for x in rng.integers(N, size=PG + 1)]
    lists[M - 1] = [N - 1, 0] + [int(x) for x in rng.integers(N, size=68)]
    return lists


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return ptr, np.asarray([i for x in lists for i in x], np.int64)


def _index(D, **kw):
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(D.shape[1], device=DEV, **kw)
    ix.add(D)
    return ix


@functools.lru_cache(maxsize=None)
def _case(kind, M, N, d):
    """Operands, targets, the float64 reference and the kernel's answer, computed once per case and shared."""
    seed = 1000 * M + N + d
    if kind == "grid8":
        Q, D = _grid_operands(M, N, d, 8, seed)
        lists = _mixed_targets(M, N, seed)
    elif kind == "grid2":
        Q, D = _grid_operands(M, N, d, 2, seed)
        lists = _mixed_targets(M, N, seed)
    else:   # unit: random unit-norm embeddings drawn on the host, five targets per row
        g = torch.Generator().manual_seed(seed)
        Q = torch.nn.functional.normalize(torch.randn(M, d, generator=g), dim=1).to(torch.bfloat16).to(DEV)
        D = torch.nn.functional.normalize(torch.randn(N, d, generator=g), dim=1).to(torch.bfloat16).to(DEV)
        lists = [[int(x) for x in row] for row in torch.randint(0, N, (M, 5), generator=g)]
    ptr, ids = _csr(lists)
    ref_r, ref_s = R.ref_rank(Q, D, ptr, ids)
    ix = _index(D)
    ranks, scores, row_ptr = ix.rank(Q, lists)
    assert ranks.dtype == torch.int64 and scores.dtype == torch.float32 and row_ptr.tolist() == ptr.tolist()
    return dict(Q=Q, D=D, lists=lists, ptr=ptr, ids=ids, ref_r=ref_r, ref_s=ref_s, ix=ix, ranks=ranks, scores=scores)


def _raw_rank(Q, D, ptr, ids, nsplit=0):
    """cx_rank_targets on (possibly row-strided) views."""
    from contrastors_amd import _C

    h = _C.lib()
    M, d = Q.shape
    N, nnz = D.shape[0], len(ids)
    ws = torch.empty(max(16, h.cx_rank_ws_bytes(M, N, nnz, nsplit)), dtype=torch.uint8, device=DEV)
    dptr, dids = torch.as_tensor(ptr).to(DEV), torch.as_tensor(ids).to(DEV)
    ranks = torch.full((nnz,), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((nnz,), float("nan"), dtype=torch.float32, device=DEV)
    rc = h.cx_rank_targets(Q.data_ptr(), D.data_ptr(), M, N, d, Q.stride(0), D.stride(0), dptr.data_ptr(), dids.data_ptr(),
                           nsplit, ws.data_ptr(), ranks.data_ptr(), scores.data_ptr(), _C.cur_stream())
    torch.cuda.synchronize()
    return rc, ranks, scores


# ---- 1. exact grid: bit-exact, no tolerance, no row left out ------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_rank_exact_grid(M, N, d):
    c = _case("grid8", M, N, d)
    assert torch.equal(c["scores"].double(), c["ref_s"])
    assert torch.equal(c["ranks"], c["ref_r"])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_rank_exact_grid_tie_break(M, N):
    c = _case("grid2", M, N, 64)
    assert torch.equal(c["scores"].double(), c["ref_s"])
    assert torch.equal(c["ranks"], c["ref_r"])
    if M >= 127 and N >= 257:   # the variant is here for its ties: most targets share their score with another column
        assert float((R.near_count(c["Q"], c["D"], c["ptr"], c["ids"], 0.0) > 0).double().mean()) > 0.9


@pytest.mark.parametrize("M,N,d", [(129, 257, 320), (300, 1000, 64)])
def test_rank_strided_operands(M, N, d):
    c = _case("grid8", M, N, d)
    qbuf = torch.zeros(M, d + 64, dtype=torch.bfloat16, device=DEV)
    dbuf = torch.zeros(N, 2 * d, dtype=torch.bfloat16, device=DEV)
    qbuf[:, :d], dbuf[:, :d] = c["Q"], c["D"]
    qbuf[:, d:], dbuf[:, d:] = 3.0, -5.0   # what lies between the rows must not be read into a score
    rc, ranks, scores = _raw_rank(qbuf[:, :d], dbuf[:, :d], c["ptr"], c["ids"])
    assert rc == 0
    assert torch.equal(ranks.long(), c["ref_r"]) and torch.equal(scores.double(), c["ref_s"])


# ---- 2. random unit-norm embeddings ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(300, 1000), (129, 257)])
def test_rank_unit_norm_embeddings(M, N):
    c = _case("unit", M, N, 64)
    near = R.near_count(c["Q"], c["D"], c["ptr"], c["ids"], 1e-5)    # the band test_search_gpu.py grants this operand kind
    share = float((near > 0).double().mean())
    print(f"unit {M}x{N}: share of targets with a column within 1e-5 = {share:.4f}, "
          f"max |rank - ref| = {int((c['ranks'] - c['ref_r']).abs().max())}, "
          f"max |score - ref| = {float((c['scores'].double() - c['ref_s']).abs().max()):.3e}")
    assert bool(((c["ranks"] - c["ref_r"]).abs() <= near).all())
    assert float((c["scores"].double() - c["ref_s"]).abs().max()) < 1e-4
    assert share <= 0.10


# ---- 3. agreement with the search kernel -----------------------------------------------------------------------------------
def _check_search_agreement(c):
    N = c["D"].shape[0]
    k = min(N, 1024)
    s, i = c["ix"].search(c["Q"], k)
    rows = torch.repeat_interleave(torch.arange(len(c["lists"])), torch.as_tensor(np.diff(c["ptr"]))).to(DEV)
    ids = torch.as_tensor(c["ids"]).to(DEV)
    sel = c["ranks"] < k
    assert bool(sel.any())
    assert torch.equal(i[rows[sel], c["ranks"][sel]], ids[sel])
    assert torch.equal(s[rows[sel], c["ranks"][sel]].view(torch.int32), c["scores"][sel].view(torch.int32))   # bitwise


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_rank_agrees_with_search_exact_grid(M, N, d):
    _check_search_agreement(_case("grid8", M, N, d))
    if d == 64:
        _check_search_agreement(_case("grid2", M, N, d))


@pytest.mark.parametrize("M,N", [(300, 1000), (129, 257)])
def test_rank_agrees_with_search_unit_norm(M, N):
    _check_search_agreement(_case("unit", M, N, 64))


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------
def test_rank_deterministic_across_splits_runs_and_batches():
    c = _case("grid2", 300, 1000, 64)
    u = _case("unit", 300, 1000, 64)
    for case in (c, u):
        for nsplit in (1, 2, 7, 0):
            for _ in range(2):
                ranks, scores, _ = case["ix"].rank(case["Q"], case["lists"], nsplit=nsplit)
                assert torch.equal(ranks, case["ranks"])
                assert torch.equal(scores.view(torch.int32), case["scores"].view(torch.int32))
        small = _index(case["D"], workspace_bytes=1024)
        assert small.rank_batch_rows(torch.as_tensor(case["ptr"])) == 128     # 300 rows: three query batches
        ranks, scores, _ = small.rank(case["Q"], case["lists"])
        assert torch.equal(ranks, case["ranks"])
        assert torch.equal(scores.view(torch.int32), case["scores"].view(torch.int32))


def test_rank_target_forms_and_numpy_round_trip():
    c = _case("grid8", 129, 257, 64)
    ix, Q = c["ix"], c["Q"]
    r2, s2, p2 = ix.rank(Q, (c["ptr"], c["ids"]))                  # a CSR pair
    assert torch.equal(r2, c["ranks"]) and torch.equal(s2, c["scores"]) and p2.tolist() == c["ptr"].tolist()
    labels = torch.as_tensor([7 * m % 257 for m in range(129)])
    r1, s1, p1 = ix.rank(Q, labels)                                # one target per row
    assert r1.shape == (129,) and s1.shape == (129,) and p1.tolist() == list(range(130))
    want, _ = R.ref_rank(Q, c["D"], np.arange(130), labels)
    assert torch.equal(r1, want)
    rn, sn, pn = ix.rank(Q.float().cpu().numpy(), labels.numpy())  # numpy in -> numpy out
    assert isinstance(rn, np.ndarray) and rn.dtype == np.int64 and sn.dtype == np.float32 and pn.dtype == np.int64
    assert rn.tolist() == r1.tolist() and sn.tolist() == s1.tolist()
    # no targets at all, and an empty index with no targets: nothing to do, nothing raised
    r0, s0, p0 = ix.rank(Q, [[] for _ in range(129)])
    assert r0.numel() == 0 and s0.numel() == 0 and p0.tolist() == [0] * 130
    from contrastors_amd.search import FlatIPIndex

    r0, _, _ = FlatIPIndex(64, device=DEV).rank(Q, [[] for _ in range(129)])
    assert r0.numel() == 0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_rank_refusals():
    from contrastors_amd import _C
    from contrastors_amd.search import FlatIPIndex

    c = _case("grid8", 129, 257, 64)
    ix, Q = c["ix"], c["Q"]
    for bad in ([[257]] + [[]] * 128, [[-1]] + [[]] * 128):
        with pytest.raises(ValueError, match="ids must lie in"):
            ix.rank(Q, bad)
    with pytest.raises(ValueError, match="ids must lie in"):
        ix.rank(Q, torch.full((129,), 257))
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.rank(Q, (np.asarray([0, 2, 1] + [3] * 127), np.asarray([1, 2, 3])))      # decreasing offsets
    with pytest.raises(ValueError, match="malformed CSR"):
        ix.rank(Q, (np.arange(130), np.arange(100)))                               # offsets past the ids
    with pytest.raises(ValueError):
        ix.rank(Q, [[0]] * 128)                                                    # 128 rows of targets for 129 queries
    with pytest.raises(ValueError):
        ix.rank(Q, torch.zeros(129))                                               # float "ids"
    with pytest.raises(ValueError):
        ix.rank(Q[:, :32], [[0]] * 129)                                            # wrong width
    with pytest.raises(ValueError):
        FlatIPIndex(96, device=DEV)
    with pytest.raises(RuntimeError):
        FlatIPIndex(64, device="cpu")
    # the C ABI: shape and alignment errors are returned before any launch
    h = _C.lib()
    args = (c["D"].data_ptr(), 129, 257)
    tail = (1, 1, 0, 1, 1, 1, None)
    assert h.cx_rank_targets(Q.data_ptr(), *args, 96, 96, 96, *tail) == -1        # d % 64
    assert h.cx_rank_targets(Q.data_ptr(), *args, 2048, 2048, 2048, *tail) == -1  # d > 1024
    assert h.cx_rank_targets(Q.data_ptr(), *args, 64, 60, 64, *tail) == -2        # ldq < d
    assert h.cx_rank_targets(Q.data_ptr() + 2, *args, 64, 64, 64, *tail) == -2    # Q not 16-B aligned
    assert h.cx_rank_targets(Q.data_ptr(), *args, 64, 64, 64, None, 1, 0, 1, 1, 1, None) == -3   # null CSR
    assert h.cx_rank_targets(None, None, 1, 2 ** 31 - 128, 64, 64, 64, *tail) == -1


# ---- 6. metrics end to end on the device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,d", [(300, 1000, 64), (129, 257, 320), (127, 129, 1024)])
def test_topk_hits_equal_dense_metrics(M, N, d):
    from contrastors_amd.zeroshot import topk_hits

    Q, D = _grid_operands(M, N, d, 2 if d == 64 else 8, 5)
    labels = torch.randint(0, N, (M,), generator=torch.Generator().manual_seed(6))
    ranks, _, _ = _index(D).rank(Q, labels)
    assert topk_hits(ranks, ks=(1, 5, 20)) == R.dense_topk_hits(R.scores64(Q, D), labels, ks=(1, 5, 20))


def test_retrieval_recall_flickr_layout_both_directions():
    """40 images x 5 captions: image retrieval = caption -> its one image, text retrieval = image -> its five captions."""
    from contrastors_amd.zeroshot import retrieval_recall

    n_img, per = 40, 5
    img, txt = _grid_operands(n_img, n_img * per, 64, 2, 11)
    # make the pairs related, so that the recalls lie strictly between 0 and 1: a caption shares ~15 % of its entries with its image
    g = torch.Generator().manual_seed(12)
    own = img.cpu().repeat_interleave(per, 0)
    keep = torch.rand(n_img * per, 64, generator=g) < 0.15
    txt = torch.where(keep, own, txt.cpu()).to(DEV)
    cap_img = torch.arange(n_img * per) // per
    ks = (1, 5, 10)
    # image retrieval: rows = captions, corpus = images, one positive each
    ranks, _, ptr = _index(img).rank(txt, cap_img)
    got_i = retrieval_recall(ranks, ptr, ks)
    pos = torch.zeros(n_img * per, n_img, dtype=torch.bool)
    pos[torch.arange(n_img * per), cap_img] = True
    assert got_i == R.dense_recall(R.scores64(txt, img), pos, ks)
    # text retrieval: rows = images, corpus = captions, five positives each
    lists = [list(range(m * per, (m + 1) * per)) for m in range(n_img)]
    ranks, _, ptr = _index(txt).rank(img, lists)
    got_t = retrieval_recall(ranks, ptr, ks)
    assert got_t == R.dense_recall(R.scores64(img, txt), pos.T, ks)
    assert 0.0 < got_i[0] < got_i[2] < 1.0 and 0.0 < got_t[0] < got_t[2] < 1.0   # a non-trivial layout
    with pytest.raises(ValueError):
        retrieval_recall(torch.zeros(1, dtype=torch.int64), torch.tensor([0, 0, 1]), ks)   # a row without positives
