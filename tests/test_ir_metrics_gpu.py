"""GPU checks of the retrieval-metrics kernel (csrc/ir_metrics.hip through contrastors_amd.retrieval_eval.ir_metrics and the C
ABI) against the list-walking yardstick of tests/ir_ref.py: per row and per cut-off over row lengths at the workgroup edges,
binary and graded gains, excluded entries before / between / after the relevant ones, ranks up to 2^31 - 2 and rows without a
relevant entry; exact counts, real-valued metrics within ir_ref.bound(n) = (2 n + 16) 2^-53 relative (measured maximum
3.78 x 2^-53, on the nDCG of a 256-entry row; each test prints its own), bitwise reproducibility, the return codes, and evaluate_embeddings end to end against the yardstick
applied to the order FlatIPIndex.search returns."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ir_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (1, 3, 10, 100, 1000)
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096)
RANK_MAX = 2 ** 31 - 2


def _row(n, rng, graded, n_excl, place, span):
    """n entries with distinct ranks: n_excl of them excluded (gain 0), sitting before / between / after the relevant ones in
    rank order (or anywhere); span: "dense" ranks within [0, 2 n] (cut-offs bite), "wide" up to 2^31 - 2 (that value included)."""
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    if span == "dense":
        ranks = np.sort(rng.choice(2 * n + 1, size=n, replace=False)).astype(np.int64)
    else:
        ranks = np.unique(np.concatenate([rng.integers(0, RANK_MAX, size=n - 1), [RANK_MAX]]).astype(np.int64))
        while ranks.size < n:
            ranks = np.unique(np.concatenate([ranks, rng.integers(0, RANK_MAX, size=n - ranks.size)]))
    n_excl = min(n_excl, n)
    slots = {"before": np.arange(n_excl), "after": np.arange(n - n_excl, n),
             "between": (n - n_excl) // 2 + np.arange(n_excl), "any": rng.choice(n, size=n_excl, replace=False)}[place]
    gains = (rng.integers(1, 4, size=n) if graded else np.ones(n)).astype(np.float32)
    gains[slots] = 0.0
    perm = rng.permutation(n)          # entries come in the caller's order, not in rank order
    return ranks[perm], gains[perm]


@functools.lru_cache(maxsize=None)
def _cases(M):
    """Rows of a launch of M queries, the yardstick's metrics (M, K, 6) and nrel, and the row lengths."""
    rng = np.random.default_rng(100 + M)
    lengths = {1: (4096,), 7: (0, 1, 63, 64, 65, 257, 4096)}.get(M) or tuple(LENGTHS[m % len(LENGTHS)] for m in range(M))
    rows = []
    for m, n in enumerate(lengths):
        n_excl = (0, 1, 5)[(m // len(LENGTHS)) % 3] if M > 7 else (0, 1, 5)[m % 3]
        place = ("before", "between", "after", "any")[(m // 3) % 4]
        if M > 7 and m % 23 == 22:
            n_excl = n                 # nothing but excluded entries: R = 0
        rows.append(_row(n, rng, graded=m % 2 == 1, n_excl=n_excl, place=place, span="wide" if m % 5 == 4 else "dense"))
    want = np.zeros((M, len(KS), 6))
    nrel = np.zeros(M, np.int64)
    for m, (ranks, gains) in enumerate(rows):
        ref = R.metrics_from_ranks(ranks.tolist(), gains.tolist(), KS)
        nrel[m] = ref["nrel"]
        for i, name in enumerate(R.NAMES):
            want[m, :, i] = ref[name]
    row_ptr = np.zeros(M + 1, np.int64)
    row_ptr[1:] = np.cumsum([len(r) for r, _ in rows])
    ranks = np.concatenate([r for r, _ in rows]) if rows else np.zeros(0, np.int64)
    gains = np.concatenate([g for _, g in rows]) if rows else np.zeros(0, np.float32)
    return row_ptr, ranks, gains, want, nrel, np.asarray(lengths)


def _stack(m):
    return np.stack([np.asarray(m[n].cpu() if isinstance(m[n], torch.Tensor) else m[n]) for n in
                     ("ndcg", "map", "recall", "precision", "mrr", "hit")], axis=-1)


def _compare(got, want, lengths, what):
    """Relative error per row against ir_ref.bound(row length); prints the measured maximum in units of 2^-53."""
    tol = np.asarray([R.bound(int(n)) for n in lengths])[:, None, None]
    assert np.isfinite(got).all()
    assert ((want == 0) == (got == 0)).all(), f"{what}: zeros differ"
    rel = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    worst = rel.max(axis=(1, 2)) if rel.size else np.zeros(0)
    m = int(worst.argmax()) if worst.size else 0
    print(f"{what}: max relative error {rel.max() / 2.0 ** -53 if rel.size else 0:.2f} x 2^-53 "
          f"(row of {int(lengths[m]) if worst.size else 0} entries; its bound {(2 * int(lengths[m]) + 16) if worst.size else 16} x 2^-53); "
          f"per metric {[float(f'{x / 2.0 ** -53:.2f}') for x in rel.max(axis=(0, 1))] if rel.size else []}")
    bad = np.argwhere(rel > tol)
    assert bad.size == 0, f"{what}: {len(bad)} values over the bound, first (row, cut-off, metric) = {bad[0].tolist()}: " \
                          f"got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r} bound {tol[bad[0][0], 0, 0]:.3e}"


@pytest.mark.parametrize("M", [1, 7, 300])
def test_kernel_against_the_yardstick(M):
    from contrastors_amd.retrieval_eval import ir_metrics

    row_ptr, ranks, gains, want, nrel, lengths = _cases(M)
    if M == 300:
        assert set(lengths.tolist()) == set(LENGTHS) and (nrel == 0).sum() >= 20 and ranks.max() == RANK_MAX
    m = ir_metrics(torch.from_numpy(ranks).to(DEV), torch.from_numpy(gains).to(DEV), row_ptr, KS)
    got = _stack(m)
    assert m["ks"] == list(KS) and got.shape == (M, len(KS), 6) and m["ndcg"].dtype == torch.float64
    # counts are exact
    got_nrel = m["nrel"].cpu().numpy()
    assert (got_nrel == nrel).all()
    assert (got[..., 5] == want[..., 5]).all()
    hits_want = np.rint(want[..., 2] * nrel[:, None])
    assert (np.rint(got[..., 2] * nrel[:, None]) == hits_want).all()
    assert (np.rint(got[..., 3] * np.asarray(KS)[None, :]) == hits_want).all()
    assert (got[nrel == 0] == 0).all()
    _compare(got, want, lengths, f"cx_ir_metrics M={M}")
    # a second run gives the same bits; numpy in -> numpy out
    again = ir_metrics(ranks, gains, row_ptr, KS)
    assert isinstance(again["ndcg"], np.ndarray) and (again["nrel"] == got_nrel).all()
    assert np.array_equal(_stack(again).view(np.int64), got.view(np.int64))


def test_return_codes_and_refusals():
    from contrastors_amd import _C
    from contrastors_amd.retrieval_eval import MAX_ROW, ir_metrics

    h = _C.lib()
    rp = torch.tensor([0, 2], dtype=torch.int64, device=DEV)
    ranks = torch.tensor([3, 0], dtype=torch.int64, device=DEV)
    gains = torch.tensor([1.0, 2.0], dtype=torch.float32, device=DEV)
    out = torch.full((1, 8, 6), -1.0, dtype=torch.float64, device=DEV)
    nrel = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    s = _C.cur_stream()

    def call(M=1, ks=(1, 10), K=None, rp_=rp, ranks_=ranks, gains_=gains, out_=out, nrel_=nrel, null_ks=False):
        arr = None if null_ks else (ctypes.c_int * max(len(ks), 1))(*ks)
        return h.cx_ir_metrics(_C.ptr(rp_), _C.ptr(ranks_), _C.ptr(gains_), M, arr, len(ks) if K is None else K, _C.ptr(out_),
                               _C.ptr(nrel_), s)

    assert call(K=0) == -1 and call(ks=tuple(range(1, 10))) == -1 and call(ks=(10, 0)) == -1 and call(ks=(-3,)) == -1
    assert call(M=-1) == -1
    assert call(null_ks=True, K=2) == -3
    for k in ("rp_", "ranks_", "gains_", "out_", "nrel_"):
        assert call(**{k: None}) == -3, k
    assert call(M=0) == 0 and call(M=0, rp_=None, out_=None) == 0          # a no-op: nothing is looked at
    torch.cuda.synchronize()
    assert float(out.max()) == -1.0 and int(nrel[0]) == -7                  # nothing above launched
    assert call(ks=tuple(range(1, 9))) == 0                                 # K = 8 is the most
    torch.cuda.synchronize()
    assert int(nrel[0]) == 2 and out[0, :, 5].tolist() == [1.0] * 8
    assert float(out[0, 0, 0]) == 1.0                                       # nDCG@1: the gain-2 entry at rank 0
    assert float(out[0, 1, 0]) == pytest.approx(2.0 / (2.0 + 1.0 / np.log2(3.0)), rel=R.bound(2))   # @2: rank 3 is outside
    # the Python layer refuses what the kernel cannot stage, and malformed input, before any launch
    big = np.arange(MAX_ROW + 1)
    with pytest.raises(ValueError, match="4097 entries"):
        ir_metrics(big, np.ones(MAX_ROW + 1, np.float32), np.array([0, MAX_ROW + 1]))
    with pytest.raises(ValueError, match="1 to 8"):
        ir_metrics(big[:4], np.ones(4, np.float32), np.array([0, 4]), ks=range(1, 10))
    with pytest.raises(ValueError, match="finite"):
        ir_metrics(big[:2], np.array([1.0, np.nan], np.float32), np.array([0, 2]))
    with pytest.raises(ValueError, match="finite and >= 0"):
        ir_metrics(big[:2], np.array([1.0, -1.0], np.float32), np.array([0, 2]))
    with pytest.raises(ValueError, match="malformed CSR"):
        ir_metrics(big[:2], np.ones(2, np.float32), np.array([0, 3]))
    with pytest.raises(ValueError, match="integers"):
        ir_metrics(np.array([0.5, 1.0]), np.ones(2, np.float32), np.array([0, 2]))
    empty = ir_metrics(np.zeros(0, np.int64), np.zeros(0, np.float32), np.array([0]))
    assert empty["ndcg"].shape == (0, 5) and empty["nrel"].shape == (0,)
    # the C entry point itself never stages a row longer than its buffers: NaNs and nrel = -1, the next row is served
    rp2 = torch.tensor([0, MAX_ROW + 1, MAX_ROW + 2], dtype=torch.int64, device=DEV)
    r2 = torch.arange(MAX_ROW + 2, dtype=torch.int64, device=DEV)
    g2 = torch.ones(MAX_ROW + 2, dtype=torch.float32, device=DEV)
    out2 = torch.zeros(2, 2, 6, dtype=torch.float64, device=DEV)
    n2 = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert call(M=2, rp_=rp2, ranks_=r2, gains_=g2, out_=out2, nrel_=n2) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out2[0]).all()) and n2.tolist() == [-1, 1] and bool(torch.isfinite(out2[1]).all())
    assert out2[1, :, 5].tolist() == [0.0, 0.0]                             # rank 4097: outside both cut-offs


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)


def _task(M, N, rng, identical_every=0):
    """Random graded qrels, 1 to 9 relevant per query; with identical_every, every such query carries the id of a document
    (which BEIR's ignore_identical_ids takes out of its ranking)."""
    from contrastors_amd.retrieval_eval import RetrievalTask

    corpus_ids = [f"d{i}" for i in range(N)]
    qids, qrels = [], []
    for m in range(M):
        rel = {int(d): float(rng.integers(1, 4)) for d in rng.choice(N, size=int(rng.integers(1, 10)), replace=False)}
        qids.append(f"d{int(rng.integers(N))}" if identical_every and m % identical_every == 0 else f"q{m}")
        qrels.append(rel)
    return RetrievalTask("synthetic", corpus_ids, [""] * N, qids, [""] * M, qrels)


@pytest.mark.parametrize("d", [64, 320])
def test_evaluate_embeddings_equals_the_yardstick_on_the_search_order(d):
    from contrastors_amd.retrieval_eval import evaluate_embeddings
    from contrastors_amd.search import FlatIPIndex

    M, N = 129, 1000
    rng = np.random.default_rng(d)
    task = _task(M, N, rng, identical_every=4)
    q, c = _unit(M, d, 1).to(DEV), _unit(N, d, 2).to(DEV)
    ks = (1, 3, 10, 100, 1000)
    got = evaluate_embeddings(q, c, task, ks, exclude_identical=True, per_query=True)
    index = FlatIPIndex(d, device=DEV)
    index.add(c)
    order = index.search(q, N)[1].cpu().tolist()
    want = np.zeros((M, len(ks), 6))
    lengths = np.zeros(M, np.int64)
    for m in range(M):
        same = task.doc_index(task.query_ids[m])
        excluded = set() if same is None else {same}
        ref = R.metrics_from_order(order[m], task.qrels[m], excluded, ks)
        lengths[m] = len(set(task.qrels[m]) | excluded)
        for i, name in enumerate(R.NAMES):
            want[m, :, i] = ref[name]
        assert got["per_query"]["nrel"][m] == ref["nrel"]
    assert sum(task.doc_index(x) is not None for x in task.query_ids) == 33
    _compare(_stack(got["per_query"]), want, lengths, f"evaluate_embeddings d={d}")
    assert got["n_queries"] + got["n_skipped"] == M and got["query_ids"] == task.query_ids
    keep = got["per_query"]["nrel"] > 0
    import math

    for i, name in enumerate(R.NAMES):
        for j, k in enumerate(ks):
            mean = math.fsum(want[keep, j, i].tolist()) / int(keep.sum())
            assert abs(got[f"{name}@{k}"] - mean) <= (R.bound(int(lengths.max())) + 2 * 2.0 ** -53) * abs(mean), (name, k)
    # without the exclusion the same-id documents stay in the ranking
    plain = evaluate_embeddings(q, c, task, ks, exclude_identical=False, per_query=True)
    want_plain = np.zeros_like(want)
    for m in range(M):
        ref = R.metrics_from_order(order[m], task.qrels[m], set(), ks)
        for i, name in enumerate(R.NAMES):
            want_plain[m, :, i] = ref[name]
    _compare(_stack(plain["per_query"]), want_plain, np.asarray([len(x) for x in task.qrels]), f"no exclusion d={d}")
    assert not np.array_equal(want_plain, want)


def test_fixed_points_and_refused_widths():
    from contrastors_amd.retrieval_eval import RetrievalTask, evaluate_embeddings

    N, M, d = 1000, 129, 64
    c = _unit(N, d, 5)
    picks = np.random.default_rng(9).choice(N, size=M, replace=False)
    q = c[picks].clone()
    ks = (1, 3, 10, 100)
    # queries that are copies of their single relevant document
    task = RetrievalTask("copies", [f"d{i}" for i in range(N)], [""] * N, [f"q{m}" for m in range(M)], [""] * M,
                         [{int(p): 1.0} for p in picks])
    got = evaluate_embeddings(q, c, task, ks)
    for k in ks:
        assert [got[f"{n}@{k}"] for n in ("ndcg", "map", "recall", "mrr", "hit")] == [1.0] * 5, k
        assert got[f"precision@{k}"] == pytest.approx(1.0 / k, rel=2.0 ** -50)
    assert got["n_queries"] == M and got["n_skipped"] == 0
    # the same corpus with each query present under the query's own id, AHEAD of the corpus (a tie goes to the lower index)
    c2 = torch.cat([q, c])
    task2 = RetrievalTask("with-self", [f"q{m}" for m in range(M)] + [f"d{i}" for i in range(N)], [""] * (M + N),
                          [f"q{m}" for m in range(M)], [""] * M, [{M + int(p): 1.0} for p in picks])
    with_excl = evaluate_embeddings(q, c2, task2, ks, exclude_identical=True)
    without = evaluate_embeddings(q, c2, task2, ks, exclude_identical=False)
    for k in ks:
        assert [with_excl[f"{n}@{k}"] for n in ("ndcg", "map", "recall", "mrr", "hit")] == [1.0] * 5, k
    assert without["mrr@10"] == 0.5 and without["mrr@1"] == 0.0 and without["recall@1"] == 0.0 and without["recall@3"] == 1.0
    # a query without a relevant document is left out of the means
    task3 = RetrievalTask("skip", task.corpus_ids, task.corpus_texts, task.query_ids, task.query_texts,
                          [{} if m == 0 else r for m, r in enumerate(task.qrels)])
    got3 = evaluate_embeddings(q, c, task3, ks)
    assert got3["n_queries"] == M - 1 and got3["n_skipped"] == 1 and got3["ndcg@10"] == 1.0
    # widths the index refuses raise its own error; mismatched shapes raise before that
    with pytest.raises(ValueError, match="multiple of 64"):
        evaluate_embeddings(_unit(M, 96, 1), _unit(N, 96, 2), task, ks)
    with pytest.raises(ValueError, match="query / 999 corpus"):
        evaluate_embeddings(q, c[:999], task, ks)
