"""tests/rank_ref.py is itself checked here, on the CPU: its ranks against torch.topk on tie-free inputs, its tie rule on a
hand-made row, its dense metrics on a worked example, and a planted off-by-one must be seen."""
import torch

from tests import rank_ref as R


def _tie_free(M, N, d, seed):
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(M, d, generator=g).to(torch.bfloat16)
    D = torch.randn(N, d, generator=g).to(torch.bfloat16)
    S = R.scores64(Q, D)
    srt = torch.sort(S, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "the generator produced a tie"
    return Q, D, S


def test_ranks_agree_with_topk_on_tie_free_inputs():
    M, N = 37, 211
    Q, D, S = _tie_free(M, N, 64, 0)
    order = torch.topk(S, N, dim=1).indices                  # order[m, r] = the id at rank r
    want = torch.empty(M, N, dtype=torch.int64)
    want.scatter_(1, order, torch.arange(N).expand(M, -1))   # want[m, id] = rank
    row_ptr = torch.arange(M + 1) * N                        # every column of every row is a target
    ids = torch.arange(N).repeat(M)
    ranks, scores = R.ref_rank(Q, D, row_ptr, ids, chunk_rows=8)
    assert torch.equal(ranks.view(M, N), want)
    assert torch.equal(scores.view(M, N), S)
    # a ragged CSR with empty rows and a repeated id
    lists = [[], [5], [0, N - 1, 5, 5], [], [17]] + [[m] for m in range(5, M)]
    ptr = torch.tensor([0] + [len(x) for x in lists]).cumsum(0)
    flat = torch.tensor([i for x in lists for i in x])
    ranks, _ = R.ref_rank(Q, D, ptr, flat, chunk_rows=3)
    e = 0
    for m, x in enumerate(lists):
        for t in x:
            assert int(ranks[e]) == int(want[m, t])
            e += 1


def test_ties_go_to_the_lower_id():
    Q = torch.tensor([[1.0] + [0.0] * 63]).to(torch.bfloat16)
    D = torch.zeros(6, 64)
    D[:, 0] = torch.tensor([0.5, 1.0, 0.5, 1.0, 0.25, 0.5])
    D = D.to(torch.bfloat16)
    ranks, scores = R.ref_rank(Q, D, [0, 6], list(range(6)))
    assert ranks.tolist() == [2, 0, 3, 1, 5, 4]
    assert scores.tolist() == [0.5, 1.0, 0.5, 1.0, 0.25, 0.5]
    assert R.dense_order(R.scores64(Q, D))[0].tolist() == [1, 3, 0, 2, 5, 4]
    assert R.near_count(Q, D, [0, 6], list(range(6)), 1e-5).tolist() == [2, 1, 2, 1, 0, 2]


def test_dense_metrics_on_a_worked_example():
    S = torch.tensor([[0.9, 0.1, 0.5, 0.3],     # order 0 2 3 1
                      [0.2, 0.8, 0.8, 0.1],     # order 1 2 0 3 (tie to the lower id)
                      [0.1, 0.2, 0.3, 0.4]],    # order 3 2 1 0
                     dtype=torch.float64)
    assert R.dense_topk_hits(S, [0, 2, 0], ks=(1, 2, 4)) == [1, 2, 3]
    pos = R.dense_positives(3, 4, [0, 2, 3, 5], [1, 3, 2, 0, 1])
    assert pos.tolist() == [[False, True, False, True], [False, False, True, False], [True, True, False, False]]
    assert R.dense_recall(S, pos, ks=(1, 2, 3)) == [0.0, 1 / 3, 1.0]


def test_a_planted_off_by_one_is_seen():
    M, N = 16, 50
    Q, D, S = _tie_free(M, N, 64, 1)
    labels = torch.randint(0, N, (M,), generator=torch.Generator().manual_seed(2))
    ranks, _ = R.ref_rank(Q, D, torch.arange(M + 1), labels)
    order = R.dense_order(S)
    assert all(int(order[m, int(ranks[m])]) == int(labels[m]) for m in range(M))
    # shift one rank by one: the id found at that position is no longer the label
    m = int(torch.argmax(ranks))
    assert int(order[m, int(ranks[m]) - 1]) != int(labels[m])
    # ... and the hit count at k = rank changes by exactly one
    k = int(ranks[m])
    hits_k, hits_k1 = R.dense_topk_hits(S, labels, ks=(k, k + 1))
    assert hits_k == int((ranks < k).sum()) and hits_k1 == int((ranks < k + 1).sum()) and hits_k1 >= hits_k + 1
