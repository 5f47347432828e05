"""The float64 reference of the windowed top-k search and of the list merge (tests/search_window_ref.py) against a brute-force
loop on tiny inputs, and against planted errors: each mistake at a window's bounds, in the tie order or in the merge's id that
the GPU tests exist to find must make the checker fail."""
import numpy as np
import pytest
import torch

from tests import search_window_ref as W


def _tiny(M=9, N=23, d=64, levels=1, seed=0):
    """Entries in {-1, 0, 1}: few distinct scores, so every row has ties."""
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randint(-levels, levels + 1, (M, d), generator=g).float() / levels).to(torch.bfloat16)
    D = (torch.randint(-levels, levels + 1, (N, d), generator=g).float() / levels).to(torch.bfloat16)
    D[N // 2:] = D[: N - N // 2].clone()              # duplicated rows: exact ties in every query row
    return Q, D


def _bounds(Q, D):
    """Windows with bounds at -1, 0, 1, N - 1, N, above N, negative, empty (end == min_id + 1) and inverted; below ON an
    attained score for some rows; a few excluded ids (one outside the window, one outside the corpus)."""
    S = W.scores64(Q, D)
    M, N = S.shape
    min_id = [-1, 0, 5, N - 2, -1, 3, 11, 7, -5][:M]
    end_id = [N, N - 1, N + 7, N, 1, 4, 0, -3, 12][:M]
    below = [float("inf")] * M
    below[0] = float(S[0].max())                      # the best score itself is not below it
    below[2] = float(S[2].median())
    exclude = [[] for _ in range(M)]
    exclude[0] = [int(S[0].argmax()), N + 3]
    exclude[1] = [1, 2, 0]
    exclude[8] = [0, 11]
    return min_id, end_id, exclude, below


def _brute(Q, D, k, min_id, end_id, exclude, below, id_map=None):
    q, dd = Q.double().numpy(), D.double().numpy()
    N = dd.shape[0]
    out_s, out_i = [], []
    for m in range(q.shape[0]):
        cands = []
        for n in range(N):
            s = float(np.dot(q[m], dd[n]))
            if min_id[m] < n < end_id[m] and s < below[m] and n not in exclude[m]:      # (0 <= n < N already)
                cands.append((-s, n if id_map is None else int(id_map[n])))
        cands.sort()
        cands = cands[:k] + [(np.inf, -1)] * (k - len(cands))
        out_s.append([-c[0] for c in cands])
        out_i.append([c[1] for c in cands])
    return out_s, out_i


@pytest.mark.parametrize("k", [1, 4, 30])
def test_reference_equals_brute_force(k):
    for seed in range(3):
        Q, D = _tiny(seed=seed)
        N = D.shape[0]
        min_id, end_id, exclude, below = _bounds(Q, D)
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
        for id_map in (None, perm):
            s, i = W.ref_window_topk(Q, D, k, min_id, end_id, exclude, below, id_map)
            bs, bi = _brute(Q, D, k, min_id, end_id, exclude, below, id_map)
            assert i.tolist() == bi and s.tolist() == bs
            W.check_exact(Q, D, k, s.float(), i, min_id, end_id, exclude, below, id_map)
        s, i = W.ref_window_topk(Q, D, k, min_id, end_id, exclude, below)
        assert (i[5] == -1).all() and (i[6] == -1).all() and (i[7] == -1).all()      # empty and inverted windows
        assert i[4].tolist() == [0] + [-1] * (k - 1)                                 # the window (-1, 1) holds id 0
        # no bounds at all is the plain top-k
        s, i = W.ref_window_topk(Q, D, k)
        bs, bi = _brute(Q, D, k, [-1] * 9, [N] * 9, [[]] * 9, [float("inf")] * 9)
        assert i.tolist() == bi and s.tolist() == bs


def test_planted_errors_are_caught():
    Q, D = _tiny(seed=1)
    N, k = D.shape[0], 6
    min_id, end_id, exclude, below = _bounds(Q, D)
    S = W.scores64(Q, D)
    mid, end = torch.tensor(min_id), torch.tensor(end_id)
    col = torch.arange(N)
    rest = W.admitted(S, None, None, exclude, below)
    lo_ok = col[None, :] > mid.clamp(-1, N)[:, None]
    hi_ok = col[None, :] < end.clamp(0, N)[:, None]
    good = W.admitted(S, min_id, end_id, exclude, below)
    assert torch.equal(good, rest & lo_ok & hi_ok)
    planted = {
        "<= at the lower bound": rest & (col[None, :] >= mid[:, None]) & hi_ok,
        "<= at the upper bound": rest & lo_ok & (col[None, :] <= end.clamp(0, N)[:, None]),
        # a negative end that is not clamped to 0 and then read as unsigned: the window is open above
        "unclamped negative end": rest & lo_ok & ((col[None, :] < end[:, None]) | (end[:, None] < 0)),
        "below not strict": W.admitted(S, min_id, end_id, exclude, None) & (S <= torch.tensor(below, dtype=torch.float64)[:, None]),
        "exclusions dropped": W.admitted(S, min_id, end_id, None, below),
    }
    for name, mask in planted.items():
        assert not torch.equal(mask, good), f"{name}: the inputs do not exercise it"
        s, i = W.topk_from_mask(S, mask, k)
        with pytest.raises(AssertionError):
            W.check_exact(Q, D, k, s.float(), i, min_id, end_id, exclude, below)
    # ties broken upward: equal scores by DESCENDING id
    s, i = W.topk_from_mask(S.flip(1), good.flip(1), k)
    i = torch.where(i >= 0, N - 1 - i, i)
    assert torch.equal(s, W.ref_window_topk(Q, D, k, min_id, end_id, exclude, below)[0])      # the same scores ...
    with pytest.raises(AssertionError, match="ids differ"):
        W.check_exact(Q, D, k, s.float(), i, min_id, end_id, exclude, below)                   # ... in another id order
    # the order of POSITIONS reported through id_map afterwards is not the order of the mapped ids
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    s, i = W.topk_from_mask(S, good, k)
    i = torch.where(i >= 0, perm[i.clamp(min=0)], i)
    with pytest.raises(AssertionError, match="ids differ"):
        W.check_exact(Q, D, k, s.float(), i, min_id, end_id, exclude, below, id_map=perm)


def _lists(M, L, k, N, seed, levels=3):
    """P = M * L sorted lists over disjoint positions per output row, scores on a coarse grid (ties inside and across lists),
    lengths 0 / 1 / k / random, padded; src with some entries -1; a random id_map."""
    g = np.random.default_rng(seed)
    id_map = g.permutation(N).astype(np.int64)
    scores = np.full((M * L, k), -np.inf, dtype=np.float32)
    ids = np.full((M * L, k), -1, dtype=np.int64)
    src = np.arange(M * L, dtype=np.int64).reshape(M, L)
    for m in range(M):
        pool = g.permutation(N)
        used = 0
        for l in range(L):
            n = [0, 1, k, int(g.integers(0, k + 1))][(m + l) % 4]
            n = min(n, N - used)
            pos = pool[used: used + n]
            used += n
            s = g.integers(-levels, levels + 1, n).astype(np.float32) / 2
            o = np.lexsort((id_map[pos], -s))
            scores[m * L + l, :n], ids[m * L + l, :n] = s[o], pos[o]
    drop = g.random((M, L)) < 0.2
    return scores, ids, np.where(drop, -1, src), id_map


@pytest.mark.parametrize("L", [1, 3, 16])
def test_merge_reference_against_a_loop(L):
    M, k, N = 7, 5, 400
    scores, ids, src, id_map = _lists(M, L, k, N, seed=L)
    for rep in (None, id_map):
        for kk in (1, k, 2 * k):
            s, i = W.merge_ref(scores, ids, src, kk, rep)
            for m in range(M):
                ent = []
                for r in src[m]:
                    if r >= 0:
                        ent += [(-float(a), int(b if rep is None else rep[b])) for a, b in zip(scores[r], ids[r]) if b >= 0]
                ent.sort()
                ent = ent[:kk] + [(np.inf, -1)] * (kk - len(ent))
                assert s[m].tolist() == [-e[0] for e in ent] and i[m].tolist() == [e[1] for e in ent]
    # merging by position and mapping afterwards is a different answer on these lists (cross-list ties)
    s, i = W.merge_ref(scores, ids, src, k, id_map)
    s2, i2 = W.merge_ref(scores, ids, src, k, None)
    i2 = np.where(i2 >= 0, id_map[np.maximum(i2, 0)], -1)
    if L > 1:
        assert np.array_equal(s, s2) and not np.array_equal(i, i2)
