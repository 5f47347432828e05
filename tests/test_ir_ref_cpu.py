"""The retrieval-metric yardstick (tests/ir_ref.py) pinned three ways: to values computed by hand on a 6-document example, to
scikit-learn's ndcg_score / average_precision_score on random distinct-score cases, and against planted errors, which the
same pins must catch."""
import math
import random

import numpy as np
import pytest

from tests import ir_ref as R

# 6 documents.  Order by score: 0, 1, 2, 3, 4, 5 (3 and 4 tie: the lower id first).  Document 1 is excluded and sits AHEAD of the
# first relevant one, so the list that is scored is 0, 2, 3, 4, 5: document 2 (gain 3) at position 1, document 4 (gain 1) at
# position 3, document 5 (gain 2) at position 4.  R = 3; the ideal list has gains 3, 2, 1.
SCORES = [0.9, 0.8, 0.7, 0.5, 0.5, 0.4]
REL = {2: 3.0, 4: 1.0, 5: 2.0}
EXCLUDED = {1}
L2 = math.log2
HAND = {   # k: (ndcg, ap, recall, precision, rr, hit)
    1: (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),                                                     # position 0 holds nothing
    2: ((3 / L2(3)) / (3 / L2(2) + 2 / L2(3)), (1 / 2) / 3, 1 / 3, 1 / 2, 1 / 2, 1.0),     # k below R
    5: ((3 / L2(3) + 1 / L2(5) + 2 / L2(6)) / (3 / L2(2) + 2 / L2(3) + 1 / L2(4)), (1 / 2 + 2 / 4 + 3 / 5) / 3, 1.0, 3 / 5,
        1 / 2, 1.0),                                                                       # k above R
}
HAND_DECIMAL = {2: (0.44412286644879784, 0.16666666666666666), 5: (0.6504121821761035, 0.5333333333333333)}   # (ndcg, ap)


def _check_hand(fn):
    got = fn(SCORES, REL, EXCLUDED, (1, 2, 5))
    assert got["nrel"] == 3
    for j, k in enumerate((1, 2, 5)):
        for name, want in zip(R.NAMES, HAND[k]):
            assert got[name][j] == pytest.approx(want, rel=4e-16, abs=0), (name, k, got[name][j], want)
    for j, k in ((1, 2), (2, 5)):
        assert got["ndcg"][j] == pytest.approx(HAND_DECIMAL[k][0], rel=4e-16)
        assert got["map"][j] == pytest.approx(HAND_DECIMAL[k][1], rel=4e-16)


def _random_case(rng, n, graded):
    scores = rng.sample(range(10 * n), n)                  # distinct
    nrel = rng.randint(1, max(1, n // 3))
    rel = {d: float(rng.choice((1, 2, 3))) if graded else 1.0 for d in rng.sample(range(n), nrel)}
    return [float(s) for s in scores], rel


def _check_sklearn(fn, cases=60):
    from sklearn.metrics import average_precision_score, ndcg_score

    rng = random.Random(11)
    worst = 0.0
    for c in range(cases):
        n = rng.randint(2, 40)
        scores, rel = _random_case(rng, n, graded=c % 2 == 0)
        y_true = np.array([[rel.get(d, 0.0) for d in range(n)]])
        for k in (1, 3, n // 2 + 1, n, n + 5):
            got = fn(scores, rel, set(), (k,))
            want = ndcg_score(y_true, np.array([scores]), k=k)
            worst = max(worst, abs(got["ndcg"][0] - want))
            assert got["ndcg"][0] == pytest.approx(want, rel=1e-13, abs=1e-15), (c, k)
        if c % 2:   # binary: AP over the whole list
            got = fn(scores, rel, set(), (n,))
            want = average_precision_score(y_true[0] > 0, np.array(scores))
            worst = max(worst, abs(got["map"][0] - want))
            assert got["map"][0] == pytest.approx(want, rel=1e-13), c
    return worst


def test_hand_computed_example():
    _check_hand(R.metrics_from_scores)
    # the sparse form sees the same query as (rank, gain) entries; the excluded document is the gain-0 entry
    sparse = R.metrics_from_ranks([2, 4, 5, 1], [3.0, 1.0, 2.0, 0.0], (1, 2, 5))
    assert sparse == R.metrics_from_scores(SCORES, REL, EXCLUDED, (1, 2, 5))
    # without the exclusion every relevant document sits one position lower
    moved = R.metrics_from_scores(SCORES, REL, set(), (2, 5))
    assert moved["hit"] == [0.0, 1.0] and moved["mrr"][1] == 1 / 3 and moved["recall"][1] == 2 / 3


def test_agrees_with_scikit_learn():
    worst = _check_sklearn(R.metrics_from_scores)
    print(f"max |yardstick - scikit-learn| over the random cases: {worst:.3e}")


def test_sparse_and_dense_forms_agree_exactly():
    rng = random.Random(5)
    for c in range(100):
        n = rng.randint(1, 50)
        scores, rel = _random_case(rng, n, graded=True)
        pool = [d for d in range(n) if d not in rel]
        excluded = set(rng.sample(pool, min(len(pool), rng.randint(0, 3))))
        order = R.ranked_ids(scores)
        rank = {d: p for p, d in enumerate(order)}
        ids = list(rel) + list(excluded)
        ks = (1, 2, 5, n, 100)
        dense = R.metrics_from_scores(scores, rel, excluded, ks)
        assert R.metrics_from_ranks([rank[d] for d in ids], [rel.get(d, 0.0) for d in ids], ks) == dense
        assert R.metrics_from_order(order, rel, excluded, ks) == dense


def test_edge_rows():
    assert R.metrics_from_ranks([], [], (1, 10)) == {**{n: [0.0, 0.0] for n in R.NAMES}, "nrel": 0}
    only_excluded = R.metrics_from_ranks([0, 3], [0.0, 0.0], (1,))
    assert only_excluded["nrel"] == 0 and only_excluded["ndcg"] == [0.0]
    big = R.metrics_from_ranks([2 ** 31 - 2, 0], [1.0, 0.0], (1, 2 ** 31 - 2))    # behind one excluded: position 2^31 - 3
    assert big["hit"] == [0.0, 1.0] and big["mrr"][1] == 1.0 / (2 ** 31 - 2) and big["ndcg"][1] == 1.0 / math.log2(2 ** 31 - 1)
    assert R.ranked_ids([1.0, 2.0, 2.0, 0.5]) == [1, 2, 0, 3]
    assert R.bound(0) == 16 * 2.0 ** -53 and R.bound(4096) == 8208 * 2.0 ** -53


# ---- planted errors: the pins above have to catch each of them ------------------------------------------------------------
def _mutant(flaw):
    def fn(scores, rel, excluded, ks):
        kept = [d for d in R.ranked_ids(scores) if d not in excluded]
        found = [(p, rel[d]) for p, d in enumerate(kept) if d in rel]
        Rn = len(rel)
        out = {n: [] for n in R.NAMES}
        for k in ks:
            top = [(p, g) for p, g in found if p < k]
            shift = 1 if flaw == "discount" else 2                      # log2(p + 1): the 1-based discount off by one
            dcg = math.fsum(g / math.log2(p + shift) if p + shift > 1 else g for p, g in top)
            pool = [g for _, g in top] if flaw == "idcg" else list(rel.values())      # the ideal list over what was retrieved
            idcg = math.fsum(g / math.log2(i + 2) for i, g in enumerate(sorted(pool, reverse=True)[:k]))
            ap = math.fsum((i + 1) / (p + 1) for i, (p, _) in enumerate(top))
            out["ndcg"].append(dcg / idcg if idcg else 0.0)
            out["map"].append(ap / (min(k, Rn) if flaw == "ap" else Rn))              # AP over min(k, R)
            out["recall"].append(len(top) / Rn)
            out["precision"].append(len(top) / k)
            out["mrr"].append(1.0 / (top[0][0] + 1) if top else 0.0)
            out["hit"].append(1.0 if top else 0.0)
        out["nrel"] = Rn
        return out
    return fn


def test_the_mutant_scaffold_itself_passes_without_a_flaw():
    _check_hand(_mutant(None))
    _check_sklearn(_mutant(None), cases=20)


@pytest.mark.parametrize("flaw", ["discount", "idcg", "ap"])
def test_planted_errors_are_caught(flaw):
    with pytest.raises(AssertionError):
        _check_hand(_mutant(flaw))
    if flaw != "ap":   # scikit-learn's AP is over the whole list, where min(k, R) = R: the hand example is what catches it
        with pytest.raises(AssertionError):
            _check_sklearn(_mutant(flaw), cases=20)
