"""Yardstick of the retrieval metrics (tests/test_ir_ref_cpu.py pins it; tests/test_ir_metrics_gpu.py measures cx_ir_metrics
against it).  Written from the ranked LIST, not from the kernel's counting formulation: sort a dense float64 score row
(descending, ties to the lower id), delete the excluded ids, walk the list and accumulate with math.fsum (correctly rounded
sums).  trec_eval's ndcg_cut / map_cut / recall / P and BEIR's MRR: linear gains, the ideal ranking over the JUDGED documents,
AP over the number of relevant documents.  Plain Python: no torch, no numpy."""
import math

NAMES = ("ndcg", "map", "recall", "precision", "mrr", "hit")


def ranked_ids(scores):
    """Document ids of a dense score row in retrieval order: score descending, ties to the lower id."""
    return sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))


def walk(ranking, gains, ks):
    """ranking: the retrieved list, as the gain of each position (0 = not relevant) -- or, for lists too long to write down,
    its non-zero part as ascending (position, gain) pairs.  gains: the gains of ALL judged-relevant documents of the query
    (retrieved or not: here every document is retrieved, so the two agree).  -> {name: [value per k]} and "nrel"."""
    if ranking and isinstance(ranking[0], tuple):
        found = list(ranking)
    else:
        found = [(p, g) for p, g in enumerate(ranking) if g > 0]
    assert all(a[0] < b[0] for a, b in zip(found, found[1:]))
    R = sum(1 for g in gains if g > 0)
    ideal = sorted((g for g in gains if g > 0), reverse=True)
    out = {n: [] for n in NAMES}
    for k in ks:
        top = [(p, g) for p, g in found if p < k]
        if R == 0:
            for n in NAMES:
                out[n].append(0.0)
            continue
        dcg = math.fsum(g / math.log2(p + 2) for p, g in top)
        idcg = math.fsum(g / math.log2(i + 2) for i, g in enumerate(ideal[:k]))
        ap = math.fsum((i + 1) / (p + 1) for i, (p, _) in enumerate(top))       # i + 1 relevant documents down to position p
        out["ndcg"].append(dcg / idcg)
        out["map"].append(ap / R)
        out["recall"].append(len(top) / R)
        out["precision"].append(len(top) / k)
        out["mrr"].append(1.0 / (top[0][0] + 1) if top else 0.0)
        out["hit"].append(1.0 if top else 0.0)
    out["nrel"] = R
    return out


def metrics_from_scores(scores, rel, excluded, ks):
    """scores: a dense row; rel: {doc id: gain > 0}; excluded: ids deleted from the ranking before anything is counted."""
    kept = [d for d in ranked_ids(scores) if d not in excluded]
    rel = {d: g for d, g in rel.items() if d not in excluded}
    return walk([rel.get(d, 0) for d in kept], list(rel.values()), ks)


def metrics_from_order(order, rel, excluded, ks):
    """The same from an already ranked id list (what FlatIPIndex.search(k = N) returns)."""
    kept = [int(d) for d in order if int(d) not in excluded]
    rel = {d: g for d, g in rel.items() if d not in excluded}
    return walk([rel.get(d, 0) for d in kept], list(rel.values()), ks)


def metrics_from_ranks(ranks, gains, ks):
    """The sparse form, for ranks too large to write the list down (up to 2^31 - 2): entries (rank, gain) of the judged
    documents, gain 0 = excluded.  Deleting an excluded document moves everything behind it up by one position."""
    removed, found = 0, []
    for r, g in sorted(zip((int(r) for r in ranks), (float(g) for g in gains))):
        if g > 0:
            found.append((r - removed, g))
        else:
            removed += 1
    return walk(found, [g for _, g in found], ks) if found else walk([], [], ks)


def bound(n):
    """Relative error allowed to an fp64 implementation on a row of n entries: two sums of at most n non-negative terms and
    their quotient, the device log2 and divisions taken as <= 2 ulp."""
    return (2 * n + 16) * 2.0 ** -53
