"""GPU checks of near-duplicate removal and decontamination (contrastors_amd.dedup and the tool on FlatIPIndex.range_search):
a planted near-duplicate corpus against the float64 reference and the planted clusters, a cluster larger than any top-k,
planted evaluation leaks, and python -m contrastors_amd.tools.dedup end to end."""
import gzip
import json

import numpy as np
import pytest
import torch

from tests import range_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _planted(n, d, sizes, seed, noise=1e-3):
    """n unit rows; cluster c = sizes[c] rows at scattered positions, each its base vector + `noise` Gaussian noise per entry,
    normalised.  Unrelated rows of this width score far below 0.9 (|cos| of random 64-d rows is ~0.125 +- 0.125).
    -> (x float32 (n, d), label (n,): the lowest row id of the row's cluster, or its own id)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    label = np.arange(n)
    rows = rng.permutation(n)[: sum(sizes)]
    at = 0
    for s in sizes:
        members = np.sort(rows[at: at + s])
        at += s
        base = rng.standard_normal(d).astype(np.float32)
        x[members] = base + noise * rng.standard_normal((s, d)).astype(np.float32) * np.linalg.norm(base) / np.sqrt(d)
        label[members] = members[0]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x, label


def _index(x):
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(x.shape[1], device=DEV)
    ix.add(torch.from_numpy(x))
    return ix


def test_planted_near_duplicates():
    from contrastors_amd.dedup import components, duplicate_edges, select_kept

    sizes = [2 + c % 8 for c in range(40)]                    # 40 clusters of sizes 2 .. 9: 220 of the 600 rows
    x, label = _planted(600, 64, sizes, 0)
    ix = _index(x)
    for batch_rows in (8192, 128, 100):
        src, dst, score = duplicate_edges(ix, 0.9, batch_rows=batch_rows)
        assert src.dtype == np.int64 and dst.dtype == np.int64 and score.dtype == np.float32
        assert bool((src < dst).all())
        key = src * 600 + dst
        assert bool((key[1:] > key[:-1]).all())               # (src, dst) order, every pair once
        # against float64: the strict upper triangle above 0.9, outside the rounding band
        D = ix.vectors
        lims = np.zeros(601, np.int64)
        lims[1:] = np.cumsum(np.bincount(src, minlength=600))
        inband = R.check_against_ref(D, D, 0.9, torch.arange(600), lims, score, dst, exact=False)
        assert inband == 0                                    # planted pairs score ~1, unrelated ones below 0.7
        assert src.size == sum(s * (s - 1) // 2 for s in sizes)
        labels = components(600, src, dst)
        assert labels.tolist() == label.tolist()              # the planted clusters, labelled by their lowest id
        for rule in ("components", "greedy"):                 # cliques: both rules keep the lowest id of each cluster
            kept = select_kept(600, src, dst, rule)
            assert kept.tolist() == (label == np.arange(600)).tolist()
            assert int(kept.sum()) == 600 - 220 + 40
    with pytest.raises(ValueError, match="max_edges = 100"):
        duplicate_edges(ix, 0.9, max_edges=100)


def test_cluster_larger_than_any_top_k():
    """One cluster of 1050 near-copies in 1100 rows: more neighbours per row than search() can return (MAX_K = 1024)."""
    from contrastors_amd.dedup import components, duplicate_edges, select_kept
    from contrastors_amd.search import MAX_K

    assert 1050 > MAX_K + 1
    x, label = _planted(1100, 64, [1050], 1)
    ix = _index(x)
    src, dst, _ = duplicate_edges(ix, 0.9, batch_rows=512)
    assert src.size == 1050 * 1049 // 2                       # the whole clique
    labels = components(1100, src, dst)
    assert labels.tolist() == label.tolist()
    assert int((labels == label[label != np.arange(1100)][0]).sum()) == 1050
    assert int(select_kept(1100, src, dst, "components").sum()) == 51
    first = int(np.flatnonzero(label != np.arange(1100))[0])
    assert int(ix.range_count(ix.vectors[label[first]: label[first] + 1], 0.9)[0]) == 1050   # itself and 1049 others


def test_contamination():
    from contrastors_amd.dedup import contaminated

    rng = np.random.default_rng(2)
    ev = rng.standard_normal((300, 64)).astype(np.float32)
    ev /= np.linalg.norm(ev, axis=1, keepdims=True)
    train = rng.standard_normal((700, 64)).astype(np.float32)
    leaks = np.sort(rng.permutation(700)[:37])
    train[leaks] = ev[rng.integers(0, 300, 37)] + 1e-3 * rng.standard_normal((37, 64)).astype(np.float32) / 8
    train /= np.linalg.norm(train, axis=1, keepdims=True)
    index = _index(ev)
    want = np.zeros(700, bool)
    want[leaks] = True
    S = R.scores64(torch.from_numpy(train).to(torch.bfloat16).to(DEV), index.vectors)
    assert ((S > 0.9).any(1).cpu().numpy() == want).all() and not bool(((S - 0.9).abs() < 1e-3).any())   # a clear-cut plant
    for batch_rows in (1 << 16, 256, 100):
        got = contaminated(train, index, 0.9, batch_rows=batch_rows)
        assert got.dtype == bool and got.tolist() == want.tolist()
    assert contaminated(torch.from_numpy(train), index, 0.9).tolist() == want.tolist()
    assert not contaminated(train, index, 1.5).any()


def test_tool_end_to_end(tmp_path):
    from contrastors_amd.tools import dedup as tool

    sizes = [2, 3, 5]
    x, label = _planted(200, 64, sizes, 3)
    ev = x[[7, 150]] + 0.0                                    # two evaluation rows that ARE training rows
    np.save(tmp_path / "x.npy", 3.0 * x)                      # not normalised on disk: the tool normalises
    np.save(tmp_path / "eval.npy", ev)
    want_dup = label == np.arange(200)
    # 1. embeddings only
    out = tmp_path / "out1"
    assert tool.main(["--embeddings", str(tmp_path / "x.npy"), "--threshold", "0.9", "--output_dir", str(out),
                      "--device", DEV]) == 0
    kept = np.load(out / "kept.npy")
    assert kept.dtype == bool and kept.tolist() == want_dup.tolist()
    dup = json.loads((out / "duplicates.json").read_text())
    assert {int(k): v for k, v in dup.items()} == {int(l): np.flatnonzero(label == l).tolist()
                                                   for l in np.unique(label[label != np.arange(200)])}
    rep = json.loads((out / "report.json").read_text())
    assert rep["n"] == 200 and rep["edges"] == sum(s * (s - 1) // 2 for s in sizes) and rep["kept"] == int(kept.sum())
    assert rep["components"] == 200 - sum(sizes) + 3 and rep["contaminated"] == 0 and rep["rule"] == "components"
    assert rep["threshold"] == 0.9 and rep["against_threshold"] is None
    assert not list(out.glob("shard-*"))
    # 2. a shard directory with precomputed embeddings, greedy rule, decontamination
    data = tmp_path / "data"
    data.mkdir()
    with gzip.open(data / "shard-00000.jsonl.gz", "wt") as f:
        for i in range(120):
            f.write(json.dumps({"document": f"text {i}", "row": i, "metadata": {"source": "a"}}) + "\n")
    with gzip.open(data / "shard-00001.jsonl.gz", "wt") as f:
        for i in range(120, 200):
            f.write(json.dumps({"document": f"text {i}", "row": i, "metadata": {"source": "b"}}) + "\n")
    out = tmp_path / "out2"
    assert tool.main(["--dataset", str(data), "--embeddings", str(tmp_path / "x.npy"), "--threshold", "0.9", "--rule", "greedy",
                      "--against", str(tmp_path / "eval.npy"), "--against_threshold", "0.95", "--output_dir", str(out),
                      "--device", DEV, "--batch_rows", "128"]) == 0
    kept = np.load(out / "kept.npy")
    leak = np.zeros(200, bool)
    leak[[7, 150]] = True
    for l in label[[7, 150]]:                                 # a leaked row's near-copies leak too
        if (label == l).sum() > 1:
            leak[label == l] = True
    assert kept.tolist() == (want_dup & ~leak).tolist()
    rep = json.loads((out / "report.json").read_text())
    assert rep["kept"] == int(kept.sum()) and rep["contaminated"] == int(leak.sum()) and rep["rule"] == "greedy"
    assert rep["against_threshold"] == 0.95
    recs = []
    for p in sorted(out.glob("shard-*.jsonl.gz")):
        with gzip.open(p, "rt") as f:
            recs += [json.loads(line) for line in f]
    assert [r["row"] for r in recs] == np.flatnonzero(kept).tolist()
    assert all(r["metadata"] == {"source": "a" if r["row"] < 120 else "b"} for r in recs)    # the records as they were
    counts = json.loads((out / "counts.json").read_text())["count_per_file"]
    assert sum(counts.values()) == len(recs) == int(kept.sum())
    with gzip.open(out / "offsets.json.gz", "rt") as f:
        offsets = json.load(f)
    assert {k: len(v) for k, v in offsets.items()} == counts
    # 3. a mismatch between records and embeddings is refused
    np.save(tmp_path / "short.npy", x[:150])
    with pytest.raises(SystemExit):
        tool.main(["--dataset", str(data), "--embeddings", str(tmp_path / "short.npy"), "--threshold", "0.9",
                   "--output_dir", str(tmp_path / "out3"), "--device", DEV])
