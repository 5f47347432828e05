"""GPU checks of the cluster-scoped near-duplicate search (contrastors_amd.dedup.clustered_duplicate_edges / edge_recall on the
windowed range search, and the tool's --clusters / --cluster_labels): the edges equal duplicate_edges filtered by equal labels,
in the same order and with the same score bits, for device / numpy / memmap inputs and every chunking; the recall estimate
against the recall computed from the exact edges; python -m contrastors_amd.tools.dedup end to end."""
import functools
import json

import numpy as np
import pytest
import torch

from tests.test_dedup_gpu import _index, _planted

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, D_ = 1300, 64
THR = 0.25        # random unit rows of width 64 score N(0, 1/8): ~2 % of the pairs, planted clusters on top


@functools.lru_cache(maxsize=None)
def _corpus():
    """Rows, an index over them, the exact edges, and labels of 9 unequal clusters that cut through the planted groups."""
    from contrastors_amd.dedup import duplicate_edges

    x, _ = _planted(N, D_, [2 + c % 8 for c in range(40)], 7)
    ix = _index(x)
    src, dst, score = duplicate_edges(ix, THR)
    rng = np.random.default_rng(11)
    labels = rng.choice(np.array([-4, 0, 1, 2, 3, 5, 8, 13, 2 ** 33]), N, p=[.3, .2, .15, .1, .1, .05, .05, .04, .01])
    return dict(x=x, ix=ix, src=src, dst=dst, score=score, labels=labels)


def _want(c, labels):
    keep = labels[c["src"]] == labels[c["dst"]]
    return c["src"][keep], c["dst"][keep], c["score"][keep]


def _equal(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape for g, w in zip(got, want)) and \
        np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and \
        np.array_equal(got[2].view(np.int32), want[2].view(np.int32))


def test_clustered_edges_equal_the_exact_edges_within_labels(tmp_path):
    from contrastors_amd.dedup import clustered_duplicate_edges

    c = _corpus()
    want = _want(c, c["labels"])
    assert 1000 < want[0].size < c["src"].size and want[0].dtype == np.int64 and want[2].dtype == np.float32
    np.save(tmp_path / "x.npy", c["x"])
    sources = {"device": torch.from_numpy(c["x"]).to(DEV), "device_bf16": c["ix"].vectors, "numpy": c["x"],
               "memmap": np.load(tmp_path / "x.npy", mmap_mode="r"), "host_tensor": torch.from_numpy(c["x"])}
    for name, vectors in sources.items():
        for chunk_rows in ((64, 257, N) if name in ("device", "memmap") else (257,)):
            got = clustered_duplicate_edges(vectors, c["labels"], THR, chunk_rows=chunk_rows, device=DEV)
            assert _equal(got, want), (name, chunk_rows)
    got = clustered_duplicate_edges(c["x"], torch.from_numpy(c["labels"]), THR, device=DEV)     # default chunk: one call
    assert _equal(got, want)
    # one label for all rows: the exact result; all rows distinct: no edges
    exact = (c["src"], c["dst"], c["score"])
    for chunk_rows in (64, 1 << 22):
        assert _equal(clustered_duplicate_edges(c["x"], np.full(N, 7), THR, chunk_rows=chunk_rows, device=DEV), exact)
    for chunk_rows in (64, 257, N):
        got = clustered_duplicate_edges(c["x"], np.arange(N)[::-1].copy(), THR, chunk_rows=chunk_rows, device=DEV)
        assert got[0].size == got[1].size == got[2].size == 0 and got[0].dtype == np.int64 and got[2].dtype == np.float32
    # max_edges refuses, exactly at the count
    assert _equal(clustered_duplicate_edges(c["x"], c["labels"], THR, chunk_rows=257, max_edges=want[0].size, device=DEV), want)
    for chunk_rows in (257, N):
        with pytest.raises(ValueError, match=f"max_edges = {want[0].size - 1}"):
            clustered_duplicate_edges(c["x"], c["labels"], THR, chunk_rows=chunk_rows, max_edges=want[0].size - 1, device=DEV)
    with pytest.raises(ValueError, match="labels has shape"):
        clustered_duplicate_edges(c["x"], c["labels"][:-1], THR, device=DEV)


def _true_recall(c, src, dst, rows):
    """From the exact edges: the degree sums over `rows` in the found and in the exact graph."""
    deg = lambda s, d: (np.bincount(s, minlength=N) + np.bincount(d, minlength=N))[rows].sum()
    return int(deg(src, dst)), int(deg(c["src"], c["dst"]))


def test_edge_recall():
    from contrastors_amd.dedup import edge_recall

    c = _corpus()
    src, dst, _ = _want(c, c["labels"])
    for sample in (N, 10 * N):                                # all rows: the recall of the edge list itself
        found, exact, recall = edge_recall(c["ix"], src, dst, THR, sample=sample)
        assert (found, exact) == (2 * src.size, 2 * c["src"].size) == _true_recall(c, src, dst, np.arange(N))
        assert recall == src.size / c["src"].size and 0.1 < recall < 0.9
    assert edge_recall(c["ix"], c["src"], c["dst"], THR, sample=N) == (2 * c["src"].size, 2 * c["src"].size, 1.0)
    assert edge_recall(c["ix"], [], [], 2.0, sample=N) == (0, 0, 1.0)          # nothing above the threshold: recall 1
    # sampled: seeded, repeatable, and exact on its own rows
    a = edge_recall(c["ix"], src, dst, THR, sample=200, seed=3)
    assert a == edge_recall(c["ix"], src, dst, THR, sample=200, seed=3)
    rows = np.sort(np.random.default_rng(3).choice(N, 200, replace=False))
    assert a[:2] == _true_recall(c, src, dst, rows) and a[2] == a[0] / a[1]
    assert a != edge_recall(c["ix"], src, dst, THR, sample=200, seed=4)


def test_tool_with_clusters_and_with_given_labels(tmp_path):
    from contrastors_amd.dedup import duplicate_edges, select_kept
    from contrastors_amd.tools import dedup as tool

    n = 600
    x, _ = _planted(n, 64, [2 + c % 8 for c in range(30)], 5, noise=0.05)      # near-copies that k-means may split
    np.save(tmp_path / "x.npy", 2.0 * x)
    src, dst, _ = duplicate_edges(_index(x), 0.9)
    assert src.size > 100

    def check(out, labels, rows):
        """rows: the rows the recall was measured on, or None."""
        keep = labels[src] == labels[dst]
        kept = np.load(out / "kept.npy")
        assert kept.dtype == bool and kept.tolist() == select_kept(n, src[keep], dst[keep]).tolist()
        rep = json.loads((out / "report.json").read_text())
        assert rep["n"] == n and rep["edges"] == int(keep.sum()) and rep["kept"] == int(kept.sum())
        assert rep["clusters"] == np.unique(labels).size and rep["largest_cluster"] == int(np.bincount(labels - labels.min()).max())
        if rows is None:
            assert rep["edge_recall"] is None and rep["edge_recall_rows"] == 0
        else:
            degree = lambda s, d: int((np.bincount(s, minlength=n) + np.bincount(d, minlength=n))[rows].sum())
            assert rep["edge_recall_rows"] == rows.size and rep["edge_recall"] == degree(src[keep], dst[keep]) / degree(src, dst)
        return rep

    base = ["--embeddings", str(tmp_path / "x.npy"), "--threshold", "0.9", "--device", DEV]
    out = tmp_path / "out1"
    assert tool.main(base + ["--output_dir", str(out), "--clusters", "8", "--recall_sample", "600", "--cluster_iters", "5",
                             "--chunk_rows", "200"]) == 0
    labels = np.load(out / "cluster_labels.npy")
    assert labels.shape == (n,) and labels.dtype == np.int64 and 0 <= labels.min() and labels.max() < 8
    assert 0.5 < check(out, labels, np.arange(n))["edge_recall"] <= 1.0
    # a given partition that cuts through the planted groups; the recall on a seeded sample, and not asked for
    given = np.random.default_rng(1).integers(-2, 3, n) * 1000
    np.save(tmp_path / "labels.npy", given)
    out = tmp_path / "out2"
    assert tool.main(base + ["--output_dir", str(out), "--cluster_labels", str(tmp_path / "labels.npy"), "--recall_sample", "250",
                             "--cluster_seed", "9"]) == 0
    assert not (out / "cluster_labels.npy").exists()
    rep = check(out, given, np.sort(np.random.default_rng(9).choice(n, 250, replace=False)))
    assert 0.05 < rep["edge_recall"] < 0.5
    out = tmp_path / "out4"
    assert tool.main(base + ["--output_dir", str(out), "--cluster_labels", str(tmp_path / "labels.npy")]) == 0
    check(out, given, None)
    # without the new flags the report has none of the new keys
    out = tmp_path / "out3"
    assert tool.main(base + ["--output_dir", str(out)]) == 0
    rep = json.loads((out / "report.json").read_text())
    assert rep["edges"] == src.size and not {"clusters", "largest_cluster", "edge_recall", "edge_recall_rows"} & set(rep)
