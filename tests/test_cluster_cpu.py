"""Host side of contrastors_amd.cluster: the V-measure against scikit-learn, the update plan on CPU tensors at the piece
edges, and the command line of contrastors_amd.tools.cluster with the refusals it reaches without a GPU."""
import math

import numpy as np
import pytest
import torch

from contrastors_amd.cluster import PIECE_ROWS, KMeans, _update_plan, evaluate_clustering, v_measure
from contrastors_amd.tools import cluster as tool


def _sk(t, p):
    from sklearn.metrics import homogeneity_completeness_v_measure

    return homogeneity_completeness_v_measure(t, p)


def test_v_measure_equals_scikit_learn():
    rng = np.random.default_rng(0)
    cases = []
    for n, kt, kp in [(50, 3, 4), (1000, 10, 10), (1000, 2, 37), (5000, 20, 5), (7, 7, 2)]:
        cases.append((rng.integers(0, kt, n), rng.integers(0, kp, n)))
    y = rng.integers(0, 5, 400)
    cases += [
        (y, np.zeros(400, dtype=np.int64)),                  # everything in one cluster: complete, not homogeneous
        (np.zeros(400, dtype=np.int64), y),                  # a single class: homogeneous in any clustering
        (np.zeros(400, dtype=np.int64), np.zeros(400, dtype=np.int64)),
        (y, np.arange(400)),                                 # all singletons: homogeneous, far from complete
        (np.arange(400), np.arange(400)[::-1].copy()),
        (y, (y + 3) % 5),                                    # the same partition under other names
        (y * 10 - 7, np.array(["a", "b", "c", "d", "e"])[y]),   # labels need not be 0..k-1, nor numbers
    ]
    for t, p in cases:
        got, want = v_measure(t, p), _sk(t, p)
        assert all(isinstance(g, float) for g in got)
        assert np.allclose(got, want, rtol=0, atol=1e-12), (got, want)
    assert v_measure(y, np.zeros(400, dtype=np.int64)) == pytest.approx((0.0, 1.0, 0.0), abs=1e-15)
    assert v_measure(y, (y + 3) % 5) == pytest.approx((1.0, 1.0, 1.0), abs=1e-15)
    hom, com, v = v_measure(y, np.arange(400))
    assert hom == pytest.approx(1.0, abs=1e-15) and 0.0 < com < 0.5 and v == pytest.approx(2 * com / (1 + com), abs=1e-15)
    assert v_measure(torch.tensor([0, 0, 1]), [5, 5, 9]) == pytest.approx((1.0, 1.0, 1.0), abs=1e-15)
    with pytest.raises(ValueError, match="3 true labels for 2"):
        v_measure([0, 1, 2], [0, 1])


def _check_plan(labels, k, P):
    N = labels.numel()
    order, start, end, cluster, ptr, n_pieces = _update_plan(labels, k, P)
    for t in (order, start, end, cluster, ptr, n_pieces):
        assert t.dtype == torch.int32 and t.device == labels.device
    bound = math.ceil(N / P) + k
    assert start.numel() == end.numel() == cluster.numel() == bound and ptr.numel() == k + 1 and n_pieces.numel() == 1
    np_ = int(n_pieces)
    assert np_ == int(ptr[k]) <= bound and int(ptr[0]) == 0
    counts = torch.bincount(labels.long(), minlength=k)
    assert sorted(order.tolist()) == list(range(N))
    pos = 0
    for c in range(k):
        p0, p1 = int(ptr[c]), int(ptr[c + 1])
        assert p1 - p0 == math.ceil(int(counts[c]) / P)
        for p in range(p0, p1):                              # the pieces tile the run exactly, in order
            assert int(start[p]) == pos and int(cluster[p]) == c
            assert 0 < int(end[p]) - pos <= P and (int(end[p]) - pos == P or p == p1 - 1)
            pos = int(end[p])
        run = order[pos - int(counts[c]): pos].tolist()
        assert run == sorted(run) and all(int(labels[i]) == c for i in run)   # ascending ids of that cluster
    assert pos == N
    assert start[np_:].tolist() == [0] * (bound - np_) == end[np_:].tolist() and cluster[np_:].tolist() == [-1] * (bound - np_)
    return counts


def test_update_plan_at_the_piece_edges():
    assert PIECE_ROWS == 256
    sizes = [0, 1, 255, 256, 257, 513]
    labels = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    labels = labels[torch.randperm(labels.numel(), generator=torch.Generator().manual_seed(0))]
    counts = _check_plan(labels, len(sizes), PIECE_ROWS)
    assert counts.tolist() == sizes
    assert int(_update_plan(labels, len(sizes))[5]) == 0 + 1 + 1 + 1 + 2 + 3
    _check_plan(labels, len(sizes) + 3, PIECE_ROWS)                              # trailing empty clusters
    _check_plan(labels, len(sizes), 7)                                           # another piece length
    _check_plan(torch.tensor([4, 1, 4]), 9, PIECE_ROWS)                          # K > N
    _check_plan(torch.full((3000,), 2), 5, PIECE_ROWS)                           # all points in one cluster
    assert int(_update_plan(torch.full((3000,), 2), 5)[5]) == 12
    _check_plan(torch.zeros(0, dtype=torch.int64), 3, PIECE_ROWS)                # no points
    _check_plan(torch.arange(600, dtype=torch.int32) % 3, 3, PIECE_ROWS)         # int32 labels, as the kernel writes them
    with pytest.raises(ValueError):
        _update_plan(torch.zeros(2, 2), 3)
    with pytest.raises(ValueError):
        _update_plan(torch.zeros(4), 0)


def test_kmeans_refusals_without_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU path"):
        KMeans(4, 64, device="cpu")
    with pytest.raises(ValueError, match="multiple of 64"):
        KMeans(4, 96)
    with pytest.raises(ValueError, match="k must be"):
        KMeans(0, 64)
    with pytest.raises(ValueError, match="for 3 labels"):
        evaluate_clustering(np.zeros((4, 64), dtype=np.float32), [0, 1, 0])


def test_cli_parser():
    ap = tool.build_parser()
    a = ap.parse_args(["--embeddings", "x.npy", "--k", "8", "--out", "l.npy"])
    assert (a.embeddings, a.k, a.out) == ("x.npy", 8, "l.npy")
    assert a.centroids_out is None and not a.spherical and a.sample is None and a.n_init == 1 and a.seed == 0
    assert a.labels is None and a.device == "cuda"
    a = ap.parse_args(["--embeddings", "x.npy", "--k", "4096", "--out", "l.npy", "--centroids_out", "c.npy", "--spherical",
                       "--sample", "100000", "--n_init", "3", "--seed", "7", "--labels", "y.npy", "--device", "cuda:1"])
    assert (a.k, a.centroids_out, a.spherical, a.sample, a.n_init, a.seed, a.labels, a.device) == \
        (4096, "c.npy", True, 100000, 3, 7, "y.npy", "cuda:1")
    for bad in (["--k", "8", "--out", "l.npy"], ["--embeddings", "x.npy", "--out", "l.npy"],
                ["--embeddings", "x.npy", "--k", "8"], ["--embeddings", "x.npy", "--k", "eight", "--out", "l.npy"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_tool_refusals_without_a_gpu(tmp_path):
    x = np.random.default_rng(0).standard_normal((10, 64)).astype(np.float32)
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "odd.npy", x[:, :48])
    np.save(tmp_path / "flat.npy", x[0])
    np.save(tmp_path / "y.npy", np.arange(9))
    out = tmp_path / "labels.npy"
    base = ["--out", str(out), "--embeddings", str(tmp_path / "x.npy")]
    for bad in (["--k", "0"], ["--k", "11"], ["--k", "2", "--n_init", "0"], ["--k", "2", "--sample", "0"],
                ["--k", "4", "--sample", "3"], ["--k", "2", "--labels", str(tmp_path / "y.npy")],
                ["--k", "2", "--labels", str(tmp_path / "missing.npy")]):
        with pytest.raises(SystemExit):
            tool.main(base + bad)
    with pytest.raises(SystemExit):
        tool.main(["--out", str(out), "--k", "2", "--embeddings", str(tmp_path / "missing.npy")])
    with pytest.raises(SystemExit):
        tool.main(["--out", str(out), "--k", "2", "--embeddings", str(tmp_path / "flat.npy")])
    # KMeans' own refusals, reached through the tool: there is no CPU path, and the width must suit the kernel
    with pytest.raises(RuntimeError, match="no CPU path"):
        tool.main(base + ["--k", "2", "--device", "cpu"])
    with pytest.raises(ValueError, match="multiple of 64"):
        tool.main(["--out", str(out), "--k", "2", "--embeddings", str(tmp_path / "odd.npy"), "--device", "cpu"])
    assert not out.exists()                                                      # nothing was written on the way
