"""Host logic of the cluster-scoped near-duplicate search: contrastors_amd.dedup.cluster_plan against brute force, the band /
workspace description of the windowed range search (contrastors_amd.search.window_band, cx_range_window_ws_bytes) against a
brute-force tile enumeration, the new flags of contrastors_amd.tools.dedup, and the exported symbols."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from contrastors_amd.tools import dedup as tool

ROOT = Path(__file__).resolve().parent.parent
RUNS = [1, 2, 127, 128, 129, 300]


def _labels(runs, names, seed):
    """Rows of len(runs) clusters (cluster c has runs[c] rows and label names[c]) in a seeded random order."""
    lab = np.repeat(np.asarray(names, dtype=np.int64), runs)
    return lab[np.random.default_rng(seed).permutation(lab.size)]


def _check_plan(labels, chunk_rows):
    from contrastors_amd.dedup import cluster_plan

    order, end, chunks = cluster_plan(labels, chunk_rows)
    n = len(labels)
    assert order.dtype == np.int64 and end.dtype == np.int64 and sorted(order.tolist()) == list(range(n))
    sl = [int(labels[i]) for i in order]
    assert sl == sorted(sl)                                                     # sorted by label ...
    for i in range(n):                                                          # ... brute force: the run of every position
        j = i
        while j < n and sl[j] == sl[i]:
            j += 1
        assert end[i] == j
        if i and sl[i - 1] == sl[i]:
            assert order[i - 1] < order[i]                                      # stable: ascending row ids within a run
    # the chunks: whole runs, in order, covering [0, n); at most chunk_rows rows unless a single longer run; greedy (a chunk
    # could not have taken the next run as well)
    at = 0
    for k, (b0, b1) in enumerate(chunks):
        assert b0 == at and b1 > b0
        assert b0 == 0 or sl[b0 - 1] != sl[b0]
        assert b1 == n or sl[b1 - 1] != sl[b1]
        assert b1 - b0 <= chunk_rows or end[b0] == b1
        if b1 < n:
            assert end[b1] - b0 > chunk_rows
        at = b1
    assert at == n
    return order, end, chunks


def test_cluster_plan_against_brute_force():
    from contrastors_amd.dedup import cluster_plan

    dense = _labels(RUNS, range(len(RUNS)), 0)
    sparse = _labels(RUNS, [-(2 ** 40), -7, -1, 0, 5, 2 ** 40], 1)               # negative, not dense
    for lab in (dense, sparse, sparse.astype(np.int32) // 2 ** 20, _labels([1] * 50, range(50), 2), np.zeros(40, np.int64)):
        for chunk_rows in (1, 2, 128, 129, 200, 430, len(lab), 10 ** 9):
            _check_plan(lab, chunk_rows)
    # a run longer than chunk_rows is a chunk of its own; chunk_rows = 1 gives one chunk per run
    assert [b1 - b0 for b0, b1 in _check_plan(dense, 200)[2]] == [1 + 2 + 127, 128, 129, 300]
    assert [b1 - b0 for b0, b1 in _check_plan(dense, 1)[2]] == RUNS
    assert _check_plan(dense, len(dense))[2] == [(0, len(dense))]
    o, e, c = cluster_plan(np.zeros(0, np.int64), 8)
    assert o.size == 0 and e.size == 0 and c == []
    with pytest.raises(ValueError, match="integers"):
        cluster_plan(np.zeros(4, np.float32), 8)


def _brute_band(min_id, end_id, M, N):
    """Per 128-row query tile, the corpus tiles between the first and the last one that holds an id of any row's window."""
    out = []
    for m0 in range(0, M, 128):
        tiles = set()
        for m in range(m0, min(M, m0 + 128)):
            lo = -1 if min_id is None else int(min_id[m])
            hi = N if end_id is None else int(end_id[m])
            ids = range(max(lo + 1, 0), min(hi, N))
            if len(ids):
                tiles.update((ids[0] // 128, ids[-1] // 128))
        out.append(max(tiles) - min(tiles) + 1 if tiles else 0)
    return out


def test_window_band_and_workspace_against_tile_enumeration():
    from contrastors_amd import _C
    from contrastors_amd.dedup import cluster_plan
    from contrastors_amd.search import FlatIPIndex, _window_ws_bytes, window_band

    h = _C.lib()
    rng = np.random.default_rng(0)
    cases = []
    for M, N in ((1, 1), (127, 300), (129, 129), (300, 1000), (1000, 1000)):
        edges = np.array([-5, -1, 0, 1, 126, 127, 128, 129, N - 2, N - 1, N, N + 500])
        cases.append((M, N, torch.from_numpy(rng.choice(edges, M)), torch.from_numpy(rng.choice(edges, M))))
        cases.append((M, N, None, torch.from_numpy(rng.choice(edges, M))))
        cases.append((M, N, torch.from_numpy(rng.choice(edges, M)), None))
        cases.append((M, N, torch.full((M,), 200), torch.full((M,), 100)))        # only empty windows
    # the sorted self-join: own position and the run's end
    _, end, _ = cluster_plan(np.repeat(np.arange(8), [1, 2, 127, 128, 129, 300, 1, 255]), 1 << 20)
    cases.append((end.size, end.size, torch.arange(end.size), torch.from_numpy(end)))
    for M, N, mid, end in cases:
        band = window_band(mid, end, M, N)
        assert band.dtype == torch.int64 and band.tolist() == _brute_band(mid, end, M, N)
        total = int(band.sum())
        assert total <= ((M + 127) // 128) * ((N + 127) // 128)
        # the workspace: 4 flag bytes per band tile on top of the partial counts, nothing proportional to tiles_m x tiles_n
        assert h.cx_range_window_ws_bytes(M, N, 0, 1) == (M * 8 + 15) // 16 * 16 + 16         # one split: 2 ints per row
        assert h.cx_range_window_ws_bytes(M, N, total, 1) - h.cx_range_window_ws_bytes(M, N, 0, 1) == 4 * total
        for nsplit in (0, 3, 64):                                                # at most 64 splits of 2 ints per row
            assert M * 8 + 4 * total <= h.cx_range_window_ws_bytes(M, N, total, nsplit) <= M * 64 * 8 + 4 * total + 32
    assert h.cx_range_window_ws_bytes(0, 5, 3, 0) == 0 and h.cx_range_window_ws_bytes(5, 0, 3, 0) == 0
    # ten million sorted rows in clusters of about 1000: megabytes, where the dense flag array is 24 GB
    n = 10_000_000
    band_tiles = (n // 128) * 9
    assert h.cx_range_window_ws_bytes(n, n, band_tiles, 0) < 100 << 20 < 20 << 30 < h.cx_range_ws_bytes(n, n, 0)
    # the query batch follows the windowed workspace size
    ix = FlatIPIndex(64, workspace_bytes=1 << 14)
    ix.ntotal = 1000                                                             # (sizes only: nothing is launched)
    ptr = np.concatenate([[0], np.cumsum(window_band(torch.arange(1000), None, 1000, 1000).numpy())])
    assert ix.range_window_batch_rows(1000, ptr) == 128                          # halved 1000 -> 384 -> 128
    assert max(_window_ws_bytes(1000, 1000, ptr, 128, 0)) <= 1 << 14 < max(_window_ws_bytes(1000, 1000, ptr, 384, 0))
    ix.workspace_bytes = 1 << 30
    assert ix.range_window_batch_rows(1000, ptr) == 1000


def test_new_flags_defaults_and_refusals(tmp_path):
    ap = tool.build_parser()
    a = ap.parse_args(["--output_dir", "o", "--threshold", "0.9"])
    assert a.clusters is None and a.cluster_labels is None and a.cluster_sample is None and a.recall_sample is None
    assert a.cluster_iters == 25 and a.cluster_seed == 0 and a.chunk_rows == 1 << 22
    a = ap.parse_args(["--output_dir", "o", "--threshold", "0.9", "--clusters", "8", "--cluster_sample", "100",
                       "--cluster_iters", "3", "--cluster_seed", "5", "--chunk_rows", "64", "--recall_sample", "10"])
    assert (a.clusters, a.cluster_sample, a.cluster_iters, a.cluster_seed, a.chunk_rows, a.recall_sample) == (8, 100, 3, 5, 64, 10)
    np.save(tmp_path / "x.npy", np.random.default_rng(0).standard_normal((20, 64)).astype(np.float32))
    np.save(tmp_path / "short.npy", np.zeros(19, np.int64))
    np.save(tmp_path / "float.npy", np.zeros(20, np.float32))
    np.save(tmp_path / "ok.npy", np.zeros(20, np.int64))
    base = ["--embeddings", str(tmp_path / "x.npy"), "--threshold", "0.9", "--output_dir", str(tmp_path / "out")]
    for extra in (["--clusters", "4", "--cluster_labels", str(tmp_path / "ok.npy")],      # mutually exclusive
                  ["--clusters", "0"], ["--clusters", "-3"],                               # K < 1
                  ["--clusters", "21"],                                                    # more clusters than rows
                  ["--cluster_labels", str(tmp_path / "short.npy")],                       # the wrong length
                  ["--cluster_labels", str(tmp_path / "float.npy")],                       # not integers
                  ["--cluster_labels", str(tmp_path / "missing.npy")],
                  ["--clusters", "4", "--chunk_rows", "0"], ["--clusters", "4", "--cluster_iters", "0"],
                  ["--clusters", "4", "--cluster_sample", "0"], ["--clusters", "4", "--recall_sample", "0"],
                  ["--recall_sample", "10"]):                                              # goes with a partition
        with pytest.raises(SystemExit):
            tool.main(base + extra)
    assert not (tmp_path / "out").exists()


def test_window_symbols_are_declared_and_exported():
    from contrastors_amd import _C

    text = (ROOT / "include" / "contrastors_hip.h").read_text()
    lib = _C.lib()
    for name in ("cx_range_window_ws_bytes", "cx_range_window_count", "cx_range_window_emit"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _C.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.cx_abi_version() == 10
