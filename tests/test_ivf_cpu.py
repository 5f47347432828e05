"""CPU checks of the IVF index's host side (contrastors_amd.search.IVFFlatIndex): the pair plan and the exclusion remap
against brute force on CPU tensors, the tools' flags, the refusals that must come before anything is launched, and the new
symbols in the header and the binding table."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent

SIZES = [0, 1, 2, 127, 128, 129, 300, 0]


def _list_ptr(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)


def _probes(M, nprobe, nlist, seed):
    """Distinct lists per query, in a random order (as a coarse search returns them: by score, not by list)."""
    g = np.random.default_rng(seed)
    return torch.tensor(np.stack([g.permutation(nlist)[:nprobe] for _ in range(M)]), dtype=torch.int64)


def _check_plan(probes, list_ptr):
    from contrastors_amd.search import ivf_pair_plan

    M, L = probes.shape
    pair_q, min_id, end_id, src = ivf_pair_plan(probes, list_ptr)
    for t in (pair_q, min_id, end_id, src):
        assert t.dtype == torch.int64
    assert pair_q.shape == min_id.shape == end_id.shape == (M * L,) and src.shape == (M, L)
    # brute force: the pairs in (list, query) order -- a stable sort of query-major pairs by list
    pairs = sorted(((int(probes[m, j]), m, j) for m in range(M) for j in range(L)), key=lambda p: p[0])
    assert pair_q.tolist() == [p[1] for p in pairs]
    assert min_id.tolist() == [int(list_ptr[p[0]]) - 1 for p in pairs]
    assert end_id.tolist() == [int(list_ptr[p[0] + 1]) for p in pairs]
    # src inverts the sort: row src[m, j] is the pair (m, probes[m, j]); every pair row is named once
    for r, (l, m, j) in enumerate(pairs):
        assert int(src[m, j]) == r
    assert sorted(src.reshape(-1).tolist()) == list(range(M * L))
    # windows: exactly the list's positions
    for r, (l, m, j) in enumerate(pairs):
        inside = [n for n in range(int(list_ptr[-1])) if int(min_id[r]) < n < int(end_id[r])]
        assert inside == list(range(int(list_ptr[l]), int(list_ptr[l + 1])))
    # rows that share a list are adjacent and in ascending query order
    lists = [p[0] for p in pairs]
    assert lists == sorted(lists)
    return pair_q, min_id, end_id, src


@pytest.mark.parametrize("M", [1, 127, 129])
@pytest.mark.parametrize("nprobe", [1, 2, len(SIZES)])
def test_pair_plan_against_brute_force(M, nprobe):
    _check_plan(_probes(M, nprobe, len(SIZES), 100 * M + nprobe), _list_ptr(SIZES))


def test_pair_plan_lists_probed_by_0_127_129_queries():
    # list 3 by nobody, list 5 by 127 queries, list 6 by 129, the rest share what is left
    M = 129
    probes = torch.zeros(M, 2, dtype=torch.int64)
    probes[:, 0] = 6
    probes[:127, 1] = 5
    probes[127:, 1] = torch.tensor([7, 0])
    pair_q, min_id, end_id, src = _check_plan(probes, _list_ptr(SIZES))
    lp = _list_ptr(SIZES)
    count = {l: int(((min_id == lp[l] - 1) & (end_id == lp[l + 1])).sum()) for l in (5, 6)}
    assert count == {5: 127, 6: 129}
    # lists 0 and 7 are EMPTY: their pair rows have an empty window (end == min_id + 1)
    empty = end_id == min_id + 1
    assert int(empty.sum()) == 2 and sorted(pair_q[empty].tolist()) == [127, 128]


def test_pair_plan_invalid_probe_is_an_empty_window():
    from contrastors_amd.search import ivf_pair_plan

    probes = torch.tensor([[2, -1], [9, 1]], dtype=torch.int64)
    _, min_id, end_id, src = ivf_pair_plan(probes, _list_ptr(SIZES))
    # sorted by list: -1 (nothing), 1 = positions [0, 1), 2 = positions [1, 3), 9 (nothing)
    assert list(zip(min_id.tolist(), end_id.tolist())) == [(0, 0), (-1, 1), (0, 3), (0, 0)]
    assert sorted(src.reshape(-1).tolist()) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        ivf_pair_plan(torch.zeros(4, dtype=torch.int64), _list_ptr(SIZES))


def test_exclusion_remap_through_order():
    from contrastors_amd.search import ivf_pair_exclusions, ivf_pair_plan

    g = np.random.default_rng(3)
    N, M, nprobe = int(sum(SIZES)), 37, 3
    order = torch.tensor(g.permutation(N), dtype=torch.int64)         # order[position] = original id
    inv = torch.empty_like(order)
    inv[order] = torch.arange(N)
    excl = [g.integers(-2, N + 2, int(g.integers(0, 5))).tolist() for _ in range(M)]     # some ids outside [0, N)
    excl[5] = []
    row_ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(e) for e in excl])]), dtype=torch.int64)
    ids = torch.tensor([i for e in excl for i in e], dtype=torch.int64)
    pair_q, _, _, _ = ivf_pair_plan(_probes(M, nprobe, len(SIZES), 9), _list_ptr(SIZES))
    pptr, pids = ivf_pair_exclusions(row_ptr, ids, pair_q, inv, nprobe)
    assert pptr.shape == (M * nprobe + 1,) and int(pptr[0]) == 0 and int(pptr[-1]) == pids.numel() == nprobe * ids.numel()
    for r in range(M * nprobe):
        got = pids[int(pptr[r]): int(pptr[r + 1])].tolist()
        want = [int(inv[i]) if 0 <= i < N else -1 for i in excl[int(pair_q[r])]]
        assert got == want
        for p, i in zip(got, excl[int(pair_q[r])]):
            assert p == -1 or int(order[p]) == i
    # no ids at all
    pptr, pids = ivf_pair_exclusions(torch.zeros(M + 1, dtype=torch.int64), ids[:0], pair_q, inv, nprobe)
    assert pids.numel() == 0 and not bool(pptr.any())


def test_label_order_is_cluster_plans_sort():
    from contrastors_amd.dedup import cluster_plan, label_order

    g = np.random.default_rng(0)
    for labels in (g.integers(0, 7, 1000), g.integers(-5, 1 << 20, 1000), np.zeros(0, np.int64)):
        order = label_order(labels)
        assert order.dtype == np.int64 and np.array_equal(order, np.argsort(labels, kind="stable"))
        assert np.array_equal(order, cluster_plan(labels, 64)[0])


# ---- the tools ---------------------------------------------------------------------------------------------------------
def _tools():
    from contrastors_amd.tools import consistency_filter, mine_negatives

    return {mine_negatives: ["--rule", "topk", "--dataset", "x", "--output_dir", "o"],
            consistency_filter: ["--output_dir", "o"]}


def test_tool_parsers_take_the_ivf_flags():
    from contrastors_amd.tools import _common

    for tool, argv in _tools().items():
        ap = tool.build_parser()
        args = ap.parse_args(argv)
        assert args.ivf_lists == 0 and args.ivf_nprobe is None and args.ivf_centroids is None
        assert args.ivf_sample is None and args.ivf_iters == 25 and args.coarse == "exact"
        assert _common.check_search_arguments(ap, args) == {}                      # the defaults route nowhere new
        args = ap.parse_args(argv + ["--ivf_lists", "64", "--ivf_nprobe", "4", "--ivf_centroids", "c.npy",
                                     "--ivf_sample", "1000", "--ivf_iters", "5"])
        assert _common.check_search_arguments(ap, args) == {"ivf_lists": 64, "ivf_nprobe": 4, "ivf_centroids": "c.npy",
                                                            "ivf_sample": 1000, "ivf_iters": 5}
        assert _common.check_search_arguments(ap, ap.parse_args(argv + ["--ivf_lists", "4"]))["ivf_nprobe"] == 4
        assert _common.check_search_arguments(ap, ap.parse_args(argv + ["--ivf_lists", "64"]))["ivf_nprobe"] == 8
        for bad in (["--ivf_lists", "4", "--coarse", "binary"], ["--ivf_lists", "4", "--ivf_nprobe", "5"],
                    ["--ivf_lists", "1024", "--ivf_nprobe", "257"], ["--ivf_lists", "4", "--ivf_nprobe", "0"],
                    ["--ivf_lists", "-1"], ["--ivf_nprobe", "2"], ["--ivf_centroids", "c.npy"],
                    ["--ivf_lists", "4", "--ivf_iters", "0"]):
            with pytest.raises(SystemExit):
                _common.check_search_arguments(ap, ap.parse_args(argv + bad))
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--coarse", "ivf"])                                 # --coarse keeps its two choices
    assert _common.COARSE == ("exact", "binary")


def test_tools_refuse_ivf_with_binary_before_any_work(tmp_path, capsys):
    from contrastors_amd.tools import consistency_filter, mine_negatives

    (tmp_path / "recs.jsonl").write_text("")
    np.save(tmp_path / "e.npy", np.zeros((2, 64), np.float32))
    e = str(tmp_path / "e.npy")
    for tool, argv in ((mine_negatives, ["--rule", "topk", "--dataset", str(tmp_path / "recs.jsonl")]),
                       (consistency_filter, [])):
        with pytest.raises(SystemExit):
            tool.main(argv + ["--output_dir", str(tmp_path / "o"), "--query_embeddings", e, "--document_embeddings", e,
                              "--ivf_lists", "4", "--coarse", "binary"])
        assert "--ivf_lists goes with --coarse exact" in capsys.readouterr().err
    assert not (tmp_path / "o").exists()


def test_common_search_refuses_ivf_with_binary():
    from contrastors_amd.tools import _common

    with pytest.raises(ValueError, match="ivf_lists"):
        _common.search(np.zeros((4, 64), np.float32), np.zeros((2, 64), np.float32), 1, "cuda", coarse="binary", ivf_lists=2)


# ---- refusals: all of them before anything is allocated or launched (this machine has no GPU) ---------------------------
def test_constructor_and_search_refusals():
    from contrastors_amd.search import MAX_NPROBE, IVFFlatIndex

    for d in (0, 32, 96, 1088):
        with pytest.raises(ValueError, match="d must be"):
            IVFFlatIndex(d, 4)
    for nlist in (0, -3):
        with pytest.raises(ValueError, match="nlist"):
            IVFFlatIndex(64, nlist)
    with pytest.raises(RuntimeError, match="GPU"):
        IVFFlatIndex(64, 4, device="cpu")
    assert MAX_NPROBE == 256
    ix = IVFFlatIndex(64, 1000)
    assert ix.ntotal == 0 and not ix.is_trained
    q = np.zeros((3, 64), np.float32)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k must be"):
            ix.search(q, k, 1)
    for nprobe in (0, 257, 1001):
        with pytest.raises(ValueError, match="nprobe"):
            ix.search(q, 10, nprobe)
    with pytest.raises(ValueError, match="nprobe"):
        IVFFlatIndex(64, 4).search(q, 10, 5)                     # nprobe > nlist
    for call in (lambda: ix.search(q, 10, 8), lambda: ix.add(q), lambda: ix.centroids, lambda: ix.list_sizes):
        with pytest.raises(RuntimeError, match="train"):
            call()
    with pytest.raises(ValueError, match="centroids"):
        ix.train(centroids=np.zeros((999, 64), np.float32))
    with pytest.raises(ValueError, match="either"):
        ix.train()
    with pytest.raises(ValueError, match="either"):
        ix.train(q, centroids=np.zeros((1000, 64), np.float32))


def test_window_symbols_are_declared_and_bound():
    from contrastors_amd import _C

    text = (ROOT / "include" / "contrastors_hip.h").read_text()
    for name in ("cx_search_window_ws_bytes", "cx_search_window_topk", "cx_topk_merge_lists"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _C.EXPORTED_SYMBOLS
    assert len(_C._SIGS["cx_search_window_topk"][1]) == 17 and len(_C._SIGS["cx_topk_merge_lists"][1]) == 12
    lib = _C.lib()
    for name in ("cx_search_window_ws_bytes", "cx_search_window_topk", "cx_topk_merge_lists"):
        assert hasattr(lib, name)
    assert lib.cx_abi_version() == 10
    # the workspace: one (score, id) list of k entries and a count per row
    assert lib.cx_search_window_ws_bytes(1000, 100) == 1000 * (100 * 8 + 4) + 16
    assert lib.cx_search_window_ws_bytes(0, 100) == 0
