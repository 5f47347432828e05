"""Host logic of near-duplicate removal (contrastors_amd.dedup: components, select_kept) on hand-made edge lists, the command
line of contrastors_amd.tools.dedup, and the refusals the tool reaches without a GPU."""
import numpy as np
import pytest

from contrastors_amd.dedup import components, select_kept
from contrastors_amd.tools import dedup as tool

# rows 0-3: a chain 0~1~2~3; 4-8: a star around 6; 9-11 and 12-14: two cliques; 15-17 isolated; 18~19 given backwards
CHAIN = [(0, 1), (1, 2), (2, 3)]
STAR = [(6, 4), (6, 5), (6, 7), (6, 8)]
CLIQUES = [(9, 10), (9, 11), (10, 11), (12, 13), (12, 14), (13, 14)]
BACK = [(19, 18)]
N = 20
WANT_LABELS = [0, 0, 0, 0, 4, 4, 4, 4, 4, 9, 9, 9, 12, 12, 12, 15, 16, 17, 18, 18]


def _split(edges):
    return [a for a, _ in edges], [b for _, b in edges]


def test_components_on_hand_made_graphs():
    edges = CHAIN + STAR + CLIQUES + BACK
    rng = np.random.default_rng(0)
    for trial in range(4):    # any order of the edges, either orientation: the same labels
        perm = rng.permutation(len(edges))
        e = [edges[i] if (trial + i) % 2 else edges[i][::-1] for i in perm]
        labels = components(N, *_split(e))
        assert labels.dtype == np.int64 and labels.tolist() == WANT_LABELS
    assert components(5, [], []).tolist() == [0, 1, 2, 3, 4]
    assert components(0, [], []).tolist() == []
    assert components(3, [1, 1], [1, 1]).tolist() == [0, 1, 2]          # self-loops join nothing
    # a long path given from the far end: the label has to travel the whole way
    n = 300
    assert components(n, list(range(n - 1, 0, -1)), list(range(n - 2, -1, -1))).tolist() == [0] * n
    # two long paths joined at their far ends
    src = list(range(0, 98, 2)) + list(range(1, 99, 2)) + [98]
    dst = list(range(2, 100, 2)) + list(range(3, 101, 2)) + [99]
    assert components(100, src, dst).tolist() == [0] * 100


def test_select_kept_rules_differ_on_the_chain_as_specified():
    edges = CHAIN + STAR + CLIQUES + BACK
    comp = select_kept(N, *_split(edges), rule="components")
    assert np.flatnonzero(comp).tolist() == [0, 4, 9, 12, 15, 16, 17, 18]        # the lowest id of every component
    greedy = select_kept(N, *_split(edges[::-1]), rule="greedy")
    # chain 0~1~2~3: 1 falls to 0, 2 survives (its only lower neighbour was dropped), 3 falls to 2.
    # star around 6: 4 and 5 are kept (not neighbours of each other), 6 falls to 4, so 7 and 8 are kept.
    assert np.flatnonzero(greedy).tolist() == [0, 2, 4, 5, 7, 8, 9, 12, 15, 16, 17, 18]
    # the case of the definition: a~b~c with a !~ c
    assert select_kept(3, [0, 1], [1, 2], rule="components").tolist() == [True, False, False]
    assert select_kept(3, [0, 1], [1, 2], rule="greedy").tolist() == [True, False, True]
    # on cliques the two rules agree
    assert select_kept(6, *_split([(0, 1), (0, 2), (1, 2), (3, 4)]), rule="greedy").tolist() == \
        select_kept(6, *_split([(0, 1), (0, 2), (1, 2), (3, 4)]), rule="components").tolist()
    assert select_kept(4, [], [], rule="greedy").tolist() == [True] * 4


def test_edge_list_refusals():
    with pytest.raises(ValueError, match="rule"):
        select_kept(3, [0], [1], rule="nearest")
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        components(3, [0], [3])
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        select_kept(3, [-1], [2])
    with pytest.raises(ValueError):
        components(3, [0, 1], [1])


def test_cli_parser():
    ap = tool.build_parser()
    a = ap.parse_args(["--embeddings", "x.npy", "--threshold", "0.9", "--output_dir", "out"])
    assert a.rule == "components" and a.threshold == 0.9 and a.key == "document" and a.device == "cuda"
    assert a.against is None and a.against_threshold is None and not a.no_normalize and a.max_edges == 1 << 27
    a = ap.parse_args(["--dataset", "dir", "--key", "text", "--model", "ckpt", "--tokenizer", "tok", "--threshold", "0.8",
                       "--rule", "greedy", "--against", "eval.npy", "--against_threshold", "0.7", "--output_dir", "o",
                       "--max_edges", "1000", "--device", "cuda:1", "--no_normalize"])
    assert (a.dataset, a.key, a.model, a.tokenizer, a.rule) == ("dir", "text", "ckpt", "tok", "greedy")
    assert (a.against, a.against_threshold, a.max_edges, a.device, a.no_normalize) == ("eval.npy", 0.7, 1000, "cuda:1", True)
    for bad in (["--threshold", "0.9", "--output_dir", "o", "--embeddings", "x.npy", "--rule", "nearest"],
                ["--output_dir", "o", "--embeddings", "x.npy"],                     # no threshold
                ["--threshold", "0.9", "--embeddings", "x.npy"]):                   # no output_dir
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_tool_refusals_without_a_gpu(tmp_path):
    x = np.random.default_rng(0).standard_normal((10, 64)).astype(np.float32)
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "odd.npy", x[:, :48])
    base = ["--threshold", "0.9", "--output_dir", str(tmp_path / "out")]
    with pytest.raises(SystemExit):                                   # nothing to embed
        tool.main(base)
    with pytest.raises(SystemExit):                                   # records but neither .npy nor an encoder
        tool.main(base + ["--dataset", str(tmp_path)])
    with pytest.raises(SystemExit):
        tool.main(base + ["--embeddings", str(tmp_path / "missing.npy")])
    with pytest.raises(SystemExit):
        tool.main(base + ["--embeddings", str(tmp_path / "x.npy"), "--against_threshold", "0.5"])
    with pytest.raises(SystemExit):
        tool.main(base + ["--embeddings", str(tmp_path / "x.npy"), "--max_edges", "0"])
    # the index's own refusals, reached through the tool: there is no CPU path, and the width must suit the kernel
    with pytest.raises(RuntimeError, match="no CPU path"):
        tool.main(base + ["--embeddings", str(tmp_path / "x.npy"), "--device", "cpu"])
    with pytest.raises(ValueError, match="multiple of 64"):
        tool.main(base + ["--embeddings", str(tmp_path / "odd.npy"), "--device", "cpu"])
    assert not (tmp_path / "out").exists()                            # nothing was written on the way
