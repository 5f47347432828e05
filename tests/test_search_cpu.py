"""CPU checks of the top-k search feature: its C-ABI entries (header, ctypes lists, ABI version), the curation tools'
selection rules against tests/golden/search_curation.json given exact scores, the shard layout read back by the streaming
loader, and the tools' argument errors.  No GPU call is made."""
import gzip
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "contrastors_hip.h"
FX = json.loads((ROOT / "tests" / "golden" / "search_curation.json").read_text())
SEARCH_SYMBOLS = {"cx_search_topk", "cx_search_ws_bytes"}


@pytest.fixture(scope="module")
def built():
    from contrastors_amd import build

    return build.build()


def test_search_symbols_in_header_ctypes_and_product_library(built):
    from contrastors_amd import _C

    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", HDR.read_text()))
    assert SEARCH_SYMBOLS <= declared
    assert declared == set(_C.EXPORTED_SYMBOLS)
    assert not SEARCH_SYMBOLS & set(_C.DEV_EXPORTED_SYMBOLS)
    lib = _C.lib()
    assert lib.cx_abi_version() == 10          # additive: no existing signature changed
    for name in SEARCH_SYMBOLS:
        assert hasattr(lib, name)
    # workspace: (M, splits, k) candidate lists of 8 bytes + one count per (row, split) + 16
    assert lib.cx_search_ws_bytes(128, 128, 10, 1) == 128 * (10 * 8 + 4) + 16
    assert lib.cx_search_ws_bytes(128, 128 * 100, 10, 7) == 128 * 7 * (10 * 8 + 4) + 16
    assert lib.cx_search_ws_bytes(128, 128 * 3, 10, 7) == 128 * 3 * (10 * 8 + 4) + 16   # at most one split per tile
    assert lib.cx_search_ws_bytes(0, 10, 10, 0) == 0
    # corpus bound: the last tile's int column indices stay below 2^31 (checked before any pointer is touched)
    args = (64, 64, 64, 1, None, None, None, 0, None, None, None, None)
    assert lib.cx_search_topk(None, None, 1, 2 ** 31 - 128, *args) == -1       # CX_ERR_SHAPE
    assert lib.cx_search_topk(None, None, 1, 2 ** 31 - 129, *args) == -3       # in bounds: the null pointers are refused


def test_search_prototypes_match_ctypes_arity_under_gcc(tmp_path, built):
    """The new entry points declare no struct; check that the header compiles as C with them and that the ctypes
    argument lists have the declared arity and integer widths."""
    from contrastors_amd import _C

    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include "contrastors_hip.h"\n'
                   "int main(void){long (*a)(int, long, int, int) = cx_search_ws_bytes;"
                   " int (*b)(const uint16_t*, const uint16_t*, int, long, int, long, long, int, const int64_t*,"
                   " const int64_t*, const float*, int, void*, float*, int64_t*, void*) = cx_search_topk;"
                   " printf(\"%d\\n\", a != 0 && b != 0); return 0;}\n")
    # compile only: a prototype that disagrees with the pointer types above is an error under -Werror
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])
    import ctypes as C

    res, args = _C._SIGS["cx_search_topk"]
    assert res is C.c_int and len(args) == 16
    assert [a for a in args[2:8]] == [C.c_int, C.c_long, C.c_int, C.c_long, C.c_long, C.c_int]
    res, args = _C._SIGS["cx_search_ws_bytes"]
    assert res is C.c_long and args == [C.c_int, C.c_long, C.c_int, C.c_int]


def exact_topk(q, d, k, exclude=None, below=None):
    """What the kernel returns for exact scores: descending, ties to the lower id, (-inf, -1) padding."""
    s = np.asarray(q, np.float64) @ np.asarray(d, np.float64).T
    out = np.full((len(q), k), -1, np.int64)
    for r in range(len(q)):
        ok = np.ones(s.shape[1], bool)
        if exclude is not None:
            ok[list(exclude[r])] = False
        if below is not None:
            ok &= s[r] < below[r]
        idx = np.nonzero(ok)[0]
        idx = idx[np.argsort(-s[r, idx], kind="stable")][:k]
        out[r, : len(idx)] = idx
    return out


def test_consistency_rule_matches_the_reference_filter_points():
    from contrastors_amd.tools.consistency_filter import keep_ids

    fx = FX["consistency"]
    ids = fx["ids"]
    pos = sorted(range(len(ids)), key=lambda i: ids[i])
    q, d = np.asarray(fx["q"])[pos], np.asarray(fx["d"])[pos]
    assert keep_ids(ids, exact_topk(q, d, 2)) == fx["kept"]


def test_topk_rule_matches_the_restatement():
    from contrastors_amd.tools.mine_negatives import select_topk

    fx = FX["topk"]
    records = [dict(r) for r in fx["records"]]
    idx = exact_topk(fx["q"], fx["d"], fx["k"])
    out = select_topk(records, fx["documents"], idx, fx["k"], "question", "positive_ctxs", "hard_negative_ctxs",
                      np.random.RandomState(fx["seed"]))
    assert out == fx["expected"]


def _write_beir(root, fx):
    root.mkdir(parents=True, exist_ok=True)
    (root / "qrels").mkdir(exist_ok=True)
    (root / "corpus.jsonl").write_text("".join(json.dumps(c) + "\n" for c in fx["corpus"]))
    (root / "queries.jsonl").write_text("".join(json.dumps(c) + "\n" for c in fx["queries"]))
    (root / "qrels" / "train.tsv").write_text("query-id\tcorpus-id\tscore\n" +
                                              "".join(f"{a}\t{b}\t{c}\n" for a, b, c in fx["qrels"]))


def test_margin_rule_matches_the_restatement(tmp_path):
    import random

    from contrastors_amd.tools.mine_negatives import load_beir, margin_pairs, select_margin

    fx = FX["margin"]
    _write_beir(tmp_path / "beir", fx)
    corpus, queries, qrels, qid2index, docid2index, documents = load_beir(tmp_path / "beir")
    assert list(queries) == [f"q{i}" for i in range(8)]                   # qrels order; queries without qrels dropped
    pairs, rows, excl, below = margin_pairs(qrels, qid2index, docid2index, fx["q"], fx["d"], fx["margin"])
    idx = exact_topk(np.asarray(fx["q"])[rows], fx["d"], fx["max_negatives"], excl, below)
    mined, dropped = select_margin(pairs, idx, corpus, queries, documents, fx["k"], "query", "pos", "neg")
    random.Random(fx["seed"]).shuffle(mined)
    assert dropped == fx["dropped"] and mined == fx["expected"]


def test_mined_shards_read_back_as_triplets(tmp_path):
    from contrastors_amd.data import StreamingShardDataset, build_index
    from contrastors_amd.tools._common import triplet_metadata, write_shards

    fx = FX["margin"]
    rows = [dict(r) for r in fx["expected"]]
    out = tmp_path / "mined"
    paths = write_shards(rows, out, triplet_metadata("query", "pos", "neg"), shard_size=8)
    assert [p.name for p in paths] == ["shard-00000.jsonl.gz", "shard-00001.jsonl.gz"]
    with gzip.open(paths[0], "rt") as f:
        first = json.loads(f.readline())
    assert first["metadata"] == {"objective": {"self": [], "paired": [], "triplet": [["query", "pos", "neg"]]}}
    build_index([str(p) for p in paths])
    spec = tmp_path / "spec.yaml"
    spec.write_text(f"datasets:\n  - name: mined\n    bucket: {out}/shard-{{00000..00001}}.jsonl.gz\n"
                    "    objective:\n      type: triplet\n      columns: [query, pos, neg]\n")
    from oracle import data_fixture as df

    ds = StreamingShardDataset(str(spec), 4, df.ToyTokenizer(), seed=0, verbose=False, num_negatives=3, run_name="m")
    got = ds._read_records(str(paths[0]))
    assert len(got) == 4
    for g, r in zip(got, rows[:4]):
        assert g["query"] == r["query"] and g["document"] == [r["pos"]] + r["neg"][:3]


def _run(tool, *args):
    return subprocess.run([sys.executable, "-m", f"contrastors_amd.tools.{tool}", *args], cwd=ROOT,
                          capture_output=True, text=True)


def test_tool_argument_errors(tmp_path):
    r = _run("mine_negatives", "--output_dir", str(tmp_path))
    assert r.returncode == 2 and "--rule" in r.stderr
    r = _run("mine_negatives", "--rule", "topk", "--dataset", str(tmp_path / "missing"), "--output_dir", str(tmp_path),
             "--query_embeddings", "q.npy", "--document_embeddings", "d.npy")
    assert r.returncode == 2 and "does not exist" in r.stderr
    (tmp_path / "x.jsonl").write_text("")
    r = _run("mine_negatives", "--rule", "topk", "--dataset", str(tmp_path / "x.jsonl"), "--output_dir", str(tmp_path),
             "--query_embeddings", "q.npy")
    assert r.returncode == 2 and "both" in r.stderr
    r = _run("mine_negatives", "--rule", "margin", "--dataset", str(tmp_path), "--output_dir", str(tmp_path),
             "--max_negatives", "2000", "--query_embeddings", "q.npy", "--document_embeddings", "d.npy")
    assert r.returncode == 2 and "1024" in r.stderr
    r = _run("mine_negatives", "--rule", "topk", "--dataset", str(tmp_path / "x.jsonl"), "--output_dir", str(tmp_path))
    assert r.returncode == 2 and "--model" in r.stderr
    r = _run("consistency_filter", "--output_dir", str(tmp_path), "--k", "0")
    assert r.returncode == 2 and "--k" in r.stderr
    r = _run("consistency_filter", "--output_dir", str(tmp_path))
    assert r.returncode == 2 and "--dataset" in r.stderr
    r = _run("mine_negatives", "--rule", "topk", "--dataset", str(tmp_path / "x.jsonl"), "--output_dir", str(tmp_path),
             "--query_embeddings", "q.npy", "--document_embeddings", "d.npy", "--query_ids", "ids.json")
    assert r.returncode == 2 and "--query_ids" in r.stderr
    r = _run("mine_negatives", "--help")
    assert r.returncode == 0 and "seeded" in r.stdout and "negatives_key" in r.stdout
