"""CPU checks of the retrieval evaluation's host side: the BEIR-layout loader on a fixture written here, the target lists it
makes, the new config keys, a reference recipe that still parses, the log names, and the tool's argument errors."""
import json
import logging
from pathlib import Path

import numpy as np
import pytest
import yaml

ROOT = Path(__file__).resolve().parent.parent
CONTRACTS = ROOT / "tests" / "golden" / "host_contracts.json"


def write_task(root: Path, name="NanoToy"):
    """5 documents (one with a title, one with an empty title, one whose id is also a query id), 4 queries (q3 has no qrels),
    qrels with a header, a zero score, a negative score and a document the corpus does not hold."""
    d = root / name
    (d / "qrels").mkdir(parents=True)
    docs = [{"_id": "d0", "title": "Alpha", "text": "first body"}, {"_id": "d1", "title": "", "text": "second body"},
            {"_id": "d2", "text": "third body"}, {"_id": "q1", "title": " ", "text": "the query itself"},
            {"_id": "d4", "title": "Echo", "text": "fifth body"}]
    (d / "corpus.jsonl").write_text("".join(json.dumps(x) + "\n" for x in docs) + "\n")
    queries = [{"_id": "q0", "text": "zero"}, {"_id": "q1", "text": "one"}, {"_id": "q2", "text": "two"}, {"_id": "q3", "text": "unjudged"}]
    (d / "queries.jsonl").write_text("".join(json.dumps(x) + "\n" for x in queries))
    (d / "qrels" / "test.tsv").write_text("query-id\tcorpus-id\tscore\n"
                                          "q1\td4\t2\nq1\td0\t1\nq1\td1\t0\n"
                                          "q0\td2\t1\nq0\tgone\t1\n"
                                          "q2\td1\t0\nq2\td0\t-1\n")
    return d


def test_loader_reads_the_beir_layout(tmp_path, caplog):
    from contrastors_amd.retrieval_eval import load_beir_task, task_targets

    d = write_task(tmp_path)
    with caplog.at_level(logging.WARNING):
        task = load_beir_task(d)
    assert task.name == "NanoToy"
    assert task.corpus_ids == ["d0", "d1", "d2", "q1", "d4"]
    assert task.corpus_texts == ["Alpha first body", "second body", "third body", "the query itself", "Echo fifth body"]
    # queries in the order of the qrels file; q3 has no qrel line and is not kept; q2 has only non-positive ones and is
    assert task.query_ids == ["q1", "q0", "q2"] and task.query_texts == ["one", "zero", "two"]
    assert task.qrels == [{4: 2.0, 0: 1.0}, {2: 1.0}, {}]
    assert task.n_qrels_dropped == 1
    assert len([r for r in caplog.records if "not in corpus.jsonl" in r.getMessage()]) == 1
    row_ptr, ids, gains = task_targets(task, exclude_identical=True)
    assert row_ptr.tolist() == [0, 3, 4, 4] and ids.tolist() == [0, 4, 3, 2] and gains.tolist() == [1.0, 2.0, 0.0, 1.0]
    assert row_ptr.dtype == np.int64 and ids.dtype == np.int64 and gains.dtype == np.float32
    row_ptr, ids, gains = task_targets(task, exclude_identical=False)
    assert row_ptr.tolist() == [0, 2, 3, 3] and ids.tolist() == [0, 4, 2] and gains.tolist() == [1.0, 2.0, 1.0]


def test_a_relevant_document_with_the_querys_id_is_excluded(tmp_path):
    from contrastors_amd.retrieval_eval import load_beir_task, task_targets

    d = write_task(tmp_path)
    with open(d / "qrels" / "test.tsv", "a") as f:
        f.write("q1\tq1\t1\n")
    task = load_beir_task(d)
    _, ids, gains = task_targets(task, exclude_identical=True)
    assert ids.tolist()[:3] == [0, 4, 3] and gains.tolist()[:3] == [1.0, 2.0, 0.0]
    _, ids, gains = task_targets(task, exclude_identical=False)
    assert ids.tolist()[:3] == [0, 3, 4] and gains.tolist()[:3] == [1.0, 1.0, 2.0]


def test_loader_errors_name_the_layout(tmp_path):
    from contrastors_amd.retrieval_eval import find_tasks, load_beir_task

    with pytest.raises(FileNotFoundError, match="corpus.jsonl.*Nothing is downloaded"):
        load_beir_task(tmp_path / "nowhere")
    d = write_task(tmp_path)
    with pytest.raises(FileNotFoundError, match="dev.tsv"):
        load_beir_task(d, split="dev")
    (d / "qrels" / "bad.tsv").write_text("query-id\tcorpus-id\tscore\nq0 d0 1\n")
    with pytest.raises(ValueError, match="bad.tsv:2"):
        load_beir_task(d, split="bad")
    (d / "qrels" / "ghost.tsv").write_text("query-id\tcorpus-id\tscore\nnobody\td0\t1\n")
    with pytest.raises(ValueError, match="not in queries.jsonl"):
        load_beir_task(d, split="ghost")
    # a directory of tasks, a single task, a filter, an empty directory
    write_task(tmp_path, "Other")
    (tmp_path / "notes").mkdir()
    assert [p.name for p in find_tasks(tmp_path)] == ["NanoToy", "Other"]
    assert [p.name for p in find_tasks(d)] == ["NanoToy"]
    assert [p.name for p in find_tasks(tmp_path, ["other"])] == ["Other"]
    with pytest.raises(FileNotFoundError, match="no task named"):
        find_tasks(tmp_path, ["scifact"])
    with pytest.raises(FileNotFoundError, match="holds no evaluation task"):
        find_tasks(tmp_path / "notes")
    with pytest.raises(FileNotFoundError, match="not a directory"):
        find_tasks(tmp_path / "nowhere")


def test_log_names_follow_the_reference():
    from contrastors_amd.retrieval_eval import beir_log_metrics, beir_log_name

    assert beir_log_name("NanoNFCorpus") == "beir/nfcorpus" and beir_log_name("scifact") == "beir/scifact"
    assert beir_log_name("nano") == "beir/nano"
    got = beir_log_metrics({"NanoArguAna": {"ndcg@10": 0.25, "map@10": 0.1}, "fiqa": {"ndcg@10": 0.75}})
    assert got == {"beir/arguana": 0.25, "beir/fiqa": 0.75, "beir/mean": 0.5}
    assert beir_log_metrics({}) == {}


def test_config_fields_and_a_reference_recipe(tmp_path):
    from contrastors_amd.config import DataArgs, ModelArgs, read_config

    assert DataArgs().retrieval_eval_path is None
    assert ModelArgs().query_prefix == "search_query: " and ModelArgs().document_prefix == "search_document: "
    assert ModelArgs(query_prefix=None, document_prefix=None).query_prefix is None      # a recipe may write null: no prefix
    distill = json.loads(CONTRACTS.read_text())["recipes"]["distill.yaml"]["model_args"]        # writes `document_prefix: null`
    assert distill["document_prefix"] is None and ModelArgs(**distill).document_prefix is None
    recipe = json.loads(CONTRACTS.read_text())["recipes"]["contrastive_finetune.yaml"]
    p = tmp_path / "contrastive_finetune.yaml"
    p.write_text(yaml.safe_dump(recipe, sort_keys=False))
    cfg = read_config(str(p))
    assert cfg.model_args.model_type == "encoder" and cfg.data_args.retrieval_eval_path is None
    assert cfg.model_args.query_prefix == recipe["model_args"].get("query_prefix", "search_query: ")
    recipe["data_args"]["retrieval_eval_path"] = "/data/nano"
    recipe["model_args"].update(query_prefix="query: ", document_prefix="passage: ")
    p.write_text(yaml.safe_dump(recipe, sort_keys=False))
    cfg = read_config(str(p))
    assert cfg.data_args.retrieval_eval_path == "/data/nano"
    assert (cfg.model_args.query_prefix, cfg.model_args.document_prefix) == ("query: ", "passage: ")


def test_argument_checks_that_need_no_gpu():
    from contrastors_amd.retrieval_eval import _check_ks, _truncate

    assert _check_ks((1, 10)) == [1, 10]
    with pytest.raises(ValueError, match="1 to 8"):
        _check_ks(range(1, 10))
    with pytest.raises(ValueError, match="1 to 8"):
        _check_ks(())
    with pytest.raises(ValueError, match="at least 1"):
        _check_ks((10, 0))
    import torch

    e = torch.nn.functional.normalize(torch.arange(1.0, 13.0).reshape(2, 6), dim=-1)
    t = _truncate(e, 3)
    assert t.shape == (2, 3) and torch.allclose(t.norm(dim=1), torch.ones(2))
    assert torch.allclose(t[0], torch.tensor([1.0, 2.0, 3.0]) / 14 ** 0.5)
    with pytest.raises(ValueError, match="prefix width"):
        _truncate(e, 7)


def test_tool_argument_errors(tmp_path, capsys):
    from contrastors_amd.tools import retrieval_eval as tool

    def fails(argv, needle):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2
        assert needle in capsys.readouterr().err

    cfg = tmp_path / "recipe.yaml"
    cfg.write_text(yaml.safe_dump({"train_args": {}, "model_args": {"model_type": "encoder"}}))
    d = write_task(tmp_path / "sets")
    fails([], "--config")
    fails(["--config", str(tmp_path / "none.yaml"), "--data", str(d)], "does not exist")
    fails(["--config", str(cfg)], "nothing to evaluate")
    fails(["--config", str(cfg), "--data", str(d), "--ks", "1,x"], "comma-separated integers")
    fails(["--config", str(cfg), "--data", str(d), "--ks", "0,10"], "positive integers")
    fails(["--config", str(cfg), "--data", str(d), "--ks", "1,2,3,4,5,6,7,8,9"], "at most 8")
    fails(["--config", str(cfg), "--data", str(d), "--dims", "64,-1"], "positive integers")
    fails(["--config", str(cfg), "--data", str(d), "--checkpoint", str(tmp_path / "sets")], "neither config.json nor model/config.json")
    fails(["--config", str(cfg), "--data", str(tmp_path / "nowhere")], "not a directory")
    fails(["--config", str(cfg), "--data", str(tmp_path / "sets"), "--tasks", "scifact"], "no task named")
    mlm = tmp_path / "mlm.yaml"
    mlm.write_text(yaml.safe_dump({"train_args": {}, "model_args": {"model_type": "mlm"}}))
    fails(["--config", str(mlm), "--data", str(d)], "not a text-text recipe")
