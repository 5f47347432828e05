"""GPU checks of the text retrieval evaluation around a model (contrastors_amd.retrieval_eval.evaluate_task / evaluate_path,
TextTextTrainer.eval_loop, tools/retrieval_eval) on a one-layer tower and a BertTokenizer over a vocabulary written here:
evaluate_task against encode + evaluate_embeddings bit for bit, the prefixes, the Matryoshka keys, the trainer's schedule,
log keys and training mode, a trainer without evaluation data, and the tool against the trainer."""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "search", "_", "query", "document", ":"] + [f"w{i}" for i in range(40)]
SEQ = 24


def _write_task(root: Path, name: str, seed: int, n_docs=24, n_queries=7):
    """Documents of 3 to 8 vocabulary words, half of them titled; each query shares words with its relevant documents; query 0
    carries the id of a document (excluded from its ranking)."""
    g = torch.Generator().manual_seed(seed)
    d = root / name
    (d / "qrels").mkdir(parents=True)
    words = lambda n: [f"w{int(x)}" for x in torch.randint(0, 40, (n,), generator=g)]    # noqa: E731
    docs = []
    for i in range(n_docs):
        rec = {"_id": f"{name}-d{i}", "text": " ".join(words(3 + i % 6))}
        if i % 2:
            rec["title"] = " ".join(words(2))
        docs.append(rec)
    queries, qrels = [], ["query-id\tcorpus-id\tscore"]
    for m in range(n_queries):
        rel = [int(x) for x in torch.randperm(n_docs, generator=g)[: 1 + m % 3]]
        qid = docs[(5 * m + 1) % n_docs]["_id"] if m == 0 else f"{name}-q{m}"
        queries.append({"_id": qid, "text": " ".join(docs[rel[0]]["text"].split()[:2] + words(1))})
        qrels += [f"{qid}\t{docs[r]['_id']}\t{1 + (j + m) % 2}" for j, r in enumerate(rel)]
    (d / "corpus.jsonl").write_text("".join(json.dumps(x) + "\n" for x in docs))
    (d / "queries.jsonl").write_text("".join(json.dumps(x) + "\n" for x in queries))
    (d / "qrels" / "test.tsv").write_text("\n".join(qrels) + "\n")
    return d


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from transformers import BertTokenizer

    tmp = tmp_path_factory.mktemp("beir")
    (tmp / "tok").mkdir()
    (tmp / "tok" / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    tok = BertTokenizer(str(tmp / "tok" / "vocab.txt"), do_lower_case=True)
    tok.save_pretrained(str(tmp / "tok"))
    _write_task(tmp / "sets", "NanoToy", 1)
    _write_task(tmp / "sets", "other", 2, n_docs=17, n_queries=5)
    recipe = {"train_args": {"learning_rate": 1e-3, "weight_decay": 0.01, "warmup_steps": 0, "grad_cache": False,
                             "schedule_type": "linear", "max_grad_norm": 1.0, "clamp_logits": False},
              "data_args": {"batch_size": 16, "seed": 7},
              "model_args": {"logit_scale": 20.0, "pooling": "mean", "model_name": "tiny", "seq_len": SEQ,
                             "tokenizer_name": str(tmp / "tok")}}
    return {"tmp": tmp, "tok": tok, "recipe": recipe, "sets": tmp / "sets"}


def _trainer(world, with_path=True, **train_args):
    from contrastors_amd.config import Config
    from contrastors_amd.nomic_bert import NomicBertConfig
    from contrastors_amd.trainers import TextTextTrainer
    from oracle.make_golden import TINY_NOMIC

    recipe = json.loads(json.dumps(world["recipe"]))
    recipe["train_args"].update(train_args)
    if with_path:
        recipe["data_args"]["retrieval_eval_path"] = str(world["sets"])
    tc = NomicBertConfig(**{**{k: v for k, v in TINY_NOMIC.items() if k in NomicBertConfig.__dataclass_fields__}, "n_layer": 1})
    return TextTextTrainer(Config(**recipe), torch.bfloat16, device="cuda", trunk_config=tc, total_steps=20, tokenizer=world["tok"])


@pytest.fixture(scope="module")
def trainer(world):
    return _trainer(world)


def _eval_kwargs(trainer):
    ma = trainer.config.model_args
    return dict(ks=(10,), query_prefix=ma.query_prefix, document_prefix=ma.document_prefix, max_length=ma.seq_len, batch_size=256)


def test_evaluate_task_equals_encode_plus_evaluate_embeddings(world, trainer):
    from contrastors_amd.retrieval_eval import _truncate, evaluate_embeddings, evaluate_task, load_beir_task
    from contrastors_amd.search import encode

    model, tok = trainer.model["model"], world["tok"]
    task = load_beir_task(world["sets"] / "NanoToy")
    assert len(task.corpus_ids) == 24 and len(task.query_ids) == 7 and task.doc_index(task.query_ids[0]) is not None
    seen = []

    def spy(texts, **kw):
        seen.extend(texts)
        return tok(texts, **kw)

    ks = (1, 3, 10)
    got = evaluate_task(model, spy, task, ks=ks, query_prefix="search_query: ", document_prefix="search_document: ",
                        max_length=SEQ, batch_size=5, dims=[128, 64])
    assert model.training
    # the prefixes reach the tokenizer: queries first, then documents, each text once
    assert seen == ["search_query: " + t for t in task.query_texts] + ["search_document: " + t for t in task.corpus_texts]
    qe = encode(model, ["search_query: " + t for t in task.query_texts], tok, batch_size=5, max_length=SEQ)
    ce = encode(model, ["search_document: " + t for t in task.corpus_texts], tok, batch_size=5, max_length=SEQ)
    want = evaluate_embeddings(qe, ce, task, ks)
    assert {k: got[k] for k in want} == want                                   # bit for bit
    assert set(want) == {f"{n}@{k}" for n in ("ndcg", "map", "recall", "precision", "mrr", "hit") for k in ks} | {"n_queries", "n_skipped"}
    assert want["n_queries"] == 7 and 0.0 < want["ndcg@10"] <= 1.0
    for d in (128, 64):
        sub = evaluate_embeddings(_truncate(qe, d), _truncate(ce, d), task, ks)
        assert {k: got[f"{k}_matryoshka_{d}"] for k in sub if "@" in k} == {k: v for k, v in sub.items() if "@" in k}
    assert len(got) == len(want) + 2 * (len(want) - 2)


def test_trainer_logs_beir_keys_every_eval_steps(world, tmp_path):
    from contrastors_amd.retrieval_eval import beir_log_metrics, evaluate_path
    from contrastors_amd.trainers import synthetic_batches

    t = _trainer(world, wandb=True, output_dir=str(tmp_path / "out"), eval_strategy="steps", eval_steps=2)
    model = t.model["model"]
    direct = {}
    real = t.eval_loop

    def spy(step):
        logged = real(step)
        assert model.training                      # the trainer leaves the model in training mode
        direct[step] = (logged, beir_log_metrics(evaluate_path(model, world["tok"], world["sets"], **_eval_kwargs(t))))
        return logged

    t.eval_loop = spy
    t.train(iter(list(synthetic_batches(4, 16, SEQ, vocab=50))))
    assert sorted(direct) == [2, 4]
    rows = [json.loads(ln) for ln in (tmp_path / "out" / "metrics.jsonl").read_text().splitlines()]
    beir = [r for r in rows if any(k.startswith("beir/") for k in r)]
    assert [r["step"] for r in beir] == [2, 4]
    for r in beir:
        assert set(r) == {"step", "beir/toy", "beir/other", "beir/mean"}
        logged, want = direct[r["step"]]
        assert {k: v for k, v in r.items() if k != "step"} == logged == want      # the same model state: the same bits
        assert r["beir/mean"] == (r["beir/toy"] + r["beir/other"]) / 2 and 0.0 < r["beir/mean"] <= 1.0


def test_trainer_without_the_path_logs_no_beir_key(world, trainer, tmp_path, capsys):
    from contrastors_amd.trainers import synthetic_batches

    t = _trainer(world, with_path=False, wandb=True, output_dir=str(tmp_path / "out"), eval_strategy="steps", eval_steps=2)
    called = []
    t.eval_loop = lambda step: called.append(step)
    t.train(iter(list(synthetic_batches(4, 16, SEQ, vocab=50))))
    rows = [json.loads(ln) for ln in (tmp_path / "out" / "metrics.jsonl").read_text().splitlines()]
    assert called == [] and t.get_eval_data() == {} and t.evaluate() == {}
    assert rows and not any(k.startswith("beir/") for r in rows for k in r)
    # without a tracker rank 0 prints
    got = trainer.eval_loop(7)
    out = capsys.readouterr().out
    assert "Step: 7" in out and "beir/toy" in out and set(got) == {"beir/toy", "beir/other", "beir/mean"}


def test_tool_prints_the_trainers_numbers(world, trainer, tmp_path):
    want = trainer.evaluate()
    assert set(want) == {"beir/toy", "beir/other", "beir/mean"} and trainer.model["model"].training
    trainer.save_state(str(tmp_path / "ckpt"))
    cfg = tmp_path / "recipe.yaml"
    cfg.write_text(yaml.safe_dump(world["recipe"]))
    out_file = tmp_path / "result.json"
    r = subprocess.run([sys.executable, "-m", "contrastors_amd.tools.retrieval_eval", "--config", str(cfg), "--checkpoint",
                        str(tmp_path / "ckpt"), "--data", str(world["sets"]), "--ks", "1,10", "--dims", "64", "--out", str(out_file),
                        "--per_query"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == json.loads(out_file.read_text())
    assert got["beir"] == want, (got["beir"], want)
    assert set(got["tasks"]) == {"NanoToy", "other"}
    toy = got["tasks"]["NanoToy"]
    assert toy["ndcg@10"] == want["beir/toy"] and "ndcg@10_matryoshka_64" in toy and "map@1" in toy
    assert len(toy["per_query"]["ndcg"]) == 7 and len(toy["query_ids"]) == 7 and toy["per_query"]["ks"] == [1, 10]
    assert got["mean"]["ndcg@10"] == want["beir/mean"]
