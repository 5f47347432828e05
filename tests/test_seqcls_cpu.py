"""Sequence classification / GLUE, host side (no GPU): the C boundary of the new entry points, the fp64 restatement of
tests/seqcls_ref.py against the reference's own class (tests/golden/seqcls_tiny.npz, written by scripts/make_golden_seqcls.py),
checkpoint routing, the GLUE metrics against sklearn / scipy, the local data path, the schedule, and the evaluation loop's
gather-and-trim on two gloo ranks."""
import ctypes as C
import json
import os
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import seqcls_ref as SR

ROOT = Path(__file__).resolve().parent.parent
HDR = ROOT / "include" / "contrastors_hip.h"
NEW_SYMBOLS = {"cx_embed_ln_fwd_typed", "cx_embed_ln_bwd_typed", "cx_embed_ln_bwd_sorted_typed", "cx_encoder_forward_typed",
               "cx_encoder_backward_typed", "cx_seqcls_ws_floats", "cx_seqcls_head_fwd", "cx_seqcls_head_bwd"}
ERR_SHAPE, ERR_ARG = -1, -3


@pytest.fixture(scope="module")
def built():
    from contrastors_amd import build

    return build.build()


# ------------------------------------------------------------------------------------------------------------ boundary
def test_new_entry_points_are_declared_bound_and_exported(built):
    from contrastors_amd import _C

    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", HDR.read_text()))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_C.EXPORTED_SYMBOLS)
    assert declared == set(_C.EXPORTED_SYMBOLS)
    assert not NEW_SYMBOLS & set(_C.DEV_EXPORTED_SYMBOLS)
    lib = _C.lib()
    assert lib.cx_abi_version() == 10          # additive: no existing signature changed
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    # the typed forms are the untyped signatures + token_type_ids + type_vocab_size (+ the workspace of the backward forms)
    for typed, plain, extra in (("cx_embed_ln_fwd_typed", "cx_embed_ln_fwd", 2), ("cx_embed_ln_bwd_typed", "cx_embed_ln_bwd", 4),
                                ("cx_embed_ln_bwd_sorted_typed", "cx_embed_ln_bwd_sorted", 4),
                                ("cx_encoder_forward_typed", "cx_encoder_forward", 1), ("cx_encoder_backward_typed", "cx_encoder_backward", 1)):
        assert len(_C._SIGS[typed][1]) == len(_C._SIGS[plain][1]) + extra and _C._SIGS[typed][0] is C.c_int
    assert lib.cx_seqcls_ws_floats(32, 768, 2) == 32 * 768 and lib.cx_seqcls_ws_floats(4096, 1024, 8) == 4096 * 1024


def test_entry_points_refuse_bad_arguments_before_touching_pointers(built):
    """Shape and argument errors are decided on the host from the integers alone: every pointer here is NULL or bogus."""
    from contrastors_amd import _C

    lib = _C.lib()
    one = 16   # a non-NULL "pointer" nobody may dereference
    for B, d, Cn in ((0, 768, 2), (4097, 768, 2), (16, 384, 2), (16, 2048, 2), (16, 768, 0), (16, 768, 9)):
        assert lib.cx_seqcls_ws_floats(B, d, Cn) == 0
        assert lib.cx_seqcls_head_fwd(one, d, one, one, one, one, one, 0, 0.0, 0, 0, one, one, one, B, d, Cn, None) == ERR_SHAPE
        assert lib.cx_seqcls_head_bwd(one, d, one, one, one, one, one, 0, 1.0, 0.0, 0, 0, one, 1 << 30, one, one, one, one, one, B, d,
                                      Cn, None) == ERR_SHAPE
    assert lib.cx_seqcls_head_fwd(one, 512, one, one, one, one, one, 0, 0.0, 0, 0, one, one, one, 16, 768, 2, None) == ERR_SHAPE   # ldx < d
    fwd = [one, 768, one, one, one, one, one, 0, 0.0, 0, 0, one, one, one, 16, 768, 2, None]
    for null in (0, 2, 3, 4, 5, 11, 12, 13):            # X, Wp, bp, Wc, bc, pooled, logits, loss_rows (with labels)
        a = list(fwd)
        a[null] = None
        assert lib.cx_seqcls_head_fwd(*a) == ERR_ARG, null
    for mode, p in ((2, 0.0), (0, 1.0), (0, -0.1)):
        a = list(fwd)
        a[7], a[8] = mode, p
        assert lib.cx_seqcls_head_fwd(*a) == ERR_ARG
    bwd = [one, 768, one, one, one, one, one, 0, 1.0, 0.0, 0, 0, one, 16 * 768, one, one, one, one, one, 16, 768, 2, None]
    for null in (0, 2, 3, 4, 5, 6, 12, 14, 15, 16, 17, 18):
        a = list(bwd)
        a[null] = None
        assert lib.cx_seqcls_head_bwd(*a) == ERR_ARG, null
    a = list(bwd)
    a[13] = 16 * 768 - 1                                 # workspace one float short
    assert lib.cx_seqcls_head_bwd(*a) == ERR_ARG
    # typed embedding: type_vocab_size other than 2
    assert lib.cx_embed_ln_fwd_typed(one, one, one, one, one, 3, one, one, one, one, one, one, 8, 8, 256, 1e-12, None) == ERR_SHAPE
    assert lib.cx_embed_ln_bwd_typed(*([one] * 7), 1, *([one] * 10), 1 << 20, 8, 8, 256, 0, None) == ERR_SHAPE
    assert lib.cx_embed_ln_bwd_sorted_typed(*([one] * 7), 4, *([one] * 10), 1 << 20, 8, 8, 256, 0, 16, one, one, one, None) == ERR_SHAPE
    # ... an unsupported width, and a workspace that holds no [2][d] partial
    assert lib.cx_embed_ln_fwd_typed(one, one, one, one, one, 2, one, one, one, one, one, one, 8, 8, 384, 1e-12, None) == ERR_SHAPE
    assert lib.cx_embed_ln_bwd_typed(*([one] * 7), 2, *([one] * 10), 4 * 256 - 1, 8, 8, 256, 0, None) == ERR_ARG
    assert lib.cx_embed_ln_bwd_typed(*([one] * 7), 2, *([one] * 9), None, 1 << 20, 8, 8, 256, 0, None) == ERR_ARG


# -------------------------------------------------------------------------------------------- restatement vs reference
def _tiny():
    from contrastors_amd.nomic_bert import NomicBertConfig
    from oracle import encoder_ref
    from oracle.make_golden import TINY_BERT, checksum

    g = np.load(ROOT / "tests" / "golden" / "seqcls_tiny.npz", allow_pickle=False)
    cfg = NomicBertConfig(**{k: v for k, v in TINY_BERT.items() if k in NomicBertConfig.__dataclass_fields__})
    assert all(np.array(v) == g["cfg/" + k] for k, v in TINY_BERT.items())
    trunk = encoder_ref.random_state_dict(SimpleNamespace(**TINY_BERT), int(g["seed"]))
    np.testing.assert_allclose(checksum(trunk), g["trunk_checksum"], rtol=1e-12)
    return g, cfg, trunk


def golden_state(g, trunk, case, dtype):
    sd = {f"bert.{k}": v.to(dtype) for k, v in trunk.items()}
    sd.update({k: torch.from_numpy(g[f"{case}/head/{k}"]).to(dtype) for k in
               ("bert.pooler.dense.weight", "bert.pooler.dense.bias", "classifier.weight", "classifier.bias")})
    return sd


@pytest.mark.parametrize("case,mode", [("c2", 0), ("c3", 0), ("c1", 1)])
def test_fp64_restatement_reproduces_the_reference_class(case, mode):
    """The reference ran in fp32: its logits (|logit| < 1, sums of 256 terms through two layers) carry ~1e-6 of rounding; 2e-5
    is the bound the fp32 encoder goldens are held to by the fp64 oracle elsewhere in this suite."""
    g, cfg, trunk = _tiny()
    ids, mask, tts = (torch.from_numpy(g[k]) for k in ("input_ids", "attention_mask", "token_type_ids"))
    labels = torch.from_numpy(g[f"{case}/labels"])
    sd = golden_state(g, trunk, case, torch.float64)
    loss, logits = SR.seqcls_twin(sd, cfg, ids, mask, tts, labels.double() if mode else labels, mode)
    np.testing.assert_allclose(logits.numpy(), g[f"{case}/logits"], atol=2e-5, rtol=0)
    assert abs(float(loss) - float(g[f"{case}/loss"])) <= 2e-5
    _, swapped = SR.seqcls_twin(sd, cfg, ids, mask, (1 - tts) * mask)
    np.testing.assert_allclose(swapped.numpy(), g[f"{case}/logits_swapped_types"], atol=2e-5, rtol=0)
    assert np.abs(g[f"{case}/logits_swapped_types"] - g[f"{case}/logits"]).max() > 1e-3, "the segment ids matter to the reference"
    # the restatement moves under a planted error: type row 1 ignored
    _, blind = SR.seqcls_twin(sd, cfg, ids, mask, torch.zeros_like(tts))
    assert np.abs(blind.numpy() - g[f"{case}/logits"]).max() > 1e-3


def test_state_dict_keys_are_the_reference_class_s():
    from contrastors_amd.seqcls import reference_keys

    g, cfg, _ = _tiny()
    for case in ("c2", "c3", "c1"):
        assert reference_keys(cfg) == sorted(g[f"{case}/state_dict_keys"].tolist())
    assert {"bert.pooler.dense.weight", "bert.pooler.dense.bias", "classifier.weight", "classifier.bias"} <= set(reference_keys(cfg))


def test_host_philox_mask_statistics_and_scaling():
    keep = SR.head_keep(1234, 8, 64, 768, 0.1)
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))
    vals = set(np.unique(keep.numpy()).tolist())
    assert vals == {0.0, float(inv)}
    n, kept = keep.numel(), int((keep > 0).sum())
    assert abs(kept - 0.9 * n) <= 6 * (n * 0.1 * 0.9) ** 0.5
    assert not torch.equal(keep, SR.head_keep(1234, 12, 64, 768, 0.1)) and torch.equal(keep, SR.head_keep(1234, 8, 64, 768, 0.1))
    assert torch.equal(SR.head_keep(1, 0, 4, 256, 0.0), torch.ones(4, 256))


def test_typed_embedding_constants_are_measured_on_the_typed_inputs():
    """tests/test_ln_ref_cpu.py::test_measured_constants for the typed tests' inputs: every TYPED_C_MEAS entry is the worst ratio of
    the fp32 emulation against fp64 rounded up -- not below it, not more than twice it -- so changing the inputs re-measures."""
    m = SR.measure_typed_constants()
    for fam, vals in SR.TYPED_C_MEAS.items():
        for what, c in vals.items():
            assert m[fam][what] <= c <= 2.0 * m[fam][what], (fam, what, m[fam][what], c)
    # the typed z is the untyped one where every token has type 0 (the row math on top of it is ln_ref's, imported)
    e = SR.typed_embed_inputs(77, 256, 512, types="zeros")
    z, tid, p, tt = SR.typed_embed_z(e["word"], e["type"], e["pos"], e["ids"], e["tts"], e["indices"], e["seq"])
    z0, tid0, p0 = SR.R.embed_z(e["word"], e["type"], e["pos"], e["ids"], e["indices"], e["seq"])
    assert torch.equal(z, z0) and torch.equal(tid, tid0) and torch.equal(p, p0) and int(tt.sum()) == 0
    e = SR.typed_embed_inputs(77, 256, 512, types="switch")
    z, _, _, tt = SR.typed_embed_z(e["word"], e["type"], e["pos"], e["ids"], e["tts"], e["indices"], e["seq"])
    z0, _, _ = SR.R.embed_z(e["word"], e["type"], e["pos"], e["ids"], e["indices"], e["seq"])
    assert 0 < int(tt.sum()) < 77 and torch.equal(z[tt == 0], z0[tt == 0]) and not torch.equal(z[tt == 1], z0[tt == 1])


# ------------------------------------------------------------------------------------------------- checkpoint routing
def test_mlm_checkpoint_routes_trunk_in_cls_out_and_leaves_the_head_fresh():
    from contrastors_amd.seqcls import split_checkpoint

    g, cfg, trunk = _tiny()
    mlm = {f"bert.{k}": v for k, v in trunk.items()}
    mlm.update({"cls.predictions.transform.dense.weight": torch.zeros(256, 256), "cls.predictions.transform.dense.bias": torch.zeros(256),
                "cls.predictions.transform.layer_norm.weight": torch.ones(256), "cls.predictions.transform.layer_norm.bias": torch.zeros(256),
                "cls.predictions.decoder.bias": torch.zeros(512), "cls.predictions.decoder.weight": trunk["embeddings.word_embeddings.weight"]})
    shapes = {"bert.pooler.dense.weight": (256, 256), "bert.pooler.dense.bias": (256,), "classifier.weight": (2, 256), "classifier.bias": (2,)}
    got, taken, report = split_checkpoint(mlm, shapes)
    assert set(got) == set(trunk) and all(got[k] is trunk[k] for k in trunk)
    assert taken == {} and report["fresh"] == list(shapes) and report["mismatched"] == []
    assert report["skipped"] == sorted(k for k in mlm if k.startswith("cls."))
    # a classification checkpoint with another label count: pooler taken, classifier left fresh (ignore_mismatched_sizes)
    own = golden_state(g, trunk, "c3", torch.float32)
    got, taken, report = split_checkpoint(own, shapes)
    assert set(got) == set(trunk) and set(taken) == {"bert.pooler.dense.weight", "bert.pooler.dense.bias"}
    assert report == {"fresh": [], "mismatched": ["classifier.weight", "classifier.bias"], "skipped": []}
    # a bi-encoder tower: trunk.* is the trunk, its projection is skipped
    tower = {f"trunk.{k}": v for k, v in trunk.items()}
    tower["proj.weight"] = torch.zeros(4, 4)
    got, taken, report = split_checkpoint(tower, shapes)
    assert set(got) == set(trunk) and not taken and report["skipped"] == ["proj.weight"] and report["fresh"] == list(shapes)


# ----------------------------------------------------------------------------------------------------------- metrics
def test_glue_metric_agrees_with_sklearn_and_scipy():
    from scipy.stats import pearsonr, spearmanr
    from sklearn.metrics import f1_score, matthews_corrcoef

    from contrastors_amd.glue import glue_metric

    r = np.random.default_rng(7)
    for n in (7, 200, 1043):
        t, p = r.integers(0, 2, n), r.integers(0, 2, n)
        assert glue_metric("cola", p, t).keys() == {"matthews_correlation"}
        assert abs(glue_metric("cola", p, t)["matthews_correlation"] - matthews_corrcoef(t, p)) <= 1e-12
        for task in ("mrpc", "qqp"):
            m = glue_metric(task, p, t)
            assert m.keys() == {"accuracy", "f1"}
            assert abs(m["f1"] - f1_score(y_true=t, y_pred=p)) <= 1e-12 and abs(m["accuracy"] - (p == t).mean()) <= 1e-12
        t3, p3 = r.integers(0, 3, n), r.integers(0, 3, n)
        for task in ("mnli", "qnli", "rte", "sst2", "wnli"):
            assert glue_metric(task, p3, t3) == {"accuracy": float((p3 == t3).mean())}
        x = r.integers(0, 6, n).astype(np.float64) / 5.0 * 5.0          # ties on both sides (STS-B scores repeat)
        y = np.round(x + r.normal(size=n), 1)
        m = glue_metric("stsb", y, x)
        assert m.keys() == {"pearson", "spearmanr"}
        assert abs(m["pearson"] - pearsonr(y, x)[0]) <= 1e-12 and abs(m["spearmanr"] - spearmanr(y, x)[0]) <= 1e-12
    # a single-class prediction: MCC = 0, F1 = 0 when that class is the negative one (sklearn's zero_division default)
    t = r.integers(0, 2, 50)
    assert glue_metric("cola", np.zeros(50, int), t) == {"matthews_correlation": 0.0} and matthews_corrcoef(t, np.zeros(50, int)) == 0.0
    assert glue_metric("mrpc", np.zeros(50, int), t)["f1"] == 0.0
    # a constant prediction: Pearson and Spearman are undefined -> NaN (what scipy returns, with a warning), never an exception
    m = glue_metric("stsb", np.full(50, 2.5), r.normal(size=50))
    assert np.isnan(m["pearson"]) and np.isnan(m["spearmanr"])
    with pytest.raises(KeyError):
        glue_metric("squad", t, t)


# -------------------------------------------------------------------------------------------------------------- data
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(40)]


def _tokenizer(tmp_path):
    from transformers import BertTokenizer

    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(VOCAB) + "\n")
    return BertTokenizer(str(vocab), do_lower_case=True)


def _records(n, seed, labels, pair=True):
    r = np.random.default_rng(seed)
    sent = lambda: " ".join(f"w{int(i)}" for i in r.integers(0, 40, int(r.integers(1, 9))))   # noqa: E731
    recs = []
    for i in range(n):
        rec = {"sentence1": sent(), "label": labels[int(r.integers(0, len(labels)))], "idx": i}
        if pair:
            rec["sentence2"] = sent()
        recs.append(rec)
    return recs


def _write_jsonl(path, recs):
    path.write_text("".join(json.dumps(r) + "\n" for r in recs))


def test_jsonl_and_saved_datasetdict_give_the_same_batches(tmp_path):
    import datasets

    from contrastors_amd.glue import ShardedBatches, encode_glue, load_glue_dir

    tok = _tokenizer(tmp_path)
    splits = {"train": _records(23, 1, labels=[5, 9]), "validation": _records(9, 2, labels=[5, 9])}   # RTE-shaped; raw labels 5 / 9
    a, b = tmp_path / "jsonl", tmp_path / "saved"
    a.mkdir()
    for s, recs in splits.items():
        _write_jsonl(a / f"{s}.jsonl", recs)
    _write_jsonl(a / "test.jsonl", _records(3, 3, labels=[5]))            # a test split is ignored (glue.py:78)
    datasets.DatasetDict({s: datasets.Dataset.from_list(recs) for s, recs in splits.items()}).save_to_disk(str(b))
    enc = [encode_glue(load_glue_dir(str(p), "rte"), "rte", tok, seq_len=12) for p in (a, b)]
    assert enc[0] == enc[1] and set(enc[0]) == {"train", "validation"}
    # label mapping through the sorted label list; pairs carry segment ids 0 ... 0 1 ... 1; truncation at seq_len
    for split, recs in splits.items():
        for row, rec in zip(enc[0][split], recs):
            assert row["labels"] == {5: 0, 9: 1}[rec["label"]]
            want = tok(rec["sentence1"], rec["sentence2"], padding=False, max_length=12, truncation=True)
            assert row["input_ids"] == want["input_ids"] and row["token_type_ids"] == want["token_type_ids"]
            assert len(row["input_ids"]) <= 12 and row["input_ids"][0] == 2 and 1 in row["token_type_ids"]
    # dynamic padding: every batch is as wide as ITS longest row, padded with the pad id / mask 0 / type 0
    for x, y in zip(ShardedBatches(enc[0]["train"], 4, shuffle=True, seed=3), ShardedBatches(enc[1]["train"], 4, shuffle=True, seed=3)):
        assert all(torch.equal(x[k], y[k]) for k in x) and x.keys() == {"input_ids", "attention_mask", "token_type_ids", "labels"}
    widths = set()
    order = ShardedBatches(enc[0]["train"], 4, shuffle=True, seed=3).order()
    assert sorted(order) == list(range(23)) and order != list(range(23))
    for i, batch in enumerate(ShardedBatches(enc[0]["train"], 4, shuffle=True, seed=3)):
        rows = [enc[0]["train"][j] for j in order[4 * i: 4 * i + 4]]
        S = max(len(r["input_ids"]) for r in rows)
        widths.add(S)
        assert batch["input_ids"].shape == (len(rows), S) and batch["labels"].dtype == torch.int64
        for k, r in enumerate(rows):
            n = len(r["input_ids"])
            assert batch["input_ids"][k, :n].tolist() == r["input_ids"] and (batch["input_ids"][k, n:] == 0).all()
            assert batch["attention_mask"][k].tolist() == [1] * n + [0] * (S - n)
            assert batch["token_type_ids"][k, :n].tolist() == r["token_type_ids"] and (batch["token_type_ids"][k, n:] == 0).all()
            assert int(batch["labels"][k]) == r["labels"]
    assert len(widths) > 1
    with pytest.raises(FileNotFoundError):
        load_glue_dir(str(a), "mnli")


def test_mnli_takes_both_validation_splits_and_stsb_keeps_float_labels(tmp_path):
    from contrastors_amd.glue import encode_glue, load_glue_dir

    tok = _tokenizer(tmp_path)
    d = tmp_path / "mnli"
    d.mkdir()
    names = ["entailment", "neutral", "contradiction"]
    for s, n in (("train", 12), ("validation_matched", 5), ("validation_mismatched", 6)):
        recs = [{"premise": r["sentence1"], "hypothesis": r["sentence2"], "label": r["label"]} for r in _records(n, len(s), labels=names)]
        _write_jsonl(d / f"{s}.jsonl", recs)
    enc = encode_glue(load_glue_dir(str(d), "mnli"), "mnli", tok, 16)
    assert {k: len(v) for k, v in enc.items()} == {"train": 12, "validation_matched": 5, "validation_mismatched": 6}
    assert {r["labels"] for r in enc["train"]} <= {0, 1, 2}     # sorted names: contradiction 0, entailment 1, neutral 2
    first = json.loads((d / "train.jsonl").read_text().splitlines()[0])
    assert enc["train"][0]["labels"] == sorted(names).index(first["label"])
    s = tmp_path / "stsb"
    s.mkdir()
    for split in ("train", "validation"):
        _write_jsonl(s / f"{split}.jsonl", _records(6, 4, labels=[0.0, 2.5, 4.2]))
    enc = encode_glue(load_glue_dir(str(s), "stsb"), "stsb", tok, 16)
    assert all(isinstance(r["labels"], float) for r in enc["train"]) and {r["labels"] for r in enc["train"]} <= {0.0, 2.5, 4.2}
    c = tmp_path / "cola"
    c.mkdir()
    for split in ("train", "validation"):
        _write_jsonl(c / f"{split}.jsonl", [{"sentence": r["sentence1"], "label": r["label"]} for r in _records(5, 5, labels=[0, 1])])
    enc = encode_glue(load_glue_dir(str(c), "cola"), "cola", tok, 16)
    assert all(set(r["token_type_ids"]) == {0} for r in enc["train"])        # single sentences: one segment


# ---------------------------------------------------------------------------------------------------------- schedule
def test_glue_recipe_parses_and_the_warm_up_follows_warmup_pct(tmp_path):
    import yaml

    from contrastors_amd.config import read_config
    from contrastors_amd.glue import task_to_keys, task_to_num_labels, task_to_problem_type, warmup_steps_for
    from contrastors_amd.train import apply_overrides
    from contrastors_amd.trainers import TRAINER_REGISTRY, _lr_lambda

    recipe = json.loads((ROOT / "tests" / "golden" / "host_contracts.json").read_text())["recipes"]["glue.yaml"]
    p = tmp_path / "glue.yaml"
    p.write_text(yaml.safe_dump(recipe, sort_keys=False))
    cfg = read_config(str(p))
    ta = cfg.train_args
    assert cfg.model_args.model_type == "glue" and cfg.data_args.task_name == "cola" and cfg.data_args.batch_size == 16
    assert (ta.num_epochs, ta.learning_rate, ta.adam_beta2, ta.weight_decay, ta.eps) == (10, 3e-5, 0.98, 1e-6, 1e-6)
    assert ta.max_grad_norm == 0.0 and ta.schedule_type == "linear" and ta.warmup_pct == 0.06 and ta.eval_strategy == "epochs"
    assert "glue" in TRAINER_REGISTRY
    cfg = apply_overrides(cfg, {"task_name": "rte", "input_shards": "/data/rte"})          # the CLI's --task_name / --input_shards
    assert cfg.data_args.task_name == "rte" and cfg.data_args.input_shards == "/data/rte"
    # sc/trainers/base.py:233-235: warmup = int(steps_per_epoch * num_epochs * warmup_pct); CoLA: 8551 rows / 16 = 535 batches
    assert warmup_steps_for(ta, 535) == int(535 * 10 * 0.06) == 321
    ta.gradient_accumulation_steps = 4
    assert warmup_steps_for(ta, 535 // 4) == int(133 * 10 * 0.06) == 79
    ta.warmup_steps = 17
    assert warmup_steps_for(ta, 535) == 17
    f = _lr_lambda("linear", 321, 5350)
    assert f(0) == 0.0 and f(321) == 1.0 and f(5350) == 0.0 and abs(f(160) - 160 / 321) < 1e-12
    assert set(task_to_num_labels) == set(task_to_problem_type) == set(task_to_keys) - {"wnli"}
    assert task_to_num_labels["mnli"] == 3 and task_to_num_labels["stsb"] == 1 and task_to_problem_type["stsb"] == "regression"
    assert task_to_keys["qnli"] == ("question", "sentence") and task_to_keys["sst2"] == ("sentence", None)


# --------------------------------------------------------------------------------------------- evaluation on two ranks
def _eval_worker(rank, world, port, out_dir, n, bs):
    sys.path.insert(0, str(ROOT))
    from contrastors_amd.distributed import gather
    from contrastors_amd.glue import ShardedBatches, trim_gathered

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    rows = [{"input_ids": [2] + [5 + (i % 7)] * (1 + i % 5), "labels": i} for i in range(n)]
    batches = ShardedBatches(rows, bs, rank, world)
    preds, seen, shapes = [], 0, []
    for i, b in enumerate(batches):
        shapes.append(int(b["labels"].shape[0]))
        p = gather(b["labels"] * 10)                      # the "prediction" of row i is 10 i
        r = gather(b["labels"])
        p, r, seen = trim_gathered(p, r, seen, n, i == len(batches) - 1, world)
        assert torch.equal(p, r * 10)
        preds.append(p)
    np.savez(f"{out_dir}/e{rank}_{n}_{bs}.npz", preds=torch.cat(preds).numpy(), shapes=np.array(shapes), steps=np.array(len(batches)))
    dist.destroy_process_group()


@pytest.mark.parametrize("n,bs", [(13, 3), (12, 3), (7, 4)])
def test_eval_gather_trims_the_duplicated_tail_on_two_ranks(tmp_path, n, bs):
    """13 rows, 2 ranks x 3: the last global batch holds 1 row, padded to 2 by wrapping -- the gathered tail is a duplicate and
    is cut (sc/trainers/glue.py:191-197); 12 rows: nothing to cut; 7 rows with 2 x 4: one short batch, padded by one."""
    port = 29900 + (os.getpid() % 90) + n
    mp.spawn(_eval_worker, args=(2, port, str(tmp_path), n, bs), nprocs=2, join=True)
    got = [np.load(tmp_path / f"e{r}_{n}_{bs}.npz") for r in range(2)]
    for g in got:
        np.testing.assert_array_equal(g["preds"], 10 * np.arange(n))          # every row once, in dataset order, on every rank
        assert int(g["steps"]) == -(-n // (2 * bs))
    np.testing.assert_array_equal(got[0]["shapes"], got[1]["shapes"])           # the ranks run equally shaped steps
