"""GPU checks of the image-text evaluation (contrastors_amd.zeroshot, ImageTextTrainer.eval_loop, tools/zeroshot_eval) on tiny
towers: the classifier against a per-class padded float64 recomputation, the two evaluators against dense float64 metrics of
the same bf16-rounded embeddings, the towers' training mode, the trainer's logging and schedule, an unchanged training
loop, and the tool."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import img_ref as I
from tests import rank_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "photo", "of", "the", "art", "."] + [f"w{i}" for i in range(20)]
CLASSES, TEMPLATES = ["w1 w2", "w3", "w4 w5 w6"], ["a photo of a {}.", "art of the {}"]
FOLDERS = ["n03", "n01", "n02"]      # class i lives in FOLDERS[i]: not the sorted order


def _trunks():
    from contrastors_amd.nomic_bert import NomicBertConfig
    from contrastors_amd.vit import ViTConfig
    from oracle.make_golden import TINY_NOMIC

    tc = NomicBertConfig(**{k: v for k, v in TINY_NOMIC.items() if k in NomicBertConfig.__dataclass_fields__})
    return tc, ViTConfig(n_embd=256, n_layer=1, n_head=4, n_inner=512, img_size=32, patch_size=8)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The data on disk (3 classes x 4 images, 12 images with captions in two tar shards, the metadata, a tokenizer), the recipe
    with and without evaluation data, and a tokenizer."""
    from transformers import BertTokenizer

    tmp = tmp_path_factory.mktemp("zs")
    (tmp / "tok").mkdir()
    (tmp / "tok" / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    tok = BertTokenizer(str(tmp / "tok" / "vocab.txt"), do_lower_case=True)
    tok.save_pretrained(str(tmp / "tok"))
    for c, folder in enumerate(FOLDERS):
        (tmp / "val" / folder).mkdir(parents=True)
        for k in range(4):
            (tmp / "val" / folder / f"{k}.png").write_bytes(I.png_bytes(I.noise_image(33 + 5 * k + c, 70 - 7 * k, 100 + 10 * c + k)))
    (tmp / "meta.json").write_text(json.dumps({"classnames": CLASSES, "templates": TEMPLATES, "folders": FOLDERS}))
    for s in range(2):
        members = []
        for k in range(6 * s, 6 * s + 6):
            caps = [f"w{k} w{(3 * k + j) % 20} w{(7 * k + 2 * j) % 20}" for j in range(2 + k % 2)]
            members += [(f"{k:04d}.png", I.png_bytes(I.noise_image(40 + k, 64 - 2 * k, 500 + k))),
                        (f"{k:04d}.json", json.dumps({"captions": caps}).encode())]
        I.write_tar(tmp / f"r{s}.tar", members)
    plain = {"train_args": {"learning_rate": 2e-3, "weight_decay": 0.01, "warmup_steps": 0, "grad_cache": False,
                            "schedule_type": "linear", "max_grad_norm": 1.0, "clamp_logits": True},
             "data_args": {"batch_size": 8, "seed": 7},
             "text_model_args": {"logit_scale": 20.0, "pooling": "mean", "model_name": "tiny-text", "seq_len": 24,
                                 "tokenizer_name": str(tmp / "tok")},
             "vision_model_args": {"logit_scale": 20.0, "pooling": "cls", "model_name": "tiny-vit", "trainable_logit_scale": True},
             "transforms": {"image_size": 32}}
    full = json.loads(json.dumps(plain))
    full["data_args"].update({"imagenet_val_path": str(tmp / "val"), "zeroshot_meta_path": str(tmp / "meta.json"),
                              "retrieval_eval_shards": f"{tmp}/r{{0..1}}.tar", "eval_batch_size": 5})
    return {"tmp": tmp, "tok": tok, "plain": plain, "full": full}


def _trainer(recipe, tok, **train_args):
    from contrastors_amd.config import Config
    from contrastors_amd.trainers import ImageTextTrainer

    recipe = json.loads(json.dumps(recipe))
    recipe["train_args"].update(train_args)
    tc, vc = _trunks()
    return ImageTextTrainer(Config(**recipe), torch.bfloat16, device="cuda", text_trunk_config=tc, vision_trunk_config=vc,
                            total_steps=20, tokenizer=tok)


@pytest.fixture(scope="module")
def trainer(world):
    return _trainer(world["full"], world["tok"])


def _batches(tok, n, seed=3):
    """A fixed synthetic stream of dense image / caption batches."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        texts = [" ".join(f"w{int(x)}" for x in torch.randint(0, 20, (3,), generator=g)) for _ in range(8)]
        t = tok(texts, padding="max_length", truncation=True, max_length=24, return_tensors="pt")
        out.append({"text": {"input_ids": t["input_ids"], "attention_mask": t["attention_mask"]},
                    "vision": {"input_ids": torch.randn(8, 3, 32, 32, generator=g).to(torch.bfloat16)}})
    return out


def test_classifier_weights_equal_the_per_class_padded_recomputation(world, trainer):
    from contrastors_amd.zeroshot import zeroshot_classifier_weights

    text, tok = trainer.model["model"].text, world["tok"]
    got = zeroshot_classifier_weights(text, tok, CLASSES, TEMPLATES, prefix="w7", seq_len=24, batch_size=4)
    assert got.shape == (3, 256) and got.dtype == torch.float32 and text.training
    text.eval()
    want = []
    with torch.no_grad():
        for c in CLASSES:     # the reference's loop: one padded-to-max batch per class
            t = tok([f"w7: {tpl.format(c)}" for tpl in TEMPLATES], padding="max_length", truncation=True, max_length=24,
                    return_tensors="pt")
            e = text(input_ids=t["input_ids"].to(DEV), attention_mask=t["attention_mask"].to(DEV))["embedding"].double()
            e = torch.nn.functional.normalize(e, dim=-1).mean(0)
            want.append(e / e.norm())
    text.train()
    err = float((got.double() - torch.stack(want)).abs().max())
    print(f"classifier: max |got - float64 recomputation| = {err:.3e}")
    assert float((got.norm(dim=1) - 1).abs().max()) < 1e-4
    assert err < 2e-3     # the bound of tests/test_search_gpu.py's encode test for the tower's bf16 embeddings


def test_evaluate_zeroshot_equals_dense_metrics(world, trainer):
    from contrastors_amd import zeroshot as zs

    model, tok = trainer.model["model"], world["tok"]
    transform, _ = trainer._eval_tools()
    ds, meta = trainer.get_eval_data()["imagenet"]
    assert ds.classes == FOLDERS and len(ds) == 12
    clf = zs.zeroshot_classifier_weights(model.text, tok, meta["classnames"], meta["templates"], seq_len=24)
    got = zs.evaluate_zeroshot(model, zs.zeroshot_loader(ds, batch_size=5), clf, transform, ks=(1, 2))
    assert model.text.training and model.vision.training and model.training
    # the same embeddings, the same batches: dense float64 metrics of their bf16 roundings
    embs, labels = [], []
    model.vision.eval()
    with torch.no_grad():
        for b in zs.zeroshot_loader(ds, batch_size=5):
            embs.append(zs._embed_vision(model.vision, transform, b["vision"]))
            labels.append(b["labels"])
    model.vision.train()
    S = R.scores64(torch.cat(embs).to(torch.bfloat16), clf.to(torch.bfloat16))
    want = R.dense_topk_hits(S, torch.cat(labels), ks=(1, 2))
    assert got["n"] == 12 and got["top1_acc"] == want[0] / 12 and got["top2_acc"] == want[1] / 12
    assert torch.cat(labels).tolist() == [0] * 4 + [1] * 4 + [2] * 4
    # two ranks' shares make up the whole: nothing is padded
    parts = [zs.evaluate_zeroshot(model, zs.zeroshot_loader(ds, batch_size=5, rank=r, world=2), clf, transform, ks=(1, 2))
             for r in range(2)]
    assert [p["n"] for p in parts] == [6, 6]


def test_evaluate_retrieval_equals_dense_metrics(world, trainer):
    from contrastors_amd import zeroshot as zs
    from contrastors_amd.search import encode

    model, tok = trainer.model["model"], world["tok"]
    transform, _ = trainer._eval_tools()
    ds = trainer.get_eval_data()["flickr"]
    got = zs.evaluate_retrieval(model, ds, tok, transform, seq_len=24, prefix="w9", batch_size=128)
    assert model.text.training and model.vision.training
    assert set(got) == {f"{d}_retrieval_recall@{k}" for d in ("image", "text") for k in (1, 5, 10)} | {"mean_recall@1"}
    samples = list(ds)
    caps = [f"w9: {c}" for _, cs in samples for c in cs]
    cap_img = torch.tensor([m for m, (_, cs) in enumerate(samples) for _ in cs])
    assert len(samples) == 12 and len(caps) == 30
    model.vision.eval()
    with torch.no_grad():
        img = zs._embed_vision(model.vision, transform, zs._vision_batch([im for im, _ in samples]))
    model.vision.train()
    txt = encode(model.text, caps, tok, batch_size=128, max_length=24)
    img, txt = img.to(torch.bfloat16), txt.to(torch.bfloat16)
    pos = torch.zeros(30, 12, dtype=torch.bool)
    pos[torch.arange(30), cap_img] = True
    want_i = R.dense_recall(R.scores64(txt, img), pos)
    want_t = R.dense_recall(R.scores64(img, txt), pos.T)
    for j, k in enumerate((1, 5, 10)):
        assert got[f"image_retrieval_recall@{k}"] == want_i[j] and got[f"text_retrieval_recall@{k}"] == want_t[j]
    assert got["mean_recall@1"] == 0.5 * (want_t[0] + want_i[0])


def test_eval_loop_logs_the_expected_keys(world, tmp_path):
    t = _trainer(world["full"], world["tok"], wandb=True, output_dir=str(tmp_path / "out"))
    metrics = t.eval_loop(3)
    rows = [json.loads(ln) for ln in (tmp_path / "out" / "metrics.jsonl").read_text().splitlines()]
    want = {"top1_acc", "top5_acc", "flickr/mean_recall@1"} | {f"flickr/{d}_retrieval_recall@{k}" for d in ("image", "text")
                                                                 for k in (1, 5, 10)}
    assert len(rows) == 1 and rows[0]["step"] == 3 and set(rows[0]) == want | {"step"} and set(metrics) == want
    assert all(0.0 <= rows[0][k] <= 1.0 for k in want) and rows[0]["top5_acc"] == 1.0      # three classes
    m = t.model["model"]
    assert m.training and m.text.training and m.vision.training


def test_eval_flickr_without_shards_warns_once(world, caplog):
    recipe = json.loads(json.dumps(world["plain"]))
    recipe["data_args"]["eval_flickr"] = True
    with caplog.at_level("WARNING"):
        t = _trainer(recipe, world["tok"])
    hits = [r for r in caplog.records if "retrieval_eval_shards" in r.getMessage()]
    assert len(hits) == 1 and t.get_eval_data() == {}
    assert t.eval_loop(0) == {}


def test_train_evaluates_every_eval_steps_and_leaves_the_loop_unchanged(world):
    """Losses are compared bit for bit between a hand-written loop of training_step calls (the loop of before), train() of a
    trainer without evaluation data and train() of one that evaluates after steps 2 and 4.  The text tower is frozen (the
    locked-text recipes' shape): with a TRAINED text tower training_step itself is not run-to-run reproducible on these
    trainers -- 3 of 12 identically built four-step runs gave 2.1886744 for 2.1886933 as the fourth loss, 12 of 12 agree with
    the tower frozen (its backward sums the word-embedding rows by fp32 atomics) -- which is not what this test
    is about."""
    tok = world["tok"]
    batches = _batches(tok, 4)
    plain_recipe, full_recipe = (json.loads(json.dumps(world[k])) for k in ("plain", "full"))
    plain_recipe["text_model_args"]["freeze"] = full_recipe["text_model_args"]["freeze"] = True
    # today's loop: training_step per batch
    a = _trainer(plain_recipe, tok)
    manual = [a.training_step(b).clone() for b in batches]
    # a trainer without evaluation data, through train(), with the steps strategy set: nothing to evaluate, the same losses
    b = _trainer(plain_recipe, tok, eval_strategy="steps", eval_steps=2)
    called = []
    b.eval_loop = lambda step: called.append(step)
    plain = b.train(iter(batches))
    print("manual", [float(x) for x in manual], "train()", [float(x) for x in plain])
    assert called == [] and all(torch.equal(x, y) for x, y in zip(manual, plain)) and len(plain) == 4
    # with evaluation data: eval_loop after optimizer steps 2 and 4, and training is not disturbed by it
    c = _trainer(full_recipe, tok, eval_strategy="steps", eval_steps=2)
    seen = []
    real = c.eval_loop

    def spy(step):
        seen.append(step)
        return real(step)

    c.eval_loop = spy
    with_eval = c.train(iter(batches))
    assert seen == [2, 4]
    assert all(torch.equal(x, y) for x, y in zip(manual, with_eval)), ([float(x) for x in manual], [float(x) for x in with_eval])


def test_tool_prints_the_trainers_numbers(world, trainer, tmp_path):
    want = trainer.evaluate()
    trainer.save_state(str(tmp_path / "ckpt"))
    cfg = tmp_path / "recipe.yaml"
    recipe = json.loads(json.dumps(world["plain"]))
    recipe["data_args"]["eval_batch_size"] = 5      # the trainer's batches: the same towers see the same batches
    cfg.write_text(yaml.safe_dump(recipe))
    r = subprocess.run([sys.executable, "-m", "contrastors_amd.tools.zeroshot_eval", "--config", str(cfg), "--checkpoint",
                        str(tmp_path / "ckpt"), "--imagenet_val_path", str(world["tmp"] / "val"), "--zeroshot_meta_path",
                        str(world["tmp"] / "meta.json"), "--retrieval_eval_shards", f"{world['tmp']}/r{{0..1}}.tar"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(got) == set(want)
    assert got == want, (got, want)
    r = subprocess.run([sys.executable, "-m", "contrastors_amd.tools.zeroshot_eval", "--config", str(cfg)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "nothing to evaluate" in r.stderr
