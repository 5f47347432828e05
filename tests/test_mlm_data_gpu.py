"""The MLM data path on the GPU: `cx_mlm_mask` against the numpy restatement of its draw rule (tests/mlm_mask_ref.py, proved in
tests/test_mlm_data_cpu.py) element for element, `GpuMlmMasker`, and `MLMTrainer.fit` / `eval_loop` / `save_state` / `load_state`
over a local corpus, up to the command line."""
import functools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from contrastors_amd import _C
from contrastors_amd.config import Config, DataArgs, ModelArgs, TrainArgs
from contrastors_amd.mlm_data import GpuMlmMasker, MlmTokenInfo, get_mlm_loaders, mlm_mask
from contrastors_amd.nomic_bert import NomicBertConfig
from contrastors_amd.trainers import TRAINER_REGISTRY
from oracle.make_golden import TINY_NOMIC
from tests import mlm_mask_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parent.parent

# (1030, 2048): 1030 * 512 = 527360 groups of four tokens > 2048 blocks * 256 lanes = 524288 -- the grid-stride loop runs
SHAPES = [(1, 1), (3, 341), (1, 1024), (1, 1025), (7, 129), (64, 2048), (1030, 2048)]
SEEDS = {"lo": (1234, 77), "hi": ((0xABCD << 32) + 99, (5 << 32) + 12345)}   # the second: seed and offset above 2^32
# every value of every variant the kernel serves appears in one of these; each runs on every shape, as int32 and int64 ids with
# row stride S and S + 3
CASES = {
    "plain":        dict(rng="lo", attn=False, spec=False, n_special=0,  p=0.3,  vocab=30522),
    "all_masks":    dict(rng="hi", attn=True,  spec=True,  n_special=16, p=0.15, vocab=250002),
    "no_targets":   dict(rng="lo", attn=True,  spec=False, n_special=1,  p=0.0,  vocab=2),
    "two_words":    dict(rng="hi", attn=False, spec=True,  n_special=1,  p=0.3,  vocab=2),
    "recipe":       dict(rng="lo", attn=True,  spec=True,  n_special=16, p=0.3,  vocab=30522),
    "recipe_val":   dict(rng="hi", attn=True,  spec=False, n_special=0,  p=0.15, vocab=30522),
}
MASK_ID = 103


@functools.lru_cache(maxsize=None)
def _draws(n, rng):
    """The Philox words of n flat positions under one of the two (seed, offset) pairs: computed once, shared, never changed."""
    u = mr.draws(n, *SEEDS[rng])
    for x in u:
        x.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def _inputs(B, S):
    rng = np.random.default_rng(B * 100003 + S)
    ids = rng.integers(0, 30522, (B, S), dtype=np.int64)
    lens = rng.integers(0, S + 1, B)
    lens[0] = S                      # a full row ...
    if B > 1:
        lens[1] = 0                  # ... and an empty one
    else:
        lens[0] = S // 2 if S > 1 else 1
    attn = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    spec = (rng.random((B, S)) < 0.1).astype(np.uint8) * rng.integers(1, 256, (B, S)).astype(np.uint8)   # any non-zero byte counts
    special_ids = rng.choice(30522, 16, replace=False).astype(np.int64)
    special_ids[:4] = ids.flatten()[: 4]    # some that do occur
    for a in (ids, attn, spec, special_ids):
        a.setflags(write=False)
    return ids, attn, spec, special_ids


def _device_ids(ids, dtype, pad):
    B, S = ids.shape
    buf = torch.full((B, S + pad), -7, dtype=dtype, device=DEV)
    buf[:, :S] = torch.tensor(ids).to(DEV, dtype)
    view = buf[:, :S]
    assert view.stride(0) == S + pad or B == 1
    return view


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement(shape, case):
    c = CASES[case]
    B, S = shape
    ids, attn, spec, special_ids = _inputs(B, S)
    seed, offset = SEEDS[c["rng"]]
    am, sm, sids = (attn if c["attn"] else None), (spec if c["spec"] else None), special_ids[: c["n_special"]]
    want_ids, want_labels = mr.mlm_mask(ids, c["p"], seed, offset, MASK_ID, c["vocab"], am, sm, sids, u=_draws(B * S, c["rng"]))
    special = mr.specialness(ids, am, sm, sids)
    assert (want_labels[special] == -100).all()
    d_am = None if am is None else torch.tensor(am).to(DEV)
    d_sm = None if sm is None else torch.tensor(sm).to(DEV)
    d_sids = torch.from_numpy(sids.copy()).to(DEV)
    first = None
    for dtype in (torch.int32, torch.int64):
        for pad in (0, 3):
            src = _device_ids(ids, dtype, pad)
            keep = src.clone()
            out, labels = mlm_mask(src, c["p"], seed, offset, MASK_ID, c["vocab"], d_am, d_sm, d_sids)
            assert out.dtype == labels.dtype == torch.int64 and out.is_contiguous() and labels.is_contiguous()
            assert torch.equal(src, keep)                                               # the input is read only
            got_ids, got_labels = out.cpu().numpy(), labels.cpu().numpy()
            bad = int((got_ids != want_ids).sum()), int((got_labels != want_labels).sum())
            assert bad == (0, 0), (str(dtype), pad, bad)
            assert (got_labels[special] == -100).all() and np.array_equal(got_ids[special], ids[special])   # specials: never targets
            if first is None:
                first = (out, labels)
                again = mlm_mask(src, c["p"], seed, offset, MASK_ID, c["vocab"], d_am, d_sm, d_sids)   # two calls: identical bits
                assert torch.equal(again[0], out) and torch.equal(again[1], labels)
            else:   # the same logical input in another dtype / stride
                assert torch.equal(out, first[0]) and torch.equal(labels, first[1])
    if c["p"] == 0.0:
        assert (want_labels == -100).all()
    elif B * S >= 1024 and not c["attn"]:
        assert (want_labels != -100).any()


def test_result_depends_on_seed_and_offset_only_through_the_rule():
    ids, _, _, _ = _inputs(7, 129)
    src = torch.tensor(ids).to(DEV)
    base = mlm_mask(src, 0.3, 5, 6, MASK_ID, 30522)
    for seed, offset in ((6, 6), (5, 7), (5 + (1 << 32), 6), (5, 6 + (1 << 32))):
        out, labels = mlm_mask(src, 0.3, seed, offset, MASK_ID, 30522)
        want = mr.mlm_mask(ids, 0.3, seed, offset, MASK_ID, 30522)
        assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(labels.cpu().numpy(), want[1])
        assert not torch.equal(labels, base[1])


def test_refused_arguments():
    lib, s = _C.lib(), _C.cur_stream()
    ids = torch.zeros(4, 8, dtype=torch.int32, device=DEV)
    out, labels = torch.zeros(4, 8, dtype=torch.int64, device=DEV), torch.full((4, 8), 5, dtype=torch.int64, device=DEV)
    sids = torch.zeros(17, dtype=torch.int64, device=DEV)

    def call(B=4, S=8, n_special=0, vocab=30522, p=0.3, stride=8, ids_ptr=ids.data_ptr(), sids_ptr=sids.data_ptr()):
        return lib.cx_mlm_mask(ids_ptr, 0, stride, None, None, sids_ptr, n_special, MASK_ID, vocab, p, 1, 2, out.data_ptr(),
                               labels.data_ptr(), B, S, s)

    SHAPE, ARG = -1, -3
    assert call() == 0
    for kw in (dict(B=0), dict(S=0), dict(B=-1), dict(n_special=17), dict(n_special=-1), dict(vocab=0), dict(p=1.0), dict(p=-0.01),
               dict(p=float("nan")), dict(p=1.5), dict(stride=7)):
        labels.fill_(5)
        assert call(**kw) == SHAPE, kw
        torch.cuda.synchronize()
        assert bool((labels == 5).all()), kw                     # nothing was launched
    assert call(ids_ptr=None) == ARG and call(n_special=1, sids_ptr=None) == ARG
    assert call(n_special=16) == 0 and call(p=0.0) == 0 and call(vocab=1) == 0
    with pytest.raises(ValueError):
        mlm_mask(ids.float(), 0.3, 1, 2, MASK_ID, 30522)
    with pytest.raises(ValueError):
        mlm_mask(ids.t(), 0.3, 1, 2, MASK_ID, 30522)
    with pytest.raises(ValueError):
        mlm_mask(ids, 0.3, 1, 2, MASK_ID, 30522, attention_mask=torch.ones(4, 8, dtype=torch.int32, device=DEV))


# ---- the masker ------------------------------------------------------------------------------------------------------------------
INFO = MlmTokenInfo(mask_token_id=4, special_ids=(0, 1, 2, 3, 4), vocab_size=500)


def _batch(seed=0, B=16, S=32):
    rng = np.random.default_rng(seed)
    ids = rng.integers(5, 500, (B, S)).astype(np.int32)
    lens = rng.integers(S // 2, S + 1, B)
    am = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    ids[:, 0] = 2
    ids = ids * am.astype(np.int32)
    return {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(am)}


def test_masker_offsets():
    batch = _batch()
    m = GpuMlmMasker(INFO, 0.3, seed=9)
    a = m(batch, ordinal=3, rank=1, world=4)
    assert set(a) == {"input_ids", "attention_mask", "labels"} and all(v.is_cuda for v in a.values())
    want = mr.mlm_mask(batch["input_ids"].numpy(), 0.3, 9, 3 * 4 + 1, 4, 500, batch["attention_mask"].numpy(), None, INFO.special_ids)
    assert np.array_equal(a["input_ids"].cpu().numpy(), want[0]) and np.array_equal(a["labels"].cpu().numpy(), want[1])
    assert torch.equal(a["attention_mask"].cpu(), batch["attention_mask"])
    lab = a["labels"].cpu()
    assert bool((lab[batch["attention_mask"] == 0] == -100).all()) and bool((lab[:, 0] == -100).all()) and bool((lab != -100).any())
    same = m(batch, ordinal=3, rank=1, world=4)
    assert torch.equal(same["labels"], a["labels"]) and torch.equal(same["input_ids"], a["input_ids"])
    for ordinal, rank in ((4, 1), (3, 2), (3, 0)):
        assert not torch.equal(m(batch, ordinal, rank, 4)["labels"], a["labels"])
    assert torch.equal(m(batch, 0, 13, 16)["labels"], a["labels"])     # offset = ordinal * world + rank, nothing else
    assert not torch.equal(GpuMlmMasker(INFO, 0.3, seed=10)(batch, 3, 1, 4)["labels"], a["labels"])
    with pytest.raises(ValueError):
        GpuMlmMasker(MlmTokenInfo(4, tuple(range(17)), 500), 0.3, 1)


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
def _corpus(path):
    """256 x 32 with a planted regularity: row r is the arithmetic progression a_r + 3 s over 40 words (a masked token follows
    from its neighbours), [CLS] = 2 in front, ragged tails padded with 0."""
    rng = np.random.default_rng(3)
    ids = 10 + (rng.integers(0, 40, (256, 1)) + 3 * np.arange(32)[None, :]) % 40
    lens = rng.integers(24, 33, 256)
    am = (np.arange(32)[None, :] < lens[:, None]).astype(np.int64)
    ids[:, 0] = 2
    ids = ids * am
    import datasets

    datasets.Dataset.from_dict({"input_ids": ids.tolist(), "attention_mask": am.tolist()}).save_to_disk(str(path))
    return str(path)


def _trainer(data_path, out_dir=None, **train):
    kw = dict(learning_rate=2e-3, weight_decay=1e-5, warmup_steps=0, schedule_type="linear", max_grad_norm=1.0, adam_beta2=0.98,
              eps=1e-6, clamp_logits=False, num_epochs=2, output_dir=out_dir)
    kw.update(train)
    cfg = Config(train_args=TrainArgs(**kw),
                 data_args=DataArgs(batch_size=32, seed=3, tokenized_dataset=data_path, val_pct=0.125, mlm_prob=0.3, val_mlm_prob=0.15),
                 model_args=ModelArgs(model_type="mlm", seq_len=64))
    tc = NomicBertConfig(**{k: v for k, v in TINY_NOMIC.items() if k in NomicBertConfig.__dataclass_fields__})
    return TRAINER_REGISTRY["mlm"](cfg, torch.bfloat16, device=DEV, trunk_config=tc, total_steps=40), cfg


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return _corpus(tmp_path_factory.mktemp("mlm") / "corpus")


def test_fit_learns_evaluates_and_logs(corpus, tmp_path):
    import json

    t, cfg = _trainer(corpus, str(tmp_path / "out"), eval_strategy="epochs", wandb=True, log_lr_every=3)
    loaders = get_mlm_loaders(cfg, INFO)
    assert len(loaders["train"]) == 7 and len(loaders["val"]) == 1          # 224 / 32 and 32 / 32
    losses = [float(l) for l in t.fit(loaders)]
    assert len(losses) == 14 and t.step == 14 and t.ordinal == 14 and t.total_steps == 14
    assert t.scheduler.last_epoch == 14 and abs(t.scheduler.get_last_lr()[0]) < 1e-12     # the horizon is len(train) * num_epochs
    assert np.isfinite(losses).all() and losses[-1] < losses[0] - 0.3, (losses[0], losses[-1])
    rows = [json.loads(ln) for ln in (tmp_path / "out" / "metrics.jsonl").read_text().splitlines()]
    evals = [r for r in rows if "val_loss" in r]
    assert [r["step"] for r in evals] == [6, 13]                                # one pair per epoch, at the epoch's last curr_step
    assert all(r["val_ppl"] == math.exp(r["val_loss"]) for r in evals) and evals[1]["val_loss"] < evals[0]["val_loss"]
    assert [r["step"] for r in rows if "loss" in r] == list(range(14))
    assert [r["step"] for r in rows if "lr" in r] == [3, 6, 10, 13]             # steps 3 and 6 of each epoch (base.py:513-515)
    # two evaluations without a step in between: the same masks, the same number
    a = t.eval_loop(loaders["val"], 14)
    b = t.eval_loop(loaders["val"], 14)
    assert math.isfinite(a["val_loss"]) and a["val_ppl"] == math.exp(a["val_loss"]) and a == b
    assert a["val_loss"] == evals[1]["val_loss"]                                # ... and the one fit() logged after its last step
    assert t.model["model"].training


def test_eval_every_n_steps_prints_without_a_tracker(corpus, capsys):
    t, cfg = _trainer(corpus, None, eval_strategy="steps", eval_steps=3, num_epochs=1)
    t.fit(get_mlm_loaders(cfg, INFO))
    out = capsys.readouterr().out
    assert out.count("val_loss") == 2 and out.count("val_ppl") == 2             # after steps 3 and 6 of 0 .. 6
    assert t.tracker is None


def _record(trainer):
    seen = []
    step = trainer.training_step

    def spy(batch):
        seen.append((batch["input_ids"].clone(), batch["labels"].clone()))
        return step(batch)

    trainer.training_step = spy
    return seen


def test_checkpoint_and_resume(corpus, tmp_path):
    """save_every = 4 writes step_4 after the micro-batch with curr_step 4 (base.py:517-518), i.e. with five micro-batches done; a
    fresh trainer pointed at it restores parameters and optimizer state bit for bit and then sees, from curr_step 5 to the end of
    the second epoch, the masked batches of the uninterrupted run."""
    out = tmp_path / "run"
    a, cfg = _trainer(corpus, str(out), save_every=4)
    seen_a = _record(a)
    snap = {}
    save = a.save_state

    def save_and_snapshot(d):
        save(d)
        m = a.model["model"]
        snap[Path(d).name] = dict(flat=m.bert.flat_param.clone(), head=[p.detach().clone() for p in m.head_parameters()],
                                  opt=[{k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()}
                                       for s in a.optimizer.state.values()], lr=a.scheduler.get_last_lr()[0])

    a.save_state = save_and_snapshot
    a.fit(get_mlm_loaders(cfg, INFO))
    assert len(seen_a) == 14
    names = sorted(p.name for p in out.iterdir())
    assert names == ["epoch_0", "epoch_0_model", "epoch_1", "epoch_1_model", "final_model", "step_11", "step_4"], names
    assert sorted(p.name for p in (out / "step_4").iterdir()) == ["model", "optimizer.pt", "scheduler.pt", "trainer_state.pt"]
    assert (out / "step_4" / "model" / "model.safetensors").exists() and (out / "final_model" / "model.safetensors").exists()
    st = torch.load(str(out / "step_4" / "trainer_state.pt"))
    assert st == {"step": 5, "ordinal": 5, "epoch": 0, "batch_in_epoch": 5}
    assert torch.load(str(out / "epoch_0" / "trainer_state.pt")) == {"step": 7, "ordinal": 7, "epoch": 0, "batch_in_epoch": 7}

    b, cfg_b = _trainer(corpus, str(tmp_path / "resumed"), save_every=100, checkpoint=str(out / "step_4"))
    b.set_total_steps(14)
    b.load_state(str(out / "step_4"))
    want, m = snap["step_4"], b.model["model"]
    assert torch.equal(m.bert.flat_param, want["flat"])
    assert all(torch.equal(p, q) for p, q in zip(m.head_parameters(), want["head"]))
    got_opt = list(b.optimizer.state.values())
    assert len(got_opt) == len(want["opt"]) > 0
    for s, w in zip(got_opt, want["opt"]):
        assert s.keys() == w.keys()
        for k in w:
            assert torch.equal(s[k].cpu(), w[k].cpu()) if torch.is_tensor(w[k]) else s[k] == w[k], k
    assert (b.step, b.ordinal, b.epoch, b.batch_in_epoch) == (5, 5, 0, 5) and b.scheduler.get_last_lr()[0] == want["lr"]

    c, cfg_c = _trainer(corpus, str(tmp_path / "resumed"), save_every=100, checkpoint=str(out / "step_4"))
    seen_c = _record(c)
    c.fit(get_mlm_loaders(cfg_c, INFO))
    assert len(seen_c) == 9 and c.step == 14 and c.ordinal == 14
    for (ids_c, lab_c), (ids_a, lab_a) in zip(seen_c, seen_a[5:]):
        assert torch.equal(ids_c, ids_a) and torch.equal(lab_c, lab_a)
    # from the end of an epoch: the next epoch's first batch
    d, cfg_d = _trainer(corpus, str(tmp_path / "resumed2"), save_every=100, checkpoint=str(out / "epoch_0"))
    seen_d = _record(d)
    d.fit(get_mlm_loaders(cfg_d, INFO))
    assert len(seen_d) == 7 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(seen_d, seen_a[7:]))


def test_host_masked_batches_train_too(corpus):
    t, cfg = _trainer(corpus, None, num_epochs=1, eval_strategy="epochs")
    cfg.data_args.mask_on = "host"
    losses = t.fit(get_mlm_loaders(cfg, INFO))
    assert len(losses) == 7 and all(torch.isfinite(l) for l in losses) and t.masker is None and t.eval_masker is None


# ---- the command line ------------------------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(45)]


def _cli(tmp_path, *extra):
    import yaml
    from transformers import BertTokenizer

    tok_dir = tmp_path / "tok"
    if not tok_dir.exists():
        (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
        BertTokenizer(str(tmp_path / "vocab.txt"), do_lower_case=True).save_pretrained(str(tok_dir))
        _corpus(tmp_path / "corpus")
        cfg = {"train_args": {"num_epochs": 1, "learning_rate": 5.0e-4, "weight_decay": 1e-5, "warmup_pct": 0.06,
                              "schedule_type": "linear", "max_grad_norm": 0.0, "adam_beta2": 0.98, "eps": 1e-6, "wandb": False,
                              "eval_strategy": "epochs", "save_every": 1000, "output_dir": str(tmp_path / "ckpts")},
               "model_args": {"model_type": "mlm", "seq_len": 32, "tokenizer_name": str(tok_dir), "model_name": "bert-base-uncased",
                              "rotary_emb_fraction": 1.0, "rotary_emb_base": 500000, "pad_vocab_to_multiple_of": 64,
                              "activation_function": "swiglu", "qkv_proj_bias": False, "mlp_fc1_bias": False, "mlp_fc2_bias": False,
                              "attn_pdrop": 0.0},
               "data_args": {"workers": 0, "batch_size": 64, "seed": 42, "shuffle": True, "mlm_prob": 0.3, "val_mlm_prob": 0.15,
                             "val_pct": 0.25}}
        (tmp_path / "mlm.yaml").write_text(yaml.safe_dump(cfg))
    return subprocess.run([sys.executable, "-m", "contrastors_amd.train", "--config", str(tmp_path / "mlm.yaml"), *extra],
                          cwd=str(ROOT), capture_output=True, text=True, timeout=600)


def test_train_cli_trains_from_a_tokenized_dataset(tmp_path):
    """The recipe's architecture keys (its trunk is bert-base geometry; the rows are 32 tokens), a tokenizer saved locally, a local
    dataset directory given on the command line: three micro-batches, one evaluation, epoch_0_model."""
    out = _cli(tmp_path, "--synthetic-steps", "0", "--tokenized_dataset", str(tmp_path / "corpus"))
    assert out.returncode == 0, out.stderr[-3000:]
    assert "val_loss" in out.stdout and "val_ppl" in out.stdout, out.stdout[-2000:]
    assert (tmp_path / "ckpts" / "epoch_0_model" / "model.safetensors").exists()


def test_train_cli_synthetic_path_is_unchanged(tmp_path):
    out = _cli(tmp_path, "--synthetic-steps", "2", "--seq-len", "32", "--batch_size", "8", "--tokenized_dataset", str(tmp_path / "corpus"))
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.count("loss") >= 2 and "val_loss" not in out.stdout and not (tmp_path / "ckpts").exists()
