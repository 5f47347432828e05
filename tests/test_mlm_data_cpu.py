"""The MLM data path without a GPU (contrastors_amd/mlm_data.py): local datasets, the reference's split, the batch order, host
masking, the recipe's keys -- and the yardstick of the GPU tests, tests/mlm_mask_ref.py, proved on its own: against the
published Philox4x32-10 vectors, against planted errors, and for the rates the draw rule promises."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from contrastors_amd.config import Config, DataArgs, ModelArgs, TrainArgs, read_config
from contrastors_amd.mlm import mask_tokens
from contrastors_amd.mlm_data import (MlmBatchOrder, MlmTokenInfo, NpyTokens, get_mlm_loaders, load_tokenized_dataset,
                                      split_train_val)
from tests import mlm_mask_ref as mr
from tests.test_host_cpu import _recipe_path

INFO = MlmTokenInfo(mask_token_id=4, special_ids=(0, 1, 2, 3, 4), vocab_size=500)


def _tokens(n=64, s=32, seed=0):
    return np.random.default_rng(seed).integers(5, 500, (n, s), dtype=np.int64)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """A 64 x 32 corpus three ways: a Dataset directory (with both mask columns), a DatasetDict directory, a .npy."""
    import datasets

    root = tmp_path_factory.mktemp("mlm_corpus")
    ids = _tokens()
    lens = np.random.default_rng(1).integers(4, 33, 64)
    am = (np.arange(32)[None, :] < lens[:, None]).astype(np.int64)
    sm = np.zeros_like(am)
    sm[:, 0] = 1
    ds = datasets.Dataset.from_dict({"input_ids": ids.tolist(), "attention_mask": am.tolist(), "special_tokens_mask": sm.tolist(),
                                     "text_len": lens.tolist()})
    ds.save_to_disk(str(root / "ds"))
    datasets.DatasetDict({"train": ds.select(range(48)), "other": ds.select(range(48, 64))}).save_to_disk(str(root / "dd"))
    datasets.DatasetDict({"other": ds.select(range(8))}).save_to_disk(str(root / "dd_no_train"))
    ds.remove_columns(["input_ids"]).save_to_disk(str(root / "no_ids"))
    np.save(root / "tok.npy", ids.astype(np.int32))
    np.save(root / "bad.npy", ids.astype(np.float32))
    return {"root": root, "ids": ids, "am": am, "sm": sm}


def _config(path, batch_size=8, **data):
    return Config(train_args=TrainArgs(warmup_steps=0), model_args=ModelArgs(model_type="mlm", seq_len=32),
                  data_args=DataArgs(batch_size=batch_size, seed=5, tokenized_dataset=str(path), mlm_prob=0.3, **data))


# ---- dataset round trip ------------------------------------------------------------------------------------------------------------
def test_dataset_round_trip(corpus):
    root, ids = corpus["root"], corpus["ids"]
    ds = load_tokenized_dataset(str(root / "ds"))
    assert len(ds) == 64 and {"input_ids", "attention_mask", "special_tokens_mask"} <= set(ds.column_names)
    assert np.array_equal(np.asarray(ds["input_ids"]), ids)
    dd = load_tokenized_dataset(str(root / "dd"))
    assert len(dd) == 48 and np.array_equal(np.asarray(dd["input_ids"]), ids[:48])
    npy = load_tokenized_dataset(str(root / "tok.npy"))
    assert isinstance(npy, NpyTokens) and len(npy) == 64 and isinstance(npy.array, np.memmap)
    assert np.array_equal(npy.rows([3, 1])["input_ids"], ids[[3, 1]])
    # the loader hands out the columns the dataset has, stacked, in the dtypes the kernel takes
    batch = next(iter(get_mlm_loaders(_config(root / "ds"), INFO)["train"]))
    assert set(batch) == {"input_ids", "attention_mask", "special_tokens_mask"}
    assert (batch["input_ids"].dtype, batch["attention_mask"].dtype, batch["special_tokens_mask"].dtype) == (
        torch.int32, torch.int64, torch.uint8)
    assert all(tuple(v.shape) == (8, 32) for v in batch.values())
    batch = next(iter(get_mlm_loaders(_config(root / "tok.npy"), INFO)["train"]))
    assert set(batch) == {"input_ids"} and batch["input_ids"].dtype == torch.int32


def test_missing_path_and_missing_column(corpus, monkeypatch):
    root = corpus["root"]
    monkeypatch.setitem(sys.modules, "datasets", None)   # an import of `datasets` now raises: the check comes before it
    with pytest.raises(FileNotFoundError, match="local"):
        load_tokenized_dataset("nomic-ai/bert-pretokenized-2048-wiki-2023")
    with pytest.raises(FileNotFoundError):
        get_mlm_loaders(_config("nomic-ai/bert-pretokenized-2048-wiki-2023"), INFO)
    monkeypatch.undo()
    with pytest.raises(KeyError, match="input_ids"):
        load_tokenized_dataset(str(root / "no_ids"))
    with pytest.raises(KeyError, match="train"):
        load_tokenized_dataset(str(root / "dd_no_train"))
    with pytest.raises(ValueError, match="integer"):
        load_tokenized_dataset(str(root / "bad.npy"))


def test_no_code_path_resolves_a_name_remotely():
    src = (Path(__file__).resolve().parent.parent / "contrastors_amd" / "mlm_data.py").read_text()
    assert "load_dataset" not in src and "load_from_disk" in src


# ---- split -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("val_pct", [0.01, 0.1, 0.25])
def test_split_is_the_references_own(corpus, val_pct):
    ds = load_tokenized_dataset(str(corpus["root"] / "ds"))
    train, val = split_train_val(ds, val_pct, seed=42)
    want = ds.shuffle(seed=42).train_test_split(test_size=val_pct, seed=42)   # sc/trainers/mlm.py:59-60
    assert train["input_ids"] == want["train"]["input_ids"] and val["input_ids"] == want["test"]["input_ids"]
    assert (len(train), len(val)) == (len(want["train"]), len(want["test"])) and len(val) == math.ceil(val_pct * 64)
    rows = [tuple(r) for r in train["input_ids"]] + [tuple(r) for r in val["input_ids"]]
    assert len(rows) == 64 and set(rows) == {tuple(r) for r in corpus["ids"].tolist()}   # disjoint and exhaustive


def test_split_of_the_npy_source_and_no_validation(corpus):
    npy = load_tokenized_dataset(str(corpus["root"] / "tok.npy"))
    train, val = split_train_val(npy, 0.1, seed=42)
    assert (len(train), len(val)) == (64 - 7, 7)
    assert sorted(np.concatenate([train.indices, val.indices]).tolist()) == list(range(64))
    again = split_train_val(npy, 0.1, seed=42)
    assert np.array_equal(again[0].indices, train.indices) and not np.array_equal(split_train_val(npy, 0.1, 43)[0].indices, train.indices)
    for none in (None, 0, 0.0):
        assert split_train_val(npy, none, 42)[1] is None
        tr, va = split_train_val(load_tokenized_dataset(str(corpus["root"] / "ds")), none, 42)
        assert va is None and len(tr) == 64
    assert get_mlm_loaders(_config(corpus["root"] / "ds"), INFO)["val"] is None
    val_loader = get_mlm_loaders(_config(corpus["root"] / "ds", val_pct=0.25, eval_batch_size=4), INFO)["val"]
    batches = list(val_loader)
    assert len(batches) == 4 and batches[0]["input_ids"].shape == (4, 32)
    want = load_tokenized_dataset(str(corpus["root"] / "ds")).shuffle(seed=5).train_test_split(test_size=0.25, seed=5)["test"]
    assert np.array_equal(torch.cat([b["input_ids"] for b in batches]).numpy(), np.asarray(want["input_ids"]))   # unshuffled


# ---- order -------------------------------------------------------------------------------------------------------------------------
def _epoch(path, rank=0, world=1, epoch=0, start_batch=0, **kw):
    return [b["input_ids"].numpy() for b in get_mlm_loaders(_config(path, **kw), INFO, rank, world, epoch, start_batch)["train"]]


def test_batch_order_is_a_function_of_seed_and_epoch(corpus):
    path = corpus["root"] / "tok.npy"
    a, b = _epoch(path), _epoch(path, workers=2)
    assert len(a) == 8 and all(np.array_equal(x, y) for x, y in zip(a, b))     # the same (seed, epoch), any worker count
    other = _epoch(path, epoch=1)
    assert not all(np.array_equal(x, y) for x, y in zip(a, other))
    rows = lambda bs: sorted(tuple(r) for b in bs for r in b)
    assert rows(a) == rows(other) == sorted(tuple(r) for r in corpus["ids"].astype(np.int32))
    tail = _epoch(path, start_batch=3)
    assert len(tail) == 5 and all(np.array_equal(x, y) for x, y in zip(tail, a[3:]))
    assert _epoch(path, start_batch=8) == []
    # set_epoch on a live loader: what fit() does between epochs and on a resume
    loader = get_mlm_loaders(_config(path), INFO)["train"]
    loader.batch_sampler.set_epoch(1, 6)
    got = [b["input_ids"].numpy() for b in loader]
    assert len(got) == 2 and all(np.array_equal(x, y) for x, y in zip(got, other[6:]))


def test_start_batch_skips_without_reading(corpus):
    order = MlmBatchOrder(64, 8, seed=5, start_batch=5)
    assert len(order) == 3 and order.num_batches == 8
    first = next(iter(order))
    assert first == MlmBatchOrder(64, 8, seed=5).indices()[40:48].tolist()


def test_two_ranks_are_disjoint_and_cover_the_epoch(corpus):
    path = corpus["root"] / "tok.npy"
    r0, r1 = _epoch(path, 0, 2), _epoch(path, 1, 2)
    assert len(r0) == len(r1) == 8 and r0[0].shape == (4, 32)   # per-rank batch = batch_size // world
    rows = [tuple(r) for b in r0 + r1 for r in b]
    assert len(set(rows)) == 64 == len(rows)
    # sharded as DistributedSampler shards the same permutation; with drop_last the tail that fills no batch is left out
    from torch.utils.data import DistributedSampler

    ds = DistributedSampler(range(60), num_replicas=2, rank=1, shuffle=True, seed=5)
    ds.set_epoch(3)
    order = MlmBatchOrder(60, 4, rank=1, world=2, seed=5, epoch=3)
    assert order.indices().tolist() == list(ds)
    assert [i for b in order for i in b] == list(ds)[:28] and order.num_batches == 7


# ---- host masking ------------------------------------------------------------------------------------------------------------------
def test_host_masking_is_the_references_collator(corpus):
    cfg = _config(corpus["root"] / "ds", mask_on="host")
    it = iter(get_mlm_loaders(cfg, INFO)["train"])   # (a DataLoader iterator draws its base seed from the global generator)
    torch.manual_seed(11)
    batches = list(it)                                 # workers = 0: the collate runs here, on the global generator
    raw = list(get_mlm_loaders(_config(corpus["root"] / "ds"), INFO)["train"])
    torch.manual_seed(11)
    for got, src in zip(batches, raw):
        ids, labels = mask_tokens(src["input_ids"].long(), src["special_tokens_mask"].bool(), 0.3, INFO.mask_token_id, INFO.vocab_size)
        assert set(got) == {"input_ids", "attention_mask", "labels"}
        assert torch.equal(got["input_ids"], ids) and torch.equal(got["labels"], labels)
        assert torch.equal(got["attention_mask"], src["attention_mask"])
    # without the column the specials come from the tokenizer's ids
    info = MlmTokenInfo(4, (0, 1, 2, 3, 4, int(corpus["ids"][0, 0])), 500)
    it = iter(get_mlm_loaders(_config(corpus["root"] / "tok.npy", mask_on="host"), info)["train"])
    torch.manual_seed(2)
    got = next(it)
    src = next(iter(get_mlm_loaders(_config(corpus["root"] / "tok.npy"), info)["train"]))["input_ids"].long()
    torch.manual_seed(2)
    ids, labels = mask_tokens(src, torch.isin(src, torch.tensor(info.special_ids)), 0.3, 4, 500)
    assert torch.equal(got["input_ids"], ids) and torch.equal(got["labels"], labels)


def test_token_info_from_a_tokenizer():
    class Tok:
        mask_token_id, all_special_ids = 103, [100, 102, 0, 101, 103]

        def __len__(self):
            return 30522

    assert MlmTokenInfo.from_tokenizer(Tok()) == MlmTokenInfo(103, (100, 102, 0, 101, 103), 30522)
    with pytest.raises(ValueError):
        MlmTokenInfo(None, (), 10)


# ---- config ------------------------------------------------------------------------------------------------------------------------
def test_recipe_keeps_its_data_block(tmp_path):
    cfg = read_config(str(_recipe_path("mlm.yaml", tmp_path)))
    da = cfg.data_args
    assert da.tokenized_dataset == "nomic-ai/bert-pretokenized-2048-wiki-2023"
    assert da.val_pct == 0.01 and da.val_mlm_prob == 0.15 and da.mlm_prob == 0.30 and da.mask_on == "device"
    with pytest.raises(ValueError, match="mask_on"):
        DataArgs(mask_on="gpu")
    assert DataArgs(mask_on="host").mask_on == "host"
    from contrastors_amd.train import apply_overrides

    cfg = apply_overrides(cfg, {"tokenized_dataset": "/data/wiki", "val_pct": "0.05", "mask_on": "host"})
    assert (cfg.data_args.tokenized_dataset, cfg.data_args.val_pct, cfg.data_args.mask_on) == ("/data/wiki", 0.05, "host")


# ---- the draw-rule yardstick -------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = mr.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)
        assert tuple(int(g[0]) for g in got) == want
    assert int(mr.threshold(0.0)) == 0 and int(mr.threshold(0.8)) == 13421773 * 256 and int(mr.threshold(0.9)) == 15099494 * 256
    assert int(mr.threshold(0.99999999)) == 4294967040   # the clamp: p rounds to 1.0f


SEED, OFFSET = 20240521, (7 << 32) + 3


def _rate_case():
    rng = np.random.default_rng(0)
    ids = rng.integers(1000, 30000, (64, 2048), dtype=np.int64)
    special = rng.random((64, 2048)) < 0.10
    return ids, special.astype(np.uint8)


def _shares(ids, special, out, labels, mask_id=103):
    target = labels != -100
    assert not (target & (special != 0)).any() and np.array_equal(labels[target], ids[target])
    assert np.array_equal(out[~target], ids[~target])
    n_free, n_t = int((special == 0).sum()), int(target.sum())
    masked = int((out[target] == mask_id).sum())
    kept = int((out[target] == ids[target]).sum())
    return n_free, n_t, masked, n_t - masked - kept, kept


def _within_six_sigma(count, n, q):
    return abs(count - n * q) <= 6.0 * math.sqrt(n * q * (1.0 - q))


def test_rates_of_the_rule_at_a_fixed_seed():
    """Targets among the non-specials and the mask / random / keep shares among the targets: each within 6 sigma of the binomial
    expectation for the actual counts.  The seed is fixed, so this is a property of the restatement, not a chance event.  (A
    random word equals the original id with probability 1 / 30522: 0.1 such tokens expected here, far inside the bound.)"""
    ids, special = _rate_case()
    out, labels = mr.mlm_mask(ids, 0.3, SEED, OFFSET, 103, 30522, special_mask=special)
    n_free, n_t, masked, rand, kept = _shares(ids, special, out, labels)
    assert 0.88 * ids.size < n_free < 0.92 * ids.size
    assert _within_six_sigma(n_t, n_free, 0.3), (n_t, n_free)
    assert _within_six_sigma(masked, n_t, 0.8) and _within_six_sigma(rand, n_t, 0.1) and _within_six_sigma(kept, n_t, 0.1), (
        n_t, masked, rand, kept)
    words = out[(labels != -100) & (out != 103) & (out != ids)]
    assert words.min() >= 0 and words.max() < 30522 and words.max() > 30000 and words.min() < 500   # the whole range is drawn


def test_planted_errors_are_caught():
    ids, special = _rate_case()
    good = mr.mlm_mask(ids, 0.3, SEED, OFFSET, 103, 30522, special_mask=special)
    for flaw in ("counter", "swap", "split"):
        bad = mr.mlm_mask(ids, 0.3, SEED, OFFSET, 103, 30522, special_mask=special, flaw=flaw)
        assert not (np.array_equal(bad[0], good[0]) and np.array_equal(bad[1], good[1])), flaw
    # 0.9 for 0.8 also leaves the rates: the mask share is 0.9, no random word is drawn
    _, n_t, masked, rand, _ = _shares(ids, special, *mr.mlm_mask(ids, 0.3, SEED, OFFSET, 103, 30522, special_mask=special, flaw="split"))
    assert not _within_six_sigma(masked, n_t, 0.8) and rand == 0
    # the result is a function of (seed, offset): either one changed gives other masks; neither changed gives the same
    again = mr.mlm_mask(ids, 0.3, SEED, OFFSET, 103, 30522, special_mask=special)
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    for seed, off in ((SEED + 1, OFFSET), (SEED, OFFSET + 1), (SEED, OFFSET & 0xFFFFFFFF), (SEED + (1 << 32), OFFSET)):
        assert not np.array_equal(mr.mlm_mask(ids[:2], 0.3, seed, off, 103, 30522)[1], mr.mlm_mask(ids[:2], 0.3, SEED, OFFSET, 103, 30522)[1])


def test_specialness_sources_and_edge_probabilities():
    ids = _tokens(4, 64)
    am = np.ones_like(ids)
    am[1, 10:] = 0
    am[2] = 0
    sm = np.zeros(ids.shape, np.uint8)
    sm[:, 0] = 7
    special_ids = [int(ids[0, 5]), int(ids[3, 9])]
    out, labels = mr.mlm_mask(ids, 0.999, 1, 2, 4, 500, attention_mask=am, special_mask=sm, special_ids=special_ids)
    sp = (am == 0) | (sm != 0) | np.isin(ids, special_ids)
    assert (labels[sp] == -100).all() and np.array_equal(out[sp], ids[sp]) and (labels[~sp] != -100).mean() > 0.98
    out, labels = mr.mlm_mask(ids, 0.0, 1, 2, 4, 500)
    assert (labels == -100).all() and np.array_equal(out, ids)
    out, _ = mr.mlm_mask(ids.astype(np.int32), 0.5, 1, 2, 4, 2)
    assert out.dtype == np.int64 and set(np.unique(out[(out != ids) & (out != 4)]).tolist()) <= {0, 1}
