"""Host side of the image-text data path, no GPU: the transform's arithmetic (tests/img_ref.py, the yardstick the GPU test
holds the kernel to) against PIL's BICUBIC; the crop sampler and the plans; the tar loader; the config keys.

Yardstick against PIL, per case: no value differs by more than 1 level and at most 0.2 % of the case's values differ (the form
was measured at <= 1 value per case, <= 0.04 %).  Each error planted through img_ref's switches has to break that condition on
at least one case: the condition, on these inputs, tells the contract from its near misses.
"""
import logging
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import img_ref as R

ROOT = Path(__file__).resolve().parent.parent
ERR_SHAPE, ERR_ARG = -1, -3
SOURCES = [(9, 13), (33, 32), (40, 40), (61, 83), (83, 61), (500, 37), (300, 517)]   # rows x columns, seeded noise
SIZES = (16, 32)
PLANTED = ({"no_intermediate_rounding": True}, {"no_half": True}, {"fixed_support": True}, {"unnormalised": True},
           {"whole_image_clamp": True})


def _images():
    return [R.noise_image(h, w, 100 + i) for i, (h, w) in enumerate(SOURCES)] + [R.pattern_image()]


def _inner_box(h, w):
    """A crop away from all four borders (so that clamping to the crop and to the image differ) with odd sides.  Odd, because a
    side that is a power-of-two fraction of S (8 -> 16: scale 1 / 2) gives weights that are multiples of 1 / 128 and sum to 1:
    about one value in a hundred then lands EXACTLY on a rounding tie, and which way PIL takes a tie is decided by its 22-bit
    fixed-point weights, not by the arithmetic under test (a 5 x 8 crop to 16 showed 3 such values of 768)."""
    top, left = h // 5 + 1, w // 7 + 1
    ch, cw = max(h - top - h // 6 - 1, 3), max(w - left - w // 5 - 1, 3)
    return top, left, ch - (ch % 2 == 0), cw - (cw % 2 == 0)


@pytest.fixture(scope="module")
def pil_cases():
    """[(name, image, plan_i, plan_f, S, PIL's levels)]: crop -> resize((S, S)) and resize((nw, nh)) -> centre crop."""
    from PIL import Image

    from contrastors_amd.image_transform import eval_plan, train_plan

    cases = []
    for img in _images():
        h, w = img.shape[:2]
        pil = Image.fromarray(img)
        for S in SIZES:
            for tag, box in (("full", (0, 0, h, w)), ("inner", _inner_box(h, w))):
                top, left, ch, cw = box
                want = np.asarray(pil.crop((left, top, left + cw, top + ch)).resize((S, S), Image.BICUBIC), np.float64)
                cases.append((f"{h}x{w}-{tag}-crop-{S}", img, *train_plan(box, S), S, want))
            plan_i, plan_f = eval_plan(h, w, S)
            new_h, new_w = (S, int(S * w / h)) if h < w else (int(S * h / w), S)
            oy, ox = int(round((new_h - S) / 2.0)), int(round((new_w - S) / 2.0))
            want = np.asarray(pil.resize((new_w, new_h), Image.BICUBIC).crop((ox, oy, ox + S, oy + S)), np.float64)
            cases.append((f"{h}x{w}-eval-{S}", img, plan_i, plan_f, S, want))
    return cases


def _agrees(got, want):
    d = np.abs(got - want)
    return d.max() <= 1 and (d > 0).mean() <= 0.002


def test_yardstick_matches_pil(pil_cases):
    worst_n, worst_frac = 0, 0.0
    for name, img, plan_i, plan_f, S, want in pil_cases:
        got = R.resize_levels(img, plan_i, plan_f, S)
        d = np.abs(got - want)
        worst_n, worst_frac = max(worst_n, int((d > 0).sum())), max(worst_frac, float((d > 0).mean()))
        assert d.max() <= 1, (name, d.max())
        assert (d > 0).mean() <= 0.002, (name, int((d > 0).sum()), d.size)
    print(f"yardstick vs PIL over {len(pil_cases)} cases: at most {worst_n} values / {worst_frac:.5f} of a case differ, by one level")


@pytest.mark.parametrize("planted", PLANTED, ids=lambda p: next(iter(p)))
def test_planted_error_is_caught(pil_cases, planted):
    assert not all(_agrees(R.resize_levels(img, plan_i, plan_f, S, **planted), want)
                   for _, img, plan_i, plan_f, S, want in pil_cases)


def test_host_resize_follows_the_plan(pil_cases):
    """The host fallback (PIL on the cropped clamp range with the plan's box) against the same PIL two-step results."""
    from contrastors_amd.image_transform import host_resize

    for name, img, plan_i, plan_f, S, want in pil_cases:
        assert _agrees(host_resize(img, plan_i, plan_f, S).astype(np.float64), want), name


# ------------------------------------------------------------------------------------------------------------ crop sampler, plans
def test_crop_sampler_boxes():
    from contrastors_amd.image_transform import random_resized_crop_params as rrc

    g = torch.Generator().manual_seed(5)
    scale = (0.3, 0.8)
    for h, w in [(40, 40), (61, 83), (300, 517), (2, 3), (1, 1)]:
        for _ in range(50):
            top, left, ch, cw = rrc(h, w, scale, generator=g)
            assert 0 <= top and 0 <= left and ch >= 1 and cw >= 1 and top + ch <= h and left + cw <= w
            if min(h, w) >= 40:   # w and h are each rounded to an integer: the area moves by at most (w' + h') / 2 + 1 / 4 (unrounded sides)
                slack = (cw + ch + 1) / 2 + 0.25
                assert scale[0] * h * w - slack <= ch * cw <= scale[1] * h * w + slack, (h, w, ch, cw)


def test_crop_sampler_central_fallback_clamps_the_ratio():
    from contrastors_amd.image_transform import random_resized_crop_params as rrc

    g = torch.Generator().manual_seed(0)
    # 1000 rows x 10 columns: no box of >= 90 % of the area has a ratio within (3/4, 4/3); w / h = 0.01 < 3/4 -> full width, h = round(10 / (3/4))
    assert rrc(1000, 10, (0.9, 1.0), generator=g) == ((1000 - 13) // 2, 0, 13, 10)
    assert rrc(10, 1000, (0.9, 1.0), generator=g) == (0, (1000 - 13) // 2, 10, 13)


def test_crop_sampler_is_seeded():
    from contrastors_amd.image_transform import GpuImageTransform

    sizes = [(61, 83), (300, 517), (40, 40)] * 3
    a = GpuImageTransform(32, seed=7).plans(sizes)
    b = GpuImageTransform(32, seed=7).plans(sizes)
    c = GpuImageTransform(32, seed=8).plans(sizes)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])
    assert a[0].dtype == np.int32 and a[1].dtype == np.float64 and a[0].shape == a[1].shape == (9, 4)


@pytest.mark.parametrize("h, w, S, new_h, new_w", [(40, 40, 16, 16, 16), (61, 83, 32, 32, 43), (83, 61, 32, 43, 32),
                                                   (500, 37, 16, 216, 16), (300, 517, 224, 224, 386)])
def test_eval_plan_matches_the_two_step_integers(h, w, S, new_h, new_w):
    from contrastors_amd.image_transform import eval_plan

    plan_i, plan_f = eval_plan(h, w, S)
    assert plan_i == (0, h, 0, w)
    oy, ox = int(round((new_h - S) / 2.0)), int(round((new_w - S) / 2.0))
    assert plan_f == (oy * (h / new_h), h / new_h, ox * (w / new_w), w / new_w)


def test_train_plan():
    from contrastors_amd.image_transform import train_plan

    assert train_plan((3, 5, 20, 10), 16) == ((3, 23, 5, 15), (3.0, 20 / 16, 5.0, 10 / 16))


# ------------------------------------------------------------------------------------------------------------ loader
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "search", "_", "query", ":"] + [f"w{i}" for i in range(20)]


@pytest.fixture()
def tokenizer(tmp_path):
    from transformers import BertTokenizer

    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(VOCAB) + "\n")
    return BertTokenizer(str(vocab), do_lower_case=True)


def _shards(tmp_path, n_shards=4, per_shard=3, size=None):
    """Shards NNN.tar of `per_shard` PNG + caption pairs; returns the brace pattern and {caption: image}."""
    images = {}
    for s in range(n_shards):
        members = []
        for i in range(per_shard):
            k = s * per_shard + i
            h, w = size or (5 + k, 7 + 2 * k)
            img = R.noise_image(h, w, 500 + k)
            images[f"w{k % 20} w{(k * 7) % 20} w{k // 20}"] = img
            members += [(f"d/{k:05d}.png", R.png_bytes(img)), (f"d/{k:05d}.txt", f"w{k % 20} w{(k * 7) % 20} w{k // 20}".encode())]
        R.write_tar(tmp_path / f"{s:03d}.tar", members)
    return str(tmp_path / f"{{000..{n_shards - 1:03d}}}.tar"), images


def _unpack(batch):
    v = batch["vision"]
    offs, sizes = v["offsets"].tolist(), v["sizes"].tolist()
    return [v["pixels_u8"][offs[b]: offs[b] + 3 * h * w].numpy().reshape(h, w, 3) for b, (h, w) in enumerate(sizes)]


def test_loader_ragged_batches_and_tokens(tmp_path, tokenizer):
    from contrastors_amd.image_data import TarImageTextDataset

    pattern, images = _shards(tmp_path)
    ds = TarImageTextDataset(pattern, batch_size=5, tokenizer=tokenizer, seq_len=12, is_train=False, add_prefix=True)
    batches = list(ds)
    assert [len(b["vision"]["sizes"]) for b in batches] == [5, 5, 2]   # eval: the partial batch too
    seen = 0
    for b in batches:
        v, t = b["vision"], b["text"]
        B = len(v["sizes"])
        assert v["pixels_u8"].dtype == torch.uint8 and v["offsets"].dtype == torch.int64 and v["sizes"].dtype == torch.int32
        assert v["offsets"][0] == 0 and v["offsets"][-1] == v["pixels_u8"].numel() and v["offsets"].shape == (B + 1,)
        assert torch.equal(v["offsets"][1:] - v["offsets"][:-1], 3 * v["sizes"][:, 0].long() * v["sizes"][:, 1].long())
        assert set(t) == {"input_ids", "token_type_ids", "attention_mask"}
        assert all(x.shape == (B, 12) and x.dtype == torch.int64 for x in t.values())
        for img, ids in zip(_unpack(b), t["input_ids"].tolist()):
            words = tokenizer.convert_ids_to_tokens([i for i in ids if i not in (0, 2, 3)])
            assert words[:4] == ["search", "_", "query", ":"]   # "search_query: " + caption
            assert np.array_equal(images[" ".join(words[4:])], img)   # eval order or not: the caption's own image, exact pixels
            seen += 1
    assert seen == len(images)
    train = TarImageTextDataset(pattern, batch_size=5, tokenizer=tokenizer, seq_len=12, is_train=True, shuffle_buffer=4)
    assert [len(b["vision"]["sizes"]) for b in train] == [5, 5]          # train: full batches only
    again = TarImageTextDataset(pattern, batch_size=5, tokenizer=tokenizer, seq_len=12, is_train=True, shuffle_buffer=4)
    for a, b in zip(train, again):                                          # the same (seed, epoch, rank, workers): the same stream
        assert torch.equal(a["vision"]["pixels_u8"], b["vision"]["pixels_u8"]) and torch.equal(a["text"]["input_ids"], b["text"]["input_ids"])
    again.set_epoch(1)
    assert any(not torch.equal(a["text"]["input_ids"], b["text"]["input_ids"]) for a, b in zip(train, again))


def test_loader_groups_by_key_and_skips_bad_samples(tmp_path, tokenizer, caplog):
    from contrastors_amd.image_data import TarImageTextDataset, iter_tar_samples

    good = [R.noise_image(4 + i, 6, 40 + i) for i in range(3)]
    png = [R.png_bytes(g) for g in good]
    R.write_tar(tmp_path / "a.tar", [
        ("x/0.png", png[0]), ("x/0.txt", b"w1 w2"), ("x/0.json", b"{}"),     # extra members of a key ride along
        ("x/1.png", png[1]),                                                  # no caption
        ("x/2.txt", b"w3 w4"),                                                # no image
        ("x/3.png", png[1][: len(png[1]) // 2]), ("x/3.txt", b"w5 w6"),       # the image does not decode
        ("x/4.png", png[1]), ("x/4.txt", b" "),                               # empty caption
        ("x/5.PNG", png[2]), ("x/5.txt", b"w7 w8")])                          # extensions are lower-cased
    raw = list(iter_tar_samples(str(tmp_path / "a.tar")))
    assert [r["__key__"] for r in raw] == [f"x/{i}" for i in range(6)]
    assert set(raw[0]) == {"__key__", "png", "txt", "json"} and "png" in raw[5]
    ds = TarImageTextDataset(str(tmp_path / "a.tar"), batch_size=8, tokenizer=tokenizer, seq_len=8, is_train=False)
    with caplog.at_level(logging.WARNING, logger="contrastors_amd.image_data"):
        (batch,) = list(ds)
    imgs = _unpack(batch)
    assert len(imgs) == 2 and np.array_equal(imgs[0], good[0]) and np.array_equal(imgs[1], good[2])   # the stream went on past x/3
    assert ds.skipped == 4 and sum("skipped" in r.message for r in caplog.records) == 4


def test_loader_partitions_shards_by_rank_and_worker(tmp_path, tokenizer):
    from contrastors_amd.image_data import TarImageTextDataset

    pattern, _ = _shards(tmp_path, n_shards=8, per_shard=1)
    for is_train in (True, False):
        parts = []
        for rank in range(2):
            ds = TarImageTextDataset(pattern, batch_size=2, tokenizer=tokenizer, seq_len=8, is_train=is_train, rank=rank, world_size=2)
            assert ds.rank_batch_size == 1
            parts += [ds.shards_for(0, rank, worker, 2) for worker in range(2)]
        flat = [u for p in parts for u in p]
        assert all(len(p) == 2 for p in parts) and len(set(flat)) == 8 and sorted(flat) == sorted(ds.urls)
    assert ds.shards_for(0, 0, 0, 1) == ds.urls[0::2]   # eval keeps the listed order
    tr = TarImageTextDataset(pattern, batch_size=2, tokenizer=tokenizer, seq_len=8, rank=0, world_size=2)
    assert tr.shards_for(0, 0, 0, 1) != tr.shards_for(1, 0, 0, 1) or tr.shards_for(1, 0, 0, 1) != tr.shards_for(2, 0, 0, 1)


def test_crop_boxes_do_not_depend_on_the_workers(tmp_path, tokenizer):
    """The loader hands out decoded images only; the boxes are drawn from the transform's generator where the batches are
    consumed, in batch order -- so one or two workers (simulated: worker = (id, count)) give the same plans."""
    from contrastors_amd.image_data import TarImageTextDataset
    from contrastors_amd.image_transform import GpuImageTransform

    pattern, _ = _shards(tmp_path, n_shards=4, per_shard=4, size=(30, 45))
    def plans(workers):
        t = GpuImageTransform(16, seed=3, scale=(0.3, 1.0))
        out = []
        for wid in range(workers):
            for b in TarImageTextDataset(pattern, batch_size=4, tokenizer=tokenizer, seq_len=8, worker=(wid, workers)):
                assert set(b["vision"]) == {"pixels_u8", "offsets", "sizes"}
                out.append(t.plans(b["vision"]["sizes"]))
        return out
    one, two = plans(1), plans(2)
    assert len(one) == len(two) == 4
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(one, two))
    assert len({tuple(p[0].reshape(-1)) for p in one}) == 4   # (and they are draws, not one box)


def test_loader_precomputed_text_embeddings(tmp_path):
    import io

    from contrastors_amd.image_data import TarImageTextDataset

    embs = np.random.default_rng(0).standard_normal((3, 8)).astype(np.float32)
    members = []
    for i in range(3):
        buf = io.BytesIO()
        np.save(buf, embs[i])
        members += [(f"{i}.png", R.png_bytes(R.noise_image(4, 4, i))), (f"{i}.npy", buf.getvalue()), (f"{i}.txt", b"w1 w2")]
    R.write_tar(tmp_path / "p.tar", members)
    (batch,) = list(TarImageTextDataset(str(tmp_path / "p.tar"), batch_size=3, precomputed=True, is_train=False))
    assert set(batch["text"]) == {"text_embs"} and np.array_equal(batch["text"]["text_embs"].numpy(), embs)


# ------------------------------------------------------------------------------------------------------------ config, refusals
RECIPE = {   # the shape of configs/train/nomic_embed_vision_v1.5.yaml
    "train_args": {"num_epochs": 3, "learning_rate": 1e-3, "chunk_size": 1536, "grad_cache": False, "clamp_logits": False},
    "data_args": {"image_text_shards": "/data/dfn/{00000000..00000003}.tar", "eval_flickr": True, "workers": 8, "batch_size": 16384,
                  "eval_batch_size": 16384, "seed": 42, "imagenet_val_path": "/data/imagenet", "dataset_resampled": False},
    "model_args": {"model_type": "locked_text"},
    "text_model_args": {"model_type": "locked_text", "seq_len": 77, "add_prefix": True, "freeze": True},
    "vision_model_args": {"model_type": "locked_text", "pooling": "map", "logit_scale": None},
    "transforms": {"image_size": 224},
}


def test_config_keeps_the_image_text_keys():
    from contrastors_amd.config import Config, DataArgs
    from contrastors_amd.image_transform import OPENAI_DATASET_MEAN, GpuImageTransform

    cfg = Config(**RECIPE)
    da = cfg.data_args
    assert da.image_text_shards == RECIPE["data_args"]["image_text_shards"] and da.eval_batch_size == 16384
    assert da.imagenet_val_path == "/data/imagenet" and da.eval_flickr is True and da.dataset_resampled is False
    assert da.train_num_samples is None
    assert cfg.transforms.image_size == 224 and tuple(cfg.transforms.mean) == OPENAI_DATASET_MEAN
    inert = DataArgs()
    assert inert.image_text_shards is None and inert.eval_batch_size is None and not inert.dataset_resampled
    assert Config(train_args={}).transforms is None
    t = GpuImageTransform.from_config(cfg.transforms, is_train=True)
    assert t.image_size == 224 and t.scale == (0.9, 1.0) and t.out_dtype == torch.bfloat16
    assert np.allclose(t.mean, OPENAI_DATASET_MEAN)
    cfg2 = Config(**{**RECIPE, "transforms": {"image_size": 32, "aug_cfg": {"scale": [0.5, 1.0], "color_jitter": 0.4}}})
    assert GpuImageTransform.from_config(cfg2.transforms, is_train=True).scale == (0.5, 1.0)


def test_refusals(tmp_path, tokenizer):
    from contrastors_amd.config import Config
    from contrastors_amd.image_data import TarImageTextDataset
    from contrastors_amd.image_transform import GpuImageTransform

    with pytest.raises(NotImplementedError):
        GpuImageTransform(224, resize_longest_max=True)
    cfg = Config(**{**RECIPE, "transforms": {"image_size": 224, "resize_longest_max": True}})
    with pytest.raises(NotImplementedError):
        GpuImageTransform.from_config(cfg.transforms, is_train=False)
    with pytest.raises(ValueError):
        GpuImageTransform(1024)
    with pytest.raises(NotImplementedError):
        TarImageTextDataset("s3://dfn-datacomp-large/{00000000..00015444}.tar", 8, tokenizer=tokenizer)
    with pytest.raises(NotImplementedError):
        TarImageTextDataset(str(tmp_path / "a.tar"), 8, tokenizer=tokenizer, dataset_resampled=True)
    with pytest.raises(NotImplementedError):
        TarImageTextDataset(str(tmp_path / "a.tar"), 8, tokenizer=tokenizer, mlm_prob=0.3)


def test_train_needs_train_num_samples(tmp_path, monkeypatch):
    import yaml

    from contrastors_amd import train

    path = tmp_path / "recipe.yaml"
    path.write_text(yaml.safe_dump(RECIPE))
    monkeypatch.setattr("sys.argv", ["train", "--config", str(path), "--synthetic-steps", "0"])
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    with pytest.raises(SystemExit, match="train_num_samples"):
        train.main()


# ------------------------------------------------------------------------------------------------------------ C boundary
@pytest.fixture(scope="module")
def built():
    from contrastors_amd import build

    return build.build()


def test_entry_point_is_declared_bound_and_checks_its_arguments(built):
    import ctypes as C

    from contrastors_amd import _C

    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", (ROOT / "include" / "contrastors_hip.h").read_text()))
    assert "cx_image_transform" in declared and "cx_image_transform" in _C.EXPORTED_SYMBOLS
    lib = _C.lib()
    assert lib.cx_abi_version() == 10
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    assert lib.cx_image_transform(None, p, p, p, p, p, 0, 1, 16, m, m, None) == ERR_ARG
    assert lib.cx_image_transform(p, p, p, p, p, p, 0, 0, 16, m, m, None) == ERR_ARG
    assert lib.cx_image_transform(p, p, p, p, p, p, 0, 1, 1024, m, m, None) == ERR_SHAPE
    assert lib.cx_image_transform(p, p, p, p, p, p, 0, 1, 16, m, m, None) == ERR_ARG   # plans in pageable memory
