"""CPU checks of contrastors_amd.zeroshot: the hit counts against the reference's recorded `accuracy`, prompt building and
cleaning, the metadata file, the two evaluation datasets, the rank partition and the config keys.  No GPU call is made."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import img_ref as I

ROOT = Path(__file__).resolve().parent.parent


def test_topk_hits_reproduce_the_recorded_reference_accuracy(gold):
    from contrastors_amd.zeroshot import topk_hits

    g = gold("zeroshot_accuracy")
    logits, target = torch.from_numpy(g["logits"]), torch.from_numpy(g["target"])
    own = logits.gather(1, target[:, None])
    ranks = (logits > own).sum(1)                       # tie-free logits: the number of classes scored above the target
    ks = [int(k) for k in g["topk"]]
    got = topk_hits(ranks, ks)
    assert got == [int(c) for c in g["correct"]] and all(isinstance(x, int) for x in got)
    assert 0 < got[0] < got[-1] < len(target)           # the recording has hits and misses at both ends
    assert topk_hits(ranks.numpy(), ks) == got


def test_retrieval_recall_counts_the_best_positive_per_row():
    from contrastors_amd.zeroshot import retrieval_recall

    ranks, ptr = [3, 0, 7, 12, 9, 4], [0, 2, 3, 6]        # best per row: 0, 7, 4
    assert retrieval_recall(ranks, ptr, ks=(1, 5, 10)) == [1 / 3, 2 / 3, 1.0]
    with pytest.raises(ValueError, match="without positives"):
        retrieval_recall([1, 2], [0, 2, 2])
    with pytest.raises(ValueError, match="delimit"):
        retrieval_recall([1, 2], [0, 1])


def test_prompt_building_and_cleaning():
    from contrastors_amd.zeroshot import build_prompts, clean_prompt

    assert clean_prompt("  a  photo\tof\n a &amp;amp; b  ") == "a photo of a & b"      # two rounds of unescaping
    assert clean_prompt("x &amp;lt; y") == "x < y"
    assert clean_prompt("fish &amp; chips") == "fish & chips"
    names, templates = ["tench", "great  white shark"], ["a photo of a {}.", "  art of the {} "]
    assert build_prompts(names, templates) == ["a photo of a tench.", "art of the tench", "a photo of a great white shark.",
                                               "art of the great white shark"]          # class-major
    assert build_prompts(["cat"], ["a {}."], prefix="search_query") == ["search_query: a cat."]
    assert build_prompts(["cat"], ["a {}."], add_eos=True, eos_token="</s>") == ["a cat.</s>"]
    # EOS first, then the prefix: the reference's order
    assert build_prompts(["cat"], ["a {}."], prefix="search_query", add_eos=True, eos_token="</s>") == ["search_query: a cat.</s>"]
    with pytest.raises(ValueError, match="eos_token"):
        build_prompts(["cat"], ["a {}."], add_eos=True, eos_token=None)


def test_load_zeroshot_meta_defaults_and_errors(tmp_path):
    from contrastors_amd.zeroshot import load_zeroshot_meta

    p = tmp_path / "meta.json"
    p.write_text(json.dumps({"classnames": ["a", "b"]}))
    assert load_zeroshot_meta(p) == {"classnames": ["a", "b"], "templates": ["a photo of a {}."], "folders": None}
    p.write_text(json.dumps({"classnames": ["a", "b"], "templates": ["x {}", "y {}"], "folders": ["n02", "n01"]}))
    assert load_zeroshot_meta(p) == {"classnames": ["a", "b"], "templates": ["x {}", "y {}"], "folders": ["n02", "n01"]}
    for bad in ({}, {"classnames": []}, {"classnames": ["a", 3]}, {"classnames": ["a"], "templates": ["no placeholder"]},
                {"classnames": ["a", "b"], "folders": ["only-one"]}, {"classnames": ["a", "b"], "folders": ["d", "d"]}, ["a"]):
        p.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            load_zeroshot_meta(p)
    with pytest.raises(FileNotFoundError):
        load_zeroshot_meta(tmp_path / "missing.json")


def _write_png(path, h, w, seed):
    path.parent.mkdir(parents=True, exist_ok=True)
    img = I.noise_image(h, w, seed)
    path.write_bytes(I.png_bytes(img))
    return img


def test_image_folder_dataset(tmp_path):
    from contrastors_amd.zeroshot import ImageFolderDataset, zeroshot_loader

    root = tmp_path / "val"
    imgs = {"b/2.png": _write_png(root / "b" / "2.png", 9, 11, 1), "b/10.png": _write_png(root / "b" / "10.png", 8, 8, 2),
            "a/x.PNG": _write_png(root / "a" / "x.PNG", 7, 13, 3), "c/sub/y.png": _write_png(root / "c" / "sub" / "y.png", 5, 6, 4),
            "c/z.png": _write_png(root / "c" / "z.png", 6, 5, 5)}
    (root / "a" / "notes.txt").write_text("not an image")
    (root / "b" / "thumbs.db").write_bytes(b"\0\1")
    (root / "stray.png").write_bytes(I.png_bytes(I.noise_image(4, 4, 6)))     # not inside a class directory
    ds = ImageFolderDataset(str(root))
    assert ds.classes == ["a", "b", "c"]
    rel = [(str(Path(p).relative_to(root)), label) for p, label in ds.samples]
    assert rel == [("a/x.PNG", 0), ("b/10.png", 1), ("b/2.png", 1), ("c/z.png", 2), ("c/sub/y.png", 2)]    # sorted walk
    for i, (name, label) in enumerate(rel):
        img, lab, path = ds[i]
        assert img.dtype == np.uint8 and np.array_equal(img, imgs[name]) and lab == label and path.endswith(name)
    ordered = ImageFolderDataset(str(root), folders=["c", "a"])
    assert ordered.classes == ["c", "a"] and [label for _, label in ordered.samples] == [0, 0, 1]
    with pytest.raises(FileNotFoundError):
        ImageFolderDataset(str(root), folders=["a", "missing"])
    with pytest.raises(FileNotFoundError):
        ImageFolderDataset(str(tmp_path / "nothing"))
    # the loader: this rank's share, ragged vision batches as the GPU transform takes them
    batches = list(zeroshot_loader(ds, batch_size=2, rank=1, world=2))
    assert [b["labels"].tolist() for b in batches] == [[1, 2]]
    v = batches[0]["vision"]
    assert v["sizes"].tolist() == [[8, 8], [6, 5]] and v["offsets"].tolist() == [0, 192, 282] and v["pixels_u8"].dtype == torch.uint8
    assert np.array_equal(v["pixels_u8"][:192].numpy().reshape(8, 8, 3), imgs["b/10.png"])


def test_retrieval_eval_dataset_reads_the_three_caption_forms(tmp_path):
    from contrastors_amd.zeroshot import RetrievalEvalDataset

    a, b, c, d = (I.noise_image(6 + k, 9 - k, 20 + k) for k in range(4))
    I.write_tar(tmp_path / "0.tar", [
        ("0000.png", I.png_bytes(a)), ("0000.json", json.dumps({"captions": ["one  ", "two", ""]}).encode()),
        ("0001.png", I.png_bytes(b)), ("0001.json", json.dumps({"caption": "single"}).encode()),
        ("0002.txt", b"no image here\n")])
    I.write_tar(tmp_path / "1.tar", [
        ("0003.png", I.png_bytes(c)), ("0003.txt", b"first line\n\n second line \n"),
        ("0004.png", I.png_bytes(d))])                                       # no caption: skipped
    ds = RetrievalEvalDataset(f"{tmp_path}/{{0..1}}.tar")
    got = list(ds)
    assert [caps for _, caps in got] == [["one", "two"], ["single"], ["first line", "second line"]]
    assert all(np.array_equal(x, y) for (x, _), y in zip(got, (a, b, c)))
    assert [caps for _, caps in RetrievalEvalDataset(f"{tmp_path}/1.tar::{tmp_path}/0.tar")][0] == ["first line", "second line"]


def test_shard_indices_is_an_exact_partition():
    from contrastors_amd.zeroshot import shard_indices

    for n, world in ((10, 4), (7, 3), (3, 8), (0, 2), (50_000, 8)):
        parts = [list(shard_indices(n, r, world)) for r in range(world)]
        assert sorted(i for p in parts for i in p) == list(range(n))         # every sample once: no padding duplicates
        assert max(map(len, parts)) - min(map(len, parts)) <= 1
    assert list(shard_indices(10, 1, 4)) == [1, 5, 9]
    with pytest.raises(ValueError):
        shard_indices(10, 4, 4)


def test_config_keys_default_to_none_and_old_recipes_parse():
    from contrastors_amd.config import Config, DataArgs

    da = DataArgs()
    assert da.zeroshot_meta_path is None and da.retrieval_eval_shards is None
    cfg = Config(**{"train_args": {"learning_rate": 1e-3, "warmup_steps": 0},
                    "data_args": {"image_text_shards": "/data/{0..3}.tar", "eval_flickr": True, "imagenet_val_path": "/data/imagenet",
                                  "batch_size": 16, "seed": 42},
                    "text_model_args": {"model_type": "locked_text", "model_name": "t"},
                    "vision_model_args": {"model_type": "locked_text", "model_name": "v"}})
    assert cfg.data_args.eval_flickr is True and cfg.data_args.retrieval_eval_shards is None
    assert cfg.data_args.imagenet_val_path == "/data/imagenet" and cfg.data_args.zeroshot_meta_path is None
    cfg = Config(**{"train_args": {"learning_rate": 1e-3, "warmup_steps": 0},
                    "data_args": {"zeroshot_meta_path": "m.json", "retrieval_eval_shards": "r/{0..1}.tar", "batch_size": 16}})
    assert cfg.data_args.zeroshot_meta_path == "m.json" and cfg.data_args.retrieval_eval_shards == "r/{0..1}.tar"


def test_package_carries_no_class_name_or_prompt_list():
    """The class names and the prompt templates arrive through load_zeroshot_meta at run time: the module holds one template."""
    from contrastors_amd import zeroshot

    text = (ROOT / "contrastors_amd" / "zeroshot.py").read_text()
    assert zeroshot.DEFAULT_TEMPLATES == ("a photo of a {}.",) and text.count("{}.") <= 6 and "tench" not in text
