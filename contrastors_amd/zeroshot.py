"""Image-text evaluation: zero-shot classification accuracy and retrieval recall@k (host-side counterpart of
sc/eval/zero_shot.py, sc/eval/imagenet/imagenet.py, clip_benchmark's zeroshot_retrieval and the eval_loop of
sc/trainers/image_text.py:198-254).

Every metric here is a function of the RANK of target columns in a row of the similarity matrix: top-k accuracy is
rank(label) < k, recall@k is min over a row's positives of rank < k.  The ranks come from `FlatIPIndex.rank`
(cx_rank_targets, csrc/rank.hip), which never writes the (rows x corpus) scores.  Embeddings are rounded to bf16 for the
kernel (the reference's loop runs its matmul under bf16 autocast too).  Ties go to the lower id, where torch.topk leaves
them unspecified.

Deviations from the reference, all deliberate:
  * the class prompts are embedded through the length-sorted `encode` path in a few large batches, not one padded-to-max
    batch per class (the embeddings do not depend on padding);
  * `ftfy.fix_text` is applied to the prompts only when the `ftfy` package is importable;
  * across ranks, images are dealt by a strided partition WITHOUT padding duplicates (`shard_indices`), hit counts and sample
    counts are summed and divided once.  The reference pads with DistributedSampler and averages per-rank means; on one
    rank the two agree, on several ranks this is the exact figure;
  * the class names / prompt templates are not part of the package: they arrive through a JSON file (`load_zeroshot_meta`);
    the retrieval set is local tar shards (`RetrievalEvalDataset`), not a hub download.
"""
from __future__ import annotations

import html
import io
import json
import logging
import os
import re
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .image_data import IMAGE_EXTS, iter_tar_samples, ragged_image_collate
from .search import FlatIPIndex, encode

log = logging.getLogger(__name__)

DEFAULT_TEMPLATES = ("a photo of a {}.",)
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")   # torchvision's list


# ---- prompts -------------------------------------------------------------------------------------------------------------------
def clean_prompt(text: str) -> str:
    """sc/eval/zero_shot.py:94-103 (basic_clean + whitespace_clean): ftfy.fix_text when the package is importable, html.unescape
    twice, strip, whitespace runs collapsed to one blank."""
    try:
        import ftfy

        text = ftfy.fix_text(text)
    except ImportError:
        pass
    text = html.unescape(html.unescape(text)).strip()
    return re.sub(r"\s+", " ", text).strip()


def build_prompts(classnames: Sequence[str], templates: Sequence[str], prefix: Optional[str] = None, add_eos: bool = False,
                  eos_token: Optional[str] = None) -> List[str]:
    """Class-major list of len(classnames) * len(templates) prompts: template.format(name), cleaned, + EOS, then "prefix: "."""
    if add_eos and not eos_token:
        raise ValueError("add_eos needs the tokenizer's eos_token")
    out = []
    for c in classnames:
        for t in templates:
            text = clean_prompt(t.format(c))
            if add_eos:
                text = text + eos_token
            if prefix:
                text = f"{prefix}: {text}"
            out.append(text)
    return out


def zeroshot_classifier_weights(text_tower, tokenizer, classnames: Sequence[str], templates: Optional[Sequence[str]] = None,
                                prefix: Optional[str] = None, add_eos: bool = False, seq_len: int = 77,
                                batch_size: int = 256) -> torch.Tensor:
    """(C, D) float32 classifier on the tower's device (sc/eval/zero_shot.py:106-157, transposed): per class the L2-normalised
    mean over templates of the L2-normalised prompt embeddings.  All C x T prompts go through `encode` (length-sorted
    batches of `batch_size`).  `ftfy.fix_text` is part of the reference's prompt cleaning and is applied here only when the
    package is importable."""
    templates = list(templates) if templates else list(DEFAULT_TEMPLATES)
    classnames = list(classnames)
    if not classnames:
        raise ValueError("zeroshot_classifier_weights: no class names")
    prompts = build_prompts(classnames, templates, prefix, add_eos, getattr(tokenizer, "eos_token", None))
    emb = encode(text_tower, prompts, tokenizer, batch_size=batch_size, max_length=seq_len)   # normalised, fp32
    emb = torch.nn.functional.normalize(emb, dim=-1).view(len(classnames), len(templates), -1).mean(1)
    return emb / emb.norm(dim=-1, keepdim=True)


# ---- metrics over ranks ------------------------------------------------------------------------------------------------------
def topk_hits(ranks, ks: Sequence[int] = (1, 5)) -> List[int]:
    """Number of entries with rank < k, per k: sc/eval/metrics.py `accuracy` (its correct-counts) given each row's label rank."""
    r = torch.as_tensor(ranks)
    return [int((r < int(k)).sum()) for k in ks]


def retrieval_recall(ranks, row_ptr, ks: Sequence[int] = (1, 5, 10)) -> List[float]:
    """Share of rows whose best-ranked positive has rank < k: clip_benchmark's `recall_at_k(...) > 0` averaged over rows.
    ranks (nnz) and row_ptr (M + 1) as FlatIPIndex.rank returns them; a row without positives is an error."""
    r = torch.as_tensor(ranks).detach().cpu().to(torch.int64)
    p = torch.as_tensor(row_ptr).detach().cpu().to(torch.int64)
    lens = p[1:] - p[:-1]
    if p.numel() < 2 or int(p[-1]) != r.numel():
        raise ValueError("retrieval_recall: row_ptr does not delimit ranks")
    if bool((lens <= 0).any()):
        raise ValueError("retrieval_recall: a row without positives")
    rows = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    best = torch.full((lens.numel(),), torch.iinfo(torch.int64).max, dtype=torch.int64).scatter_reduce(0, rows, r, "amin")
    return [int((best < int(k)).sum()) / lens.numel() for k in ks]


# ---- data --------------------------------------------------------------------------------------------------------------------------
def load_zeroshot_meta(path: str) -> dict:
    """{"classnames": [...], "templates": [...], "folders": [...]} from a JSON file.  templates default to the single
    "a photo of a {}."; folders (the image directory of each class, in class order) are optional."""
    with open(path) as f:
        meta = json.load(f)
    if not isinstance(meta, dict) or not isinstance(meta.get("classnames"), list) or not meta["classnames"]:
        raise ValueError(f"{path}: expected an object with a non-empty `classnames` list")
    names = meta["classnames"]
    if not all(isinstance(c, str) for c in names):
        raise ValueError(f"{path}: classnames must be strings")
    templates = meta.get("templates") or list(DEFAULT_TEMPLATES)
    if not isinstance(templates, list) or not all(isinstance(t, str) and "{}" in t for t in templates):
        raise ValueError(f"{path}: templates must be strings with a {{}} placeholder")
    folders = meta.get("folders")
    if folders is not None and (not isinstance(folders, list) or len(folders) != len(names)
                                or len(set(folders)) != len(folders)):
        raise ValueError(f"{path}: folders must name one distinct directory per class ({len(names)})")
    return {"classnames": list(names), "templates": list(templates), "folders": None if folders is None else list(folders)}


def _decode_rgb(data) -> np.ndarray:
    from PIL import Image

    with Image.open(data) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class ImageFolderDataset(torch.utils.data.Dataset):
    """torchvision `ImageFolder` semantics without torchvision: classes = the sorted sub-directory names of `root` (or
    `folders`, in the order given: label i = folders[i]); per class the files of a sorted walk with an image extension.
    Item: (H x W x 3 uint8 array, label, path)."""

    def __init__(self, root: str, folders: Optional[Sequence[str]] = None):
        if folders is None:
            folders = sorted(e.name for e in os.scandir(root) if e.is_dir())
        self.root, self.classes = str(root), list(folders)
        if not self.classes:
            raise FileNotFoundError(f"no class directories in {root}")
        self.samples: List[Tuple[str, int]] = []
        for label, name in enumerate(self.classes):
            d = os.path.join(self.root, name)
            if not os.path.isdir(d):
                raise FileNotFoundError(f"class directory {d} does not exist")
            for base, _, files in sorted(os.walk(d, followlinks=True)):
                for fn in sorted(files):
                    if fn.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(base, fn), label))
        if not self.samples:
            raise FileNotFoundError(f"no image files under {root}")

    def __len__(self) -> int:
        return len(self.samples)

    def __getitem__(self, i: int):
        path, label = self.samples[i]
        return _decode_rgb(path), label, path


class RetrievalEvalDataset:
    """Image / captions samples for retrieval evaluation from local tar shards (`iter_tar_samples`): a local stand-in for the
    hub dataset the reference downloads (nlphuji/flickr_1k_test_image_text_retrieval).  Per key one image and its captions,
    from `<key>.json` {"captions": [...]} or {"caption": "..."}, else `<key>.txt` with one caption per line.  Iterating yields
    (H x W x 3 uint8 array, [captions]) in shard order; samples without an image or a caption are skipped with a log line."""

    def __init__(self, shards: str):
        from .data import expand_urls

        self.urls = [u for part in str(shards).split("::") for u in expand_urls(part)]
        if not self.urls:
            raise ValueError("RetrievalEvalDataset: no shards")

    @staticmethod
    def captions_of(raw: dict) -> List[str]:
        if "json" in raw:
            meta = json.loads(raw["json"].decode("utf-8"))
            caps = meta.get("captions") if isinstance(meta, dict) else None
            if caps is None and isinstance(meta, dict) and "caption" in meta:
                caps = [meta["caption"]]
            if caps is not None:
                return [str(c).strip() for c in caps if str(c).strip()]
        if "txt" in raw:
            return [ln.strip() for ln in raw["txt"].decode("utf-8").splitlines() if ln.strip()]
        return []

    def __iter__(self) -> Iterator[Tuple[np.ndarray, List[str]]]:
        for path in self.urls:
            for raw in iter_tar_samples(path):
                ext = next((e for e in IMAGE_EXTS if e in raw), None)
                try:
                    caps = self.captions_of(raw)
                    if ext is None or not caps:
                        log.warning("retrieval sample %s: no %s; skipped", raw["__key__"], "image" if ext is None else "caption")
                        continue
                    image = _decode_rgb(io.BytesIO(raw[ext]))
                except Exception as e:   # noqa: BLE001 -- whatever a broken member raises
                    log.warning("retrieval sample %s: %r; skipped", raw["__key__"], e)
                    continue
                yield image, caps


def shard_indices(n: int, rank: int = 0, world: int = 1) -> range:
    """This rank's share of n samples: rank, rank + world, ...  An exact partition -- unlike DistributedSampler nothing is
    padded, so no sample is counted twice and the ranks' shares may differ in size by one."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} of {world}")
    return range(rank, n, world)


def _vision_batch(images: List[np.ndarray]) -> dict:
    # the vision half of the ragged batch (image_data.ragged_image_collate); the text slot carries a placeholder embedding
    return ragged_image_collate([(im, np.zeros(1, np.float32)) for im in images])["vision"]


def _collate_labelled(items):
    return {"vision": _vision_batch([it[0] for it in items]), "labels": torch.tensor([it[1] for it in items], dtype=torch.int64)}


def zeroshot_loader(dataset, batch_size: int = 128, rank: int = 0, world: int = 1, workers: int = 0):
    """Batches {"vision": ragged batch, "labels": (b) int64} over this rank's shard_indices of a map-style dataset of
    (image, label, ...) items; the workers decode only."""
    sub = torch.utils.data.Subset(dataset, list(shard_indices(len(dataset), rank, world)))
    return torch.utils.data.DataLoader(sub, batch_size=batch_size, shuffle=False, num_workers=workers,
                                       collate_fn=_collate_labelled)


# ---- evaluation --------------------------------------------------------------------------------------------------------------
class _eval_mode:
    """eval() + no_grad over `model` and its towers (a DualEncoder's `text` / `vision`); training modes restored on exit."""

    def __init__(self, model):
        self.mods = [model] + [t for t in (getattr(model, "text", None), getattr(model, "vision", None)) if t is not None]

    def __enter__(self):
        self.was = [m.training for m in self.mods]
        for m in self.mods:
            m.eval()
        self.ng = torch.no_grad()
        self.ng.__enter__()

    def __exit__(self, *exc):
        self.ng.__exit__(*exc)
        for m, w in zip(self.mods, self.was):
            m.train(w)


def _embed_vision(vision_tower, image_transform, vision) -> torch.Tensor:
    px = image_transform(vision) if "pixels_u8" in vision else vision["input_ids"].to(vision_tower.device)
    return vision_tower(input_ids=px, normalize=True)["embedding"].float()


def _index_of(x: torch.Tensor) -> FlatIPIndex:
    d = x.shape[1]
    if d % 64 or not 64 <= d <= 1024:
        raise ValueError(f"the rank kernel takes embedding widths that are multiples of 64 in [64, 1024], got {d}")
    ix = FlatIPIndex(d, device=x.device)
    ix.add(x)
    return ix


def evaluate_zeroshot(model, loader, classifier: torch.Tensor, image_transform, ks: Sequence[int] = (1, 5)) -> Dict[str, float]:
    """{"top1_acc", "top5_acc", "n"} of the image tower of `model` (a DualEncoder, or the vision BiEncoder itself) against the
    (C, D) `classifier` over `loader` (zeroshot_loader batches).  image_transform: an eval-mode GpuImageTransform.  Under an
    initialised process group the hit and sample counts are summed over ranks before the one division."""
    vision = getattr(model, "vision", model)
    ix = _index_of(classifier.to(vision.device))
    hits, n = [0] * len(ks), 0
    with _eval_mode(model):
        for batch in loader:
            emb = _embed_vision(vision, image_transform, batch["vision"])
            ranks, _, _ = ix.rank(emb, batch["labels"])
            hits = [h + x for h, x in zip(hits, topk_hits(ranks, ks))]
            n += int(batch["labels"].numel())
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        tot = torch.tensor(hits + [n], dtype=torch.int64, device=vision.device)
        dist.all_reduce(tot)
        hits, n = [int(x) for x in tot[:-1]], int(tot[-1])
    if n == 0:
        raise ValueError("evaluate_zeroshot: no samples")
    out = {f"top{k}_acc": h / n for k, h in zip(ks, hits)}
    out["n"] = n
    return out


def evaluate_retrieval(model, dataset, tokenizer, image_transform, seq_len: int = 77, prefix: Optional[str] = None,
                       add_eos: bool = False, batch_size: int = 128, ks: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
    """clip_benchmark's zeroshot_retrieval metrics of a DualEncoder over (image, [captions]) samples:
    image_retrieval_recall@k (rows = captions, corpus = images, one positive each), text_retrieval_recall@k (rows = images,
    corpus = captions, all of an image's captions positive) and mean_recall@1 = 0.5 (text@1 + image@1)
    (sc/trainers/image_text.py:236).  Runs on the calling rank alone, as the reference does on rank 0."""
    images, texts, cap_img = [], [], []
    with _eval_mode(model):
        pend: List[np.ndarray] = []

        def flush():
            if pend:
                images.append(_embed_vision(model.vision, image_transform, _vision_batch(pend)))
                pend.clear()

        n_img = 0
        for image, caps in dataset:
            pend.append(image)
            texts += caps
            cap_img += [n_img] * len(caps)
            n_img += 1
            if len(pend) == batch_size:
                flush()
        flush()
        if not n_img:
            raise ValueError("evaluate_retrieval: no samples")
        img = torch.cat(images)
        eos = getattr(tokenizer, "eos_token", None)
        if add_eos and not eos:
            raise ValueError("add_eos needs the tokenizer's eos_token")
        texts = [(t + eos if add_eos else t) for t in texts]
        if prefix:
            texts = [f"{prefix}: {t}" for t in texts]
        txt = encode(model.text, texts, tokenizer, batch_size=batch_size, max_length=seq_len)
    cap_img_t = torch.tensor(cap_img, dtype=torch.int64)
    out = {}
    ranks, _, ptr = _index_of(img).rank(txt, cap_img_t)
    for k, v in zip(ks, retrieval_recall(ranks, ptr, ks)):
        out[f"image_retrieval_recall@{k}"] = v
    lists = [[] for _ in range(n_img)]
    for c, m in enumerate(cap_img):
        lists[m].append(c)
    ranks, _, ptr = _index_of(txt).rank(img, lists)
    for k, v in zip(ks, retrieval_recall(ranks, ptr, ks)):
        out[f"text_retrieval_recall@{k}"] = v
    if 1 in ks:
        out["mean_recall@1"] = 0.5 * (out["text_retrieval_recall@1"] + out["image_retrieval_recall@1"])
    return out


def eval_data_from_config(config) -> dict:
    """{"imagenet": (ImageFolderDataset, meta)} when data_args.imagenet_val_path and zeroshot_meta_path are set, {"flickr":
    RetrievalEvalDataset} when retrieval_eval_shards is; empty when the recipe names no evaluation data."""
    da, data = config.data_args, {}
    if da.imagenet_val_path and da.zeroshot_meta_path:
        meta = load_zeroshot_meta(da.zeroshot_meta_path)
        data["imagenet"] = (ImageFolderDataset(da.imagenet_val_path, meta["folders"]), meta)
    if da.retrieval_eval_shards:
        data["flickr"] = RetrievalEvalDataset(da.retrieval_eval_shards)
    return data


def evaluate_from_config(model, config, data: dict, tokenizer, image_transform, rank: int = 0, world: int = 1) -> dict:
    """One evaluation of a DualEncoder as the recipe describes it (sc/trainers/image_text.py:198-254): top1_acc / top5_acc over
    data["imagenet"], flickr/<metric> over data["flickr"].  The prompts and captions get the "search_query" prefix under
    add_prefix and no EOS token, as the reference's eval_loop calls its evaluators.  The classifier is built here, at every call.  Zero-shot runs on every rank over its share of the
    images; retrieval on rank 0 alone, as in the reference, with a barrier behind it."""
    import torch.distributed as dist

    ta, da = config.text_model_args, config.data_args
    prefix = "search_query" if ta.add_prefix else None
    bs = da.eval_batch_size or 128
    out = {}
    if "imagenet" in data:
        ds, meta = data["imagenet"]
        clf = zeroshot_classifier_weights(model.text, tokenizer, meta["classnames"], meta["templates"], prefix=prefix,
                                          seq_len=ta.seq_len)
        loader = zeroshot_loader(ds, batch_size=max(1, bs // world), rank=rank, world=world, workers=da.workers)
        res = evaluate_zeroshot(model, loader, clf, image_transform)
        out.update({"top1_acc": res["top1_acc"], "top5_acc": res["top5_acc"]})
    if "flickr" in data:
        if rank == 0:
            res = evaluate_retrieval(model, data["flickr"], tokenizer, image_transform, seq_len=ta.seq_len, prefix=prefix,
                                     batch_size=min(bs, 128))
            out.update({"flickr/" + k: v for k, v in res.items()})
        if world > 1 and dist.is_available() and dist.is_initialized():
            dist.barrier()
    return out
