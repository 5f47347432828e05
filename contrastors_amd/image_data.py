"""Image-text loader (host-side counterpart of sc/dataset/image_text_loader.py:367-545): webdataset-style tar shards of
`<key>.jpg|jpeg|png|webp` + `<key>.txt` (or `<key>.npy` text embeddings for LiT's `precomputed: true`) on a local / mounted
file system, read with the stdlib `tarfile`.  The workers decode only (`Image.open(...).convert("RGB")` -> uint8 array);
crop, resize and normalize run on the GPU (image_transform.GpuImageTransform), so a batch leaves here RAGGED:

    {"vision": {"pixels_u8": (sum 3 h w) uint8, "offsets": (B + 1) int64, "sizes": (B, 2) int32}, "text": {...}}

`text` is what the reference's `tokenize` gives, stacked (`padding="max_length"`, `truncation=True`, the text tower's
`seq_len`, `"search_query: "` prefix under `add_prefix`), or {"text_embs": (B, d)} when precomputed.

Order: shards are shuffled per (seed, epoch) -- the same permutation on every rank --, dealt to ranks, then to loader
workers; each worker shuffles samples through a bounded buffer seeded by (seed, epoch, rank, worker).  The stream is this
loader's own and repeatable for one (seed, epoch, rank, workers); it is not webdataset's.  Train yields full batches only,
eval also the last partial one.  The S3 transport, `dataset_resampled` and the MLM collator (`mlm_prob`) are not built.
"""
from __future__ import annotations

import io
import logging
import random
import re
import tarfile
from typing import Iterator, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, IterableDataset, get_worker_info

from .data import expand_urls

IMAGE_EXTS = ("jpg", "jpeg", "png", "webp")
SAMPLE_SHUFFLE_SIZE = 5000   # sc/dataset/image_text_loader.py:25
_BASE_PLUS_EXT = re.compile(r"^((?:.*/|)[^.]+)[.]([^/]*)$")   # webdataset's base_plus_ext: the key ends at the first dot

log = logging.getLogger(__name__)


def tokenize_texts(texts: List[str], tokenizer, seq_len: int, add_eos: bool = False, add_prefix: bool = False) -> dict:
    """sc/dataset/image_text_loader.py:367-376 over a list: one tokenizer call per batch, rows as the reference stacks them."""
    if add_eos:
        texts = [t + tokenizer.eos_token for t in texts]
    if add_prefix:
        texts = [f"search_query: {t}" for t in texts]
    tok = tokenizer(texts, padding="max_length", truncation=True, max_length=seq_len, return_tensors="pt")
    if add_eos:
        tok["input_ids"][:, -1] = tokenizer.eos_token_id
    return dict(tok)


def ragged_image_collate(samples: List[Tuple[np.ndarray, object]], tokenizer=None, seq_len: Optional[int] = None,
                         add_eos: bool = False, add_prefix: bool = False) -> dict:
    """[(H x W x 3 uint8 image, caption str | embedding array)] -> the ragged batch above."""
    images = [np.ascontiguousarray(s[0], dtype=np.uint8) for s in samples]
    for im in images:
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f"expected H x W x 3 images, got {im.shape}")
    offsets = np.zeros(len(images) + 1, np.int64)
    np.cumsum([im.size for im in images], out=offsets[1:])
    vision = {"pixels_u8": torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])),
              "offsets": torch.from_numpy(offsets),
              "sizes": torch.tensor([im.shape[:2] for im in images], dtype=torch.int32)}
    texts = [s[1] for s in samples]
    if isinstance(texts[0], np.ndarray):
        text = {"text_embs": torch.from_numpy(np.stack(texts))}
    else:
        text = tokenize_texts(texts, tokenizer, seq_len, add_eos=add_eos, add_prefix=add_prefix)
    return {"vision": vision, "text": text}


def iter_tar_samples(path: str) -> Iterator[dict]:
    """Consecutive members of one key -> {"__key__", ext: bytes, ...} (extensions lower-cased), as webdataset groups them.
    A tar that breaks off mid-way ends its own stream with a log line, not the caller's."""
    current = None
    try:
        with tarfile.open(path, "r|*") as tf:
            for member in tf:
                if not member.isfile():
                    continue
                m = _BASE_PLUS_EXT.match(member.name)
                if not m:
                    continue
                key, ext = m.group(1), m.group(2).lower()
                if current is None or key != current["__key__"] or ext in current:
                    if current is not None:
                        yield current
                    current = {"__key__": key}
                current[ext] = tf.extractfile(member).read()
    except (tarfile.TarError, EOFError, OSError) as e:
        log.warning("image-text shard %s: %r; the rest of the shard is skipped", path, e)
    if current is not None:
        yield current


class TarImageTextDataset(IterableDataset):
    def __init__(self, shards: str, batch_size: int, tokenizer=None, seq_len: int = 77, is_train: bool = True, seed: int = 42,
                 epoch: int = 0, add_eos: bool = False, add_prefix: bool = False, precomputed: bool = False,
                 shuffle_buffer: int = SAMPLE_SHUFFLE_SIZE, rank: Optional[int] = None, world_size: Optional[int] = None,
                 dataset_resampled: bool = False, mlm_prob: Optional[float] = None, infinite: bool = False, worker=None):
        if dataset_resampled:
            raise NotImplementedError("data_args.dataset_resampled (sampling shards with replacement) is not served")
        if mlm_prob:
            raise NotImplementedError("data_args.mlm_prob with image-text shards (the MLM collator of three-tower training)")
        self.urls = [u for part in str(shards).split("::") for u in expand_urls(part)]
        if any(u.startswith("s3://") for u in self.urls):
            raise NotImplementedError("s3:// shards: mount the bucket and point `image_text_shards` at the local path")
        if not precomputed and tokenizer is None:
            raise ValueError("a tokenizer is needed unless the shards carry precomputed text embeddings")
        if dist.is_available() and dist.is_initialized():
            rank = dist.get_rank() if rank is None else rank
            world_size = dist.get_world_size() if world_size is None else world_size
        self.rank, self.world_size = rank or 0, world_size or 1
        if batch_size % self.world_size:
            raise ValueError(f"global batch {batch_size} is not divisible by {self.world_size} ranks")
        self.rank_batch_size = batch_size // self.world_size
        self.tokenizer, self.seq_len, self.is_train, self.seed, self.epoch = tokenizer, seq_len, is_train, seed, epoch
        self.add_eos, self.add_prefix, self.precomputed = add_eos, add_prefix, precomputed
        self.shuffle_buffer, self.infinite = max(int(shuffle_buffer), 1), infinite
        self.worker = worker   # (id, count) instead of torch's worker info: tests, or a caller with its own process pool
        self.skipped = 0

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    # ---- which shards ------------------------------------------------------------------------------------------------
    def _worker(self) -> Tuple[int, int]:
        if self.worker is not None:
            return self.worker
        info = get_worker_info()
        return (info.id, info.num_workers) if info is not None else (0, 1)

    def shards_for(self, epoch: int, rank: int, worker: int, num_workers: int) -> List[str]:
        urls = list(self.urls)
        if self.is_train:
            random.Random(self.seed + epoch).shuffle(urls)
        return urls[rank::self.world_size][worker::num_workers]

    # ---- samples -----------------------------------------------------------------------------------------------------
    def _decode(self, raw: dict):
        """(image array, caption | embedding) or None (logged): a sample without an image or a text part, an empty caption
        (sc/dataset/image_text_loader.py:221-227) or bytes that do not decode."""
        from PIL import Image

        img_ext = next((e for e in IMAGE_EXTS if e in raw), None)
        text_ext = "npy" if self.precomputed else "txt"
        if img_ext is None or text_ext not in raw:
            log.warning("image-text sample %s: no %s; skipped", raw["__key__"], "image" if img_ext is None else text_ext)
            return None
        try:
            if self.precomputed:
                text = np.load(io.BytesIO(raw["npy"]), allow_pickle=False)
            else:
                text = raw["txt"].decode("utf-8").strip()
                if len(text) < 2:
                    log.warning("image-text sample %s: empty caption; skipped", raw["__key__"])
                    return None
            with Image.open(io.BytesIO(raw[img_ext])) as im:
                image = np.asarray(im.convert("RGB"), dtype=np.uint8)
        except Exception as e:   # noqa: BLE001 -- whatever a broken member raises (PIL has no common base class for it)
            log.warning("image-text sample %s: %r; skipped", raw["__key__"], e)
            return None
        return image, text

    def _samples(self, epoch: int) -> Iterator[tuple]:
        wid, nw = self._worker()
        rng = random.Random(f"{self.seed}-{epoch}-{self.rank}-{wid}-{nw}")
        buf = []
        for path in self.shards_for(epoch, self.rank, wid, nw):
            for raw in iter_tar_samples(path):
                sample = self._decode(raw)
                if sample is None:
                    self.skipped += 1
                    continue
                if not self.is_train:
                    yield sample
                    continue
                buf.append(sample)
                if len(buf) >= self.shuffle_buffer:
                    i = rng.randrange(len(buf))
                    buf[i], buf[-1] = buf[-1], buf[i]
                    yield buf.pop()
        rng.shuffle(buf)
        yield from buf

    def __iter__(self) -> Iterator[dict]:
        epoch = self.epoch
        batch = []
        while True:
            n = 0
            for sample in self._samples(epoch):
                n += 1
                batch.append(sample)
                if len(batch) == self.rank_batch_size:
                    yield self._collate(batch)
                    batch = []
            if not (self.infinite and self.is_train and n):
                break
            epoch += 1   # the next pass: a new shard order and sample shuffle, the open batch carries over
        if batch and not self.is_train:
            yield self._collate(batch)

    def _collate(self, batch):
        return ragged_image_collate(batch, self.tokenizer, self.seq_len, add_eos=self.add_eos, add_prefix=self.add_prefix)


def get_image_text_loader(config, tokenizer, is_train: bool = True, epoch: int = 0, infinite: bool = False) -> DataLoader:
    """The construction sc/trainers/image_text.py:70-90 does from the YAML sections (the dataset yields whole per-rank batches)."""
    da, ta = config.data_args, config.text_model_args
    if not da.image_text_shards:
        raise ValueError("data_args.image_text_shards is not set")
    batch = da.batch_size if is_train or not da.eval_batch_size else da.eval_batch_size
    ds = TarImageTextDataset(da.image_text_shards, batch, tokenizer, seq_len=ta.seq_len, is_train=is_train, seed=da.seed,
                             epoch=epoch, add_eos=ta.nomic_encoder is not True, add_prefix=ta.add_prefix,
                             precomputed=bool(ta.precomputed), dataset_resampled=bool(da.dataset_resampled),
                             mlm_prob=da.mlm_prob, infinite=infinite)
    if is_train and da.workers * ds.world_size > len(ds.urls):   # image_text_loader.py:500-502
        raise ValueError(f"number of shards must be >= total workers: {len(ds.urls)} >= {da.workers * ds.world_size}")
    return DataLoader(ds, batch_size=None, shuffle=False, num_workers=da.workers, persistent_workers=da.workers > 0)
