"""The data path of the MLM recipe (sc/trainers/mlm.py:54-99): a LOCAL pre-tokenized dataset, the reference's train / validation
split, a map-style loader whose batch order is a pure function of (seed, epoch), and the masking.

The reference draws the masks in the collator on its CPU workers (transformers.DataCollatorForLanguageModeling).  Here the
workers only read rows: `GpuMlmMasker` draws the masks on the device with `cx_mlm_mask` (csrc/mlm_mask.hip), one
launch per micro-batch, from the Philox generator of the dropout kernels -- the masks depend on (seed, micro-batch ordinal, rank,
token position) and on nothing else: not on the worker count, and a resumed run redraws the ones the interrupted run would have
seen.  `data_args.mask_on: host` keeps the reference's collator (`contrastors_amd.mlm.mask_tokens`, bit for bit under the same
generator state) for anyone who needs that stream.

Sources: a directory written by `datasets.Dataset.save_to_disk` / `DatasetDict.save_to_disk` (its `train` split), or a `.npy`
of shape (N, S) with an integer dtype (memory-mapped).  Nothing here resolves a name remotely: a path that does not exist is a
FileNotFoundError before any library is called (the recipe's literal `tokenized_dataset` is a hub id and needs a local copy).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_SPECIAL_IDS = 16   # the special-id list of cx_mlm_mask


@dataclass(frozen=True)
class MlmTokenInfo:
    """What the masking needs from the tokenizer: `mask_token_id`, `all_special_ids`, and `len(tokenizer)` -- the range of the
    random replacement words as the collator draws them (NOT the padded vocabulary of the model)."""
    mask_token_id: int
    special_ids: Tuple[int, ...]
    vocab_size: int

    def __post_init__(self):
        object.__setattr__(self, "special_ids", tuple(int(i) for i in self.special_ids))
        if self.mask_token_id is None:
            raise ValueError("the tokenizer has no mask token: masked language modelling needs one")
        if int(self.vocab_size) < 1:
            raise ValueError(f"vocab_size {self.vocab_size} < 1")

    @classmethod
    def from_tokenizer(cls, tok) -> "MlmTokenInfo":
        return cls(mask_token_id=tok.mask_token_id, special_ids=tuple(tok.all_special_ids), vocab_size=len(tok))


# ---- sources --------------------------------------------------------------------------------------------------------------------
class NpyTokens:
    """Rows of a memory-mapped (N, S) integer array (optionally a subset of them, in a given order): column `input_ids` only."""
    column_names = ["input_ids"]

    def __init__(self, array, indices: Optional[np.ndarray] = None):
        if array.ndim != 2 or not np.issubdtype(array.dtype, np.integer):
            raise ValueError(f"a tokenized .npy is (N, S) of an integer dtype, got {array.shape} {array.dtype}")
        self.array = array
        self.indices = None if indices is None else np.asarray(indices, dtype=np.int64)

    def __len__(self):
        return int(self.array.shape[0] if self.indices is None else self.indices.shape[0])

    def select(self, indices) -> "NpyTokens":
        indices = np.asarray(indices, dtype=np.int64)
        return NpyTokens(self.array, indices if self.indices is None else self.indices[indices])

    def rows(self, idx: Sequence[int]) -> Dict[str, np.ndarray]:
        idx = np.asarray(idx, dtype=np.int64)
        if self.indices is not None:
            idx = self.indices[idx]
        return {"input_ids": np.stack([self.array[i] for i in idx])}


def load_tokenized_dataset(path: str):
    """A `datasets.Dataset` (a `save_to_disk` directory; of a DatasetDict, its `train` split) or `NpyTokens` (a .npy file)."""
    path = os.fspath(path)
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"data_args.tokenized_dataset {path!r} is not a local path: this loader reads a local copy only (a directory written "
            "by datasets' save_to_disk, or an (N, S) .npy); a hub id such as the recipe's needs to be saved to disk first")
    if os.path.isfile(path):
        if not path.endswith(".npy"):
            raise ValueError(f"{path!r}: a tokenized dataset file is a .npy of shape (N, S)")
        return NpyTokens(np.load(path, mmap_mode="r", allow_pickle=False))
    import datasets

    ds = datasets.load_from_disk(path)
    if isinstance(ds, datasets.DatasetDict):
        if "train" not in ds:
            raise KeyError(f"{path!r}: a DatasetDict without a 'train' split (has {sorted(ds)})")
        ds = ds["train"]
    if "input_ids" not in ds.column_names:
        raise KeyError(f"{path!r}: no 'input_ids' column (has {ds.column_names})")
    return ds


def split_train_val(ds, val_pct: Optional[float], seed: int):
    """(train, val); val is None when val_pct is None or 0.  A `datasets.Dataset` is split by the reference's own two calls
    (sc/trainers/mlm.py:59-60).  The .npy source is split by THIS project's rule (there is no reference for it): a numpy
    permutation under `seed`, the first ceil(val_pct * N) rows of it are the validation set, the rest the training set."""
    if isinstance(ds, NpyTokens):
        if not val_pct:
            return ds, None
        n = len(ds)
        perm = np.random.default_rng(seed).permutation(n)
        n_val = int(math.ceil(val_pct * n))
        if not 0 < n_val < n:
            raise ValueError(f"val_pct {val_pct} of {n} rows leaves an empty split")
        return ds.select(perm[n_val:]), ds.select(perm[:n_val])
    if not val_pct:
        return ds.shuffle(seed=seed), None
    split = ds.shuffle(seed=seed).train_test_split(test_size=val_pct, seed=seed)
    return split["train"], split["test"]


_COLUMNS = ("input_ids", "attention_mask", "special_tokens_mask")


class MlmRows(torch.utils.data.Dataset):
    """Map-style view of a source: a whole batch of rows per fetch, as numpy arrays of the columns the source has."""

    def __init__(self, source):
        self.columns = [c for c in _COLUMNS if c in source.column_names]
        if "input_ids" not in self.columns:
            raise KeyError(f"no 'input_ids' column (has {list(source.column_names)})")
        self.npy = isinstance(source, NpyTokens)
        self.source = source if self.npy else source.with_format("numpy", columns=self.columns)

    def __len__(self):
        return len(self.source)

    def __getitems__(self, idx: List[int]) -> Dict[str, np.ndarray]:
        if self.npy:
            return self.source.rows(idx)
        got = self.source[list(idx)]
        out = {}
        for c in self.columns:
            v = got[c]
            out[c] = v if isinstance(v, np.ndarray) and v.dtype != object else np.stack([np.asarray(r) for r in v])
        return out


class MlmBatchOrder(torch.utils.data.Sampler):
    """The batches of one rank for one epoch, as index lists.  Shuffled: the permutation `torch.randperm(N)` under
    `seed + epoch`, padded by its own head to a multiple of `world` and sharded `[rank::world]` -- what DistributedSampler does
    (the reference's sampler, sc/trainers/mlm.py:63-65); unshuffled: `arange(N)` sharded the same way.  The rank's run is cut
    into batches of `batch` rows, the short last one dropped (`drop_last=True` there).  `set_epoch(epoch, start_batch)` moves to
    another epoch and / or skips the first batches WITHOUT reading them (a resume)."""

    def __init__(self, n: int, batch: int, rank: int = 0, world: int = 1, seed: int = 0, epoch: int = 0, shuffle: bool = True,
                 start_batch: int = 0):
        if batch < 1:
            raise ValueError(f"per-rank batch {batch} < 1 (batch_size smaller than the world size?)")
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside 0..{world - 1}")
        self.n, self.batch, self.rank, self.world, self.seed, self.shuffle = int(n), int(batch), rank, world, int(seed), shuffle
        self.num_batches = ((self.n + world - 1) // world) // self.batch   # of a whole epoch, whatever start_batch is
        self.set_epoch(epoch, start_batch)

    def set_epoch(self, epoch: int, start_batch: int = 0):
        if not 0 <= start_batch <= self.num_batches:
            raise ValueError(f"start_batch {start_batch} outside 0..{self.num_batches}")
        self.epoch, self.start_batch = int(epoch), int(start_batch)

    def indices(self) -> np.ndarray:
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            order = torch.randperm(self.n, generator=g).numpy()
        else:
            order = np.arange(self.n, dtype=np.int64)
        total = (self.n + self.world - 1) // self.world * self.world
        if total > self.n:
            order = np.concatenate([order, order[: total - self.n]])
        return order[self.rank:total:self.world]

    def __len__(self):
        return self.num_batches - self.start_batch

    def __iter__(self) -> Iterator[List[int]]:
        mine = self.indices()
        for b in range(self.start_batch, self.num_batches):
            yield mine[b * self.batch:(b + 1) * self.batch].tolist()


class MlmCollate:
    """device: stack only -- int32 ids and the masks the dataset has (`GpuMlmMasker` finishes the batch on the GPU).
    host: the reference's collator, `mask_tokens` on the global torch generator, special tokens from the dataset's
    `special_tokens_mask` or else from the tokenizer's special ids."""

    def __init__(self, info: MlmTokenInfo, p: float, mask_on: str = "device"):
        if mask_on not in ("device", "host"):
            raise ValueError(f"mask_on must be device or host, got {mask_on!r}")
        self.info, self.p, self.mask_on = info, float(p), mask_on

    def __call__(self, rows: Dict[str, np.ndarray]) -> Dict[str, torch.Tensor]:
        ids = np.ascontiguousarray(rows["input_ids"])
        am = rows.get("attention_mask")
        sm = rows.get("special_tokens_mask")
        if self.mask_on == "device":
            out = {"input_ids": torch.from_numpy(ids.astype(np.int32, copy=False))}
            if am is not None:
                out["attention_mask"] = torch.from_numpy(np.ascontiguousarray(am).astype(np.int64, copy=False))
            if sm is not None:
                out["special_tokens_mask"] = torch.from_numpy(np.ascontiguousarray(sm).astype(np.uint8, copy=False))
            return out
        from .mlm import mask_tokens

        ids_t = torch.from_numpy(ids.astype(np.int64, copy=False))
        if sm is not None:
            special = torch.from_numpy(np.ascontiguousarray(sm).astype(np.bool_, copy=False))
        else:
            special = torch.isin(ids_t, torch.tensor(self.info.special_ids, dtype=torch.long))
        masked, labels = mask_tokens(ids_t, special, self.p, self.info.mask_token_id, self.info.vocab_size)
        out = {"input_ids": masked, "labels": labels}
        if am is not None:
            out["attention_mask"] = torch.from_numpy(np.ascontiguousarray(am).astype(np.int64, copy=False))
        return out


def _loader(source, order: MlmBatchOrder, collate: MlmCollate, workers: int):
    return torch.utils.data.DataLoader(MlmRows(source), batch_sampler=order, collate_fn=collate, num_workers=workers,
                                       persistent_workers=workers > 0)


def get_mlm_loaders(config, info: MlmTokenInfo, rank: int = 0, world: int = 1, epoch: int = 0, start_batch: int = 0) -> dict:
    """{"train": DataLoader, "val": DataLoader or None, "test": None, "info": info} for `MLMTrainer.fit` (the dictionary of
    sc/trainers/mlm.py:99).  Per-rank batch `batch_size // world`, `drop_last`, `workers` from the recipe; the training order is
    `MlmBatchOrder` under (data_args.seed, epoch), the validation set is unshuffled with `eval_batch_size` (or `batch_size`)."""
    da = config.data_args
    if not da.tokenized_dataset:
        raise ValueError("data_args.tokenized_dataset is not set")
    train, val = split_train_val(load_tokenized_dataset(da.tokenized_dataset), da.val_pct, da.seed)
    p = da.mlm_prob if da.mlm_prob is not None else 0.3
    p_val = da.val_mlm_prob if da.val_mlm_prob is not None else p
    order = MlmBatchOrder(len(train), da.batch_size // world, rank, world, seed=da.seed, epoch=epoch, shuffle=True,
                          start_batch=start_batch)
    if order.num_batches < 1:
        raise ValueError(f"{len(train)} training rows do not fill one batch of {da.batch_size}")
    loaders = {"train": _loader(train, order, MlmCollate(info, p, da.mask_on), da.workers), "val": None, "test": None, "info": info}
    if val is not None:
        vorder = MlmBatchOrder(len(val), (da.eval_batch_size or da.batch_size) // world, rank, world, shuffle=False)
        loaders["val"] = _loader(val, vorder, MlmCollate(info, p_val, da.mask_on), da.workers)
    return loaders


# ---- masking on the device ------------------------------------------------------------------------------------------------------
def mlm_mask(ids: torch.Tensor, p: float, seed: int, offset: int, mask_token_id: int, random_vocab: int,
             attention_mask: Optional[torch.Tensor] = None, special_mask: Optional[torch.Tensor] = None,
             special_ids: Optional[torch.Tensor] = None):
    """`cx_mlm_mask` on device tensors: ids (B, S) int32 / int64 with unit column stride (any row stride >= S), attention_mask
    (B, S) int64 and special_mask (B, S) uint8 contiguous, special_ids a device int64 vector of at most 16 -> (out_ids, labels)
    int64.  Enqueues one kernel on the current stream; allocates the two outputs."""
    from . import _C

    if ids.dim() != 2 or not ids.is_cuda or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"ids: a (B, S) int32 / int64 device tensor, got {tuple(ids.shape)} {ids.dtype} on {ids.device}")
    B, S = ids.shape
    if S > 1 and ids.stride(1) != 1:
        raise ValueError("ids: the token axis must be contiguous")
    stride = ids.stride(0) if B > 1 else max(S, 1)
    for name, t, dt in (("attention_mask", attention_mask, torch.int64), ("special_mask", special_mask, torch.uint8)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (B, S) or not t.is_contiguous() or t.device != ids.device):
            raise ValueError(f"{name}: a contiguous (B, S) {dt} tensor on the device of ids")
    n_special = 0
    if special_ids is not None and special_ids.numel():
        if special_ids.dtype != torch.int64 or special_ids.dim() != 1 or not special_ids.is_contiguous() or special_ids.device != ids.device:
            raise ValueError("special_ids: a contiguous int64 vector on the device of ids")
        n_special = special_ids.numel()
    out = torch.empty((B, S), dtype=torch.int64, device=ids.device)
    labels = torch.empty((B, S), dtype=torch.int64, device=ids.device)
    with torch.cuda.device(ids.device):
        rc = _C.lib().cx_mlm_mask(_C.ptr(ids), int(ids.dtype == torch.int64), stride, _C.ptr(attention_mask), _C.ptr(special_mask),
                                  _C.ptr(special_ids) if n_special else None, n_special, int(mask_token_id), int(random_vocab),
                                  float(p), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _C.ptr(out), _C.ptr(labels),
                                  B, S, _C.cur_stream())
    _C.check(rc, "cx_mlm_mask")
    return out, labels


class GpuMlmMasker:
    """`masker(batch, ordinal, rank, world)`: a stacked batch of the loader -> {"input_ids", "attention_mask", "labels"} on the
    device.  The Philox offset is `ordinal * world + rank`: in training `ordinal` is the micro-batch count since the start of the
    run (saved with the trainer state); in evaluation it is the position of the batch in the validation set, under `seed + 1`
    and `val_mlm_prob`, so every evaluation sees the same masks."""

    def __init__(self, info: MlmTokenInfo, p: float, seed: int, device=None):
        if len(info.special_ids) > MAX_SPECIAL_IDS:
            raise ValueError(f"{len(info.special_ids)} special token ids: the masking kernel takes at most {MAX_SPECIAL_IDS} "
                             "(pass the rest through the dataset's special_tokens_mask, or use mask_on: host)")
        if not 0.0 <= float(p) < 1.0:
            raise ValueError(f"mlm probability {p} outside [0, 1)")
        self.info, self.p, self.seed = info, float(p), int(seed)
        self.device = torch.device(device or f"cuda:{torch.cuda.current_device()}")
        self._special = torch.tensor(info.special_ids, dtype=torch.int64, device=self.device)

    def __call__(self, batch: Dict[str, torch.Tensor], ordinal: int, rank: int = 0, world: int = 1) -> Dict[str, torch.Tensor]:
        ids = batch["input_ids"].to(self.device, non_blocking=True)
        am, sm = batch.get("attention_mask"), batch.get("special_tokens_mask")
        if am is not None:
            am = am.to(self.device, torch.int64, non_blocking=True).contiguous()
        if sm is not None:
            sm = sm.to(self.device, torch.uint8, non_blocking=True).contiguous()
        out, labels = mlm_mask(ids, self.p, self.seed, int(ordinal) * int(world) + int(rank), self.info.mask_token_id,
                               self.info.vocab_size, am, sm, self._special)
        return {"input_ids": out, "attention_mask": am, "labels": labels}
