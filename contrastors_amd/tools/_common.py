"""Shared pieces of the curation tools: the reference's shard layout, embedding sources, exact search."""
from __future__ import annotations

import gzip
import json
from pathlib import Path
from typing import List, Optional

import numpy as np

SHARD_SIZE = 100_000   # records per shard-%05d.jsonl.gz (get_negatives.py:199, mine_beir_negatives_full.py:147)


def triplet_metadata(query_key: str, document_key: str, negatives_key: str) -> dict:
    return {"objective": {"self": [], "paired": [], "triplet": [[query_key, document_key, negatives_key]]}}


def write_shards(records: List[dict], output_dir, metadata: dict, shard_size: int = SHARD_SIZE) -> List[Path]:
    """Every record gets `metadata` (None: the records keep their own); shard-00000.jsonl.gz, ... of `shard_size` records
    each (the reference's writer)."""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    paths = []
    for start in range(0, len(records), shard_size):
        p = out / f"shard-{start // shard_size:05d}.jsonl.gz"
        with gzip.open(p, "wt") as f:
            for rec in records[start: start + shard_size]:
                if metadata is not None:
                    rec["metadata"] = metadata
                f.write(json.dumps(rec) + "\n")
        paths.append(p)
    return paths


def load_npy(path, n: Optional[int], what: str, mmap: bool = False) -> np.ndarray:
    """mmap: map the file instead of reading it (the binary coarse search only ever gathers candidate rows from it).
    n = None: any number of rows."""
    x = np.load(path, mmap_mode="r" if mmap else None)
    if x.ndim != 2 or (n is not None and x.shape[0] != n):
        raise SystemExit(f"error: {what} embeddings {path} have shape {x.shape}, expected ({'n' if n is None else n}, d)")
    return x


def encode_texts(texts: List[str], checkpoint: Optional[str], tokenizer_path: Optional[str], batch_size: int,
                 max_length: int, device: str, prefix: str = ""):
    """Embeddings of `texts` from a local BiEncoder checkpoint (save_pretrained layout) and a local tokenizer."""
    if not checkpoint or not tokenizer_path:
        raise SystemExit("error: without .npy embeddings both --model and --tokenizer (local paths) are required")
    from transformers import AutoTokenizer

    from ..biencoder import BiEncoder, BiEncoderConfig
    from ..nomic_bert import NomicBertConfig
    from ..search import encode

    cfg = json.loads((Path(checkpoint) / "config.json").read_text())
    fields = {k: v for k, v in cfg.items() if k in BiEncoderConfig.__dataclass_fields__ and k != "trunk_config"}
    if cfg.get("trunk_type") != "NomicBertConfig":
        raise SystemExit(f"error: {checkpoint} is not a text BiEncoder (trunk_type {cfg.get('trunk_type')!r})")
    fields["trunk_config"] = NomicBertConfig(**cfg["trunk_config"])
    model = BiEncoder(BiEncoderConfig(**fields), device=device)
    model.load_pretrained(checkpoint)
    tok = AutoTokenizer.from_pretrained(tokenizer_path, local_files_only=True)
    return encode(model, [prefix + t for t in texts], tok, batch_size=batch_size, max_length=max_length)


def load_tower(checkpoint, device: str):
    """A text or image BiEncoder from a local save_pretrained directory (config.json with the explicit trunk architecture)."""
    from ..biencoder import BiEncoder, BiEncoderConfig
    from ..nomic_bert import NomicBertConfig
    from ..vit import ViTConfig

    cfg = json.loads((Path(checkpoint) / "config.json").read_text())
    kinds = {"NomicBertConfig": NomicBertConfig, "ViTConfig": ViTConfig}
    if cfg.get("trunk_type") not in kinds:
        raise SystemExit(f"error: {checkpoint}: trunk_type {cfg.get('trunk_type')!r} is not one of {sorted(kinds)}")
    fields = {k: v for k, v in cfg.items() if k in BiEncoderConfig.__dataclass_fields__ and k != "trunk_config"}
    kind = kinds[cfg["trunk_type"]]
    fields["trunk_config"] = kind(**{k: v for k, v in cfg["trunk_config"].items() if k in kind.__dataclass_fields__})
    model = BiEncoder(BiEncoderConfig(**fields), device=device)
    model.load_pretrained(str(checkpoint))
    return model


COARSE = ("exact", "binary")
ADD_ROWS = 1 << 18   # binary: document rows binarised per upload


def add_search_arguments(ap) -> None:
    ap.add_argument("--coarse", choices=COARSE, default="exact",
                    help="exact: bf16 inner-product search of the whole corpus on the device; binary: Hamming search over "
                         "sign codes (1/16 of the memory), then exact re-scoring of k * rescore_factor candidates against "
                         "the memory-mapped document .npy")
    ap.add_argument("--rescore_factor", type=int, default=4,
                    help="binary: candidates re-scored per returned neighbour (k * rescore_factor, at most 4096)")


def search(doc_emb, query_emb, k: int, device: str, exclude=None, below=None, coarse: str = "exact",
           rescore_factor: int = 4):
    """-> (scores, ids) numpy.  coarse="exact": exact inner-product top-k over the bf16 corpus (FlatIPIndex).
    coarse="binary": Hamming top-(k * rescore_factor) over sign codes (BinaryFlatIndex), re-scored exactly against doc_emb,
    which stays on the host (an array or a memmap); equal to "exact" once the candidates cover the corpus."""
    import torch

    from ..search import BinaryFlatIndex, FlatIPIndex, search_binary_rescored

    if coarse not in COARSE:
        raise ValueError(f"coarse must be one of {COARSE}, got {coarse!r}")
    if coarse == "binary":
        n, d = np.shape(doc_emb)
        index = BinaryFlatIndex(d, device=device)
        index.reserve(n)
        for r0 in range(0, n, ADD_ROWS):
            index.add(torch.as_tensor(np.asarray(doc_emb[r0: r0 + ADD_ROWS], dtype=np.float32)))
        return search_binary_rescored(index, doc_emb, np.asarray(query_emb, dtype=np.float32), k, rescore_factor,
                                      exclude=exclude, below=below)
    index = FlatIPIndex(np.shape(doc_emb)[1], device=device)
    index.add(torch.as_tensor(np.asarray(doc_emb, dtype=np.float32)))
    return index.search(np.asarray(query_emb, dtype=np.float32), k, exclude=exclude, below=below)
