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
    """Every record gets `metadata`; shard-00000.jsonl.gz, ... of `shard_size` records each (the reference's writer)."""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    paths = []
    for start in range(0, len(records), shard_size):
        p = out / f"shard-{start // shard_size:05d}.jsonl.gz"
        with gzip.open(p, "wt") as f:
            for rec in records[start: start + shard_size]:
                rec["metadata"] = metadata
                f.write(json.dumps(rec) + "\n")
        paths.append(p)
    return paths


def load_npy(path, n: int, what: str) -> np.ndarray:
    x = np.load(path)
    if x.ndim != 2 or x.shape[0] != n:
        raise SystemExit(f"error: {what} embeddings {path} have shape {x.shape}, expected ({n}, d)")
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


def search(doc_emb, query_emb, k: int, device: str, exclude=None, below=None):
    """-> (scores, ids) numpy: exact inner-product top-k over the bf16 corpus (FlatIPIndex)."""
    import torch

    from ..search import FlatIPIndex

    index = FlatIPIndex(np.shape(doc_emb)[1], device=device)
    index.add(torch.as_tensor(np.asarray(doc_emb, dtype=np.float32)))
    return index.search(np.asarray(query_emb, dtype=np.float32), k, exclude=exclude, below=below)
