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
STORAGE = ("bf16", "int8")
IVF_STORAGE = ("bf16", "int8")
PQ_DSUB = (0, 8, 16, 32, 64)   # --pq_dsub: 0 = off
ADD_ROWS = 1 << 18   # binary / int8 / pq: document rows encoded per upload


def host_documents(args) -> bool:
    """The searches that keep the document rows on the host: the .npy is memory-mapped, not read."""
    return (args.coarse == "binary" or args.storage == "int8" or getattr(args, "ivf_storage", "bf16") == "int8"
            or bool(getattr(args, "pq_dsub", 0)))


def add_search_arguments(ap) -> None:
    ap.add_argument("--coarse", choices=COARSE, default="exact",
                    help="exact: bf16 inner-product search of the whole corpus on the device; binary: Hamming search over "
                         "sign codes (1/16 of the memory), then exact re-scoring of k * rescore_factor candidates against "
                         "the memory-mapped document .npy")
    ap.add_argument("--rescore_factor", type=int, default=4,
                    help="binary / int8 / pq: candidates re-scored per returned neighbour (k * rescore_factor, at most 4096)")
    ap.add_argument("--storage", choices=STORAGE, default="bf16",
                    help="bf16: the corpus on the device as bf16 rows; int8: as int8 codes + one fp32 scale per row (half the "
                         "memory), searched by int8 score, then exact re-scoring of k * rescore_factor candidates against the "
                         "memory-mapped document .npy (with --coarse exact, without --ivf_lists)")
    ap.add_argument("--ivf_lists", type=int, default=0,
                    help="exact: search inside K k-means lists of the corpus instead of all of it (IVFFlatIndex); 0 = off")
    ap.add_argument("--ivf_nprobe", type=int, default=None,
                    help="lists probed per query, at most min(K, 256) (default: min(8, K)); K probes give the exact result")
    ap.add_argument("--ivf_centroids", default=None, help="(K, d) .npy centroid table to use instead of fitting one")
    ap.add_argument("--ivf_sample", type=int, default=None, help="fit the centroids on that many sampled documents")
    ap.add_argument("--ivf_iters", type=int, default=25, help="k-means iterations of the fit")
    ap.add_argument("--ivf_storage", choices=IVF_STORAGE, default="bf16",
                    help="with --ivf_lists K: bf16: the lists hold bf16 rows (IVFFlatIndex); int8: int8 codes + one fp32 scale "
                         "per row (IVFInt8Index, half the memory), searched by int8 score, then exact re-scoring of "
                         "k * rescore_factor candidates against the memory-mapped document .npy")
    ap.add_argument("--pq_dsub", type=int, choices=PQ_DSUB, default=0,
                    help="S > 0: the corpus on the device as product-quantiser codes, one byte per S dimensions "
                         "(PQFlatIndex; S = 8: 1/16 of the bf16 memory), searched by PQ score, then exact re-scoring of "
                         "k * rescore_factor candidates against the memory-mapped document .npy (with --coarse exact and "
                         "--storage bf16, without --ivf_lists); 0 = off")
    ap.add_argument("--pq_sample", type=int, default=None,
                    help="fit the PQ codebooks on that many sampled documents (default min(n, 65536); 256 to 262144)")
    ap.add_argument("--pq_iters", type=int, default=25, help="Lloyd iterations of the PQ codebook fit")
    ap.add_argument("--pq_codebooks", default=None, help="(d / S, 256, S) .npy codebooks to use instead of fitting them")


def check_pq_arguments(ap, args) -> dict:
    """Refuse --pq_* combinations the search cannot serve (ap.error) -> the pq_* keyword arguments of search() (none when off)."""
    if not args.pq_dsub:
        if args.pq_sample is not None or args.pq_codebooks is not None:
            ap.error("--pq_sample and --pq_codebooks need --pq_dsub S")
        return {}
    if args.coarse != "exact":
        ap.error("--pq_dsub goes with --coarse exact only")
    if getattr(args, "storage", "bf16") != "bf16":
        ap.error("--pq_dsub does not go with --storage int8")
    if args.ivf_lists:
        ap.error("--pq_dsub does not go with --ivf_lists")
    if args.pq_iters < 0 or (args.pq_sample is not None and not 256 <= args.pq_sample <= 262144):
        ap.error("--pq_iters must not be negative and --pq_sample must be in [256, 262144]")
    return {"pq_dsub": args.pq_dsub, "pq_sample": args.pq_sample, "pq_iters": args.pq_iters,
            "pq_codebooks": args.pq_codebooks}


def check_search_arguments(ap, args) -> dict:
    """Refuse flag combinations the search cannot serve (ap.error) -> the ivf_* (and, with --pq_dsub, pq_*) keyword arguments
    of search()."""
    pq = check_pq_arguments(ap, args) if hasattr(args, "pq_dsub") else {}
    if getattr(args, "storage", "bf16") == "int8":
        if args.coarse != "exact":
            ap.error("--storage int8 goes with --coarse exact only")
        if args.ivf_lists:
            ap.error("--storage int8 does not go with --ivf_lists")
    if args.ivf_lists < 0:
        ap.error("--ivf_lists must not be negative")
    if args.ivf_lists == 0:
        if args.ivf_nprobe is not None or args.ivf_centroids is not None or args.ivf_sample is not None:
            ap.error("--ivf_nprobe, --ivf_centroids and --ivf_sample need --ivf_lists K")
        if getattr(args, "ivf_storage", "bf16") != "bf16":
            ap.error("--ivf_storage needs --ivf_lists K")
        return pq
    if args.coarse != "exact":
        ap.error("--ivf_lists goes with --coarse exact only")
    nprobe = min(8, args.ivf_lists) if args.ivf_nprobe is None else args.ivf_nprobe
    if not 1 <= nprobe <= min(args.ivf_lists, 256):
        ap.error(f"--ivf_nprobe must be in [1, {min(args.ivf_lists, 256)}]")
    if args.ivf_iters < 1 or (args.ivf_sample is not None and args.ivf_sample < 1):
        ap.error("--ivf_iters and --ivf_sample must be positive")
    ivf = {"ivf_lists": args.ivf_lists, "ivf_nprobe": nprobe, "ivf_centroids": args.ivf_centroids,
           "ivf_sample": args.ivf_sample, "ivf_iters": args.ivf_iters}
    if getattr(args, "ivf_storage", "bf16") != "bf16":
        ivf["ivf_storage"] = args.ivf_storage   # (the default adds no key)
    return ivf


def _fit_sample(doc_emb, sample: Optional[int], seed: int = 0):
    """The rows KMeans.fit(doc_emb, sample=sample) fits on -- its seeded subsample, in ascending row order -- gathered on the
    host, so that a memory-mapped corpus is not uploaded to be sampled."""
    import torch

    n = np.shape(doc_emb)[0]
    if sample is None or int(sample) >= n:
        return doc_emb
    g = torch.Generator().manual_seed(seed)
    return np.asarray(doc_emb[torch.randperm(n, generator=g)[: int(sample)].sort().values.numpy()], dtype=np.float32)


def search(doc_emb, query_emb, k: int, device: str, exclude=None, below=None, coarse: str = "exact",
           rescore_factor: int = 4, ivf_lists: int = 0, ivf_nprobe: Optional[int] = None, ivf_centroids=None,
           ivf_sample: Optional[int] = None, ivf_iters: int = 25, storage: str = "bf16", ivf_storage: str = "bf16",
           pq_dsub: int = 0, pq_sample: Optional[int] = None, pq_iters: int = 25, pq_codebooks=None):
    """-> (scores, ids) numpy.  coarse="exact": exact inner-product top-k over the bf16 corpus (FlatIPIndex).
    coarse="binary": Hamming top-(k * rescore_factor) over sign codes (BinaryFlatIndex), re-scored exactly against doc_emb,
    which stays on the host (an array or a memmap); equal to "exact" once the candidates cover the corpus.
    ivf_lists = K > 0 (with "exact"): the top-k of the ivf_nprobe (default min(8, K)) nearest of K k-means lists
    (IVFFlatIndex; centroids fitted to doc_emb with ivf_iters iterations on ivf_sample rows, or read from the .npy path /
    array ivf_centroids); equal to "exact" when every list is probed.
    storage="int8" (with "exact", without ivf_lists): int8 top-(k * rescore_factor) over per-row quantised codes
    (Int8FlatIndex), re-scored exactly against doc_emb, which stays on the host; equal to "bf16" once the candidates cover the
    corpus.
    ivf_storage="int8" (with ivf_lists): the lists hold int8 codes (IVFInt8Index): doc_emb stays on the host and is added
    ADD_ROWS rows at a time; the centroids are fitted on the ivf_sample rows gathered on the host (without ivf_sample: on all
    of doc_emb, uploaded as bf16 for the fit); the int8 top-(k * rescore_factor) of the probed lists are re-scored exactly
    against doc_emb; equal to "exact" when every list is probed and the candidates cover the corpus.
    pq_dsub = S > 0 (with "exact" and "bf16", without ivf_lists): PQ top-(k * rescore_factor) over one-byte-per-S-dimensions
    codes (PQFlatIndex; codebooks fitted to doc_emb with pq_iters Lloyd steps on pq_sample rows gathered on the host, or read
    from the .npy path / array pq_codebooks), re-scored exactly against doc_emb, which stays on the host; equal to "exact" once
    the candidates cover the corpus."""
    import torch

    from ..search import (BinaryFlatIndex, FlatIPIndex, Int8FlatIndex, IVFFlatIndex, IVFInt8Index, PQFlatIndex,
                          search_binary_rescored, search_int8_rescored, search_ivf_int8_rescored, search_pq_rescored)

    if coarse not in COARSE:
        raise ValueError(f"coarse must be one of {COARSE}, got {coarse!r}")
    if storage not in STORAGE:
        raise ValueError(f"storage must be one of {STORAGE}, got {storage!r}")
    if ivf_storage not in IVF_STORAGE:
        raise ValueError(f"ivf_storage must be one of {IVF_STORAGE}, got {ivf_storage!r}")
    if ivf_storage != "bf16" and not ivf_lists:
        raise ValueError("ivf_storage goes with ivf_lists only")
    if ivf_lists and coarse != "exact":
        raise ValueError("ivf_lists goes with coarse='exact' only")
    if storage == "int8" and (coarse != "exact" or ivf_lists):
        raise ValueError("storage='int8' goes with coarse='exact' and without ivf_lists only")
    if pq_dsub not in PQ_DSUB:
        raise ValueError(f"pq_dsub must be one of {PQ_DSUB}, got {pq_dsub!r}")
    if pq_dsub and (coarse != "exact" or storage != "bf16" or ivf_lists):
        raise ValueError("pq_dsub goes with coarse='exact', storage='bf16' and without ivf_lists only")
    if pq_dsub:
        n, d = np.shape(doc_emb)
        index = PQFlatIndex(d, int(pq_dsub), device=device)
        if pq_codebooks is not None:
            table = np.load(pq_codebooks) if isinstance(pq_codebooks, (str, Path)) else pq_codebooks
            index.train(codebooks=np.asarray(table, dtype=np.float32))
        else:
            index.train(doc_emb, max_iter=pq_iters, sample=pq_sample)
        index.reserve(n)
        for r0 in range(0, n, ADD_ROWS):
            index.add(np.asarray(doc_emb[r0: r0 + ADD_ROWS], dtype=np.float32))
        return search_pq_rescored(index, doc_emb, np.asarray(query_emb, dtype=np.float32), k, rescore_factor,
                                  exclude=exclude, below=below)
    if storage == "int8":
        n, d = np.shape(doc_emb)
        index = Int8FlatIndex(d, device=device)
        index.reserve(n)
        for r0 in range(0, n, ADD_ROWS):
            index.add(np.asarray(doc_emb[r0: r0 + ADD_ROWS], dtype=np.float32))
        return search_int8_rescored(index, doc_emb, np.asarray(query_emb, dtype=np.float32), k, rescore_factor,
                                    exclude=exclude, below=below)
    if coarse == "binary":
        n, d = np.shape(doc_emb)
        index = BinaryFlatIndex(d, device=device)
        index.reserve(n)
        for r0 in range(0, n, ADD_ROWS):
            index.add(torch.as_tensor(np.asarray(doc_emb[r0: r0 + ADD_ROWS], dtype=np.float32)))
        return search_binary_rescored(index, doc_emb, np.asarray(query_emb, dtype=np.float32), k, rescore_factor,
                                      exclude=exclude, below=below)
    if ivf_lists and ivf_storage == "int8":
        n, d = np.shape(doc_emb)
        index = IVFInt8Index(d, int(ivf_lists), device=device)
        if ivf_centroids is not None:
            table = np.load(ivf_centroids) if isinstance(ivf_centroids, (str, Path)) else ivf_centroids
            index.train(centroids=np.asarray(table, dtype=np.float32))
        else:
            index.train(_fit_sample(doc_emb, ivf_sample, index.seed), max_iter=ivf_iters)
        for r0 in range(0, n, ADD_ROWS):
            index.add(np.asarray(doc_emb[r0: r0 + ADD_ROWS], dtype=np.float32))
        nprobe = min(8, int(ivf_lists)) if ivf_nprobe is None else int(ivf_nprobe)
        return search_ivf_int8_rescored(index, doc_emb, np.asarray(query_emb, dtype=np.float32), k, nprobe, rescore_factor,
                                        exclude=exclude, below=below)
    if ivf_lists:
        docs = torch.as_tensor(np.asarray(doc_emb, dtype=np.float32))
        index = IVFFlatIndex(np.shape(doc_emb)[1], int(ivf_lists), device=device)
        if ivf_centroids is not None:
            table = np.load(ivf_centroids) if isinstance(ivf_centroids, (str, Path)) else ivf_centroids
            index.train(centroids=np.asarray(table, dtype=np.float32))
        else:
            index.train(docs, max_iter=ivf_iters, sample=ivf_sample)
        index.add(docs)
        nprobe = min(8, int(ivf_lists)) if ivf_nprobe is None else int(ivf_nprobe)
        return index.search(np.asarray(query_emb, dtype=np.float32), k, nprobe, exclude=exclude, below=below)
    index = FlatIPIndex(np.shape(doc_emb)[1], device=device)
    index.add(torch.as_tensor(np.asarray(doc_emb, dtype=np.float32)))
    return index.search(np.asarray(query_emb, dtype=np.float32), k, exclude=exclude, below=below)
