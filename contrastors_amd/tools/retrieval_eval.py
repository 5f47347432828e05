"""Retrieval metrics of a text bi-encoder over local BEIR-layout evaluation sets (contrastors_amd.retrieval_eval), outside training.

nDCG / MAP / recall / precision / MRR / hit rate at every cut-off of --ks, per task and averaged over tasks, for the towers of
--checkpoint (a BiEncoder save_pretrained directory, or a trainer's save_state directory holding model/) or, without it, the
recipe's own model.  --data is one task directory (corpus.jsonl, queries.jsonl, qrels/<split>.tsv) or a directory with one
such directory per task; nothing is downloaded.  Queries and documents get model_args.query_prefix / document_prefix and are
cut at model_args.seq_len, as in the trainer's eval_loop.  Prints one JSON line: {"tasks": {name: {metric@k: ...}}, "mean":
{metric@k: ...}, "beir": {the trainer's beir/<task> keys}}.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

from ._common import load_tower


def _int_list(what: str):
    def parse(text: str):
        try:
            vals = [int(t) for t in text.split(",") if t.strip()]
        except ValueError:
            raise argparse.ArgumentTypeError(f"{what}: expected comma-separated integers, got {text!r}") from None
        if not vals or any(v < 1 for v in vals):
            raise argparse.ArgumentTypeError(f"{what}: expected positive integers, got {text!r}")
        return vals
    return parse


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m contrastors_amd.tools.retrieval_eval", description=__doc__.split("\n\n")[0],
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, help="the training recipe (YAML)")
    ap.add_argument("--checkpoint", help="a BiEncoder save_pretrained directory, or a save_state directory holding model/")
    ap.add_argument("--data", help="a BEIR-layout task directory or a directory of them (default: data_args.retrieval_eval_path)")
    ap.add_argument("--tasks", help="comma-separated task directory names (default: all)")
    ap.add_argument("--ks", type=_int_list("--ks"), default=[1, 3, 5, 10, 100], help="cut-offs, at most 8 (default 1,3,5,10,100)")
    ap.add_argument("--dims", type=_int_list("--dims"), help="Matryoshka widths evaluated besides the full one, e.g. 768,512,256")
    ap.add_argument("--split", default="test")
    ap.add_argument("--tokenizer", help="local tokenizer directory (default: model_args.tokenizer_name)")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--out", help="also write the JSON to this file")
    ap.add_argument("--per_query", action="store_true", help="add the per-query metric arrays and query ids to every task")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not Path(args.config).is_file():
        ap.error(f"--config {args.config} does not exist")
    if len(args.ks) > 8:
        ap.error(f"--ks holds {len(args.ks)} cut-offs; at most 8")
    ckpt = None
    if args.checkpoint:
        ckpt = Path(args.checkpoint)
        if (ckpt / "model" / "config.json").is_file():
            ckpt = ckpt / "model"
        if not (ckpt / "config.json").is_file():
            ap.error(f"--checkpoint {args.checkpoint} holds neither config.json nor model/config.json")
    from ..config import read_config

    config = read_config(args.config)
    if config.model_args.model_type not in ("encoder", "distill"):
        ap.error(f"model_type {config.model_args.model_type!r}: not a text-text recipe")
    data = args.data or config.data_args.retrieval_eval_path
    if not data:
        ap.error("nothing to evaluate: give --data or set data_args.retrieval_eval_path")
    from ..retrieval_eval import beir_log_metrics, evaluate_task, find_tasks, load_beir_task

    try:
        task_dirs = find_tasks(data, [t for t in args.tasks.split(",") if t.strip()] if args.tasks else None)
    except FileNotFoundError as e:
        ap.error(str(e))

    import torch
    from transformers import AutoTokenizer

    if ckpt is not None:
        model = load_tower(ckpt, args.device)
    else:
        from ..trainers import TextTextTrainer

        model = TextTextTrainer(config, torch.bfloat16, device=args.device).model["model"]
    tok = AutoTokenizer.from_pretrained(args.tokenizer or config.model_args.tokenizer_name, local_files_only=True)
    ma = config.model_args
    tasks = {}
    for p in task_dirs:
        r = evaluate_task(model, tok, load_beir_task(p, args.split), ks=args.ks, query_prefix=ma.query_prefix or "",
                          document_prefix=ma.document_prefix or "", max_length=ma.seq_len, batch_size=args.batch_size, dims=args.dims,
                          per_query=args.per_query)
        if args.per_query:
            r["per_query"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r["per_query"].items()}
        tasks[p.name] = r
    keys = [k for k in next(iter(tasks.values())) if "@" in k]
    result = {"tasks": tasks, "mean": {k: sum(t[k] for t in tasks.values()) / len(tasks) for k in keys}}
    if "ndcg@10" in keys:
        result["beir"] = beir_log_metrics(tasks)
    line = json.dumps(result)
    if args.out:
        Path(args.out).write_text(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
