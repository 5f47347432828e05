"""Zero-shot accuracy and retrieval recall@k of an image-text model (contrastors_amd.zeroshot), outside training.

The numbers of the trainer's eval_loop (sc/trainers/image_text.py:198-254) for a recipe: `top1_acc` / `top5_acc` over
data_args.imagenet_val_path (an ImageFolder tree) with the class names and prompt templates of data_args.zeroshot_meta_path,
and `flickr/*_recall@k` over data_args.retrieval_eval_shards (local tar shards of image + captions).  The three paths can be
given here instead of in the recipe.  The towers come from --checkpoint (a directory with text/ and vision/ as the trainer's
save_state writes them) or, without it, from the recipe's own model names.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

from ._common import load_tower


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m contrastors_amd.tools.zeroshot_eval", description=__doc__.split("\n\n")[0],
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, help="the training recipe (YAML)")
    ap.add_argument("--checkpoint", help="directory holding text/ and vision/ (save_pretrained layout)")
    ap.add_argument("--imagenet_val_path")
    ap.add_argument("--zeroshot_meta_path")
    ap.add_argument("--retrieval_eval_shards")
    ap.add_argument("--tokenizer", help="local tokenizer directory (default: text_model_args.tokenizer_name)")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if not Path(args.config).is_file():
        ap.error(f"--config {args.config} does not exist")
    if args.checkpoint and not all((Path(args.checkpoint) / t / "config.json").is_file() for t in ("text", "vision")):
        ap.error(f"--checkpoint {args.checkpoint} does not hold text/config.json and vision/config.json")
    from ..config import read_config

    config = read_config(args.config)
    if config.text_model_args is None or config.vision_model_args is None:
        ap.error("the recipe has no text_model_args / vision_model_args: not an image-text recipe")
    for key in ("imagenet_val_path", "zeroshot_meta_path", "retrieval_eval_shards"):
        if getattr(args, key):
            setattr(config.data_args, key, getattr(args, key))
    da = config.data_args
    if bool(da.imagenet_val_path) != bool(da.zeroshot_meta_path) and not da.retrieval_eval_shards:
        ap.error("zero-shot evaluation needs both imagenet_val_path and zeroshot_meta_path")
    if not (da.imagenet_val_path and da.zeroshot_meta_path) and not da.retrieval_eval_shards:
        ap.error("nothing to evaluate: give imagenet_val_path + zeroshot_meta_path and / or retrieval_eval_shards")

    import torch
    from transformers import AutoTokenizer

    from ..image_transform import GpuImageTransform
    from ..zeroshot import eval_data_from_config, evaluate_from_config

    if args.checkpoint:
        from types import SimpleNamespace

        from ..biencoder import DualEncoder, LogitScale

        va = config.vision_model_args
        scale = LogitScale(SimpleNamespace(logit_scale=va.logit_scale, trainable_logit_scale=va.trainable_logit_scale))
        text, vision = (load_tower(Path(args.checkpoint) / t, args.device) for t in ("text", "vision"))
        model = DualEncoder(text, vision, scale.to(args.device))
    else:
        from ..trainers import ImageTextTrainer

        model = ImageTextTrainer(config, torch.bfloat16, device=args.device).model["model"]
    tok = AutoTokenizer.from_pretrained(args.tokenizer or config.text_model_args.tokenizer_name, local_files_only=True)
    transform = GpuImageTransform.from_config(config.transforms, is_train=False, out_dtype=torch.bfloat16, device=args.device)
    metrics = evaluate_from_config(model, config, eval_data_from_config(config), tok, transform)
    print(json.dumps(metrics))
    return 0


if __name__ == "__main__":
    sys.exit(main())
