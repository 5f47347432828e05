"""YAML -> Config for the contrastive text-text recipes (host-side mirror of sc/config.py:8-241 and sc/read.py:5-11).

Field names and defaults follow the reference's pydantic models for the keys the north-star path reads
(`train_args`, `model_args`, `data_args`); the reference's own YAMLs (e.g. configs/train/contrastive_pretrain.yaml)
load unchanged -- unknown keys such as `use_fp8` are ignored exactly as there.  The two validators that guard this path
are kept: Matryoshka + GradCache is rejected (config.py:70-77) and eval_strategy needs eval_steps (:49-68).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple, Union

import yaml
from pydantic import BaseModel, ConfigDict, model_validator


class TrainArgs(BaseModel):
    model_config = ConfigDict(extra="ignore", validate_assignment=True)
    num_epochs: int = 1
    num_train_steps: Optional[int] = None
    learning_rate: float = 2e-4
    weight_decay: float = 0.01
    eps: Optional[float] = 1e-8
    warmup_steps: Optional[int] = None
    warmup_pct: Optional[float] = None
    cooldown_steps: Optional[int] = None
    checkpoint: Optional[str] = None
    wandb: bool = False
    wandb_project_name: str = ""
    wandb_entity: str = ""
    wandb_run_name: Optional[str] = None
    wandb_group: Optional[str] = None
    log_grads_every: int = 100
    log_lr_every: int = 10
    save_every: Optional[int] = None
    eval_steps: Optional[int] = None
    eval_strategy: Optional[str] = None
    output_dir: Optional[str] = None
    gradient_accumulation_steps: Optional[int] = 1
    schedule_type: str = "cosine"
    max_grad_norm: float = 1.0
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    loss_fn: Optional[str] = "clip"
    grad_cache: Optional[bool] = None
    chunk_size: Optional[int] = None
    clamp_logits: Optional[bool] = True
    logit_max: Optional[float] = 100.0
    matryoshka_dims: Optional[List[int]] = None
    matryoshka_loss_weights: Optional[List[float]] = None
    profile: Optional[bool] = False
    # the reference YAMLs carry this key (contrastive_pretrain.yaml:24) without a TrainArgs field or any code behind it;
    # here it selects the fp8 matrix-core similarity GEMM of the fused InfoNCE (BASELINE configs[4])
    use_fp8: Optional[bool] = False
    # MI355X scheduling of the GradCache step (contrastors_amd.loss.GradCachePolicy; not reference keys).  The environment
    # variables CX_GRADCACHE_CHUNK / CX_GRADCACHE_RESIDENT / CX_EXCHANGE override these when set.
    gradcache_chunk: Union[int, str, None] = "auto"       # auto: chunk_size is a lower bound | exact | n
    gradcache_resident: Union[bool, str, None] = "auto"   # auto: keep pass 1's activations when they fit | true | false
    exchange: Optional[str] = "auto"                       # embedding exchange: auto (validated + timed at start-up) | rccl | oneshot
    exchange_timeout_s: float = 120.0                      # one-shot exchange: how long a GPU polls for a peer's signal before giving up
    overlap_grad_reduce: bool = True                       # per-block gradient all-reduce inside the step's last backward (DDP-style)
    # model_args.gradient_checkpointing is a memory knob sized for 80 GB parts: auto = the top blocks keep their activations
    # as far as the free HBM allows (bit-identical results, less re-forward) | n blocks | 0 = recompute every block
    checkpoint_keep_layers: Union[int, str, None] = "auto"
    # model_type: distill (sc/config.py:46-47, 79-84; sc/trainers/distill.py:341-385)
    distill_loss_fn: str = "mse"
    distill_temperature: float = 1.0

    @model_validator(mode="after")
    def _checks(self):
        from .policy import _parse_chunk, _parse_keep, _parse_resident   # (validate here, not at the first training step)

        _parse_chunk(self.gradcache_chunk, "train_args.gradcache_chunk")
        _parse_resident(self.gradcache_resident, "train_args.gradcache_resident")
        _parse_keep(self.checkpoint_keep_layers, "train_args.checkpoint_keep_layers")
        if self.distill_loss_fn not in ("mse", "kd", "towers", "stella"):   # sc/config.py:79-84
            raise ValueError(f"Loss function {self.distill_loss_fn} not found in loss function registry")
        if self.exchange not in (None, "auto", "rccl", "oneshot"):
            raise ValueError(f"train_args.exchange must be auto, rccl or oneshot, got {self.exchange!r}")
        if self.use_fp8 and self.matryoshka_dims is not None:
            bad = [d for d in self.matryoshka_dims if d not in (256, 512, 768, 1024)]
            if bad:
                raise ValueError(f"use_fp8 covers similarity widths 256 / 512 / 768 / 1024; matryoshka_dims has {bad}")
        if self.eval_strategy is not None and self.eval_strategy not in ("steps", "epochs"):
            raise ValueError(f"Eval strategy {self.eval_strategy} not found in eval strategy registry")
        if self.eval_strategy == "steps" and self.eval_steps is None:
            raise ValueError("Eval steps must be set if eval strategy is set to steps")
        if self.matryoshka_dims is not None and self.grad_cache:
            raise ValueError("Matryoshka dims cannot be set if grad cache is set")
        return self


class DataArgs(BaseModel):
    model_config = ConfigDict(extra="ignore")
    shuffle: bool = False
    workers: int = 0
    batch_size: int = 16384
    seed: int = 42
    input_shards: Optional[str] = None
    download: Optional[bool] = False
    streaming: Optional[bool] = True
    process_one_shard: Optional[bool] = False
    weighted_sampling: Optional[bool] = False
    verbose: Optional[bool] = False
    sample_negatives: Optional[bool] = False
    query_max_length: Optional[int] = None
    document_max_length: Optional[int] = None
    mlm_prob: Optional[float] = None
    # model_type: mlm (sc/config.py MLMDataArgs; sc/trainers/mlm.py:54-99; contrastors_amd/mlm_data.py).  tokenized_dataset is a
    # LOCAL path here (a datasets save_to_disk directory or an (N, S) .npy); mask_on is this path's key: device = cx_mlm_mask
    # draws the masks on the GPU, host = the reference's collator on the loader workers
    tokenized_dataset: Optional[str] = None
    val_pct: Optional[float] = None
    val_mlm_prob: Optional[float] = None
    mask_on: str = "device"
    task_name: Optional[str] = None   # model_type: glue (sc/trainers/glue.py:50): cola, mnli, mrpc, qnli, qqp, rte, sst2, stsb
    # model_type: image_text / locked_text (sc/config.py:123-136 ImageTextDataArgs; contrastors_amd/image_data.py).  All inert
    # unless image_text_shards is set.  Evaluation (contrastors_amd/zeroshot.py): imagenet_val_path (an ImageFolder tree) is
    # evaluated zero-shot when zeroshot_meta_path names the JSON with the class names / prompt templates; retrieval recall@k
    # runs over the local tar shards of retrieval_eval_shards.  eval_flickr alone (the reference's hub download) parses and
    # evaluates nothing: the trainer logs one warning that names retrieval_eval_shards
    image_text_shards: Optional[str] = None
    eval_batch_size: Optional[int] = None
    imagenet_val_path: Optional[str] = None
    eval_flickr: Optional[bool] = False
    zeroshot_meta_path: Optional[str] = None
    retrieval_eval_shards: Optional[str] = None
    train_num_samples: Optional[int] = None
    dataset_resampled: Optional[bool] = False
    # model_type: encoder (this path's key; contrastors_amd/retrieval_eval.py): a LOCAL directory in the BEIR on-disk layout
    # (corpus.jsonl, queries.jsonl, qrels/test.tsv), or one with such a directory per task.  TextTextTrainer logs nDCG@10 per
    # task as beir/<task> every train_args.eval_steps.  Nothing is downloaded; inert when unset
    retrieval_eval_path: Optional[str] = None

    @model_validator(mode="after")
    def _mlm_keys(self):
        if self.mask_on not in ("device", "host"):
            raise ValueError(f"data_args.mask_on must be device or host, got {self.mask_on!r}")
        if self.val_pct is not None and not 0.0 <= self.val_pct < 1.0:
            raise ValueError(f"data_args.val_pct must be in [0, 1), got {self.val_pct}")
        if self.val_mlm_prob is not None and not 0.0 <= self.val_mlm_prob < 1.0:
            raise ValueError(f"data_args.val_mlm_prob must be in [0, 1), got {self.val_mlm_prob}")
        return self


class TransformsConfig(BaseModel):
    """sc/config.py:215-221: the recipe's `transforms:` block (contrastors_amd/image_transform.py serves it)."""
    model_config = ConfigDict(extra="ignore")
    image_size: Union[int, Tuple[int, int]] = 224
    mean: Optional[Union[float, Tuple[float, float, float]]] = (0.48145466, 0.4578275, 0.40821073)
    std: Optional[Union[float, Tuple[float, float, float]]] = (0.26862954, 0.26130258, 0.27577711)
    resize_longest_max: bool = False
    fill_color: int = 0
    aug_cfg: Optional[Dict[str, Any]] = None


class ModelArgs(BaseModel):
    model_config = ConfigDict(extra="ignore", protected_namespaces=())
    model_type: str = "encoder"
    model_name: Optional[str] = "nomic-ai/nomic-bert-2048"
    tokenizer_name: Optional[str] = "bert-base-uncased"
    seq_len: int = 2048
    logit_scale: Optional[float] = 1 / 0.07   # (None, as nomic_embed_vision_v1.5.yaml writes it, is the default: sc/config.py:193-197)
    trainable_logit_scale: bool = False
    pooling: str = "mean"
    nomic_encoder: bool = True
    add_prefix: bool = False
    num_negatives: Optional[int] = 7
    precomputed: Optional[bool] = False  # LiT: the batch carries `text_embs`, the (frozen) text tower is not run
    # architecture overrides of the MLM recipe (sc/config.py:152-170, configs/train/mlm.yaml); None = not given
    rotary_emb_fraction: Optional[float] = None
    rotary_emb_base: Optional[int] = 10_000
    pad_vocab_to_multiple_of: Optional[int] = None
    use_rms_norm: Optional[bool] = None
    activation_function: Optional[str] = "gelu"
    qkv_proj_bias: Optional[bool] = True
    mlp_fc1_bias: Optional[bool] = True
    mlp_fc2_bias: Optional[bool] = True
    attn_pdrop: Optional[float] = 0.0
    pretrained: Optional[bool] = True       # sc/config.py:161 (the reference default)
    checkpoint: Optional[str] = None         # sc/config.py:162: a BiEncoder.save_pretrained directory
    gradient_checkpointing: bool = False
    projection_dim: Optional[int] = None
    freeze: bool = False
    hamming: bool = False
    # sc/config.py:187 -> NomicBertModel.from_pretrained(..., resid_pdrop=) (modeling_biencoder.py:237): residual dropout of a
    # PRETRAINED nomic text trunk (None = the checkpoint's own value); served by the engine's Philox dropout
    resid_pdrop: Optional[float] = None
    ema: bool = False          # sc/config.py:179 + sc/trainers/base.py:387-391: an EMA copy of the weights, updated every step
    ema_decay: float = 0.9999  # (this path's key: the reference leaves the weighting as a TODO)
    # sc/config.py:189-190: what the retrieval evaluation prepends to queries / documents (contrastors_amd/retrieval_eval.py)
    # (a recipe may write null, as distill.yaml does: no prefix)
    query_prefix: Optional[str] = "search_query: "
    document_prefix: Optional[str] = "search_document: "
    patch_dropout: float = 0.0   # sc/config.py:180 -> PatchEmbedding's PatchDropout (image towers; sc/layers/embedding.py:415-418)
    # keys of the reference schema this path does not serve: accepted at their inert defaults, refused otherwise (a recipe
    # that sets them must not train as if it had not)
    num_experts: int = 0
    # model_type: distill (sc/config.py:190-191; sc/trainers/distill.py:116-269).  ffn_div is read by DistillTrainer, which refuses
    # the one branch it cannot serve; the YAML keeps parsing (contrastive_finetune_distill.yaml carries ffn_div: 2)
    distill_init_pretrained: bool = False
    ffn_div: Optional[int] = None

    @model_validator(mode="after")
    def _model_type(self):
        if self.model_type not in ("encoder", "mlm", "glue", "locked_text", "image_text", "mmlm", "distill"):   # sc/config.py:198-203
            raise ValueError(f"Model type {self.model_type} not found in model registry")
        if not self.logit_scale:   # sc/config.py:193-196: `scale or 1 / 0.07`
            self.logit_scale = 1 / 0.07
        if not 0.0 <= self.ema_decay <= 1.0:
            raise ValueError(f"model_args.ema_decay must be in [0, 1], got {self.ema_decay}")
        if not 0.0 <= float(self.patch_dropout or 0.0) < 1.0:
            raise ValueError(f"model_args.patch_dropout must be in [0, 1), got {self.patch_dropout}")
        if self.num_experts and self.num_experts > 0:
            raise ValueError("model_args.num_experts > 0: mixture-of-experts trunks (megablocks) are out of scope")
        if self.resid_pdrop is not None and not (0.0 <= self.resid_pdrop < 1.0):
            raise ValueError(f"model_args.resid_pdrop must be in [0, 1), got {self.resid_pdrop}")
        return self


class Config(BaseModel):
    model_config = ConfigDict(extra="ignore", protected_namespaces=())
    train_args: TrainArgs
    data_args: DataArgs = DataArgs()
    model_args: ModelArgs = ModelArgs()
    # image-text recipes (sc/config.py:238-240): one ModelArgs per tower; `tower_model_args` (three towers) is not built
    text_model_args: Optional[ModelArgs] = None
    vision_model_args: Optional[ModelArgs] = None
    tower_model_args: Optional[ModelArgs] = None
    transforms: Optional[TransformsConfig] = None   # sc/config.py:236 (image-text recipes)
    deepspeed: Optional[bool] = False
    deepspeed_config: Optional[dict] = None


def read_config(path: str) -> Config:
    with open(path) as f:
        return Config(**yaml.safe_load(f))
