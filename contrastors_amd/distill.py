"""DistillTrainer: a student text encoder trained against a frozen teacher (host-side mirror of sc/trainers/distill.py).

The teacher is a BiEncoder built and loaded as TextTextTrainer builds one; its forward is the engine's no-grad forward.  The
student is a BiEncoder of the same width with cls pooling and dropout 0; its step is the ordinary direct step.  The loss forms
are contrastors_amd.loss.distill_loss (`mse`, `kd`, `towers`); the `kd` term is the fused similarity-KL kernel.

What raises instead of training as something else: `distill_loss_fn: stella` (at the first loss), `ffn_div` without a
`checkpoint` (a student narrower than the teacher: the engine's LayerNorm widths are 256 / 512 / 768 / 1024), and
`grad_cache: true` (the reference's distillation step has no GradCache form).
"""
from __future__ import annotations

import dataclasses
import json
import os
import re
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from .biencoder import BiEncoder, BiEncoderConfig, LogitScale
from .config import Config
from .distributed import check_exchange
from .loss import distill_loss
from .nomic_bert import NomicBertConfig
from .trainers import TextTextTrainer, _load_initial_weights, encode_pair


def uniform_element_selection(wt: torch.Tensor, s_shape) -> torch.Tensor:
    """Weight selection (Xu et al., "Initializing Models with Larger Ones"): the student tensor takes evenly spaced elements of
    the teacher's along every axis -- a stride of teacher // student where that divides, round(linspace(0, teacher - 1, student))
    otherwise.  The identity at equal shapes."""
    s_shape = tuple(int(n) for n in s_shape)
    if wt.dim() != len(s_shape):
        raise ValueError(f"teacher tensor has {wt.dim()} axes, the student's has {len(s_shape)}")
    out = wt
    for axis, (nt, ns) in enumerate(zip(wt.shape, s_shape)):
        if ns > nt:
            raise ValueError(f"axis {axis}: the student ({ns}) is larger than the teacher ({nt})")
        if nt == ns:
            continue
        if nt % ns == 0:
            idx = torch.arange(ns) * (nt // ns)
        else:
            idx = torch.round(torch.linspace(0, nt - 1, ns)).long()
        out = torch.index_select(out, axis, idx.to(out.device))
    return out.clone()


def distill_layer_map(student_layers: int, teacher_layers: int, from_checkpoint: bool) -> Dict[int, int]:
    """student block -> the teacher block it is initialised from.  With a `checkpoint` (sc/trainers/distill.py:133-149) the
    student has half the teacher's depth and block i takes block 2i.  Without one (:210-211, `distill_init_pretrained`) the
    student keeps the teacher's depth and block i takes block i // 2 -- the reference's literal indexing: every teacher block of
    the lower half is used twice, the upper half not at all."""
    want = teacher_layers // 2 if from_checkpoint else teacher_layers
    if student_layers != want:
        raise ValueError(f"a student of {student_layers} blocks against a teacher of {teacher_layers}: this branch builds {want}")
    return {i: (2 * i if from_checkpoint else i // 2) for i in range(student_layers)}


_LAYER_KEY = re.compile(r"encoder\.layers\.(\d+)\.")


def _teacher_key(key: str, layer_map: Dict[int, int]) -> str:
    m = _LAYER_KEY.search(key)
    if m is None:
        return key
    return key[: m.start(1)] + str(layer_map[int(m.group(1))]) + key[m.end(1):]


@torch.no_grad()
def init_student_from_teacher(student: BiEncoder, teacher: BiEncoder, layer_map: Dict[int, int], embeddings: bool):
    """Copy the mapped blocks (and, with `embeddings`, the embedding tables and their LayerNorm) of the teacher's trunk into the
    student's, every tensor through uniform_element_selection."""
    src = teacher.trunk.reference_state_dict()
    sd = {}
    for key, cur in student.trunk.reference_state_dict().items():
        is_layer = _LAYER_KEY.search(key) is not None
        if is_layer or embeddings:
            sd[key] = uniform_element_selection(src[_teacher_key(key, layer_map)], cur.shape)
        else:
            sd[key] = cur.clone()
    student.trunk.load_reference_state_dict(sd)


def _checkpoint_trunk_config(path: str):
    """The architecture a BiEncoder.save_pretrained directory was written with (config.json: trunk_config), or None."""
    cfg_path = os.path.join(path, "config.json")
    if not os.path.exists(cfg_path):
        return None
    with open(cfg_path) as f:
        cfg = json.load(f)
    if cfg.get("trunk_type", "NomicBertConfig") != "NomicBertConfig" or "trunk_config" not in cfg:
        return None
    fields = NomicBertConfig.__dataclass_fields__
    return NomicBertConfig(**{k: v for k, v in cfg["trunk_config"].items() if k in fields})


class DistillTrainer(TextTextTrainer):
    def __init__(self, config: Config, dtype=torch.bfloat16, device=None, trunk_config: Optional[NomicBertConfig] = None,
                 total_steps: Optional[int] = None):
        ma, ta = config.model_args, config.train_args
        if ta.grad_cache:
            raise NotImplementedError("model_type 'distill' with grad_cache: true -- the reference's distillation step has no "
                                      "GradCache form (sc/trainers/distill.py:309-429)")
        if ma.ffn_div is not None and not ma.checkpoint:
            raise NotImplementedError(f"model_args.ffn_div = {ma.ffn_div} without a checkpoint asks for a student narrower than the "
                                      "teacher; the engine's widths are 256 / 512 / 768 / 1024 (768 / 2 is none of them)")
        self.loss_fn = ta.distill_loss_fn
        super().__init__(config, dtype=dtype, device=device, trunk_config=trunk_config, total_steps=total_steps)

    # sc/trainers/distill.py:116-269
    def get_model(self, config: Config, trunk_config=None) -> Dict[str, torch.nn.Module]:
        ma, ta = config.model_args, config.train_args
        from_checkpoint = bool(ma.checkpoint)
        teacher_cfg = trunk_config
        if teacher_cfg is None and from_checkpoint:
            teacher_cfg = _checkpoint_trunk_config(ma.checkpoint)
        explicit = trunk_config is not None
        tc = BiEncoderConfig(model_name=ma.model_name or "", pooling=ma.pooling, logit_scale=ma.logit_scale,
                             projection_dim=ma.projection_dim, freeze=True, hamming=ma.hamming,
                             nomic_encoder=ma.nomic_encoder, seq_len=ma.seq_len, trunk_config=teacher_cfg)
        teacher = BiEncoder(tc, device=self.device)
        _load_initial_weights(teacher, ma, explicit_arch=explicit)
        teacher.broadcast_parameters(0)
        teacher.eval()
        for p in teacher.parameters():
            p.requires_grad = False
        arch = teacher.trunk.config
        if not isinstance(arch, NomicBertConfig):
            raise NotImplementedError("distillation serves text trunks")
        depth = arch.n_layer // 2 if from_checkpoint else arch.n_layer
        if depth < 1:
            raise ValueError(f"a teacher of {arch.n_layer} blocks has no half-depth student")
        student_cfg = dataclasses.replace(arch, n_layer=depth, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
        # `towers` with a checkpoint and ffn_div: the reference trains a Linear(width, teacher width) on the student output before
        # normalisation (:157-158, 333-335) -- the student BiEncoder's own projection head
        project = from_checkpoint and ma.ffn_div is not None and ta.distill_loss_fn == "towers"
        out_width = int(ma.projection_dim) if ma.projection_dim else arch.n_embd
        sc = BiEncoderConfig(model_name=ma.model_name or "", pooling="cls", logit_scale=ma.logit_scale,
                             projection_dim=out_width if project else None, hamming=False,
                             gradient_checkpointing=ma.gradient_checkpointing, nomic_encoder=ma.nomic_encoder,
                             seq_len=ma.seq_len, trunk_config=student_cfg)
        student = BiEncoder(sc, device=self.device).train()
        student.overlap_reduce = bool(ta.overlap_grad_reduce)
        if from_checkpoint:
            init_student_from_teacher(student, teacher, distill_layer_map(depth, arch.n_layer, True), embeddings=True)
        elif ma.distill_init_pretrained:
            init_student_from_teacher(student, teacher, distill_layer_map(depth, arch.n_layer, False), embeddings=False)
        student.broadcast_parameters(0)
        # (no loss form of this trainer reads it; the inherited optimizer / checkpoint code expects the entry)
        scale = LogitScale(SimpleNamespace(logit_scale=ma.logit_scale, trainable_logit_scale=False))
        return {"model": student, "teacher": teacher, "logit_scale": scale.to(self.device)}

    @staticmethod
    def _encode(model, q, d):
        pair = encode_pair(model, q, d, True)
        if pair is None:
            pair = model(**q, normalize=True)["embedding"], model(**d, normalize=True)["embedding"]
        return pair[0].float(), pair[1].float()   # (a projection head answers in bf16; the loss kernels read fp32)

    # sc/trainers/distill.py:309-429
    def forward_step(self, batch) -> Dict[str, torch.Tensor]:
        student, teacher = self.model["model"], self.model["teacher"]
        q, d = self._inputs(batch, "query"), self._inputs(batch, "document")
        with torch.no_grad():
            tq, td = self._encode(teacher, q, d)
        # all four come out L2-normalised (normalize=True: fused into the pooling kernel, or after the projection head)
        sq, sd = self._encode(student, q, d)
        return distill_loss(self.loss_fn, sq, sd, tq, td, self.config.train_args.distill_temperature)

    def backward(self, loss):
        if isinstance(loss, dict):
            loss = loss["loss"]
        self.model["model"].arm_overlapped_reduce(when_last_outstanding=True)
        loss.backward()
        self.model["model"].sync_gradients()

    def training_step(self, batch) -> torch.Tensor:
        out = self._micro_step(batch)
        self.step += 1
        if self.world > 1:
            check_exchange(sync=True)
        if self.tracker is not None:   # sc/trainers/distill.py:460-462: every entry of the dictionary
            self.log({k: v.detach().cpu().item() for k, v in out.items()}, step=self.step - 1)
        return out["loss"].detach()
