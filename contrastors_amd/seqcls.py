"""Sequence classification on the native trunk: host-side mirror of `NomicBertForSequenceClassification` / `NomicBertPooler`
(sc/models/encoder/modeling_nomic_bert.py:398-414, 672-757), the model the GLUE trainer fine-tunes (sc/trainers/glue.py).

One typed encoder call (`cx_encoder_forward_typed`, pooling "cls", not normalised) yields the first token's hidden state
of every sequence; the whole head -- pooler dense + tanh, dropout, Linear(d, num_labels), cross-entropy or MSE -- is
`cx_seqcls_head_fwd` / `cx_seqcls_head_bwd` (csrc/seqcls.hip): two launches each way instead of a dozen torch ops on 16-32
rows.  State-dict keys are the reference's (`bert.*` with `bert.pooler.dense.*`, `classifier.*`).
"""
from __future__ import annotations

import dataclasses
import json
import os
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import _C
from .nomic_bert import NomicBertConfig, NomicBertEngine, VarlenBatch

PROBLEM_TYPES = ("regression", "single_label_classification", "multi_label_classification")
IGNORE_INDEX = -100   # torch.nn.CrossEntropyLoss's default, which the reference uses (:743)
_POOLER_W, _POOLER_B = "bert.pooler.dense.weight", "bert.pooler.dense.bias"
_CLS_W, _CLS_B = "classifier.weight", "classifier.bias"


def infer_problem_type(num_labels: int, labels: torch.Tensor) -> str:
    """sc/models/encoder/modeling_nomic_bert.py:728-734."""
    if num_labels == 1:
        return "regression"
    if num_labels > 1 and labels.dtype in (torch.long, torch.int):
        return "single_label_classification"
    return "multi_label_classification"


class NomicBertForSequenceClassification(torch.nn.Module):
    def __init__(self, config: NomicBertConfig, num_labels: int, problem_type: Optional[str] = None,
                 classifier_dropout: Optional[float] = None, device="cuda", seed: Optional[int] = None):
        super().__init__()
        if problem_type is not None and problem_type not in PROBLEM_TYPES:
            raise ValueError(f"problem_type {problem_type!r} is not one of {PROBLEM_TYPES}")
        if problem_type == "multi_label_classification":
            raise NotImplementedError("multi_label_classification (BCE-with-logits): no GLUE task uses it")
        if not 1 <= int(num_labels) <= 8:
            raise NotImplementedError(f"num_labels = {num_labels}: the fused head serves 1 to 8 outputs")
        self.config = config
        self.num_labels = int(num_labels)
        self.problem_type = problem_type
        # :685 `getattr(config, "classifier_dropout", config.embd_pdrop)`
        self.classifier_dropout = float(config.embd_pdrop if classifier_dropout is None else classifier_dropout)
        if not 0.0 <= self.classifier_dropout < 1.0:
            raise ValueError("classifier_dropout must be in [0, 1)")
        self.bert = NomicBertEngine(config, device=device, pooling="cls", normalize=False, seed=seed)
        self.lib = self.bert.lib
        d, C, dev = config.n_embd, self.num_labels, self.bert.device_
        # head parameters live in two flat fp32 buffers like the trunk's (decay: the matrices; no decay: the biases,
        # sc/optimizer.py:16-25), the gradients in one: one memset clears them, two AdamW launches step them
        self._n_w, self._n_b = d * d + C * d, d + _round4(C)
        self._head_param = torch.zeros(self._n_w + self._n_b, dtype=torch.float32, device=dev)
        self._head_grad = torch.zeros_like(self._head_param)
        self._head_scratch = torch.zeros_like(self._head_param)   # where a backward writes while gradients accumulate
        self.head_decay = torch.nn.Parameter(self._head_param[: self._n_w])
        self.head_nodecay = torch.nn.Parameter(self._head_param[self._n_w:])
        self.head_decay.grad = self._head_grad[: self._n_w]
        self.head_nodecay.grad = self._head_grad[self._n_w:]
        self._grads_clean = True
        self.reset_head(seed)

    # ---- head parameters ------------------------------------------------------------------------------------------------
    def _views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        d, C = self.config.n_embd, self.num_labels
        w, b = flat[: self._n_w], flat[self._n_w:]
        return {_POOLER_W: w[: d * d].view(d, d), _CLS_W: w[d * d:].view(C, d), _POOLER_B: b[:d], _CLS_B: b[d: d + C]}

    def head(self) -> Dict[str, torch.Tensor]:
        return self._views(self._head_param)

    def head_grads(self) -> Dict[str, torch.Tensor]:
        return self._views(self._head_grad)

    @torch.no_grad()
    def reset_head(self, seed: Optional[int] = None):
        """The reference's `_init_weights` (:284-292) for the two Linear layers: weights N(0, initializer_range), biases 0."""
        gen = torch.Generator(device="cpu").manual_seed(2 if seed is None else seed + 2)
        h = self.head()
        for k in (_POOLER_W, _CLS_W):
            h[k].copy_(torch.empty(h[k].shape).normal_(0.0, self.config.initializer_range, generator=gen))
        h[_POOLER_B].zero_()
        h[_CLS_B].zero_()

    def param_groups(self, weight_decay: float):
        """sc/optimizer.py:16-25: matrices decay, biases / LayerNorm do not."""
        return [{"params": [self.bert.flat_decay, self.head_decay], "weight_decay": weight_decay},
                {"params": [self.bert.flat_nodecay, self.head_nodecay], "weight_decay": 0.0}]

    def zero_grad(self, set_to_none: bool = False):
        self.bert.zero_grad()
        self._head_grad.zero_()
        self._grads_clean = True

    def sync_gradients(self):
        """DDP's job in the reference (sc/trainers/glue.py:66-71): average every gradient over ranks, once per step."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            W = dist.get_world_size()
            for g in (self.bert.flat_grad, self._head_grad):
                dist.all_reduce(g)
                g.div_(W)

    def gradient_checkpointing_enable(self, enabled: bool = True, keep_layers=None):
        self.bert.gradient_checkpointing_enable(enabled, keep_layers)

    # ---- compute --------------------------------------------------------------------------------------------------------
    def _mode(self, labels: torch.Tensor) -> int:
        if self.problem_type is None:
            self.problem_type = infer_problem_type(self.num_labels, labels)
        if self.problem_type == "multi_label_classification":
            raise NotImplementedError("multi_label_classification (BCE-with-logits): no GLUE task uses it")
        return 1 if self.problem_type == "regression" else 0

    def _labels(self, labels: torch.Tensor, mode: int, B: int):
        """-> (device labels in the kernel's layout, number of rows the mean runs over).  Counted on the host when the labels
        arrive on the host (a dataloader's do): no device round trip."""
        C, dev = self.num_labels, self.bert.device_
        if mode == 1:
            lab = labels.to(dev, torch.float32).reshape(B, C).contiguous()   # (C = 1: the reference squeezes both sides, :739)
            return lab, B
        lab = labels.reshape(B)
        count = int((lab != IGNORE_INDEX).sum())
        if lab.device.type == "cpu" and bool(((lab != IGNORE_INDEX) & ((lab < 0) | (lab >= C))).any()):
            raise ValueError(f"labels must be in [0, {C}) or {IGNORE_INDEX}")
        return lab.to(dev, torch.int64).contiguous(), count

    def _draw_dropout(self):
        """(p, seed, offset) of the head's mask: torch's generator of this device, advanced like a torch dropout op would."""
        p = self.classifier_dropout if self.training else 0.0
        if p <= 0.0:
            return 0.0, 0, 0
        dev = self.bert.device_
        gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
        off = gen.get_offset()
        gen.set_offset(off + 4)
        return p, gen.initial_seed() & (2**64 - 1), off

    def _head_fwd(self, emb: torch.Tensor, lab: Optional[torch.Tensor], mode: int, drop):
        B, d, C = emb.shape[0], self.config.n_embd, self.num_labels
        f32 = dict(dtype=torch.float32, device=emb.device)
        pooled, logits = torch.empty(B, d, **f32), torch.empty(B, C, **f32)
        rows = torch.empty(B, **f32) if lab is not None else None
        h = self.head()
        rc = self.lib.cx_seqcls_head_fwd(emb.data_ptr(), emb.stride(0), h[_POOLER_W].data_ptr(), h[_POOLER_B].data_ptr(),
                                         h[_CLS_W].data_ptr(), h[_CLS_B].data_ptr(), _C.ptr(lab), mode, drop[0], drop[1], drop[2],
                                         pooled.data_ptr(), logits.data_ptr(), _C.ptr(rows), B, d, C, _C.cur_stream())
        _C.check(rc, "cx_seqcls_head_fwd")
        return pooled, logits, rows

    def _head_bwd(self, emb, pooled, logits, lab, mode: int, coef: float, drop) -> torch.Tensor:
        """Head gradients into the flat gradient buffer (written in place while it is clean, added otherwise); -> dX."""
        B, d, C = emb.shape[0], self.config.n_embd, self.num_labels
        ws = torch.empty(self.lib.cx_seqcls_ws_floats(B, d, C), dtype=torch.float32, device=emb.device)
        dx = torch.empty(B, d, dtype=torch.float32, device=emb.device)
        h, g = self.head(), self._views(self._head_grad if self._grads_clean else self._head_scratch)
        rc = self.lib.cx_seqcls_head_bwd(emb.data_ptr(), emb.stride(0), h[_POOLER_W].data_ptr(), h[_CLS_W].data_ptr(),
                                         pooled.data_ptr(), logits.data_ptr(), lab.data_ptr(), mode, coef, drop[0], drop[1],
                                         drop[2], ws.data_ptr(), ws.numel(), g[_POOLER_W].data_ptr(), g[_POOLER_B].data_ptr(),
                                         g[_CLS_W].data_ptr(), g[_CLS_B].data_ptr(), dx.data_ptr(), B, d, C, _C.cur_stream())
        _C.check(rc, "cx_seqcls_head_bwd")
        if not self._grads_clean:
            self._head_grad.add_(self._head_scratch)
        self._grads_clean = False
        return dx

    def _batch(self, input_ids, attention_mask, token_type_ids) -> VarlenBatch:
        dev = self.bert.device_
        vb = VarlenBatch.from_mask(input_ids.to(dev), None if attention_mask is None else attention_mask.to(dev))
        return vb.with_token_types(None if token_type_ids is None else token_type_ids.to(dev, torch.int64))

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None):
        """-> SimpleNamespace(loss, logits).  In training mode with gradients enabled the loss carries the backward of the
        whole model (its incoming gradient is read on the host: one synchronisation; `forward_backward` has none)."""
        vb = self._batch(input_ids, attention_mask, token_type_ids)
        if labels is None:
            emb, _ = self.bert.forward_chunk(vb, False, normalize=False)
            _, logits, _ = self._head_fwd(emb, None, 0, self._draw_dropout())
            return SimpleNamespace(loss=None, logits=logits)
        mode = self._mode(labels)
        lab, count = self._labels(labels, mode, vb.B)
        if torch.is_grad_enabled() and self.training:
            loss, logits = _SeqClsFn.apply(self.bert.flat_decay, self, vb, lab, mode, count)
            return SimpleNamespace(loss=loss, logits=logits)
        emb, _ = self.bert.forward_chunk(vb, False, normalize=False)
        _, logits, rows = self._head_fwd(emb, lab, mode, self._draw_dropout())
        return SimpleNamespace(loss=rows.sum() / max(count, 1), logits=logits)

    def forward_backward(self, input_ids, attention_mask=None, token_type_ids=None, labels=None, loss_scale: float = 1.0):
        """One training micro-step without autograd and without a host synchronisation: forward, then the backward of
        `loss_scale * loss` accumulated into every gradient buffer.  -> SimpleNamespace(loss, logits), both detached."""
        vb = self._batch(input_ids, attention_mask, token_type_ids)
        mode = self._mode(labels)
        lab, count = self._labels(labels, mode, vb.B)
        emb, arena = self.bert.forward_chunk(vb, True, normalize=False)
        drop = self._draw_dropout()
        pooled, logits, rows = self._head_fwd(emb, lab, mode, drop)
        dx = self._head_bwd(emb, pooled, logits, lab, mode, float(loss_scale) / max(count, 1), drop)
        self.bert.backward_chunk(vb, arena, dx)
        return SimpleNamespace(loss=rows.sum() / max(count, 1), logits=logits)

    # ---- weights on disk ------------------------------------------------------------------------------------------------
    def reference_state_dict(self) -> Dict[str, torch.Tensor]:
        sd = {f"bert.{k}": v for k, v in self.bert.reference_state_dict().items()}
        sd.update({k: v.detach() for k, v in self.head().items()})
        return sd

    def reference_grad_dict(self) -> Dict[str, torch.Tensor]:
        sd = {f"bert.{k}": v for k, v in self.bert.reference_grad_dict().items()}
        sd.update(self.head_grads())
        return sd

    @torch.no_grad()
    def load_reference_state_dict(self, sd: Dict[str, torch.Tensor]) -> Dict[str, List[str]]:
        """`from_pretrained(..., strict=False, ignore_mismatched_sizes=True)` (sc/trainers/glue.py:59-61), see split_checkpoint.
        The trunk must be complete.  -> what happened to every key that was not simply loaded."""
        head = self.head()
        trunk, taken, report = split_checkpoint(sd, {k: tuple(v.shape) for k, v in head.items()})
        self.bert.load_reference_state_dict(trunk, strict=True)
        for k, v in taken.items():
            head[k].copy_(v.to(head[k].device, torch.float32))
        return report

    def save_pretrained(self, output_dir: str):
        """model.safetensors with the reference's keys + config.json (the trunk architecture, which no hub can be asked for
        here, and the head's three settings)."""
        from safetensors.torch import save_file

        os.makedirs(output_dir, exist_ok=True)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.reference_state_dict().items()},
                  os.path.join(output_dir, "model.safetensors"))
        with open(os.path.join(output_dir, "config.json"), "w") as f:
            json.dump({"architectures": ["NomicBertForSequenceClassification"], "trunk_config": dataclasses.asdict(self.config),
                       "trunk_type": "NomicBertConfig", "num_labels": self.num_labels, "problem_type": self.problem_type,
                       "classifier_dropout": self.classifier_dropout}, f, indent=1)

    def load_pretrained(self, model_path: str) -> Dict[str, List[str]]:
        from safetensors.torch import load_file

        report = self.load_reference_state_dict(load_file(os.path.join(model_path, "model.safetensors")))
        self.bert.sync_shadows()
        return report


def _round4(n: int) -> int:
    return (n + 3) // 4 * 4


def split_checkpoint(sd: Dict[str, torch.Tensor], head_shapes: Dict[str, tuple]):
    """Sort a checkpoint's tensors for this model: -> (trunk state dict without its prefix, head tensors to take, report).
    The trunk is `bert.*` (this class, NomicBertForPreTraining) or `trunk.*` (a bi-encoder tower).  A head tensor is taken when
    it is there with this model's shape; report["fresh"] names the head tensors the checkpoint lacks (they keep their fresh
    initialisation), report["mismatched"] those it has in another shape (ignore_mismatched_sizes: fresh too), report["skipped"]
    every other key (`cls.*` of an MLM checkpoint, a projection head)."""
    prefix = "trunk." if any(k.startswith("trunk.") for k in sd) and not any(k.startswith("bert.") for k in sd) else "bert."
    as_head = lambda k: "bert." + k[len(prefix):] if k.startswith(prefix) else k   # noqa: E731  (trunk.pooler.* -> bert.pooler.*)
    trunk = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix) and as_head(k) not in head_shapes}
    taken, report = {}, {"fresh": [], "mismatched": [], "skipped": []}
    found = {as_head(k): v for k, v in sd.items() if as_head(k) in head_shapes}
    for k, shape in head_shapes.items():
        if k not in found:
            report["fresh"].append(k)
        elif tuple(found[k].shape) != tuple(shape):
            report["mismatched"].append(k)
        else:
            taken[k] = found[k]
    report["skipped"] = sorted(k for k in sd if not k.startswith(prefix) and k not in head_shapes)
    return trunk, taken, report


def reference_keys(config: NomicBertConfig) -> List[str]:
    """The state-dict keys of this model for `config`, which are the reference's (no device needed)."""
    fake = SimpleNamespace(config=config, _LAYER_PREFIX=NomicBertEngine._LAYER_PREFIX)
    fake._layer_specs = lambda l: NomicBertEngine._layer_specs(fake, l)
    decay, nodecay = NomicBertEngine._param_specs(fake)
    keys = []
    for name, _ in decay + nodecay:
        if ".mlp.fc1_fused." in name:
            keys += [name.replace("fc1_fused", n) for n in (("fc11", "fc12") if config.gated else ("fc1",))]
        else:
            keys.append(name)
    return sorted(["bert." + k for k in keys] + [_POOLER_W, _POOLER_B, _CLS_W, _CLS_B])


def checkpoint_trunk_config(path: str) -> Optional[NomicBertConfig]:
    """The trunk architecture a checkpoint directory was written with (config.json: trunk_config), or None."""
    cfg_path = os.path.join(path, "config.json")
    if not os.path.exists(cfg_path):
        return None
    with open(cfg_path) as f:
        cfg = json.load(f)
    tc = cfg.get("trunk_config")
    if tc is None:
        return None
    return NomicBertConfig(**{k: v for k, v in tc.items() if k in NomicBertConfig.__dataclass_fields__})


class _SeqClsFn(torch.autograd.Function):
    """autograd bridge of `forward`: the backward runs the head's and the trunk's backward and accumulates into the flat
    gradient buffers (as `_EncodeFn` does for the trunk); the logits are an output without gradient."""

    @staticmethod
    def forward(ctx, _anchor, model: NomicBertForSequenceClassification, vb: VarlenBatch, lab, mode: int, count: int):
        emb, arena = model.bert.forward_chunk(vb, True, normalize=False)
        drop = model._draw_dropout()
        pooled, logits, rows = model._head_fwd(emb, lab, mode, drop)
        ctx.model, ctx.vb, ctx.arena, ctx.state = model, vb, arena, (emb, pooled, logits, lab, mode, count, drop)
        ctx.mark_non_differentiable(logits)
        return rows.sum() / max(count, 1), logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        model, arena = ctx.model, ctx.arena
        ctx.arena = None
        emb, pooled, logits, lab, mode, count, drop = ctx.state
        dx = model._head_bwd(emb, pooled, logits, lab, mode, float(dloss) / max(count, 1), drop)
        model.bert.backward_chunk(ctx.vb, arena, dx)
        return None, None, None, None, None, None
