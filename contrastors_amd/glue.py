"""GLUE fine-tuning on the native trunk: host-side mirror of `GlueTrainer` (sc/trainers/glue.py:13-250) and of the parts of
`BaseTrainer` it uses (sc/trainers/base.py:228-265 scheduler, :366-393 training step, :395-520 epoch loop).

What differs from the reference is only where things come from: there is no hub, so the task's data is a LOCAL directory
(`data_args.input_shards`: a `datasets.load_from_disk` DatasetDict, or `<split>.jsonl` files), the tokenizer a local one, the
checkpoint a directory written by `save_pretrained`, and the GLUE metrics (`evaluate.load("glue", task)`) are restated in numpy
(`glue_metric`).  The model is `contrastors_amd.seqcls.NomicBertForSequenceClassification`: typed embeddings, fused head.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Iterable, Iterator, List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from .config import Config
from .distributed import gather
from .nomic_bert import NomicBertConfig
from .optimizer import FusedAdamW
from .seqcls import NomicBertForSequenceClassification, checkpoint_trunk_config

# sc/trainers/glue.py:13-45
task_to_keys = {
    "cola": ("sentence", None),
    "mnli": ("premise", "hypothesis"),
    "mrpc": ("sentence1", "sentence2"),
    "qnli": ("question", "sentence"),
    "qqp": ("question1", "question2"),
    "rte": ("sentence1", "sentence2"),
    "sst2": ("sentence", None),
    "stsb": ("sentence1", "sentence2"),
    "wnli": ("sentence1", "sentence2"),
}
task_to_problem_type = {
    "cola": "single_label_classification",
    "mnli": "single_label_classification",
    "mrpc": "single_label_classification",
    "qnli": "single_label_classification",
    "qqp": "single_label_classification",
    "rte": "single_label_classification",
    "sst2": "single_label_classification",
    "stsb": "regression",
}
task_to_num_labels = {"cola": 2, "mnli": 3, "mrpc": 2, "qnli": 2, "qqp": 2, "rte": 2, "sst2": 2, "stsb": 1}


# ---- metrics: evaluate.load("glue", task).compute(predictions=, references=) in numpy ---------------------------------------
def _average_ranks(x: np.ndarray) -> np.ndarray:
    """Ranks 1..n, ties share the mean of the ranks they span (scipy.stats.rankdata, method="average")."""
    order = np.argsort(x, kind="mergesort")
    xs = x[order]
    first = np.r_[True, xs[1:] != xs[:-1]]
    group = np.cumsum(first)                              # 1-based tie-group index of every sorted element
    bounds = np.r_[np.nonzero(first)[0], len(x)]          # start of every group, then n
    ranks = np.empty(len(x), np.float64)
    ranks[order] = 0.5 * (bounds[group] + bounds[group - 1] + 1)
    return ranks


def pearson(x, y) -> float:
    """scipy.stats.pearsonr(x, y)[0]; NaN when either side is constant (the correlation is undefined; scipy returns NaN too)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    xm, ym = x - x.mean(), y - y.mean()
    nx, ny = np.linalg.norm(xm), np.linalg.norm(ym)
    if nx == 0.0 or ny == 0.0:
        return float("nan")
    return float(np.clip(np.dot(xm / nx, ym / ny), -1.0, 1.0))


def spearman(x, y) -> float:
    """scipy.stats.spearmanr(x, y)[0]: Pearson of the average ranks; NaN when either side is constant."""
    return pearson(_average_ranks(np.asarray(x, np.float64)), _average_ranks(np.asarray(y, np.float64)))


def matthews_corrcoef(references, predictions) -> float:
    """sklearn.metrics.matthews_corrcoef (multi-class form); 0.0 when either side has a single class."""
    t, p = np.asarray(references), np.asarray(predictions)
    classes = np.unique(np.concatenate([t, p]))
    ti, pi = np.searchsorted(classes, t), np.searchsorted(classes, p)
    cm = np.zeros((len(classes), len(classes)), np.float64)
    np.add.at(cm, (ti, pi), 1.0)
    t_sum, p_sum, correct, n = cm.sum(1), cm.sum(0), np.trace(cm), cm.sum()
    cov_tp = correct * n - np.dot(t_sum, p_sum)
    cov_pp, cov_tt = n * n - np.dot(p_sum, p_sum), n * n - np.dot(t_sum, t_sum)
    if cov_pp * cov_tt == 0:
        return 0.0
    return float(cov_tp / np.sqrt(cov_tt * cov_pp))


def f1_binary(references, predictions) -> float:
    """sklearn.metrics.f1_score(y_true, y_pred) for labels {0, 1}, positive class 1; 0.0 when nothing is or is called positive."""
    t, p = np.asarray(references), np.asarray(predictions)
    tp = float(np.sum((t == 1) & (p == 1)))
    fp, fn = float(np.sum((t != 1) & (p == 1))), float(np.sum((t == 1) & (p != 1)))
    return 0.0 if 2 * tp + fp + fn == 0 else 2 * tp / (2 * tp + fp + fn)


def glue_metric(task: str, predictions, references) -> Dict[str, float]:
    if task not in task_to_keys and task not in ("mnli_matched", "mnli_mismatched"):
        raise KeyError(f"unknown GLUE task {task!r}")
    p, r = np.asarray(predictions), np.asarray(references)
    if task == "cola":
        return {"matthews_correlation": matthews_corrcoef(r, p)}
    if task == "stsb":
        return {"pearson": pearson(p, r), "spearmanr": spearman(p, r)}
    acc = float((p == r).mean())
    if task in ("mrpc", "qqp"):
        return {"accuracy": acc, "f1": f1_binary(r, p)}
    return {"accuracy": acc}


# ---- data: a local directory instead of load_dataset("glue", task) (sc/trainers/glue.py:75-156) ------------------------------
def _splits_for(task: str) -> Sequence[str]:
    return ("train", "validation_matched", "validation_mismatched") if task == "mnli" else ("train", "validation")


def load_glue_dir(path: str, task: str) -> Dict[str, List[dict]]:
    """{split: records} of the splits the trainer uses (test splits are dropped, :78-82).  `path` holds either what
    `datasets.DatasetDict.save_to_disk` wrote or `<split>.jsonl` files; records carry the task's text columns and `label`."""
    if task not in task_to_num_labels:
        raise ValueError(f"task_name {task!r} is not one of {sorted(task_to_num_labels)}")
    want = _splits_for(task)
    if os.path.exists(os.path.join(path, "dataset_dict.json")):
        from datasets import load_from_disk

        dd = load_from_disk(path)
        missing = [s for s in want if s not in dd]
        if missing:
            raise FileNotFoundError(f"{path}: no split {missing} for task {task}")
        return {s: [dict(r) for r in dd[s]] for s in want}
    out = {}
    for s in want:
        f = os.path.join(path, f"{s}.jsonl")
        if not os.path.exists(f):
            raise FileNotFoundError(f"{f}: task {task} needs {list(want)} as .jsonl files or a saved DatasetDict")
        with open(f) as fh:
            out[s] = [json.loads(line) for line in fh if line.strip()]
    return out


def encode_glue(raw: Dict[str, List[dict]], task: str, tokenizer, seq_len: int) -> Dict[str, List[dict]]:
    """The reference's preprocess_function (:98-114): tokenizer(*texts, padding=False, max_length=seq_len, truncation=True);
    classification labels go through the sorted label list of the train split, regression labels stay floats."""
    k1, k2 = task_to_keys[task]
    label_to_id = None
    if task_to_problem_type[task] != "regression":
        label_to_id = {v: i for i, v in enumerate(sorted({r["label"] for r in raw["train"]}))}
    out = {}
    for split, recs in raw.items():
        texts = ([r[k1] for r in recs],) if k2 is None else ([r[k1] for r in recs], [r[k2] for r in recs])
        enc = tokenizer(*texts, padding=False, max_length=seq_len, truncation=True) if recs else {"input_ids": []}
        rows = []
        for i, r in enumerate(recs):
            row = {"input_ids": list(enc["input_ids"][i])}
            if "token_type_ids" in enc:
                row["token_type_ids"] = list(enc["token_type_ids"][i])
            if "label" in r:
                row["labels"] = label_to_id[r["label"]] if label_to_id is not None else float(r["label"])
            rows.append(row)
        out[split] = rows
    return out


def collate(rows: List[dict], pad_token_id: int = 0) -> Dict[str, torch.Tensor]:
    """DataCollatorWithPadding (:126): right-pad to the longest row of THIS batch; segment ids pad with 0."""
    S = max(len(r["input_ids"]) for r in rows)
    B = len(rows)
    ids = torch.full((B, S), pad_token_id, dtype=torch.int64)
    mask = torch.zeros(B, S, dtype=torch.int64)
    typed = "token_type_ids" in rows[0]
    tt = torch.zeros(B, S, dtype=torch.int64) if typed else None
    for i, r in enumerate(rows):
        n = len(r["input_ids"])
        ids[i, :n] = torch.as_tensor(r["input_ids"], dtype=torch.int64)
        mask[i, :n] = 1
        if typed:
            tt[i, :n] = torch.as_tensor(r["token_type_ids"], dtype=torch.int64)
    batch = {"input_ids": ids, "attention_mask": mask}
    if typed:
        batch["token_type_ids"] = tt
    if "labels" in rows[0]:
        lab = [r["labels"] for r in rows]
        batch["labels"] = torch.tensor(lab, dtype=torch.float32 if isinstance(lab[0], float) else torch.int64)
    return batch


class ShardedBatches:
    """The batches of one rank for one pass over `rows`.  Global batch g holds rows [g * bs * world, (g + 1) * bs * world) of the
    (shuffled) order and rank r its r-th contiguous share, so a rank-ordered gather restores the order; the last global batch
    is padded to a multiple of `world` by wrapping around (every rank runs the same number of equally shaped steps, as under
    DistributedSampler), which puts the duplicates at the very end of the gathered batch -- where the evaluation loop trims
    them (sc/trainers/glue.py:191-197)."""

    def __init__(self, rows: List[dict], batch_size: int, rank: int = 0, world: int = 1, shuffle: bool = False, seed: int = 0,
                 pad_token_id: int = 0):
        self.rows, self.bs, self.rank, self.world = rows, int(batch_size), rank, world
        self.shuffle, self.seed, self.pad_token_id, self.epoch = shuffle, seed, pad_token_id, 0
        if self.bs <= 0:
            raise ValueError("batch_size must be positive")

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def __len__(self) -> int:
        return -(-len(self.rows) // (self.bs * self.world))

    def order(self) -> List[int]:
        n = len(self.rows)
        if not self.shuffle:
            return list(range(n))
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        return torch.randperm(n, generator=g).tolist()

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        order, n, span = self.order(), len(self.rows), self.bs * self.world
        for start in range(0, n, span):
            idx = order[start: start + span]
            share = -(-len(idx) // self.world)
            idx = idx + [order[i % n] for i in range(share * self.world - len(idx))]   # wrap-around padding
            mine = idx[self.rank * share: (self.rank + 1) * share]
            yield collate([self.rows[i] for i in mine], self.pad_token_id)


def trim_gathered(predictions, references, seen: int, total: int, last: bool, world: int):
    """sc/trainers/glue.py:191-197: on several ranks the last gathered batch ends in duplicates; keep what is still missing.
    -> (predictions, references, samples seen so far)."""
    if world > 1 and last:
        predictions, references = predictions[: total - seen], references[: total - seen]
    return predictions, references, seen + int(references.shape[0])


def warmup_steps_for(train_args, steps_per_epoch: int) -> int:
    """sc/trainers/base.py:228-238: warmup_steps as given, else int(steps_per_epoch * num_epochs * warmup_pct), else 0."""
    if train_args.warmup_steps is not None:
        return int(train_args.warmup_steps)
    if train_args.warmup_pct is not None:
        return int(steps_per_epoch * train_args.num_epochs * train_args.warmup_pct)
    return 0


class GlueTrainer:
    """sc/trainers/glue.py on the native path.  `datasets`: already encoded {split: rows} (tests, synthetic tasks); otherwise
    `data_args.input_shards` + a local tokenizer.  `trunk_config`: the architecture when the checkpoint directory does not
    carry one (or there is no checkpoint: a freshly initialised trunk)."""

    def __init__(self, config: Config, dtype=torch.bfloat16, device=None, trunk_config: Optional[NomicBertConfig] = None,
                 total_steps: Optional[int] = None, tokenizer=None, datasets: Optional[Dict[str, List[dict]]] = None):
        if dtype != torch.bfloat16:
            raise NotImplementedError("the native path computes in bf16 with fp32 master weights (--dtype=bf16)")
        from .trainers import _lr_lambda

        self.config = config
        ta, ma, da = config.train_args, config.model_args, config.data_args
        self.task = da.task_name
        if self.task not in task_to_num_labels:   # (wnli has text columns but no problem type in the reference either)
            raise ValueError(f"data_args.task_name {self.task!r} is not one of {sorted(task_to_num_labels)}")
        self.is_regression = task_to_problem_type[self.task] == "regression"
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size() if self.distributed else 1
        self.rank = dist.get_rank() if self.distributed else 0
        self.device = torch.device(device or f"cuda:{torch.cuda.current_device()}")
        torch.manual_seed(da.seed)
        # ---- data (before the model: the schedule's horizon is the train split's length)
        if datasets is None:
            if not da.input_shards:
                raise ValueError("GLUE needs data_args.input_shards: a local directory with the task's splits (there is no hub)")
            if tokenizer is None:
                from transformers import AutoTokenizer

                tokenizer = AutoTokenizer.from_pretrained(ma.tokenizer_name, local_files_only=True)
            datasets = encode_glue(load_glue_dir(da.input_shards, self.task), self.task, tokenizer, ma.seq_len)
        pad_id = getattr(tokenizer, "pad_token_id", None) or 0
        self.datasets = datasets
        self.train_batches = ShardedBatches(datasets["train"], da.batch_size, self.rank, self.world, shuffle=True, seed=da.seed,
                                            pad_token_id=pad_id)
        val = ("validation_matched", "validation_mismatched") if self.task == "mnli" else ("validation",)
        self.val_batches = {s: ShardedBatches(datasets[s], da.batch_size, self.rank, self.world, pad_token_id=pad_id)
                            for s in val if s in datasets}
        self.accum = max(1, int(ta.gradient_accumulation_steps or 1))
        self.steps_per_epoch = len(self.train_batches) // self.accum            # glue.py:150 total_num_steps
        self.max_steps = total_steps                                              # optional cap on micro-steps (smoke runs)
        # ---- model (glue.py:54-73)
        ckpt = ma.checkpoint
        if ckpt is not None and not os.path.isdir(ckpt):
            raise FileNotFoundError(f"model_args.checkpoint {ckpt!r}: not a local directory (there is no hub)")
        tc = trunk_config or (checkpoint_trunk_config(ckpt) if ckpt else None)
        if tc is None:
            raise ValueError("no trunk architecture: model_args.checkpoint must be a directory whose config.json carries "
                             "trunk_config (save_pretrained writes it), or pass trunk_config")
        model = NomicBertForSequenceClassification(tc, task_to_num_labels[self.task], task_to_problem_type[self.task],
                                                   device=self.device, seed=da.seed).train()
        self.load_report = model.load_pretrained(ckpt) if ckpt else None
        if self.load_report and self.rank == 0:
            print(f"glue: {ckpt}: head tensors at their fresh initialisation {self.load_report['fresh']}, shape mismatches "
                  f"{self.load_report['mismatched']}, skipped {self.load_report['skipped']}", flush=True)
        if ma.gradient_checkpointing:
            model.gradient_checkpointing_enable(True, ta.checkpoint_keep_layers)
        if self.world > 1:
            dist.broadcast(model.bert.flat_param, 0)
            dist.broadcast(model._head_param, 0)
            model.bert.sync_shadows()
        self.model = {"model": model}
        self.optimizer = FusedAdamW(model.param_groups(ta.weight_decay), lr=ta.learning_rate,
                                    betas=(ta.adam_beta1, ta.adam_beta2), eps=ta.eps)
        self.total_steps = self.steps_per_epoch * ta.num_epochs                  # base.py:230,234
        self.warmup_steps = warmup_steps_for(ta, self.steps_per_epoch)
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer,
                                                           _lr_lambda(ta.schedule_type, self.warmup_steps, self.total_steps))
        self.step = 0
        self.epoch = 0
        self.history: List[dict] = []

    # ---- one micro-batch (base.py:366-393; the quirks MLMTrainer.training_step documents are the same code there)
    def training_step(self, batch) -> torch.Tensor:
        ta, model = self.config.train_args, self.model["model"]
        out = model.forward_backward(batch["input_ids"], batch.get("attention_mask"), batch.get("token_type_ids"), batch["labels"])
        clip = ta.max_grad_norm is not None and ta.max_grad_norm > 0      # glue.yaml: 0.0 = no clipping (base.py:376)
        fire = (self.step + 1) % self.accum == 0 or self.step == self.total_steps - 1
        if fire:
            model.sync_gradients()
        if clip and self.accum > 1 and self.step % self.accum == 0:
            params = [p for g in self.optimizer.param_groups for p in g["params"] if p.grad is not None]
            torch.nn.utils.clip_grad_norm_(params, ta.max_grad_norm)
        if fire:
            self.optimizer.step(max_grad_norm=ta.max_grad_norm if (clip and self.accum == 1) else None)
            self.scheduler.step()
            model.bert.sync_shadows()
            model.zero_grad()
        self.step += 1
        return out.loss.detach()

    def train(self, batches: Optional[Iterable[dict]] = None, max_steps: Optional[int] = None, log_every: int = 0):
        """base.py:395-520: `num_epochs` passes over the train split (reshuffled per epoch), evaluation after every epoch for
        eval_strategy "epochs".  With `batches` given: the plain driver loop of the other trainers (one call = one micro-batch)."""
        ta = self.config.train_args
        cap = max_steps if max_steps is not None else self.max_steps
        losses = []

        def run(it, limit):
            for i, batch in enumerate(it):
                if (limit is not None and i >= limit) or (cap is not None and len(losses) >= cap):
                    break
                losses.append(self.training_step(batch))
                if log_every and len(losses) % log_every == 0 and self.rank == 0:
                    print(f"step {self.step} loss {float(losses[-1]):.4f} lr {self.scheduler.get_last_lr()[0]:.3e}", flush=True)

        if batches is not None:
            run(batches, None)
            return losses
        for epoch in range(self.epoch, ta.num_epochs):
            self.train_batches.set_epoch(epoch)
            run(self.train_batches, self.steps_per_epoch)      # base.py:465 `if step >= total_training_steps: break`
            self.epoch = epoch + 1
            if ta.eval_strategy == "epochs":
                metrics = self.evaluate()
                self.history.append({"epoch": epoch, **metrics})
                if self.rank == 0:
                    print({**metrics, "epoch": epoch}, flush=True)
            if cap is not None and len(losses) >= cap:
                break
        return losses

    # ---- evaluation (glue.py:175-231)
    @torch.no_grad()
    def predict(self, batches: ShardedBatches):
        """-> (predictions, references) of the whole split in dataset order, the same on every rank."""
        model = self.model["model"]
        was = model.training
        model.eval()
        preds, refs, seen, total = [], [], 0, len(batches.rows)
        try:
            for i, batch in enumerate(batches):
                logits = model(batch["input_ids"], batch.get("attention_mask"), batch.get("token_type_ids")).logits
                p = logits.squeeze(-1) if self.is_regression else logits.argmax(dim=-1)
                p, r = gather(p.contiguous()), gather(batch["labels"].to(p.device))
                p, r, seen = trim_gathered(p, r, seen, total, i == len(batches) - 1, self.world)
                preds.append(p.cpu())
                refs.append(r.cpu())
        finally:
            model.train(was)
        return torch.cat(preds).numpy(), torch.cat(refs).numpy()

    def evaluate(self) -> Dict[str, dict]:
        """{"val_metric": ...} and, for MNLI, {"val_mm_metric": ...} (glue.py:224-229)."""
        out = {}
        for split, batches in self.val_batches.items():
            key = "val_mm_metric" if split == "validation_mismatched" else "val_metric"
            out[key] = glue_metric(self.task, *self.predict(batches))
        return out

    # ---- state on disk (base.py:292-344)
    def save_state(self, output_dir: str):
        os.makedirs(output_dir, exist_ok=True)
        if self.rank == 0:
            self.model["model"].save_pretrained(os.path.join(output_dir, "model"))
            torch.save(self.optimizer.state_dict(), os.path.join(output_dir, "optimizer.pt"))
            torch.save(self.scheduler.state_dict(), os.path.join(output_dir, "scheduler.pt"))
            torch.save({"step": self.step, "epoch": self.epoch}, os.path.join(output_dir, "trainer_state.pt"))
        if self.distributed:
            dist.barrier()
        torch.save({"torch": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(self.device)},
                   os.path.join(output_dir, f"random_states_{self.rank}.pt"))

    def load_state(self, input_dir: str):
        model = self.model["model"]
        model.load_pretrained(os.path.join(input_dir, "model"))
        self.optimizer.load_state_dict(torch.load(os.path.join(input_dir, "optimizer.pt"), map_location=self.device))
        self.scheduler.load_state_dict(torch.load(os.path.join(input_dir, "scheduler.pt")))
        st = torch.load(os.path.join(input_dir, "trainer_state.pt"))
        self.step, self.epoch = int(st["step"]), int(st["epoch"])
        rs = torch.load(os.path.join(input_dir, f"random_states_{self.rank}.pt"), weights_only=False)
        torch.set_rng_state(rs["torch"])
        torch.cuda.set_rng_state(rs["cuda"], self.device)
        model.zero_grad()
