"""Microbenchmark of the fused sequence-classification head (cx_seqcls_head_fwd / cx_seqcls_head_bwd) inside one GLUE step.

    python scripts/seqcls_microbench.py [--batch 32] [--seq 128] [--labels 2] [--reps 9] [--out FILE]

One bert-base training micro-step (typed embeddings, 12 layers, dropout 0.1 as the converted HF config has it, forward +
backward, no optimizer) at B = 32, S = 128, timed two ways, alternated repetition by repetition in one process after a warm-up
of both, medians of `reps` (>= 7):
  (a) the fused head: NomicBertForSequenceClassification.forward_backward;
  (b) the same trunk calls with the head composed from torch ops in fp32 (linear, tanh, dropout, linear, cross_entropy; autograd),
      its d(loss)/d(X) handed to the same trunk backward.
The head alone (the trunk's output held fixed) is timed the same way.  Times are device events around each call; the kernel count
of one step comes from torch.profiler (reported as n/a where the profiler is not available).  Needs the GPU: there is no fallback."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from contrastors_amd.nomic_bert import NomicBertConfig, VarlenBatch  # noqa: E402
from contrastors_amd.seqcls import NomicBertForSequenceClassification  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def kernel_count(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower()
                   and "memset" not in ev.name.lower())
    except Exception as exc:   # noqa: BLE001  (a measurement aid: the timings do not depend on it)
        print(f"kernel count not available: {type(exc).__name__}: {exc}")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--labels", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seqcls_microbench needs the GPU")
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    B, S, C = args.batch, args.seq, args.labels
    dev = "cuda"
    torch.manual_seed(0)
    cfg = NomicBertConfig.bert_base_uncased(hf_dropout=True)
    model = NomicBertForSequenceClassification(cfg, C, "single_label_classification", device=dev, seed=0).train()
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(S // 2, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = (torch.randint(1000, cfg.vocab_size, (B, S), generator=g) * mask).to(dev)
    cut = (lens // 2)[:, None]
    tts = ((torch.arange(S)[None] >= cut) & mask.bool()).long().to(dev)
    mask = mask.to(dev)
    labels = torch.randint(0, C, (B,), generator=g)          # on the host, as a dataloader hands them over
    p = model.classifier_dropout
    head = {k: v.detach().clone().requires_grad_() for k, v in model.head().items()}
    Wp, bp = head["bert.pooler.dense.weight"], head["bert.pooler.dense.bias"]
    Wc, bc = head["classifier.weight"], head["classifier.bias"]

    def torch_head(emb):
        x = emb.detach().requires_grad_()
        logits = F.linear(F.dropout(torch.tanh(F.linear(x, Wp, bp)), p, training=True), Wc, bc)
        loss = F.cross_entropy(logits, labels.to(dev))       # (both paths take the labels from the host, every step)
        loss.backward()
        return loss.detach(), x.grad

    def step_fused():
        return model.forward_backward(ids, mask, tts, labels).loss

    def step_torch():
        vb = VarlenBatch.from_mask(ids, mask).with_token_types(tts)
        emb, arena = model.bert.forward_chunk(vb, True, normalize=False)
        loss, dx = torch_head(emb)
        model.bert.backward_chunk(vb, arena, dx)
        return loss

    vb0 = VarlenBatch.from_mask(ids, mask).with_token_types(tts)
    emb0, _ = model.bert.forward_chunk(vb0, False, normalize=False)
    count = B

    def head_fused():
        lab0, _ = model._labels(labels, 0, B)
        drop = model._draw_dropout()
        pooled, logits, rows = model._head_fwd(emb0, lab0, 0, drop)
        model._grads_clean = True
        return model._head_bwd(emb0, pooled, logits, lab0, 0, 1.0 / count, drop)

    def head_torch():
        return torch_head(emb0)

    paths = {"step_fused": step_fused, "step_torch": step_torch, "head_fused": head_fused, "head_torch": head_torch}
    times = {k: [] for k in paths}
    for rep in range(args.warmup + args.reps):
        for k, fn in paths.items():
            model.zero_grad()
            t, _ = timed(fn)
            if rep >= args.warmup:
                times[k].append(t)
    counts = {}
    for k, fn in paths.items():
        model.zero_grad()
        counts[k] = kernel_count(fn)
    med = {k: statistics.median(v) for k, v in times.items()}
    names = {"step_fused": "(a) step, fused head", "step_torch": "(b) step, head from torch ops", "head_fused": "(a) head alone, fused",
             "head_torch": "(b) head alone, torch ops"}
    lines = [f"sequence-classification microbench: bert-base, B = {B}, S = {S} (ragged, {int(lens.sum())} tokens), {C} labels, classifier "
             f"dropout {p}; {args.reps} timed repetitions after {args.warmup} warm-up, paths alternated; device {torch.cuda.get_device_name(0)}",
             f"{'path':34s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'kernels':>8s}"]
    for k in paths:
        n = "n/a" if counts[k] is None else str(counts[k])
        lines.append(f"{names[k]:34s} {med[k]:10.3f} {min(times[k]):8.3f} {max(times[k]):8.3f} {n:>8s}")
    lines.append(f"step: (b) - (a) = {med['step_torch'] - med['step_fused']:.3f} ms ((b)/(a) = {med['step_torch'] / med['step_fused']:.3f});  "
                 f"head alone: (b)/(a) = {med['head_torch'] / med['head_fused']:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
