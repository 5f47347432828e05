"""Microbenchmark of MLM masking at the recipe's per-micro-batch shape (mlm.yaml: batch 1024 / accumulation 4 -> 256 x 2048).

    python scripts/mlm_mask_microbench.py [--batch 256] [--seq 2048] [--reps 11] [--out FILE]

Paths, alternated repetition by repetition in one process after a warm-up of every path, medians of `reps` (>= 7):
  (a) device masking: the stacked int32 ids (pinned) copied to the GPU, then one cx_mlm_mask launch; the kernel is also timed
      alone, with and without the two mask inputs (int64 attention mask, uint8 special-tokens mask);
  (b) host masking: `mask_tokens` (the reference's collator) on the CPU in this process, then the int64 masked ids and labels
      (pinned) copied to the GPU.  In training the collator runs in the loader workers, where it can hide behind the step: the
      figure here is what one batch costs, not what the step waits for;
  (c) cx_calib_copy over as many bytes as the kernel moves (read + write), the HBM stream yardstick.
The kernel-only and copy rows are device events around `--inner` back-to-back launches through the C-ABI into preallocated
outputs, divided by `--inner` (a window around one call of the Python wrapper measures the wrapper); the two paths are a host
clock around work that ends in a synchronise.  Bytes are counted from the shapes.  Needs the GPU: there is no fallback."""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from contrastors_amd import _C  # noqa: E402
from contrastors_amd.mlm import mask_tokens  # noqa: E402
from contrastors_amd.mlm_data import mlm_mask  # noqa: E402


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--p", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="launches per timed window of the kernel-only and copy rows")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlm_mask_microbench needs the GPU")
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    B, S, p, dev = args.batch, args.seq, args.p, "cuda"
    n = B * S
    g = torch.Generator().manual_seed(0)
    ids64 = torch.randint(1000, 30522, (B, S), generator=g)
    ids64[:, 0], ids64[:, -1] = 101, 102
    special = torch.zeros(B, S, dtype=torch.bool)
    special[:, 0] = special[:, -1] = True
    ids32_pinned = ids64.to(torch.int32).pin_memory()
    d_ids = ids32_pinned.to(dev)
    d_attn = torch.ones(B, S, dtype=torch.int64, device=dev)
    d_spec = special.to(torch.uint8).to(dev)
    d_special_ids = torch.tensor([0, 100, 101, 102, 103], dtype=torch.int64, device=dev)
    pin_ids, pin_labels = torch.empty(B, S, dtype=torch.int64).pin_memory(), torch.empty(B, S, dtype=torch.int64).pin_memory()
    lib, stream = _C.lib(), _C.cur_stream()
    bytes_plain, bytes_masks = n * (4 + 16), n * (4 + 8 + 1 + 16)
    copy_src = torch.empty(bytes_masks // 2 // 16 * 16, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)
    offset = [0]

    out_ids, out_labels = torch.empty(B, S, dtype=torch.int64, device=dev), torch.empty(B, S, dtype=torch.int64, device=dev)

    def kernel(attn, spec):
        """`inner` back-to-back launches straight through the C-ABI into preallocated outputs: the window is device time, not the
        Python of the wrapper."""
        def run():
            for _ in range(args.inner):
                offset[0] += 1
                _C.check(lib.cx_mlm_mask(d_ids.data_ptr(), 0, S, _C.ptr(attn), _C.ptr(spec), d_special_ids.data_ptr(), 5, 103, 30522, p,
                                         42, offset[0], out_ids.data_ptr(), out_labels.data_ptr(), B, S, stream), "cx_mlm_mask")
        return run

    kernel_plain, kernel_masks = kernel(None, None), kernel(d_attn, d_spec)

    def device_path():
        offset[0] += 1
        return mlm_mask(ids32_pinned.to(dev, non_blocking=True), p, 42, offset[0], 103, 30522, None, None, d_special_ids)

    def host_path():
        masked, labels = mask_tokens(ids64, special, p, 103, 30522)
        pin_ids.copy_(masked)
        pin_labels.copy_(labels)
        return pin_ids.to(dev, non_blocking=True), pin_labels.to(dev, non_blocking=True)

    def host_mask_only():
        return mask_tokens(ids64, special, p, 103, 30522)

    def copy(nbytes):
        def run():
            for _ in range(args.inner):
                _C.check(lib.cx_calib_copy(copy_src.data_ptr(), copy_dst.data_ptr(), nbytes // 2 // 16 * 16, stream), "copy")
        return run

    paths = {"kernel_plain": (device_ms, kernel_plain), "kernel_masks": (device_ms, kernel_masks),
             "copy_plain": (device_ms, copy(bytes_plain)), "copy_masks": (device_ms, copy(bytes_masks)),
             "device_path": (host_ms, device_path), "host_path": (host_ms, host_path), "host_mask_only": (host_ms, host_mask_only)}
    moved = {"kernel_plain": bytes_plain, "kernel_masks": bytes_masks, "copy_plain": bytes_plain // 2 // 16 * 16 * 2,
             "copy_masks": bytes_masks // 2 // 16 * 16 * 2}
    times = {k: [] for k in paths}
    for rep in range(args.warmup + args.reps):
        for k, (clock, fn) in paths.items():
            ms, _ = clock(fn)
            if k in moved:
                ms /= args.inner
            if rep >= args.warmup:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    names = {"kernel_plain": "(a) cx_mlm_mask, int32 ids only", "kernel_masks": "(a) cx_mlm_mask + attention / special masks",
             "copy_plain": "(c) cx_calib_copy, bytes of the first", "copy_masks": "(c) cx_calib_copy, bytes of the second",
             "device_path": "(a) H2D int32 ids + cx_mlm_mask [host clock]", "host_path": "(b) mask_tokens + H2D ids, labels [host clock]",
             "host_mask_only": "(b) mask_tokens alone [host clock]"}
    lines = [f"MLM masking microbench: batch {B} x seq {S} = {n} tokens, p = {p}; {args.reps} timed repetitions after {args.warmup} "
             f"warm-up, paths alternated, {args.inner} launches per window in the kernel-only and copy rows; "
             f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}",
             f"{'path':52s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'MB moved':>9s} {'GB/s':>8s}"]
    for k in paths:
        mb = moved.get(k)
        lines.append(f"{names[k]:52s} {med[k]:10.4f} {min(times[k]):9.4f} {max(times[k]):9.4f} " +
                     (f"{mb / 1e6:9.2f} {mb / med[k] / 1e6:8.1f}" if mb else f"{'':9s} {'':8s}"))
    lines += [f"kernel / copy of the same bytes: {med['kernel_plain'] / med['copy_plain']:.2f} (ids only), "
              f"{med['kernel_masks'] / med['copy_masks']:.2f} (with masks)",
              f"one batch end to end, host clock: device path {med['device_path']:.3f} ms, host path {med['host_path']:.3f} ms "
              f"(of which mask_tokens {med['host_mask_only']:.3f} ms); the host path's share runs in loader workers during training"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
