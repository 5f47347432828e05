"""Microbenchmark of the fused similarity-KL loss (cx_simkl_fwd / cx_simkl_bwd) at a large in-batch distillation shape.

    python scripts/distill_loss_microbench.py [--n 16384] [--g 16384] [--dim 768] [--tau 0.2] [--reps 9] [--out FILE]

Three paths, alternated repetition by repetition in one process after a warm-up of every path, medians of `reps` (>= 7):
  (a) the fused kernel: forward (both products + both soft-maxes, one launch + combine) and backward (recompute, Gm / Gm^T, two GEMMs);
  (b) two cx_infonce_fwd / cx_infonce_bwd calls at the same shape -- that kernel does ONE of the two products with ONE of the
      two soft-maxes, so twice its time is the structural yardstick for (a);
  (c) the fp32 eager torch restatement (two matmuls, softmax, log_softmax, the sum; autograd), with its peak memory.
Times are device events around each call.  FLOP counts come from the shapes.  Needs the GPU: there is no fallback."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from contrastors_amd import _C  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--g", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--tau", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_loss_microbench needs the GPU")
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    N, G, dim, tau = args.n, args.g, args.dim, args.tau
    dev = "cuda"
    lib = _C.lib()
    S = _C.cur_stream()
    f32 = dict(dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(0)
    norm = torch.nn.functional.normalize
    tq, td = norm(torch.randn(N, dim, generator=g), dim=-1).to(dev), norm(torch.randn(G, dim, generator=g), dim=-1).to(dev)
    sq = norm(tq + 0.3 * torch.randn(N, dim, generator=g).to(dev) / dim ** 0.5, dim=-1)
    sd = norm(td + 0.3 * torch.randn(G, dim, generator=g).to(dev) / dim ** 0.5, dim=-1)
    labels = torch.arange(N, device=dev) * (G // N)
    inv, coef = 1.0 / tau, 1.0 / N

    # caller-owned buffers, allocated once (both native paths share the backward scratch: 2 x (N, G) fp32)
    ws = torch.empty(max(lib.cx_simkl_ws_floats(N, G), lib.cx_infonce_ws_floats(N, G)), **f32)
    lse_s, lse_t, rows = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, **f32)
    gm, gmt = torch.empty(N, G, **f32), torch.empty(G, N, **f32)
    qt, dt = torch.empty(dim, N, **f32), torch.empty(dim, G, **f32)
    dq, dd = torch.empty(N, dim, **f32), torch.empty(G, dim, **f32)
    P = lambda t: t.data_ptr()  # noqa: E731

    def a_fwd():
        _C.check(lib.cx_simkl_fwd(P(sq), P(sd), P(tq), P(td), inv, P(ws), P(lse_s), P(lse_t), P(rows), N, G, dim, dim, dim, dim,
                                  dim, dim, S), "cx_simkl_fwd")

    def a_bwd():
        _C.check(lib.cx_simkl_bwd(P(sq), P(sd), P(tq), P(td), P(lse_s), P(lse_t), inv, coef, P(gm), P(gmt), P(qt), P(dt), P(dq),
                                  P(dd), N, G, dim, dim, dim, dim, dim, dim, S), "cx_simkl_bwd")

    def b_fwd():
        for q_, d_, l_ in ((sq, sd, lse_s), (tq, td, lse_t)):
            _C.check(lib.cx_infonce_fwd(P(q_), P(d_), P(labels), inv, P(ws), P(l_), P(rows), N, G, dim, dim, dim, S), "cx_infonce_fwd")

    def b_bwd():
        for q_, d_, l_ in ((sq, sd, lse_s), (tq, td, lse_t)):
            _C.check(lib.cx_infonce_bwd(P(q_), P(d_), P(labels), P(l_), inv, coef, P(gm), P(gmt), P(qt), P(dt), P(dq), P(dd), None,
                                        N, G, dim, dim, dim, S), "cx_infonce_bwd")

    def c_fwd():
        q, d = sq.detach().requires_grad_(), sd.detach().requires_grad_()
        s, t = (q @ d.T) / tau, (tq @ td.T) / tau
        loss = (torch.softmax(t, -1) * (torch.log_softmax(t, -1) - torch.log_softmax(s, -1))).sum() / N
        return loss, q, d

    times = {k: [] for k in ("a_fwd", "a_bwd", "b_fwd", "b_bwd", "c_fwd", "c_bwd")}
    peak_c = 0
    check = {}
    for rep in range(args.warmup + args.reps):
        keep = rep >= args.warmup
        ta, _ = timed(a_fwd)
        loss_a = float(rows.sum() * coef)
        tab, _ = timed(a_bwd)
        if rep == 0:
            check["dq_a"], check["dd_a"] = dq.clone(), dd.clone()
        tb, _ = timed(b_fwd)
        tbb, _ = timed(b_bwd)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tc, (loss_c, q, d) = timed(c_fwd)
        tcb, _ = timed(loss_c.backward)
        peak_c = max(peak_c, torch.cuda.max_memory_allocated() - base)
        if rep == 0:
            check["loss_a"], check["loss_c"] = loss_a, float(loss_c.detach())
            check["e_dq"] = float((check["dq_a"] - q.grad).norm() / q.grad.norm())
            check["e_dd"] = float((check["dd_a"] - d.grad).norm() / d.grad.norm())
        del loss_c, q, d
        if keep:
            for k, v in zip(times, (ta, tab, tb, tbb, tc, tcb)):
                times[k].append(v)

    med = {k: statistics.median(v) for k, v in times.items()}
    lo = {k: min(v) for k, v in times.items()}
    hi = {k: max(v) for k, v in times.items()}
    prod = 2.0 * N * G * dim                      # one (N, G) product
    flop = {"a_fwd": 2 * prod, "a_bwd": 4 * prod, "b_fwd": 2 * prod, "b_bwd": 6 * prod}   # (b_bwd: per call 1 recompute + 2 output GEMMs)
    lines = [f"similarity-KL microbench: N = {N}, G = {G}, dim_s = dim_t = {dim}, tau = {tau}; {args.reps} timed repetitions after "
             f"{args.warmup} warm-up, paths alternated; device {torch.cuda.get_device_name(0)}",
             f"{'path':34s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'TFLOP':>7s} {'TFLOP/s':>8s}"]
    names = {"a_fwd": "(a) cx_simkl_fwd", "a_bwd": "(a) cx_simkl_bwd", "b_fwd": "(b) 2 x cx_infonce_fwd", "b_bwd": "(b) 2 x cx_infonce_bwd",
             "c_fwd": "(c) fp32 eager forward", "c_bwd": "(c) fp32 eager backward"}
    for k in times:
        fl = flop.get(k)
        lines.append(f"{names[k]:34s} {med[k]:10.3f} {lo[k]:8.3f} {hi[k]:8.3f} " +
                     (f"{fl / 1e12:7.3f} {fl / med[k] / 1e9:8.1f}" if fl else f"{'':7s} {'':8s}"))
    a, b, c = med["a_fwd"] + med["a_bwd"], med["b_fwd"] + med["b_bwd"], med["c_fwd"] + med["c_bwd"]
    native_bytes = 4 * (ws.numel() + gm.numel() + gmt.numel() + qt.numel() + dt.numel() + dq.numel() + dd.numel() + 3 * N)
    lines += [f"forward + backward: (a) {a:.3f} ms   (b) {b:.3f} ms   (c) {c:.3f} ms   (a)/(b) = {a / b:.3f}   (c)/(a) = {c / a:.2f}",
              f"forward only:       (a)/(b) = {med['a_fwd'] / med['b_fwd']:.3f}    backward only: (a)/(b) = {med['a_bwd'] / med['b_bwd']:.3f}",
              f"memory beyond the inputs: (a) {native_bytes / 2**30:.2f} GiB of caller-owned scratch and outputs (the forward alone: "
              f"{4 * ws.numel() / 2**20:.1f} MiB);  (c) peak {peak_c / 2**30:.2f} GiB",
              f"agreement at this shape: loss (a) {check['loss_a']:.8f}  (c) {check['loss_c']:.8f};  gradient (a) against (c): "
              f"dQs {check['e_dq']:.2e}, dDs {check['e_dd']:.2e} (relative, both fp32)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
