"""The logit-free MLM head (contrastors_amd.linear_xent.linear_cross_entropy) next to the logit path (fused_dense_func +
CrossEntropyLoss(inplace_backward=True)) on the same inputs, by scripts/attn_window_microbench.py's method: same box, ONE process
in which all legs ALTERNATE run by run, device events, one warm-up round of all, medians of --reps runs with p10 - p90.

  shapes : K = 768, V = 30528, M in --rows: both paths; V = 250002, M in --big-rows: the logit-free path alone (the logits of
           the other would be M x 250002 x 2 bytes)
  legs   : forward (under no_grad) and forward + backward (gradients of x, weight and bias) of each path
  flops  : 2 M V K per GEMM-sized product: 1 forward; forward + backward 3 on the logit path, 4 on the logit-free one (it
           recomputes the logits); tflops below counts what each path executes

usage: python scripts/linear_xent_microbench.py [--rows 16384 65536] [--big-rows 16384] [--reps 11]
                                                [--out profiles/linear_xent_microbench.json]
The JSON record on stdout and, in a list, in --out.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from ivf_int8_microbench import DEV, alternate, summary  # noqa: E402

K = 768


def legs_for(M, V, with_logit_path, reps):
    import torch

    from contrastors_amd.flash_attn_api.losses.cross_entropy import CrossEntropyLoss
    from contrastors_amd.flash_attn_api.ops.fused_dense import fused_dense_func
    from contrastors_amd.linear_xent import linear_cross_entropy

    g = torch.Generator(device=DEV).manual_seed(M + V)
    x = (torch.randn(M, K, device=DEV, generator=g) * 4 / K ** 0.5).bfloat16().requires_grad_()
    w = (torch.randn(V, K, device=DEV, generator=g) * 4 / K ** 0.5).bfloat16().requires_grad_()
    b = torch.zeros(V, device=DEV, requires_grad=True)
    lab = torch.randint(V, (M,), device=DEV, generator=g)
    xent = CrossEntropyLoss(inplace_backward=True)
    paths = {"free": lambda: linear_cross_entropy(x, w, b, lab)}
    if with_logit_path:
        paths["logit"] = lambda: xent(fused_dense_func(x, w, b), lab)

    def fwd(f):
        with torch.no_grad():
            f()

    def fwdbwd(f):
        f().backward()
        x.grad = w.grad = b.grad = None

    fns = {}
    for n, f in paths.items():
        fns[f"{n}_fwd"] = lambda f=f: fwd(f)
        fns[f"{n}_fwdbwd"] = lambda f=f: fwdbwd(f)
    legs = {n: summary(v) for n, v in alternate(fns, reps).items()}
    for n, leg in legs.items():
        path, direction = n.split("_")
        products = 1 if direction == "fwd" else (4 if path == "free" else 3)
        leg["flops"] = 2.0 * M * V * K * products
        leg["tflops"] = leg["flops"] / leg["median_s"] / 1e12
        if with_logit_path:
            leg["over_logit_path"] = leg["median_s"] / legs[f"logit_{direction}"]["median_s"]
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[16384, 65536])
    ap.add_argument("--big-rows", type=int, nargs="+", default=[16384])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "linear_xent_microbench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    rec = {"what": "logit-free MLM head vs the logit path, public Python entry points, seconds per call", "K": K,
           "reps": args.reps, "shapes": {}}
    for M in args.rows:
        rec["shapes"][f"M{M}_V30528"] = legs_for(M, 30528, True, args.reps)
    for M in args.big_rows:
        rec["shapes"][f"M{M}_V250002"] = legs_for(M, 250002, False, args.reps)
    print(json.dumps(rec), flush=True)
    Path(args.out).write_text(json.dumps([rec], indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
