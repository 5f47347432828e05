"""Head_dim 32 attention (cx_attn_varlen_d32_fwd / _bwd, H = --heads) next to the head_dim 64 path (cx_attn_varlen_fwd / _bwd, no
tables, H = --heads / 2) on the same byte count -- the same n_embd, the same FLOPs, twice the softmax work -- by
scripts/attn_window_microbench.py's method: same box, ONE process in which all legs ALTERNATE run by run, device events, one
warm-up round of all, medians of --reps runs with p10 - p90.  A run is --inner back-to-back calls; every time below is per call.

  shapes : S in --seqlens, B = --tokens / S equal-length sequences
  legs   : forward and forward + backward of both head widths
  flops  : 4 * d * S^2 per head and sequence for the forward, 3.5 x that for forward + backward (the same number for both widths)

usage: python scripts/attn_d32_microbench.py [--seqlens 128 512 2048] [--heads 12] [--tokens 16384] [--reps 21] [--inner 20]
                                             [--out profiles/attn_d32_microbench.json]
The JSON record on stdout and, in a list, in --out.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from ivf_int8_microbench import DEV, alternate, summary  # noqa: E402


def bench(args):
    import torch

    from contrastors_amd import _C

    lib, st, H = _C.lib(), _C.cur_stream(), args.heads
    rec = {"what": "head_dim 32 attention (H heads) vs head_dim 64 (H / 2 heads) on the same bytes, C-ABI calls", "heads_d32": H,
           "heads_d64": H // 2, "tokens": args.tokens, "reps": args.reps, "inner": args.inner, "shapes": {}}
    P = lambda t: t.data_ptr()  # noqa: E731
    for S in args.seqlens:
        B = max(1, args.tokens // S)
        T = B * S
        g = torch.Generator(device=DEV).manual_seed(S)
        qkv = torch.randn(T, 3, H, 32, device=DEV, generator=g).to(torch.bfloat16)   # read as (T, 3, H / 2, 64) by the d = 64 legs
        dout = torch.randn(T, H, 32, device=DEV, generator=g).to(torch.bfloat16)
        cu = torch.arange(0, T + 1, S, dtype=torch.int32, device=DEV)
        out, lse, delta = torch.empty_like(dout), torch.empty(H, T, device=DEV), torch.empty(H, T, device=DEV)
        dqkv = torch.empty_like(qkv)

        def d64(bwd):
            _C.check(lib.cx_attn_varlen_fwd(P(qkv), P(cu), None, None, P(out), P(lse), B, H // 2, T, S, 0.125, st), "fwd")
            if bwd:
                _C.check(lib.cx_attn_varlen_bwd(P(dout), P(qkv), P(out), P(lse), P(cu), None, None, P(delta), P(dqkv), B, H // 2, T, S,
                                                0.125, st), "bwd")

        def d32(bwd):
            _C.check(lib.cx_attn_varlen_d32_fwd(P(qkv), P(cu), P(out), P(lse), B, H, T, S, 1 / math.sqrt(32), st), "d32 fwd")
            if bwd:
                _C.check(lib.cx_attn_varlen_d32_bwd(P(dout), P(qkv), P(out), P(lse), P(cu), P(delta), P(dqkv), B, H, T, S,
                                                    1 / math.sqrt(32), st), "d32 bwd")

        fns = {"d64_fwd": lambda: d64(False), "d64_fwdbwd": lambda: d64(True), "d32_fwd": lambda: d32(False), "d32_fwdbwd": lambda: d32(True)}
        runs = alternate({n: (lambda f=f: [f() for _ in range(args.inner)]) for n, f in fns.items()}, args.reps)
        legs = {n: summary([t / args.inner for t in v]) for n, v in runs.items()}
        for n, leg in legs.items():
            direction = n.rsplit("_", 1)[1]
            leg["flops"] = 4.0 * 32 * S * S * B * H * (3.5 if direction == "fwdbwd" else 1.0)
            leg["tflops"] = leg["flops"] / leg["median_s"] / 1e12
            leg["over_d64"] = leg["median_s"] / legs[f"d64_{direction}"]["median_s"]
        rec["shapes"][str(S)] = {"B": B, "legs": legs}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqlens", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attn_d32_microbench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    if args.heads % 2:
        ap.error("--heads must be even (the d = 64 legs read head pairs as one head)")
    Path(args.out).write_text(json.dumps([bench(args)], indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
