"""Attention with ALiBi (cx_attn_varlen_alibi_fwd / _bwd, the standard slope set of --heads heads) next to the plain path
(cx_attn_varlen_fwd / _bwd, no tables) on the same buffers -- the same FLOPs -- by scripts/attn_window_microbench.py's method: same
box, ONE process in which all legs ALTERNATE run by run, device events, one warm-up round of all, medians of --reps runs with
p10 - p90.  A run is --inner back-to-back calls; every time below is per call.

  shapes : S in --seqlens, B = --tokens / S equal-length sequences
  legs   : forward and forward + backward of both paths
  flops  : 4 * 64 * S^2 per head and sequence for the forward, 3.5 x that for forward + backward (the bias is not counted)
  inside : per direction, whether the ALiBi median lies inside the plain path's p10 - p90

At S <= 256 the plain path runs single-pass kernels the ALiBi path does not have; from S = 512 on both stream.

usage: python scripts/attn_alibi_microbench.py [--seqlens 512 2048 8192] [--heads 12] [--tokens 16384] [--reps 21] [--inner 20]
                                               [--out profiles/attn_alibi_microbench.json]
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


def standard_slopes(n):
    """The ALiBi paper's slope set: 2^(-8 i / n), i = 1 .. n, for n a power of two; else the set of the power of two below n
    followed by every other slope of the set of twice that."""
    def pow2(m):
        return [2.0 ** (-8.0 * (i + 1) / m) for i in range(m)]
    below = 2 ** int(math.floor(math.log2(n)))
    return pow2(n) if below == n else pow2(below) + pow2(2 * below)[0::2][:n - below]


def bench(args):
    import torch

    from contrastors_amd import _C

    lib, st, H = _C.lib(), _C.cur_stream(), args.heads
    slopes = torch.tensor(standard_slopes(H), dtype=torch.float32, device=DEV)
    rec = {"what": "attention with ALiBi vs the plain path on the same buffers, C-ABI calls", "heads": H, "tokens": args.tokens,
           "slopes": slopes.tolist(), "reps": args.reps, "inner": args.inner, "shapes": {}}
    P = lambda t: t.data_ptr()  # noqa: E731
    for S in args.seqlens:
        B = max(1, args.tokens // S)
        T = B * S
        g = torch.Generator(device=DEV).manual_seed(S)
        qkv = torch.randn(T, 3, H, 64, device=DEV, generator=g).to(torch.bfloat16)
        dout = torch.randn(T, H, 64, device=DEV, generator=g).to(torch.bfloat16)
        cu = torch.arange(0, T + 1, S, dtype=torch.int32, device=DEV)
        out, lse, delta = torch.empty_like(dout), torch.empty(H, T, device=DEV), torch.empty(H, T, device=DEV)
        dqkv = torch.empty_like(qkv)

        def plain(bwd):
            _C.check(lib.cx_attn_varlen_fwd(P(qkv), P(cu), None, None, P(out), P(lse), B, H, T, S, 0.125, st), "fwd")
            if bwd:
                _C.check(lib.cx_attn_varlen_bwd(P(dout), P(qkv), P(out), P(lse), P(cu), None, None, P(delta), P(dqkv), B, H, T, S,
                                                0.125, st), "bwd")

        def alibi(bwd):
            _C.check(lib.cx_attn_varlen_alibi_fwd(P(qkv), P(cu), P(slopes), 0, P(out), P(lse), B, H, T, S, 0.125, st), "alibi fwd")
            if bwd:
                _C.check(lib.cx_attn_varlen_alibi_bwd(P(dout), P(qkv), P(out), P(lse), P(cu), P(slopes), 0, P(delta), P(dqkv), B, H, T,
                                                      S, 0.125, st), "alibi bwd")

        fns = {"plain_fwd": lambda: plain(False), "plain_fwdbwd": lambda: plain(True), "alibi_fwd": lambda: alibi(False),
               "alibi_fwdbwd": lambda: alibi(True)}
        runs = alternate({n: (lambda f=f: [f() for _ in range(args.inner)]) for n, f in fns.items()}, args.reps)
        legs = {n: summary([t / args.inner for t in v]) for n, v in runs.items()}
        for n, leg in legs.items():
            direction = n.rsplit("_", 1)[1]
            leg["flops"] = 4.0 * 64 * S * S * B * H * (3.5 if direction == "fwdbwd" else 1.0)
            leg["tflops"] = leg["flops"] / leg["median_s"] / 1e12
            leg["over_plain"] = leg["median_s"] / legs[f"plain_{direction}"]["median_s"]
        inside = {d: legs[f"plain_{d}"]["p10_s"] <= legs[f"alibi_{d}"]["median_s"] <= legs[f"plain_{d}"]["p90_s"] for d in ("fwd", "fwdbwd")}
        rec["shapes"][str(S)] = {"B": B, "legs": legs, "alibi_median_inside_plain_p10_p90": inside}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqlens", type=int, nargs="+", default=[512, 2048, 8192])
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attn_alibi_microbench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    Path(args.out).write_text(json.dumps([bench(args)], indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
