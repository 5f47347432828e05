"""Sliding-window attention (cx_attn_varlen_window_fwd / _bwd) next to the full-attention path (cx_attn_varlen_fwd / _bwd, no
tables) on the same inputs, by scripts/ivf_int8_microbench.py's method: same box, ONE process in which all legs ALTERNATE run by
run, device events, one warm-up round of all, medians of --reps runs with p10 - p90.  A run is --inner back-to-back calls (a single banded
call is tens of microseconds: too short for an event pair); every time below is per call.

  shapes : H = --heads, S in --seqlens, B = --tokens / S equal-length sequences
  legs   : forward and forward + backward of the full path and of every window in --windows
  flops  : 4 * 64 * (visible pairs) per head for the forward, 3.5 x that for forward + backward (2 of 7 products); the banded
           legs count band pairs only, `of_full_tflops` is their TFLOP/s over the full path's
  holds  : per S >= 2048 and direction, whether the (64, 64) median lies below the full path's p10

usage: python scripts/attn_window_microbench.py [--seqlens 512 2048 8192] [--windows 64 256] [--heads 12] [--tokens 16384]
                                                [--reps 21] [--inner 20] [--out profiles/attn_window_microbench.json]
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


def band_pairs(S, w):
    return sum(min(i + w, S - 1) - max(i - w, 0) + 1 for i in range(S))


def bench(args):
    import torch

    from contrastors_amd import _C

    lib, st, H = _C.lib(), _C.cur_stream(), args.heads
    rec = {"what": "sliding-window attention vs the full-attention path, C-ABI calls", "heads": H, "tokens": args.tokens,
           "reps": args.reps, "inner": args.inner, "shapes": {}}
    for S in args.seqlens:
        B = max(1, args.tokens // S)
        T = B * S
        g = torch.Generator(device=DEV).manual_seed(S)
        qkv = torch.randn(T, 3, H, 64, device=DEV, generator=g).to(torch.bfloat16)
        dout = torch.randn(T, H, 64, device=DEV, generator=g).to(torch.bfloat16)
        cu = torch.arange(0, T + 1, S, dtype=torch.int32, device=DEV)
        out, lse, delta = torch.empty_like(dout), torch.empty(H, T, device=DEV), torch.empty(H, T, device=DEV)
        dqkv = torch.empty_like(qkv)
        P = lambda t: t.data_ptr()  # noqa: E731

        def full(bwd):
            _C.check(lib.cx_attn_varlen_fwd(P(qkv), P(cu), None, None, P(out), P(lse), B, H, T, S, 0.125, st), "fwd")
            if bwd:
                _C.check(lib.cx_attn_varlen_bwd(P(dout), P(qkv), P(out), P(lse), P(cu), None, None, P(delta), P(dqkv), B, H, T, S,
                                                0.125, st), "bwd")

        def banded(w, bwd):
            _C.check(lib.cx_attn_varlen_window_fwd(P(qkv), P(cu), P(out), P(lse), B, H, T, S, w, w, 0.125, st), "window fwd")
            if bwd:
                _C.check(lib.cx_attn_varlen_window_bwd(P(dout), P(qkv), P(out), P(lse), P(cu), P(delta), P(dqkv), B, H, T, S, w, w,
                                                       0.125, st), "window bwd")

        fns = {"full_fwd": lambda: full(False), "full_fwdbwd": lambda: full(True)}
        pairs = {"full": S * S}
        for w in args.windows:
            fns[f"w{w}_fwd"] = (lambda w=w: banded(w, False))
            fns[f"w{w}_fwdbwd"] = (lambda w=w: banded(w, True))
            pairs[f"w{w}"] = band_pairs(S, w)
        runs = alternate({n: (lambda f=f: [f() for _ in range(args.inner)]) for n, f in fns.items()}, args.reps)
        legs = {n: summary([t / args.inner for t in v]) for n, v in runs.items()}
        for n, leg in legs.items():
            kind, direction = n.rsplit("_", 1)
            leg["flops"] = 4.0 * 64 * pairs[kind] * B * H * (3.5 if direction == "fwdbwd" else 1.0)
            leg["tflops"] = leg["flops"] / leg["median_s"] / 1e12
        for n, leg in legs.items():
            direction = n.rsplit("_", 1)[1]
            leg["over_full"] = leg["median_s"] / legs[f"full_{direction}"]["median_s"]
            leg["of_full_tflops"] = leg["tflops"] / legs[f"full_{direction}"]["tflops"]
        shape = {"B": B, "legs": legs}
        if S >= 2048 and 64 in args.windows:
            shape["w64_median_below_full_p10"] = {d: legs[f"w64_{d}"]["median_s"] < legs[f"full_{d}"]["p10_s"] for d in ("fwd", "fwdbwd")}
        rec["shapes"][str(S)] = shape
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqlens", type=int, nargs="+", default=[512, 2048, 8192])
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attn_window_microbench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the record is a median)")
    Path(args.out).write_text(json.dumps([bench(args)], indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
