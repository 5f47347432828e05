"""Fused top-k search (cx_search_topk) against the plain v6 GEMM (cx_gemm_bf16_nt) at the same (M, N, d), same box,
same run.  The GEMM writes the bf16 scores in column slabs (the search never writes them); both count 2 M N d FLOP.
The merge kernel's share comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats).

usage: python scripts/search_microbench.py [--m 65536] [--n 4194304] [--d 768] [--k 2 16 100 1024] [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from contrastors_amd import _C  # noqa: E402
from contrastors_amd.search import FlatIPIndex  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4194304)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, nargs="+", default=[2, 16, 100, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slab", type=int, default=65536)
    args = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    Q = torch.nn.functional.normalize(torch.randn(args.m, args.d, device=dev, generator=g), dim=1).to(torch.bfloat16)
    D = torch.nn.functional.normalize(torch.randn(args.n, args.d, device=dev, generator=g), dim=1).to(torch.bfloat16)
    flop = 2.0 * args.m * args.n * args.d
    h = _C.lib()
    out = torch.empty(args.m, args.slab, dtype=torch.bfloat16, device=dev)

    def gemm():
        for c0 in range(0, args.n, args.slab):
            w = min(args.slab, args.n - c0)
            _C.check(h.cx_gemm_bf16_nt(Q.data_ptr(), D[c0].data_ptr(), out.data_ptr(), None, args.m, w, args.d, args.d,
                                       args.d, args.slab, 0, 1, 1.0, _C.cur_stream()), "gemm")

    t = timed(gemm, args.reps)
    rec = {"shape": [args.m, args.n, args.d], "gemm_s": t, "gemm_tflops": flop / t / 1e12}
    print(json.dumps(rec), flush=True)
    ix = FlatIPIndex(args.d, device=dev, workspace_bytes=4 << 30)
    ix.add(D)
    for k in args.k:
        t = timed(lambda: ix.search(Q, k), args.reps)
        rec = {"k": k, "search_s": t, "search_tflops": flop / t / 1e12, "batch_rows": ix.batch_rows(args.m, k)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
