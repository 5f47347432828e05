"""EVA-02 B/16 (cx_vit_*_ex) vs google/vit B/16 (cx_vit_*) at 224 x 224, same process, same box: images/s of forward +
backward at the nomic-embed-vision-v1.5 recipe's chunk (1536 images), with and without activation checkpointing, and the
fraction of the 2.5 PF bf16 peak.  Per-kernel times of the new kernels come from a separate run of this script under
`rocprofv3 --kernel-trace --stats` (--reps 1).  usage: python scripts/eva02_microbench.py [--batch 1536] [--reps 3]"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from contrastors_amd.vit import ViTConfig, ViTEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1536)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
PEAK = 2.5e15
S, d, L = 197, 768, 12


def gemm_flop_per_image(inner, gated):
    wfc1 = 2 * inner if gated else inner
    per_tok = L * 2 * (d * 3 * d + d * d + d * wfc1 + inner * d) + L * 4 * S * d   # projections + attention (QK^T, PV)
    return S * per_tok + 196 * 2 * 768 * 768


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps


pix = torch.randn(a.batch, 3, 224, 224, device="cuda").to(torch.bfloat16)
print(f"B/16 224x224, batch {a.batch} ({a.batch * S} tokens), {a.reps} timed reps")
for name, cfg in (("ViT-B/16", ViTConfig.vit_base_patch16_224()), ("EVA-02 B/16", ViTConfig.eva02_base_patch16_224())):
    eng = ViTEngine(cfg, device="cuda", seed=0).train()
    probe = torch.randn(a.batch, cfg.n_embd, device="cuda")
    fwd = gemm_flop_per_image(cfg.n_inner, cfg.gated)
    for ckpt in (False, True):
        eng.gradient_checkpointing_enable(ckpt, keep_layers=0)

        def step():
            _, arena = eng.forward_chunk(pix, True)
            eng.backward_chunk(a.batch, arena, probe)

        t = timed(step)
        flop = a.batch * fwd * (4 if ckpt else 3)
        print(f"{name:12s} checkpoint={int(ckpt)}  {t:9.2f} ms  {a.batch / t * 1e3:8.0f} img/s  "
              f"{flop / a.batch / 1e9:6.1f} GFLOP/img  {flop / t / 1e9:7.1f} TFLOP/s  {flop / t * 1e3 / PEAK * 100:5.1f} % of peak")
    del eng
    torch.cuda.empty_cache()
