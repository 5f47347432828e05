"""Record tests/golden/zeroshot_accuracy.npz: inputs and outputs of the reference's top-k accuracy on tie-free logits.

    python scripts/make_zeroshot_golden.py /path/to/reference/checkout

The reference's `eval/metrics.py` is imported BY PATH at generation time (it needs numpy and torch only); the file written
holds data only -- logits (B, C) float32, target (B) int64, topk (K) int64, correct (K) float64 = accuracy(logits, target,
topk).  tests/test_zeroshot_cpu.py checks `contrastors_amd.zeroshot.topk_hits` against it from the ranks of the targets; no
test reads the reference tree."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent


def main(reference_root: str) -> None:
    src = Path(reference_root) / "src" / "contrastors" / "eval" / "metrics.py"
    spec = importlib.util.spec_from_file_location("reference_metrics", src)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(20240)
    B, C = 257, 101
    logits = torch.randn(B, C, generator=g)
    srt = torch.sort(logits, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "tie in the recorded logits"
    # targets: a mix of each row's rank-0 .. rank-14 class, so that every k below sees hits and misses
    order = torch.argsort(logits, dim=1, descending=True)
    pick = torch.randint(0, 15, (B,), generator=g)
    target = order[torch.arange(B), pick]
    topk = (1, 2, 5, 10)
    correct = mod.accuracy(logits, target, topk=topk)
    out = ROOT / "tests" / "golden" / "zeroshot_accuracy.npz"
    np.savez(out, logits=logits.numpy(), target=target.numpy(), topk=np.asarray(topk, np.int64),
             correct=np.asarray(correct, np.float64))
    print(f"wrote {out}: correct = {correct} of {B}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
