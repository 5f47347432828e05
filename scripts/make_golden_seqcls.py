"""Generate tests/golden/seqcls_tiny.npz: the reference's own NomicBertForSequenceClassification run on the CPU in fp32.

Run where the reference checkout is present:  python scripts/make_golden_seqcls.py

The class is the reference's eager twin (models/huggingface/modeling_hf_nomic_bert.py, the one oracle/make_golden.py runs for
the encoder and MLM fixtures): the flash-attn class of models/encoder composes GPU-only kernels and cannot run on a CPU.  Tiny
BERT-style trunk (2 layers, d = 256, 4 heads, learned positions), B = 4, S = 16, ragged lengths, segment ids that switch
inside every sequence; one case each for 2 labels, 3 labels and 1 label (regression).  The trunk weights are
oracle.encoder_ref.random_state_dict(cfg, seed) (4 MB in fp32, so they are pinned by seed + checksum like the other
fixtures', not stored); the head weights, the key list of the reference's state dict, inputs, logits and loss are stored.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import encoder_ref, ref_import  # noqa: E402
from oracle.make_golden import TINY_BERT, cfg_ns, checksum, make_inputs, ref_model  # noqa: E402

SEED, B, S = 31, 4, 16
CASES = {"c2": (2, "single_label_classification"), "c3": (3, "single_label_classification"), "c1": (1, "regression")}


def head_state_dict(d: int, C: int, seed: int):
    """Weights at the scale the reference initialises them with (_init_weights: N(0, initializer_range = 0.02)) -- the state a
    GLUE run starts from -- and biases of the same scale instead of its zeros, so that they are seen by the outputs."""
    g = torch.Generator().manual_seed(seed)
    return {"bert.pooler.dense.weight": torch.randn(d, d, generator=g) * 0.02, "bert.pooler.dense.bias": torch.randn(d, generator=g) * 0.02,
            "classifier.weight": torch.randn(C, d, generator=g) * 0.02, "classifier.bias": torch.randn(C, generator=g) * 0.02}


def inputs(seed: int):
    ids, mask, lens = make_inputs(TINY_BERT, B, S, seed)
    g = torch.Generator().manual_seed(seed + 5)
    cut = torch.stack([torch.randint(1, int(n), (1,), generator=g)[0] for n in lens])
    tts = ((torch.arange(S)[None, :] >= cut[:, None]) & mask.bool()).long()      # 0 ... 0 1 ... 1 inside every sequence
    return ids, mask, tts


def main():
    _, _, rmod = ref_import.load()
    cfg = cfg_ns(TINY_BERT)
    trunk = encoder_ref.random_state_dict(cfg, SEED)
    ids, mask, tts = inputs(SEED + 1)
    out = {"seed": np.array(SEED), "input_ids": ids.numpy(), "attention_mask": mask.numpy(), "token_type_ids": tts.numpy(),
           "trunk_checksum": checksum(trunk), **{"cfg/" + k: np.array(v) for k, v in TINY_BERT.items()}}
    for name, (C, problem) in CASES.items():
        c = ref_model(TINY_BERT, trunk).config
        c.num_labels, c.problem_type = C, problem
        m = rmod.NomicBertForSequenceClassification(c)
        head = head_state_dict(cfg.n_embd, C, SEED + 10 + C)
        missing, unexpected = m.load_state_dict({**{f"bert.{k}": v for k, v in trunk.items()}, **head}, strict=False)
        assert not unexpected and all("inv_freq" in k or "norm_factor" in k for k in missing), (missing, unexpected)
        m.eval()
        g = torch.Generator().manual_seed(SEED + 20 + C)
        labels = torch.randn(B, generator=g) if C == 1 else torch.randint(0, C, (B,), generator=g)
        with torch.no_grad():
            res = m(ids, attention_mask=mask, token_type_ids=tts, labels=labels)
            swapped = m(ids, attention_mask=mask, token_type_ids=(1 - tts) * mask)
        out.update({f"{name}/labels": labels.numpy(), f"{name}/logits": res.logits.numpy(), f"{name}/loss": np.array(float(res.loss)),
                    f"{name}/logits_swapped_types": swapped.logits.numpy(),
                    f"{name}/state_dict_keys": np.array(sorted(k for k in m.state_dict() if "inv_freq" not in k and "norm_factor" not in k)),
                    **{f"{name}/head/{k}": v.numpy() for k, v in head.items()}})
        print(name, "loss", float(res.loss), "logits", res.logits.flatten().tolist()[:4])
    np.savez_compressed(ROOT / "tests" / "golden" / "seqcls_tiny.npz", **out)


if __name__ == "__main__":
    main()
