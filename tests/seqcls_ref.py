"""References of the sequence-classification feature (contrastors_amd/csrc/seqcls.hip, the typed embedding kernels of
layernorm.hip, contrastors_amd/seqcls.py).  Plain torch / numpy, any device; tests/test_seqcls_cpu.py pins the restatement to
tests/golden/seqcls_tiny.npz (the reference's own class on the CPU), tests/test_seqcls_gpu.py holds the kernels to it.

  head_ref            pooler dense + tanh -> mask -> Linear -> cross-entropy / MSE and every gradient, in the dtype asked for
                      (fp64: the reference; fp32: the "fp32 eager" whose error sets the kernels' tolerance)
  head_keep           the head's dropout mask on the host: Philox4x32-10 keyed as cx_common.h dropout_keep4 keys it
  typed_embed_z       z = (word[id] + pos[p]) + type[tt] in fp32, the kernels' order; the LayerNorm on top of it is
                      tests/ln_ref.py's row math (ln_fwd_ref / ln_bwd_ref), imported, not restated
  seqcls_twin         the whole model in torch: oracle.encoder_ref's trunk (which only knows type row 0) on an equivalent
                      problem -- the vocabulary doubled, id + V carrying word[id] + (type[1] - type[0]) -- then head_ref's math
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import encoder_ref
from tests import ln_ref as R

HEAD_DROP_SITE = 1 << 20
IGNORE_INDEX = -100


# ------------------------------------------------------------------------------------------------------------ the head
def head_forward(X, Wp, bp, Wc, bc, keep=None):
    """-> (pooled, logits).  keep: (B, d) factors 0 or 1 / (1 - p), or None."""
    pooled = torch.tanh(F.linear(X, Wp, bp))
    h = pooled if keep is None else pooled * keep
    return pooled, F.linear(h, Wc, bc)


def loss_rows(logits, labels, mode):
    """mode 0: cross-entropy per row, 0 on rows labelled IGNORE_INDEX; mode 1: mean over the outputs of the squared error."""
    if mode == 0:
        valid = labels != IGNORE_INDEX
        rows = F.cross_entropy(logits, labels.clamp(min=0), reduction="none")
        return torch.where(valid, rows, torch.zeros_like(rows))
    return ((logits - labels.reshape(logits.shape).to(logits.dtype)) ** 2).mean(-1)


def head_ref(X, Wp, bp, Wc, bc, labels, mode, coef, keep=None, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """pooled, logits, loss_rows and the gradients of coef * sum(loss_rows) with respect to Wp, bp, Wc, bc, X -- autograd over
    the restatement in `dtype`."""
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in (X, Wp, bp, Wc, bc)]
    pooled, logits = head_forward(*leaves, None if keep is None else keep.to(dtype))
    rows = loss_rows(logits, labels, mode)
    (coef * rows.sum()).backward()
    g = [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves]
    return dict(pooled=pooled.detach(), logits=logits.detach(), loss_rows=rows.detach(), dX=g[0], dWp=g[1], dbp=g[2], dWc=g[3],
                dbc=g[4])


def _philox4x32_10(c, k):
    """c: 4 uint64 arrays holding 32-bit words, k: 2 ints.  Salmon et al.; the rounds of cx_common.h philox4x32_10."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [x.astype(np.uint64) for x in c]
    kx, ky = np.uint64(k[0]), np.uint64(k[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ kx, lo1, hi0 ^ c[3] ^ ky, lo0]
        kx, ky = (kx + np.uint64(0x9E3779B9)) & m32, (ky + np.uint64(0xBB67AE85)) & m32
    return c


def head_keep(seed: int, offset: int, B: int, d: int, p: float) -> torch.Tensor:
    """(B, d) fp32 keep factors of the head's dropout: element (b, j) is word j % 4 of Philox(counter = (group, offset + site),
    key = seed) with group = (b * d + j) / 4, kept when the word is >= p * 2^32, scaled 1 / (1 - p) (fp32 arithmetic)."""
    if p <= 0:
        return torch.ones(B, d)
    g = np.arange(B * d // 4, dtype=np.uint64)
    off = offset + HEAD_DROP_SITE
    zeros = np.zeros_like(g)
    words = _philox4x32_10([g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), zeros + np.uint64(off & 0xFFFFFFFF),
                            zeros + np.uint64((off >> 32) & 0xFFFFFFFF)], (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    r = np.stack(words, axis=1).reshape(B, d)
    thr = np.uint64(min(np.float32(p) * np.float32(4294967296.0), np.float32(4294967040.0)))
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(np.where(r >= thr, inv, np.float32(0.0)).astype(np.float32))


# ------------------------------------------------------------------------------------------------- the typed embedding
def typed_embed_z(word, type_e, pos_e, ids, tts, indices, seq):
    """ln_ref.embed_z with the token's own type row.  Returns z (fp32: sums of two and three fp32 values are correctly rounded
    on any device, so this IS the kernels' z), the token ids, the positions, the token types (0 / 1)."""
    tok = indices.long()
    tid, p, tt = ids.reshape(-1)[tok], tok % seq, (tts.reshape(-1)[tok] != 0).long()
    z = word[tid]
    if pos_e is not None:
        z = z + pos_e[p]
    return z + type_e[tt], tid, p, tt


def typed_embed_inputs(T, d, vocab, lens=(1, 5, 128), seq=128, seed=900, types="switch", pad_id=3, n_pad=3):
    """Operands of the typed embedding kernels on the CPU, in the layout of ln_ref.embed_inputs: sequences of the given
    lengths, repeated until T tokens are there (the last one cut), `n_pad` tokens carrying the padding id, and segment ids
    "zeros" / "ones" / "switch" (0 up to a seeded place inside every sequence, 1 from there on)."""
    ls, n = [], 0
    while n < T:
        ls.append(lens[len(ls) % len(lens)])
        n += ls[-1]
    indices = torch.cat([torch.arange(ln) + b * seq for b, ln in enumerate(ls)])[:T].to(torch.int32)
    g = torch.Generator().manual_seed(seed + d)
    ids = torch.randint(0, vocab, (len(ls), seq), generator=g)
    place = torch.randperm(T, generator=g)[:n_pad]
    ids.view(-1)[indices.long()[place]] = pad_id
    if types == "switch":
        cut = torch.tensor([int(torch.randint(0, ln + 1, (1,), generator=g)) if ln > 1 else b % 2 for b, ln in enumerate(ls)])
        tts = (torch.arange(seq)[None, :] >= cut[:, None]).long()
    else:
        tts = torch.full((len(ls), seq), 1 if types == "ones" else 0, dtype=torch.long)
    gamma, beta = R.params(d)
    return dict(ids=ids, tts=tts, indices=indices, seq=seq, vocab=vocab, T=T, gamma=gamma, beta=beta, pad_id=pad_id,
                word=R.rows_like(vocab, d, seed + d + 1, dtype=torch.float32),
                pos=0.5 * R.rows_like(seq, d, seed + d + 2, centred=True, dtype=torch.float32),
                type=0.1 * torch.randn(2, d, generator=g),
                da=R.rows_like(T, d, seed + d + 3, centred=True, shift=2), db=R.rows_like(T, d, seed + d + 4, centred=True, shift=3))


# ------------------------------------------------------------------------------------------------------ the whole model
def typed_trunk_state(trunk: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The trunk state dict of the equivalent untyped problem: rows V .. 2V - 1 of the word table are word + (type[1] - type[0]),
    so that encoder_ref (which adds type[0] to every token) sees word[id] + type[1] for the ids shifted by V.  Built with
    differentiable ops: gradients reach the original word table and both type rows."""
    sd = dict(trunk)
    word, ty = trunk["embeddings.word_embeddings.weight"], trunk["embeddings.token_type_embeddings.weight"]
    sd["embeddings.word_embeddings.weight"] = torch.cat([word, word + (ty[1] - ty[0])], 0)
    return sd


def seqcls_twin(sd: Dict[str, torch.Tensor], cfg, input_ids, attention_mask, token_type_ids, labels=None, mode=0,
                keep: Optional[torch.Tensor] = None):
    """NomicBertForSequenceClassification.forward (sc/models/encoder/modeling_nomic_bert.py:692-757) in the dtype of `sd`, whose
    keys are the reference's (`bert.*`, `bert.pooler.dense.*`, `classifier.*`).  -> (loss or None, logits)."""
    trunk = typed_trunk_state({k[5:]: v for k, v in sd.items() if k.startswith("bert.") and not k.startswith("bert.pooler.")})
    V = trunk["embeddings.word_embeddings.weight"].shape[0] // 2
    ids = input_ids if token_type_ids is None else input_ids + V * (token_type_ids != 0).long()
    hidden = encoder_ref.encoder_hidden_states(trunk, cfg, ids, attention_mask)
    _, logits = head_forward(hidden[:, 0], sd["bert.pooler.dense.weight"], sd["bert.pooler.dense.bias"], sd["classifier.weight"],
                             sd["classifier.bias"], keep)
    if labels is None:
        return None, logits
    rows = loss_rows(logits, labels, mode)
    count = int((labels != IGNORE_INDEX).sum()) if mode == 0 else logits.shape[0]
    return rows.sum() / max(count, 1), logits


# ------------------------------------------------------------------------------ the synthetic sentence-pair task + twin
PAIR_VOCAB, PAIR_CLS, PAIR_SEP = 512, 101, 102
PAIR_SETS = ((200, 300), (300, 400))     # the token ranges of class 0 and class 1


def pair_task(n: int, seed: int, regression: bool = False):
    """Encoded rows of a sentence-pair task that only segment ids solve: [CLS] a ... [SEP] b ... [SEP], every token of sentence
    A drawn from the range of a random class, every token of sentence B from the range of the LABEL's class, both 2 to 6 tokens
    long.  Half the rows have A and B from different ranges, and which of the two ranges belongs to B is told by nothing but
    the segment ids (and, weakly, by position): a model blind to both sees a bag of two ranges and cannot beat chance on
    those rows.  regression: the label is the float 0.0 / 1.0 (an STS-B-shaped task)."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(n):
        y, ca = int(torch.randint(0, 2, (1,), generator=g)), int(torch.randint(0, 2, (1,), generator=g))
        na, nb = int(torch.randint(2, 7, (1,), generator=g)), int(torch.randint(2, 7, (1,), generator=g))
        a = torch.randint(*PAIR_SETS[ca], (na,), generator=g).tolist()
        b = torch.randint(*PAIR_SETS[y], (nb,), generator=g).tolist()
        rows.append({"input_ids": [PAIR_CLS] + a + [PAIR_SEP] + b + [PAIR_SEP], "token_type_ids": [0] * (na + 2) + [1] * (nb + 1),
                     "labels": float(y) if regression else y})
    return rows


def pair_initial_state(cfg_dict, seed: int, num_labels: int = 2) -> Dict[str, torch.Tensor]:
    """Initial weights of the trainer test and of its twin: oracle.encoder_ref.random_state_dict + an N(0, 0.02) head."""
    from types import SimpleNamespace

    sd = {f"bert.{k}": v for k, v in encoder_ref.random_state_dict(SimpleNamespace(**cfg_dict), seed).items()}
    g = torch.Generator().manual_seed(seed + 1)
    d = cfg_dict["n_embd"]
    sd.update({"bert.pooler.dense.weight": torch.randn(d, d, generator=g) * 0.02, "bert.pooler.dense.bias": torch.zeros(d),
               "classifier.weight": torch.randn(num_labels, d, generator=g) * 0.02, "classifier.bias": torch.zeros(num_labels)})
    return sd


def twin_train(cfg_dict, sd, batches_per_epoch, epochs, val_batches, lr, warmup_pct, betas=(0.9, 0.98), eps=1e-6,
               weight_decay=1e-6, mode=0):
    """The fp32 torch twin of GlueTrainer on the CPU: seqcls_twin + torch.optim.AdamW (matrices decay, the rest does not) + the
    linear schedule.  batches_per_epoch(epoch) -> the collated batches.  -> (per-step losses, per-epoch predictions/references)."""
    from types import SimpleNamespace

    from contrastors_amd.trainers import _lr_lambda

    cfg = SimpleNamespace(**cfg_dict)
    params = {k: v.clone().float().requires_grad_() for k, v in sd.items()}
    decay = [p for k, p in params.items() if p.ndim >= 2]
    nodecay = [p for k, p in params.items() if p.ndim < 2]
    opt = torch.optim.AdamW([{"params": decay, "weight_decay": weight_decay}, {"params": nodecay, "weight_decay": 0.0}], lr=lr,
                            betas=betas, eps=eps)
    steps = len(batches_per_epoch(0)) * epochs
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _lr_lambda("linear", int(steps * warmup_pct), steps))
    losses, evals = [], []
    for epoch in range(epochs):
        for b in batches_per_epoch(epoch):
            loss, _ = seqcls_twin(params, cfg, b["input_ids"], b["attention_mask"], b["token_type_ids"], b["labels"], mode)
            opt.zero_grad()
            loss.backward()
            opt.step()
            sched.step()
            losses.append(float(loss.detach()))
        with torch.no_grad():
            preds, refs = [], []
            for b in val_batches:
                _, logits = seqcls_twin(params, cfg, b["input_ids"], b["attention_mask"], b["token_type_ids"])
                preds.append(logits.squeeze(-1) if mode else logits.argmax(-1))
                refs.append(b["labels"])
            evals.append((torch.cat(preds).numpy(), torch.cat(refs).numpy()))
    return losses, evals


PAIR_RUN = dict(n_train=256, n_val=128, batch=16, epochs=4, lr=1e-3, warmup_pct=0.06, seed=11)


def pair_twin_curves(regression: bool = False):
    """The twin's run of the trainer test's recipe (what its docstring records): python -m tests.seqcls_ref"""
    from contrastors_amd.glue import ShardedBatches
    from oracle.make_golden import TINY_BERT

    r = PAIR_RUN
    train, val = pair_task(r["n_train"], r["seed"], regression), pair_task(r["n_val"], r["seed"] + 1, regression)
    tb = ShardedBatches(train, r["batch"], shuffle=True, seed=r["seed"])

    def per_epoch(epoch):
        tb.set_epoch(epoch)
        return list(tb)

    sd = pair_initial_state(TINY_BERT, r["seed"], 1 if regression else 2)
    return twin_train(TINY_BERT, sd, per_epoch, r["epochs"], list(ShardedBatches(val, r["batch"])), r["lr"], r["warmup_pct"],
                      mode=1 if regression else 0)


if __name__ == "__main__":
    losses, evals = pair_twin_curves()
    print("steps", len(losses), "first ten", np.mean(losses[:10]), "last ten", np.mean(losses[-10:]))
    print("loss every 8th step", [round(x, 3) for x in losses[::8]])
    print("accuracy per epoch", [float((p == t).mean()) for p, t in evals], "majority", max(evals[0][1].mean(), 1 - evals[0][1].mean()))


# --------------------------------------------------------------------------------- bounds of the typed embedding tests
# The criterion is tests/ln_ref.py's for the untyped embedding kernels: |got - ref| <= (half a bf16 ulp +) C 2^-24 S per
# element, C = 4 x the worst ratio of an fp32 emulation of the kernel's arithmetic against the fp64 reference ON THE INPUTS OF
# THE TEST.  The typed tests have other inputs than the untyped ones (1- and 5-token sequences, two type rows, up to 8193 rows
# instead of 8197 at one width only), so their constants are measured on those inputs -- by the same emulation
# (tests/test_ln_ref_cpu.py emu_fwd / emu_bwd), never by a kernel; tests/test_seqcls_cpu.py asserts them.
TYPED_FWD_SHAPES = ((256, 1025), (768, 8191), (768, 8192), (768, 8193), (1024, 1025))
TYPED_BWD_SHAPES = (("atomic", 768, 1023), ("atomic", 768, 1024), ("atomic", 768, 1025), ("atomic", 256, 1025), ("atomic", 1024, 1025),
                    ("sorted", 768, 4095), ("sorted", 768, 4096), ("sorted", 768, 4097), ("sorted", 256, 4097), ("sorted", 1024, 4097))
TYPED_TYPES = ("zeros", "ones", "switch")
TYPED_FWD_VOCAB, TYPED_BWD_VOCAB = 512, 300
TYPED_SMALL_WS_BLOCKS = 7                       # the grid of the small-workspace case (d = 768, "switch", both forms)
TYPED_C_MEAS = {
    "embed_fwd": {"out": 1.5e5, "out_tight": 3.9, "mean": 3.4, "rstd": 2.8},
    # dgamma / dbeta / dtype: the typed backward reduces them in a fixed order (kernel_order_colsum), which the emulation follows;
    # "scatter" = dpos / dword, sums of fp32 dz rows as in tests/ln_ref.py
    "embed_bwd": {"dz": 580.0, "dgamma": 1.4, "dbeta": 0.52, "dtype": 1.9, "scatter": 38.0},
}


def typed_bwd_grid(form: str, T: int) -> int:
    """The blocks cx_embed_ln_bwd_typed / _sorted_typed launch when the workspace does not cap them."""
    return min(256 if form == "atomic" else 1024, (T + 3) // 4)


def kernel_order_colsum(terms: torch.Tensor, grid: int) -> torch.Tensor:
    """fp32 column sums of `terms` (T, n) in the order the typed backward adds them: token t is the (t // (4 grid))-th token of wave
    t % 4 of block (t // 4) % grid; a block folds its four waves as ((w0 + w1) + w2) + w3; ln_param_reduce_kernel sums the partials
    of blocks g, g + 4, g + 8, ... in that order for g = 0 .. 3 and adds the four as ((s0 + s1) + s2) + s3.  fp32 adds are
    correctly rounded on any device, and adding the zero rows that pad the ragged tail changes nothing."""
    T, n = terms.shape
    terms = terms.float()
    K = -(-T // (4 * grid))
    x = torch.cat([terms, terms.new_zeros(K * 4 * grid - T, n)]).view(K, grid, 4, n)
    acc = x[0].clone()
    for k in range(1, K):
        acc = acc + x[k]
    blk = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    G = -(-grid // 4)
    v = torch.cat([blk, blk.new_zeros(G * 4 - grid, n)]).view(G, 4, n)
    s4 = v[0].clone()
    for i in range(1, G):
        s4 = s4 + v[i]
    return ((s4[0] + s4[1]) + s4[2]) + s4[3]


def TC(family: str, what: str) -> float:
    return R.C_FACTOR * TYPED_C_MEAS[family][what]


def check_typed_out(name, got, fwd, family="embed_fwd"):
    """ln_ref.check_out with the typed tests' constants: the bound on S and -- never wider -- the bound on scale_tight."""
    half = 0.5 * R.bf16_ulp(fwd.out) if got.dtype == torch.bfloat16 else 0.0
    b = torch.minimum(TC(family, "out") * fwd.scale, TC(family, "out_tight") * fwd.scale_tight)
    return R.check_rows(name, got, fwd.out, half + R.EPS24 * b, free=half)


def measure_typed_constants():
    """The worst emulation ratios over the inputs of tests/test_seqcls_gpu.py's typed embedding tests (as test_ln_ref_cpu.measure
    has them for the untyped families)."""
    from tests.test_ln_ref_cpu import _ratio, emu_bwd, emu_fwd, ratio_cols, ratio_result, ratio_stats

    m = {k: dict.fromkeys(v, 0.0) for k, v in TYPED_C_MEAS.items()}

    def up(fam, **kw):
        for k, v in kw.items():
            m[fam][k] = max(m[fam][k], float(v))

    for d, T in TYPED_FWD_SHAPES:
        for types in TYPED_TYPES:
            e = typed_embed_inputs(T, d, TYPED_FWD_VOCAB, types=types)
            z, _, _, _ = typed_embed_z(e["word"], e["type"], e["pos"], e["ids"], e["tts"], e["indices"], e["seq"])
            f = R.ln_fwd_ref(z, None, e["gamma"], e["beta"], 1e-12)
            _, mean, rstd, out = emu_fwd(z, None, e["gamma"], e["beta"], 1e-12)
            cm, cr = ratio_stats(mean, rstd, f)
            up("embed_fwd", out=ratio_result(out, f.out, f.scale), out_tight=ratio_result(out, f.out, f.scale_tight), mean=cm, rstd=cr)
    cases = [(form, d, T, types, typed_bwd_grid(form, T)) for form, d, T in TYPED_BWD_SHAPES for types in TYPED_TYPES]
    cases += [("atomic", 768, 1025, "switch", TYPED_SMALL_WS_BLOCKS), ("sorted", 768, 4097, "switch", TYPED_SMALL_WS_BLOCKS)]
    for form, d, T, types, grid in cases:
        e = typed_embed_inputs(T, d, TYPED_BWD_VOCAB, types=types)
        z, tid, p, tt = typed_embed_z(e["word"], e["type"], e["pos"], e["ids"], e["tts"], e["indices"], e["seq"])
        st = R.ln_fwd_ref(z, None, e["gamma"], None, 1e-12)
        mean, rstd = st.mean.float(), st.rstd.float()
        real = tid != e["pad_id"]
        xh = (z - mean[:, None]) * rstd[:, None]
        for two in (True, False):
            ref = R.ln_bwd_ref(e["da"], e["db"] if two else None, z, e["gamma"], mean, rstd, None)
            dy = e["da"].float() + e["db"].float() if two else e["da"].float()
            o, _, _ = emu_bwd(dy, z, e["gamma"], mean, rstd, None)
            sc = max(float(_ratio((R.scatter_rows(o[sel], idx[sel], n).double() - R.scatter_rows(ref.dz[sel], idx[sel], n)).abs(),
                                  R.scatter_rows(ref.scale[sel], idx[sel], n)).max())
                     for idx, n, sel in ((p, e["seq"], torch.ones_like(real)), (tid, e["vocab"], real)))
            dty = torch.stack([kernel_order_colsum(o * (tt == row)[:, None], grid) for row in (0, 1)])
            up("embed_bwd", dz=ratio_result(o, ref.dz, ref.scale, torch.float32), scatter=sc,
               dgamma=ratio_cols(kernel_order_colsum(dy * xh, grid), ref.dgamma, ref.dgamma_abs),
               dbeta=ratio_cols(kernel_order_colsum(dy, grid), ref.dbeta, ref.dbeta_abs),
               dtype=float(_ratio((dty.double() - R.scatter_rows(ref.dz, tt, 2)).abs(), R.scatter_rows(ref.scale, tt, 2)).max()))
    return m
