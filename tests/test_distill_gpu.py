"""Distillation on the device: the fused similarity-KL kernel through the C ABI, the loss layer, and DistillTrainer.

Tolerance rule (no invented number): the kernel's rel_err against the float64 restatement of tests/distill_ref.py is compared
with the error the SAME restatement carries when it runs in fp32 eager torch on the same inputs --
    rows / loss values:  err <= max(3 * err_fp32_eager, 1e-5)          gradients:  err <= max(3 * err_fp32_eager, 1e-4)
(the factor 3 is the project's parity rule, the floors its fp32 InfoNCE tolerances: tests/test_loss_gpu.py).  A relative rule
is needed because kl_i is a difference of nearly equal terms when the student is close to its teacher: at mean kl 0.003 the
fp32 eager form itself is ~1e-4 off."""
import dataclasses
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from contrastors_amd import _C
from contrastors_amd.loss import distill_loss, similarity_kl_loss
from tests.distill_ref import distill_loss_ref, kl_rows_ref, noisy_student, unit_rows
from tests.gpu_util import L, S, rel_err, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROW_FLOOR, GRAD_FLOOR = 1e-5, 1e-4


def simkl_fwd(sq, sd, tq, td, tau):
    N, G = sq.shape[0], sd.shape[0]
    f32 = dict(dtype=torch.float32, device=sq.device)
    ws = torch.empty(L().cx_simkl_ws_floats(N, G), **f32)
    lse_s, lse_t, rows = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, **f32)
    _C.check(L().cx_simkl_fwd(sq.data_ptr(), sd.data_ptr(), tq.data_ptr(), td.data_ptr(), 1.0 / tau, ws.data_ptr(),
                              lse_s.data_ptr(), lse_t.data_ptr(), rows.data_ptr(), N, G, sq.shape[1], tq.shape[1],
                              sq.stride(0), sd.stride(0), tq.stride(0), td.stride(0), S()), "cx_simkl_fwd")
    return rows, lse_s, lse_t


def simkl_bwd(sq, sd, tq, td, lse_s, lse_t, tau, coef):
    N, G, ds = sq.shape[0], sd.shape[0], sq.shape[1]
    f32 = dict(dtype=torch.float32, device=sq.device)
    gm, gmt = torch.empty(N, G, **f32), torch.empty(G, N, **f32)
    qt, dt = torch.empty(ds, N, **f32), torch.empty(ds, G, **f32)
    dq, dd = torch.empty(N, ds, **f32), torch.empty(G, ds, **f32)
    _C.check(L().cx_simkl_bwd(sq.data_ptr(), sd.data_ptr(), tq.data_ptr(), td.data_ptr(), lse_s.data_ptr(), lse_t.data_ptr(),
                              1.0 / tau, coef, gm.data_ptr(), gmt.data_ptr(), qt.data_ptr(), dt.data_ptr(), dq.data_ptr(),
                              dd.data_ptr(), N, G, ds, tq.shape[1], sq.stride(0), sd.stride(0), tq.stride(0), td.stride(0),
                              S()), "cx_simkl_bwd")
    return dq, dd


def _ref(sq, sd, tq, td, tau, dtype):
    """(rows, lse_s, lse_t, dq, dd) of the restatement in `dtype`; the gradients are those of sum(rows) / N."""
    q = sq.detach().to(dtype).requires_grad_()
    d = sd.detach().to(dtype).requires_grad_()
    rows = kl_rows_ref(q, d, tq, td, tau, dtype)
    (rows.sum() / sq.shape[0]).backward()
    lse_s = torch.logsumexp(q.detach() @ d.detach().T / tau, -1)
    lse_t = torch.logsumexp(tq.to(dtype) @ td.to(dtype).T / tau, -1)
    return rows.detach(), lse_s, lse_t, q.grad, d.grad


def _inputs(N, G, dim_s, dim_t, noise, ld=None):
    """Teacher rows of width dim_t, a student `noise` away on the first dim_s of them.  ld: every matrix is the (rows, dim) prefix
    view of a (rows, ld) buffer."""
    tq, td = unit_rows(N, dim_t, 11, DEV), unit_rows(G, dim_t, 12, DEV)
    sq, sd = noisy_student(tq, noise, 13, dim_s), noisy_student(td, noise, 14, dim_s)
    if ld is not None:
        def view(t):
            buf = torch.full((t.shape[0], ld), 7.0, device=DEV)   # (what lies past the width must not be read)
            buf[:, : t.shape[1]] = t
            return buf[:, : t.shape[1]]
        sq, sd, tq, td = view(sq), view(sd), view(tq), view(td)
    return sq, sd, tq, td


CASES = {
    # name: (N, G, dim_s, dim_t, tau, noise, ld)
    "tile_edges_tau0.2": (132, 200, 128, 128, 0.2, 0.3, None),      # 2 x 2 ragged tiles, rows clamped to N - 1 on load
    "tile_edges_tau0.02": (132, 200, 128, 128, 0.02, 1.0, None),    # logits reach +-50: the online maximum
    "width_tails": (36, 40, 72, 100, 0.2, 0.3, None),               # unequal widths, multiples of 4 but not of the 16-wide K tile
    "one_wave": (4, 8, 64, 64, 0.2, 0.3, None),
    "66_slices": (8, 4224, 64, 64, 0.2, 0.3, None),                 # the combine kernel's strided loop takes a second trip
    "leading_dims": (36, 44, 256, 256, 0.2, 0.3, 768),
}


@pytest.mark.parametrize("name", list(CASES))
def test_simkl_kernel_matches_float64_by_the_fp32_eager_rule(name):
    N, G, dim_s, dim_t, tau, noise, ld = CASES[name]
    sq, sd, tq, td = _inputs(N, G, dim_s, dim_t, noise, ld)
    rows, lse_s, lse_t = simkl_fwd(sq, sd, tq, td, tau)
    dq, dd = simkl_bwd(sq, sd, tq, td, lse_s, lse_t, tau, 1.0 / N)
    r64 = _ref(sq, sd, tq, td, tau, torch.float64)
    r32 = _ref(sq, sd, tq, td, tau, torch.float32)
    got = (rows, lse_s, lse_t, dq, dd)
    names = ("rows", "lse_s", "lse_t", "dq", "dd")
    errs = {n: rel_err(g, w) for n, g, w in zip(names, got, r64)}
    eager = {n: rel_err(g, w) for n, g, w in zip(names, r32, r64)}
    print(f"simkl {name}: mean kl {r64[0].mean().item():.4g}  kernel {errs}  fp32 eager {eager}")
    report("simkl", case=name, mean_kl=r64[0].mean().item(), **{f"e_{k}": v for k, v in errs.items()},
           **{f"eager_{k}": v for k, v in eager.items()})
    for t in got:
        assert torch.isfinite(t).all()
    for n in names:
        floor = GRAD_FLOOR if n in ("dq", "dd") else ROW_FLOOR
        assert errs[n] <= max(3 * eager[n], floor), f"{name}/{n}: kernel {errs[n]:.3e}, fp32 eager {eager[n]:.3e}"
    # determinism: no atomics anywhere in the path, a second call gives the same bits
    rows2, lse_s2, lse_t2 = simkl_fwd(sq, sd, tq, td, tau)
    dq2, dd2 = simkl_bwd(sq, sd, tq, td, lse_s2, lse_t2, tau, 1.0 / N)
    for a, b in zip(got, (rows2, lse_s2, lse_t2, dq2, dd2)):
        assert torch.equal(a, b)


def test_simkl_student_equal_to_teacher_is_exactly_zero():
    """Same tensors on both sides: both products run the same instruction sequence on the same bits and both log-sum-exps the same
    code, so kl_rows and both gradients are exactly 0.0 -- and nothing is NaN, which (-inf) - (-inf) on the masked columns of the
    ragged tiles would make it."""
    tq, td = unit_rows(132, 128, 21, DEV), unit_rows(200, 128, 22, DEV)
    for tau in (0.2, 0.02):
        rows, lse_s, lse_t = simkl_fwd(tq, td, tq, td, tau)
        dq, dd = simkl_bwd(tq, td, tq, td, lse_s, lse_t, tau, 1.0 / 132)
        for t in (rows, lse_s, lse_t, dq, dd):
            assert not torch.isnan(t).any()
        assert torch.equal(lse_s, lse_t)
        assert torch.equal(rows, torch.zeros_like(rows))
        assert torch.equal(dq, torch.zeros_like(dq)) and torch.equal(dd, torch.zeros_like(dd))
    # separate copies of the same values, other leading dimension: still the same bits in, the same bits out
    buf = torch.zeros(132, 256, device=DEV)
    buf[:, :128] = tq
    rows, _, _ = simkl_fwd(buf[:, :128], td.clone(), tq, td, 0.2)
    assert torch.equal(rows, torch.zeros_like(rows))


def test_simkl_error_codes_launch_nothing():
    sq, sd, tq, td = _inputs(8, 8, 64, 64, 0.3)
    f32 = dict(dtype=torch.float32, device=DEV)
    ws = torch.empty(L().cx_simkl_ws_floats(8, 8), **f32)
    sentinel = 123.0
    outs = [torch.full((8,), sentinel, **f32) for _ in range(3)]

    def fwd(Qs=sq, N=8, G=8, dim_s=64, dim_t=64, ldqs=64, lddt=64):
        return L().cx_simkl_fwd(_C.ptr(Qs), sd.data_ptr(), tq.data_ptr(), td.data_ptr(), 5.0, ws.data_ptr(), outs[0].data_ptr(),
                                outs[1].data_ptr(), outs[2].data_ptr(), N, G, dim_s, dim_t, ldqs, 64, 64, lddt, S())

    assert fwd(Qs=None) == -3                      # CX_ERR_ARG: a null pointer
    assert fwd(dim_s=62) == -1                     # CX_ERR_SHAPE: width not a multiple of 4
    assert fwd(dim_t=30) == -1
    assert fwd(ldqs=66) == -2                      # CX_ERR_ALIGN: leading dimension not a multiple of 4
    assert fwd(lddt=70) == -2
    gm = torch.full((8 * 8,), sentinel, **f32)
    scratch = [torch.full((64 * 8,), sentinel, **f32) for _ in range(5)]

    def bwd(N=8, G=8, lse=outs[0]):
        return L().cx_simkl_bwd(sq.data_ptr(), sd.data_ptr(), tq.data_ptr(), td.data_ptr(), _C.ptr(lse), outs[1].data_ptr(), 5.0,
                                1.0, gm.data_ptr(), scratch[0].data_ptr(), scratch[1].data_ptr(), scratch[2].data_ptr(),
                                scratch[3].data_ptr(), scratch[4].data_ptr(), N, G, 64, 64, 64, 64, 64, 64, S())

    assert bwd(N=6) == -1 and bwd(G=7) == -1       # CX_ERR_SHAPE: N, G are the K of the two output GEMMs
    assert bwd(lse=None) == -3
    torch.cuda.synchronize()
    for t in outs + [gm] + scratch:
        assert (t == sentinel).all(), "a refused call wrote to its outputs"
    assert _C.lib().cx_simkl_ws_floats(2048, 16384) == 2048 * 5 * 2 * 128


# ------------------------------------------------------------------------------------------------------ loss layer
def _loss_inputs():
    tq, td = unit_rows(132, 256, 31, DEV), unit_rows(132, 256, 32, DEV)
    return noisy_student(tq, 0.3, 33), noisy_student(td, 0.3, 34), tq, td


def _loss_and_grads(fn, loss_fn, sq, sd, tq, td, tau, dtype):
    q = sq.detach().to(dtype).requires_grad_()
    d = sd.detach().to(dtype).requires_grad_()
    out = fn(loss_fn, q, d, tq.to(dtype), td.to(dtype), tau)
    out["loss"].backward()
    return {k: v.detach() for k, v in out.items()}, q.grad, d.grad


@pytest.mark.parametrize("loss_fn,tau", [("kd", 0.2), ("mse", 1.0), ("towers", 0.2)])
def test_distill_loss_forms_match_float64_restatements(loss_fn, tau):
    sq, sd, tq, td = _loss_inputs()
    tq_g, td_g = tq.clone().requires_grad_(), td.clone().requires_grad_()
    q, d = sq.clone().requires_grad_(), sd.clone().requires_grad_()
    out = distill_loss(loss_fn, q, d, tq_g, td_g, tau)
    out["loss"].backward()
    assert tq_g.grad is None and td_g.grad is None, "the teacher side gets no gradient"
    w64, q64, d64 = _loss_and_grads(lambda *a: distill_loss_ref(*a, dtype=torch.float64), loss_fn, sq, sd, tq, td, tau, torch.float64)
    w32, q32, d32 = _loss_and_grads(lambda *a: distill_loss_ref(*a, dtype=torch.float32), loss_fn, sq, sd, tq, td, tau, torch.float32)
    assert set(out) == set(w64)
    for k in w64:
        e, e32 = rel_err(out[k].detach(), w64[k]), rel_err(w32[k], w64[k])
        print(f"distill_loss {loss_fn}/{k}: {out[k].item():.8g} vs {w64[k].item():.8g}  err {e:.3e}  fp32 eager {e32:.3e}")
        assert e <= max(3 * e32, ROW_FLOOR), f"{loss_fn}/{k}: {e:.3e} vs fp32 eager {e32:.3e}"
    for name, g, w, w32g in (("dq", q.grad, q64, q32), ("dd", d.grad, d64, d32)):
        e, e32 = rel_err(g, w), rel_err(w32g, w)
        print(f"distill_loss {loss_fn}/{name}: err {e:.3e}  fp32 eager {e32:.3e}")
        assert e <= max(3 * e32, GRAD_FLOOR), f"{loss_fn}/{name}: {e:.3e} vs fp32 eager {e32:.3e}"


def test_similarity_kl_loss_autograd_surface():
    sq, sd, tq, td = _loss_inputs()
    q, d = sq.clone().requires_grad_(), sd.clone().requires_grad_()
    tq_g = tq.clone().requires_grad_()
    loss = similarity_kl_loss(q, d, tq_g, td, 0.2)
    loss.backward()
    g1q, g1d = q.grad.clone(), d.grad.clone()
    assert tq_g.grad is None
    q.grad = d.grad = None
    (2.5 * similarity_kl_loss(q, d, tq_g, td, 0.2)).backward()     # a scaled upstream gradient scales the result: one fp32 product
    assert torch.equal(q.grad, g1q * 2.5) and torch.equal(d.grad, g1d * 2.5)
    # bf16 / non-contiguous operands are converted as in the InfoNCE function; no gradient asked: any N, G
    with torch.no_grad():
        v = similarity_kl_loss(sq[:131], sd[:130], tq[:131], td[:130], 0.2)
    assert torch.isfinite(v)
    with pytest.raises(ValueError):
        similarity_kl_loss(sq[:131].clone().requires_grad_(), sd, tq[:131], td, 0.2)   # the backward needs N % 4 == 0: refused in the forward
    with pytest.raises(NotImplementedError):
        distill_loss("stella", sq, sd, tq, td, 0.2)


# --------------------------------------------------------------------------------------------------------- trainer
def _tiny4():
    from contrastors_amd.nomic_bert import NomicBertConfig
    from oracle.make_golden import TINY_NOMIC

    fields = NomicBertConfig.__dataclass_fields__
    return NomicBertConfig(**{k: v for k, v in dict(TINY_NOMIC, n_layer=4).items() if k in fields})


@pytest.fixture(scope="module")
def teacher_dir(tmp_path_factory):
    from contrastors_amd.biencoder import BiEncoder, BiEncoderConfig

    path = tmp_path_factory.mktemp("teacher") / "model"
    BiEncoder(BiEncoderConfig(pooling="mean", trunk_config=_tiny4()), device=DEV, seed=5).save_pretrained(str(path))
    return str(path)


def _config(loss_fn, **model_kw):
    from contrastors_amd.config import Config, DataArgs, ModelArgs, TrainArgs

    ta = dict(learning_rate=1e-4, weight_decay=0.01, warmup_steps=0, grad_cache=False, schedule_type="constant",
              max_grad_norm=1.0, clamp_logits=False, distill_loss_fn=loss_fn, distill_temperature=0.2)
    ta.update(model_kw.pop("train", {}))
    return Config(train_args=TrainArgs(**ta), data_args=DataArgs(batch_size=16, seed=7),
                  model_args=ModelArgs(model_type="distill", pooling="mean", model_name="tiny", pretrained=False, **model_kw))


def _batch():
    from contrastors_amd.trainers import synthetic_batches

    return next(iter(synthetic_batches(1, 16, 32, vocab=512, ragged=True)))


def test_student_is_the_even_blocks_of_the_checkpoint_teacher(teacher_dir):
    from contrastors_amd.trainers import TRAINER_REGISTRY

    tr = TRAINER_REGISTRY["distill"](_config("mse", checkpoint=teacher_dir), torch.bfloat16, device=DEV, total_steps=10)
    student, teacher = tr.model["model"], tr.model["teacher"]
    assert teacher.trunk.config.n_layer == 4 and student.trunk.config.n_layer == 2
    assert student.config.pooling == "cls" and teacher.config.pooling == "mean" and not teacher.training and student.training
    t_sd, s_sd = teacher.trunk.reference_state_dict(), student.trunk.reference_state_dict()
    seen = 0
    for k, v in s_sd.items():
        tk = k.replace("encoder.layers.1.", "encoder.layers.2.")
        assert torch.equal(v, t_sd[tk]), k
        seen += 1
    assert seen == len(s_sd) and any(k.startswith("embeddings.") for k in s_sd) and "emb_ln.weight" in s_sd
    assert not torch.equal(t_sd["encoder.layers.1.attn.Wqkv.weight"], t_sd["encoder.layers.2.attn.Wqkv.weight"])


@pytest.mark.parametrize("loss_fn,extra", [("mse", {}), ("kd", {}), ("towers", {}), ("towers", {"ffn_div": 2})])
def test_training_steps_lower_the_loss_and_leave_the_teacher_alone(teacher_dir, loss_fn, extra):
    from contrastors_amd.distill import DistillTrainer

    tr = DistillTrainer(_config(loss_fn, checkpoint=teacher_dir, **extra), torch.bfloat16, device=DEV, total_steps=10)
    teacher, student = tr.model["teacher"], tr.model["model"]
    assert (student.config.projection_dim == 256) == bool(extra)      # `towers` + checkpoint + ffn_div: the trained projection head
    before = teacher.trunk.flat_param.clone()
    s_before = student.trunk.flat_param.clone()
    batch = _batch()
    losses = [float(tr.training_step(batch)) for _ in range(5)]
    print(f"distill trainer {loss_fn} {extra}: {losses}")
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0], losses
    assert torch.equal(teacher.trunk.flat_param, before), "the teacher moved"
    assert not torch.equal(student.trunk.flat_param, s_before)
    assert all(not p.requires_grad for p in teacher.parameters())
    held = {p.data_ptr() for g in tr.optimizer.param_groups for p in g["params"]}
    assert teacher.trunk.flat_decay.data_ptr() not in held and teacher.trunk.flat_nodecay.data_ptr() not in held
    assert student.trunk.flat_decay.data_ptr() in held
    out = tr.forward_step(batch)
    want = {"mse": {"loss", "query_mse", "document_mse"}, "kd": {"loss", "kd_loss", "infonce_loss"},
            "towers": {"loss", "loss_infonce_student", "loss_teacher_query", "loss_teacher_document", "loss_infonce_teacher"}}
    assert set(out) == want[loss_fn]


def test_tracker_gets_every_entry_and_checkpoints_hold_the_student(teacher_dir, tmp_path):
    """sc/trainers/distill.py:460-462: with a tracker every entry of the loss dictionary is logged.  save_state / load_state are the
    inherited ones and save the student (the teacher stays where its checkpoint is)."""
    import json

    from contrastors_amd.distill import DistillTrainer
    from contrastors_amd.trainers import JsonlTracker

    def make():
        cfg = _config("kd", checkpoint=teacher_dir, train={"wandb": True, "output_dir": str(tmp_path / "run")})
        return DistillTrainer(cfg, torch.bfloat16, device=DEV, total_steps=10)

    tr = make()
    batch = _batch()
    tr.training_step(batch)
    if isinstance(tr.tracker, JsonlTracker):   # (a machine with the wandb package gets the reference's tracker instead)
        rows = [json.loads(ln) for ln in open(tmp_path / "run" / "metrics.jsonl")]
        assert {"loss", "kd_loss", "infonce_loss"} <= set(rows[0]) and rows[0]["step"] == 0
    tr.save_state(str(tmp_path / "ckpt"))
    saved = json.load(open(tmp_path / "ckpt" / "model" / "config.json"))
    assert saved["trunk_config"]["n_layer"] == 2 and saved["pooling"] == "cls"
    student_at_save = tr.model["model"].trunk.flat_param.clone()
    want = float(tr.training_step(batch))
    again = make()
    again.load_state(str(tmp_path / "ckpt"))
    assert again.step == 1 and torch.equal(again.model["model"].trunk.flat_param, student_at_save)
    # the resumed step's loss is a forward of the restored student: the same kernels on the same bits
    assert float(again.training_step(batch)) == want


def test_branch_without_checkpoint_and_what_the_trainer_refuses(teacher_dir):
    from contrastors_amd.distill import DistillTrainer

    # no checkpoint, explicit architecture (a declared random init): full depth, block i <- teacher block i // 2, own embeddings
    tr = DistillTrainer(_config("mse", distill_init_pretrained=True), torch.bfloat16, device=DEV, trunk_config=_tiny4(), total_steps=10)
    t_sd, s_sd = tr.model["teacher"].trunk.reference_state_dict(), tr.model["model"].trunk.reference_state_dict()
    assert tr.model["model"].trunk.config.n_layer == 4
    for i in range(4):
        k = f"encoder.layers.{i}.attn.Wqkv.weight"
        assert torch.equal(s_sd[k], t_sd[k.replace(f".{i}.", f".{i // 2}.")])
    with pytest.raises(NotImplementedError, match="ffn_div"):
        DistillTrainer(_config("mse", ffn_div=2), torch.bfloat16, device=DEV, trunk_config=_tiny4())
    with pytest.raises(NotImplementedError, match="grad_cache"):
        DistillTrainer(_config("kd", checkpoint=teacher_dir, train={"grad_cache": True, "chunk_size": 4}), torch.bfloat16, device=DEV)
    tr = DistillTrainer(_config("stella", checkpoint=teacher_dir), torch.bfloat16, device=DEV, total_steps=10)
    with pytest.raises(NotImplementedError, match="stella"):
        tr.training_step(_batch())


def test_train_cli_runs_a_distill_recipe(tmp_path):
    """`python -m contrastors_amd.train --config <yaml with model_type: distill>`: registry dispatch, the checkpoint branch with the
    architecture read from the checkpoint, two synthetic steps of the recipe's `kd` loss.  (The command line's synthetic batches
    draw token ids below 30522: the teacher is the tiny architecture with the full vocabulary.)"""
    import numpy as np
    import yaml

    from contrastors_amd.biencoder import BiEncoder, BiEncoderConfig

    teacher_dir = str(tmp_path / "teacher")
    BiEncoder(BiEncoderConfig(pooling="mean", trunk_config=dataclasses.replace(_tiny4(), vocab_size=30528)), device=DEV,
              seed=6).save_pretrained(teacher_dir)
    cfg = {"train_args": {"num_epochs": 1, "learning_rate": 2.0e-4, "weight_decay": 0.01, "warmup_steps": 0, "chunk_size": 32,
                          "schedule_type": "linear", "max_grad_norm": 1.0, "adam_beta1": 0.9, "adam_beta2": 0.999,
                          "grad_cache": False, "loss_fn": "clip", "clamp_logits": False, "logit_max": 100, "wandb": False,
                          "distill_loss_fn": "kd", "distill_temperature": 0.2},
           "model_args": {"model_type": "distill", "logit_scale": 50, "trainable_logit_scale": False, "seq_len": 512,
                          "pooling": "mean", "nomic_encoder": True, "add_prefix": True, "num_negatives": 0,
                          "model_name": "tiny", "pretrained": True, "checkpoint": teacher_dir},
           "data_args": {"workers": 0, "batch_size": 256, "seed": 42, "shuffle": False}}
    path = tmp_path / "distill.yaml"
    path.write_text(yaml.safe_dump(cfg))
    root = str(Path(__file__).resolve().parent.parent)
    out = subprocess.run([sys.executable, "-m", "contrastors_amd.train", "--config", str(path), "--synthetic-steps", "2",
                          "--seq-len", "32", "--batch_size", "16"], cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(ln.split("loss")[1].split()[0].strip(":=")) for ln in out.stdout.splitlines() if "loss" in ln]
    assert len(losses) >= 2 and all(np.isfinite(losses))
