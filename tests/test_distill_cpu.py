"""Distillation, host side: the yardsticks of tests/distill_ref.py checked against torch's own loss functions and against planted
errors, the two weight-selection functions, and the configuration surface.  No GPU."""
import json
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests.distill_ref import distill_loss_ref, infonce_ref, kl_ref, kl_rows_ref, noisy_student, unit_rows

CONTRACTS = Path(__file__).resolve().parent / "golden" / "host_contracts.json"


def _case(tau_noise=0.3, n=40, g=56, d=64):
    tq, td = unit_rows(n, d, 1), unit_rows(g, d, 2)
    return noisy_student(tq, tau_noise, 3), noisy_student(td, tau_noise, 4), tq, td


@pytest.mark.parametrize("tau", [0.2, 0.02])
def test_kl_restatement_is_torch_kl_div_batchmean(tau):
    sq, sd, tq, td = (t.double() for t in _case())
    want = F.kl_div(F.log_softmax(sq @ sd.T / tau, dim=-1), F.softmax(tq @ td.T / tau, dim=-1), reduction="batchmean")
    got = kl_ref(sq, sd, tq, td, tau)
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
    rows = kl_rows_ref(sq, sd, tq, td, tau)
    assert rows.shape == (40,) and (rows > 0).all()          # Gibbs: KL > 0 for a student that differs
    # the closed form the kernel evaluates: sum_j p (t - s) - lse_t + lse_s
    s, t = sq @ sd.T / tau, tq @ td.T / tau
    closed = (torch.softmax(t, -1) * (t - s)).sum(-1) - torch.logsumexp(t, -1) + torch.logsumexp(s, -1)
    assert torch.allclose(rows, closed, rtol=1e-10, atol=1e-14)


def test_kl_restatement_moves_under_planted_errors():
    sq, sd, tq, td = (t.double() for t in _case())
    tau = 0.2
    good = kl_ref(sq, sd, tq, td, tau).item()
    s, t = sq @ sd.T / tau, tq @ td.T / tau
    p = torch.softmax(t, -1)
    dropped_lse_t = ((p * (t - s)).sum(-1) + torch.logsumexp(s, -1)).sum().item() / 40      # "- lse_t" forgotten
    swapped = kl_ref(tq, td, sq, sd, tau).item()                                              # KL(q || p)
    unscaled = kl_ref(sq, sd, tq, td, 1.0).item()                                             # temperature ignored
    summed = kl_rows_ref(sq, sd, tq, td, tau).sum().item()                                    # "/ N" forgotten
    for wrong in (dropped_lse_t, swapped, unscaled, summed):
        assert abs(wrong - good) > 1e-3 * abs(good), (wrong, good)
    assert kl_ref(tq, td, tq, td, tau).item() == 0.0


def test_loss_form_restatements():
    sq, sd, tq, td = (t.double() for t in _case(n=24, g=24))
    out = distill_loss_ref("kd", sq, sd, tq, td, 0.2)
    assert set(out) == {"loss", "kd_loss", "infonce_loss"}
    want_nce = F.cross_entropy(sq @ sd.T / 0.02, torch.arange(24))
    assert out["infonce_loss"].item() == pytest.approx(want_nce.item(), rel=1e-12)
    assert out["loss"].item() == pytest.approx(1000 * out["kd_loss"].item() + want_nce.item(), rel=1e-12)
    tw = distill_loss_ref("towers", sq, sd, tq, td, 0.2)
    assert set(tw) == {"loss", "loss_infonce_student", "loss_teacher_query", "loss_teacher_document", "loss_infonce_teacher"}
    assert tw["loss"].item() == pytest.approx(sum(v.item() for k, v in tw.items() if k != "loss") / 4, rel=1e-12)
    assert tw["loss_teacher_query"].item() == pytest.approx(infonce_ref(sq, tq, 5.0).item(), rel=1e-12)
    ms = distill_loss_ref("mse", sq, sd, tq, td, 1.0)
    assert set(ms) == {"loss", "query_mse", "document_mse"}
    assert ms["query_mse"].item() == pytest.approx(((sq - tq) ** 2).mean().item(), rel=1e-12)
    # negatives: 2 documents per query, the positive first
    assert infonce_ref(sq[:12], sd, 5.0).item() == pytest.approx(
        F.cross_entropy(sq[:12] @ sd.T * 5.0, torch.arange(12) * 2).item(), rel=1e-12)


def test_uniform_element_selection():
    from contrastors_amd.distill import uniform_element_selection

    wt = torch.arange(12).reshape(3, 4)
    # 3 rows -> 2: 2 does not divide 3, round(linspace(0, 2, 2)) = [0, 2]; 4 columns -> 2: a stride of 2
    assert uniform_element_selection(wt, (2, 2)).tolist() == [[0, 2], [8, 10]]
    same = uniform_element_selection(wt, (3, 4))
    assert torch.equal(same, wt) and same.data_ptr() != wt.data_ptr()
    assert uniform_element_selection(torch.arange(7), (3,)).tolist() == [0, 3, 6]
    assert uniform_element_selection(torch.arange(8.0), torch.Size([4])).tolist() == [0.0, 2.0, 4.0, 6.0]
    with pytest.raises(ValueError):
        uniform_element_selection(wt, (4, 4))
    with pytest.raises(ValueError):
        uniform_element_selection(wt, (12,))


def test_layer_map_of_both_branches():
    from contrastors_amd.distill import _teacher_key, distill_layer_map

    half = distill_layer_map(6, 12, True)
    assert half == {0: 0, 1: 2, 2: 4, 3: 6, 4: 8, 5: 10}
    full = distill_layer_map(12, 12, False)      # the reference's literal `teacher.encoder.layer[i // 2]`
    assert full == {i: i // 2 for i in range(12)} and max(full.values()) == 5
    assert distill_layer_map(2, 5, True) == {0: 0, 1: 2}
    with pytest.raises(ValueError):
        distill_layer_map(12, 12, True)
    with pytest.raises(ValueError):
        distill_layer_map(6, 12, False)
    assert _teacher_key("encoder.layers.3.attn.Wqkv.weight", half) == "encoder.layers.6.attn.Wqkv.weight"
    assert _teacher_key("encoder.layers.11.mlp.fc2.weight", full) == "encoder.layers.5.mlp.fc2.weight"
    assert _teacher_key("emb_ln.weight", half) == "emb_ln.weight"


def test_config_surface(tmp_path):
    import yaml

    from contrastors_amd.config import ModelArgs, TrainArgs, read_config
    from contrastors_amd.trainers import TRAINER_REGISTRY

    ta, ma = TrainArgs(), ModelArgs()
    assert ta.distill_loss_fn == "mse" and ta.distill_temperature == 1.0
    assert ma.distill_init_pretrained is False and ma.ffn_div is None
    for fn in ("mse", "kd", "towers", "stella"):
        assert TrainArgs(distill_loss_fn=fn).distill_loss_fn == fn
    with pytest.raises(ValueError):
        TrainArgs(distill_loss_fn="cosine")
    assert "distill" in TRAINER_REGISTRY
    recipes = json.loads(CONTRACTS.read_text())["recipes"]
    seen = {}
    for name in ("distill.yaml", "contrastive_finetune_distill.yaml"):
        p = tmp_path / name
        p.write_text(yaml.safe_dump(recipes[name], sort_keys=False))
        seen[name] = read_config(str(p))
        assert seen[name].model_args.model_type == "distill"
    kd = seen["distill.yaml"]
    assert kd.train_args.distill_loss_fn == "kd" and kd.train_args.distill_temperature == 0.2
    assert kd.model_args.distill_init_pretrained is True and kd.train_args.grad_cache is False
    ft = seen["contrastive_finetune_distill.yaml"]
    assert ft.train_args.distill_loss_fn == recipes["contrastive_finetune_distill.yaml"]["train_args"]["distill_loss_fn"]
    assert ft.model_args.ffn_div == recipes["contrastive_finetune_distill.yaml"]["model_args"].get("ffn_div")   # parses; the trainer decides


def test_loss_layer_refuses_the_cpu_and_stella():
    from contrastors_amd.loss import distill_loss, similarity_kl_loss

    sq, sd, tq, td = _case(n=8, g=8)
    with pytest.raises(RuntimeError):
        similarity_kl_loss(sq, sd, tq, td, 0.2)
    with pytest.raises(NotImplementedError, match="stella"):
        distill_loss("stella", sq, sd, tq, td, 0.2)
    with pytest.raises(ValueError):
        distill_loss("mse", sq[:, :32], sd[:, :32], tq, td, 1.0)
    with pytest.raises(ValueError):
        similarity_kl_loss(sq, sd, tq, td, 0.0)


def test_trainer_refuses_at_construction_what_it_cannot_serve():
    """Both refusals come before any model is built (no device is touched)."""
    from contrastors_amd.config import Config, ModelArgs, TrainArgs
    from contrastors_amd.distill import DistillTrainer
    from contrastors_amd.trainers import TRAINER_REGISTRY

    narrow = Config(train_args=TrainArgs(warmup_steps=0), model_args=ModelArgs(model_type="distill", ffn_div=2))
    with pytest.raises(NotImplementedError, match="ffn_div"):
        DistillTrainer(narrow)
    with pytest.raises(NotImplementedError, match="ffn_div"):
        TRAINER_REGISTRY["distill"](narrow, torch.bfloat16)
    cached = Config(train_args=TrainArgs(warmup_steps=0, grad_cache=True, chunk_size=32), model_args=ModelArgs(model_type="distill"))
    with pytest.raises(NotImplementedError, match="grad_cache"):
        DistillTrainer(cached)
