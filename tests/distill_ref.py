"""Yardsticks of the distillation tests: torch restatements of the loss forms of sc/trainers/distill.py:341-385 for one
process (world 1), run in float64 as the reference value and in float32 as the error an eager implementation carries.
tests/test_distill_cpu.py checks them against F.kl_div / F.cross_entropy and against planted errors."""
import torch
import torch.nn.functional as F


def kl_rows_ref(sq, sd, tq, td, tau, dtype=torch.float64):
    """kl_i = sum_j p_ij (log p_ij - log q_ij),  p = softmax_j(tq td^T / tau),  q = softmax_j(sq sd^T / tau)."""
    s = (sq.to(dtype) @ sd.to(dtype).T) / tau
    t = (tq.to(dtype) @ td.to(dtype).T) / tau
    p = torch.softmax(t, dim=-1)
    return (p * (torch.log_softmax(t, dim=-1) - torch.log_softmax(s, dim=-1))).sum(-1)


def kl_ref(sq, sd, tq, td, tau, dtype=torch.float64):
    return kl_rows_ref(sq, sd, tq, td, tau, dtype).sum() / sq.shape[0]


def infonce_ref(q, d, scale, dtype=torch.float64):
    """The trainer's infonce for one process: cross entropy of q d^T * scale against the diagonal (strided by G // N)."""
    n, g = q.shape[0], d.shape[0]
    labels = torch.arange(n, device=q.device) * (g // n)
    return F.cross_entropy((q.to(dtype) @ d.to(dtype).T) * scale, labels)


def distill_loss_ref(loss_fn, sq, sd, tq, td, tau, dtype=torch.float64):
    if loss_fn == "mse":
        qm, dm = F.mse_loss(sq.to(dtype), tq.to(dtype)), F.mse_loss(sd.to(dtype), td.to(dtype))
        return {"loss": qm + dm, "query_mse": qm, "document_mse": dm}
    if loss_fn == "kd":
        kd = kl_ref(sq, sd, tq, td, tau, dtype)
        nce = infonce_ref(sq, sd, 1 / 0.02, dtype)
        return {"loss": 1000 * kd + nce, "kd_loss": kd, "infonce_loss": nce}
    if loss_fn == "towers":
        a = infonce_ref(sq, sd, 1 / tau, dtype)
        b = infonce_ref(sq, tq, 1 / tau, dtype)
        c = infonce_ref(sd, td, 1 / tau, dtype)
        e = infonce_ref(sq, td, 1 / tau, dtype)
        return {"loss": (a + b + c + e) / 4, "loss_infonce_student": a, "loss_teacher_query": b,
                "loss_teacher_document": c, "loss_infonce_teacher": e}
    raise KeyError(loss_fn)


def unit_rows(n, d, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, d, generator=g), dim=-1).to(device)


def noisy_student(teacher, noise, seed, width=None):
    """normalize(teacher[:, :width] + noise * randn / sqrt(width)): a student `noise` away from its teacher."""
    width = width or teacher.shape[1]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(teacher.shape[0], width, generator=g).to(teacher.device)
    return F.normalize(teacher[:, :width] + noise * z / width ** 0.5, dim=-1)
