"""EVA-02 image tower on the MI355X: the three new kernels (2-D RoPE, SwiGLU + sub-LN forward / backward) against fp32 torch,
the tower (cx_vit_*_ex) against the fixture written by the reference's own ViTModel and against the fp32 restatement at
B/16, the map head on it, checkpointing bit-identity, and ext == NULL bit-identity with the plain entry points."""
from types import SimpleNamespace

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from contrastors_amd import _C
from contrastors_amd.vit import ViTConfig, ViTEngine
from oracle import vit_ref
from tests import eva02_ref
from tests.gpu_util import L, S, max_err, rel_err, report

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tiny(gold):
    g = gold("vit_eva02_tiny")
    d = {k[4:]: g[k].tolist() for k in g.files if k.startswith("cfg/")}
    d["ref_feat_shape"] = tuple(d["ref_feat_shape"])
    cfg = ViTConfig.eva02_base_patch16_224(**d)
    return g, cfg, SimpleNamespace(**d)


# ---- kernels ----------------------------------------------------------------------------------------------------------
def test_rope2d_matches_fp32_rounded_once_and_inverts():
    H, d, P, n_prefix = 12, 768, 196, 1
    cfg = ViTConfig.eva02_base_patch16_224()
    cos, sin = eva02_ref.rope_tables(cfg)
    cos_d, sin_d = cos.to(DEV).contiguous(), sin.to(DEV).contiguous()
    B = 3
    S_ = P + n_prefix
    T = B * S_
    cu = torch.arange(0, (B + 1) * S_, S_, dtype=torch.int32, device=DEV)
    qkv = torch.randn(T, 3 * d, device=DEV).to(torch.bfloat16)
    x = qkv.clone()
    _C.check(L().cx_rope2d_qkv_inplace(x.data_ptr(), cu.data_ptr(), cos_d.data_ptr(), sin_d.data_ptr(), P, B, H, T, n_prefix, 1,
                                       S()), "rope2d")
    v = qkv.view(B, S_, 3, H, 64)
    want = v.clone()
    for i in (0, 1):
        want[:, 1:, i] = torch.stack([eva02_ref.rope_apply(v[b, 1:, i], cos_d, sin_d) for b in range(B)]).to(torch.bfloat16)
    got = x.view(B, S_, 3, H, 64)
    assert torch.equal(got[:, 0], v[:, 0]), "the [cls] token is not rotated"
    assert torch.equal(got[:, :, 2], v[:, :, 2]), "V is untouched"
    assert torch.equal(got, want), "bit-exact vs the fp32 rotation rounded once"
    y = x.clone()
    _C.check(L().cx_rope2d_qkv_inplace(y.data_ptr(), cu.data_ptr(), cos_d.data_ptr(), sin_d.data_ptr(), P, B, H, T, n_prefix, -1,
                                       S()), "rope2d inverse")
    assert max_err(y.float(), qkv.float()) < 3e-2 and rel_err(y.float(), qkv.float()) < 5e-3


def _fwd_ref(yg, gamma, beta, I):
    y = yg.view(-1, I // 32, 2, 32)[:, :, 0].reshape(-1, I).float()
    g = yg.view(-1, I // 32, 2, 32)[:, :, 1].reshape(-1, I).float()
    a = (F.silu(g) * y).to(torch.bfloat16)
    return y, g, a


@pytest.mark.parametrize("I", [512, 2048])
@pytest.mark.parametrize("T, ws_rows", [(37, 1024), (300, 1024), (300, 4), (2051, 7)])
def test_swiglu_subln_fwd_bwd_vs_fp32(I, T, ws_rows):
    """ws_rows = the partial vectors the workspace holds: 1024 -> one row per block at these T; 4 / 7 -> every block loops over
    many rows (75 / 293 each, a ragged last block), the regime of a real chunk (1536 images: ~296 rows per block)."""
    gen = torch.Generator(device="cpu").manual_seed(I + T)
    yg = (torch.randn(T, 2 * I, generator=gen) * 2).to(torch.bfloat16).to(DEV)
    gamma = (1 + 0.1 * torch.randn(I, generator=gen)).to(DEV)
    beta = (0.1 * torch.randn(I, generator=gen)).to(DEV)
    dz = torch.randn(T, I, generator=gen).to(torch.bfloat16).to(DEV)
    gate = torch.empty(T, I, dtype=torch.bfloat16, device=DEV)
    act, z = torch.empty_like(gate), torch.empty_like(gate)
    mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
    _C.check(L().cx_swiglu_subln_fwd(yg.data_ptr(), gamma.data_ptr(), beta.data_ptr(), gate.data_ptr(), act.data_ptr(), z.data_ptr(),
                                     mean.data_ptr(), rstd.data_ptr(), T, I, 1e-5, S()), "subln fwd")
    y, g, a_ref = _fwd_ref(yg, gamma, beta, I)
    assert torch.equal(gate.float(), g)
    assert max_err(act.float(), a_ref.float()) <= 2 ** -7 * a_ref.float().abs().max()   # (one bf16 ulp at most)
    a32 = act.float()
    z_ref = F.layer_norm(a32, (I,), gamma, beta, 1e-5)
    assert rel_err(z.float(), z_ref) < 4e-3
    assert rel_err(mean, a32.mean(-1)) < 1e-5 and rel_err(rstd, torch.rsqrt(a32.var(-1, unbiased=False) + 1e-5)) < 1e-4

    ws = torch.empty(ws_rows * 4 * I, device=DEV)

    def bwd():
        dyg = torch.empty(T, 2 * I, dtype=torch.bfloat16, device=DEV)
        dgam, dbet, dbias = (torch.zeros(n, device=DEV) for n in (I, I, 2 * I))
        _C.check(L().cx_swiglu_subln_bwd(dz.data_ptr(), act.data_ptr(), gate.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         gamma.data_ptr(), dyg.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), dbias.data_ptr(),
                                         ws.data_ptr(), ws.numel(), T, I, S()), "subln bwd")
        return dyg, dgam, dbet, dbias

    dyg, dgam, dbet, dbias = bwd()
    # fp32 reference: gradients through LN (on the saved a) and silu(g) * y with y = the fc11 output
    yr, gr = y.clone().requires_grad_(), g.clone().requires_grad_()
    ar = a32.clone().requires_grad_()
    gm, bt = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.layer_norm(ar, (I,), gm, bt, 1e-5).backward(dz.float())
    (F.silu(gr) * yr).backward(ar.grad)
    want = torch.stack([yr.grad.view(T, I // 32, 32), gr.grad.view(T, I // 32, 32)], 2).reshape(T, 2 * I)
    e_dyg = rel_err(dyg.float(), want)
    e_g, e_b = rel_err(dgam, gm.grad), rel_err(dbet, bt.grad)
    e_bias = rel_err(dbias, dyg.float().sum(0))
    e_bias_ref = rel_err(dbias, want.sum(0))
    report("eva_swiglu_subln", I=I, T=T, ws_rows=ws_rows, e_dyg=e_dyg, e_dgamma=e_g, e_dbeta=e_b, e_dbias=e_bias, e_dbias_ref=e_bias_ref)
    assert e_dyg < 1e-2 and e_g < 1e-4 and e_b < 1e-5 and e_bias < 1e-5 and e_bias_ref < 1e-2
    again = bwd()
    assert all(torch.equal(u, v) for u, v in zip((dyg, dgam, dbet, dbias), again)), "run-to-run bit equality"


def test_swiglu_subln_refuses_widths_it_does_not_cover():
    x = torch.zeros(64, 2 * 4352, dtype=torch.bfloat16, device=DEV)
    rc = L().cx_swiglu_subln_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, x.data_ptr(), x.data_ptr(), x.data_ptr(),
                                 x.data_ptr(), 4, 4352, 1e-5, S())
    assert rc == -1
    rc = L().cx_swiglu_subln_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, x.data_ptr(), x.data_ptr(), x.data_ptr(),
                                 x.data_ptr(), 4, 320, 1e-5, S())
    assert rc == -1


# ---- the tower ----------------------------------------------------------------------------------------------------------
def _oracle(sd, ns, pix, pooling, bf16):
    sdd = {k: v.detach().to(DEV).requires_grad_() for k, v in sd.items()}
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        emb = eva02_ref.eva_embedding(sdd, ns, pix, pooling)
    return emb.float(), sdd


def _run(cfg, sd, pix, pooling, probe, checkpoint=False, keep=0):
    eng = ViTEngine(cfg, device=DEV, pooling=pooling)
    eng.load_reference_state_dict(sd)
    eng.train()
    if checkpoint:
        eng.gradient_checkpointing_enable(keep_layers=keep)
    emb, arena = eng.forward_chunk(pix, True)
    emb2, _ = eng.forward_chunk(pix, False)
    assert torch.equal(emb, emb2), "no-grad (single slot) forward must equal the saving forward"
    eng.zero_grad()
    eng.backward_chunk(pix, arena, probe)
    return emb, eng.reference_grad_dict(), eng


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_eva02_matches_reference_golden(gold, pooling):
    g, cfg, ns = _tiny(gold)
    sd = eva02_ref.random_state_dict(ns, int(g["seed"]))
    pix = torch.from_numpy(g["pixels"]).to(DEV)
    probe = torch.from_numpy(g[f"{pooling}/probe"]).to(DEV)
    emb, grads, eng = _run(cfg, sd, pix, pooling, probe)
    assert "ln_f.weight" not in grads
    hid = eng.forward_hidden_chunk(pix, False)[0]
    gold_h = torch.from_numpy(g["hidden"]).to(DEV)
    assert rel_err(hid.float(), gold_h) < 2e-2
    gold_emb = torch.from_numpy(g[f"{pooling}/embedding"]).to(DEV)
    emb16, sd16 = _oracle(sd, ns, pix, pooling, True)
    (emb16 * probe).sum().backward()
    e_hip, e_b = max_err(emb, gold_emb), max_err(emb16, gold_emb)
    worst = 0.0
    n_checked = 0
    for k in g.files:
        if not k.startswith(f"{pooling}/gnorm/"):
            continue
        n = k[len(pooling) + 7:]
        want, got, bf = float(g[k]), float(grads[n].norm()), float(sd16[n].grad.norm())
        worst = max(worst, abs(got - want) / max(want, 1e-6))
        n_checked += 1
        assert abs(got - want) <= 3 * abs(bf - want) + 2e-2 * want + 1e-5, f"{n}: |grad| {got} vs reference {want} (bf16 {bf})"
    assert n_checked == len(grads)
    errs = {}
    for k in g.files:
        if not k.startswith(f"{pooling}/g/"):
            continue
        n = k[len(pooling) + 3:]
        name, sl = (n[:-9], 16) if n.endswith("[:16,:16]") else (n, None)
        got = grads[name] if sl is None else grads[name][:sl, :sl]
        errs[n] = rel_err(got.reshape(-1), torch.from_numpy(g[k]).to(DEV).reshape(-1))
    report("eva02_golden", pooling=pooling, e_emb_hip=e_hip, e_emb_bf16=e_b, worst_gnorm_rel=worst,
           **{k: v for k, v in errs.items()})
    assert e_hip <= 5e-3 and e_hip <= 3 * e_b + 1e-4
    assert all(v < 5e-2 for v in errs.values()), errs


@pytest.mark.parametrize("keep", [0, 1])
def test_eva02_checkpointing_is_bit_identical(gold, keep):
    g, cfg, ns = _tiny(gold)
    sd = eva02_ref.random_state_dict(ns, int(g["seed"]))
    pix = torch.from_numpy(g["pixels"]).to(DEV)
    probe = torch.from_numpy(g["cls/probe"]).to(DEV)
    e0, g0, _ = _run(cfg, sd, pix, "cls", probe)
    e1, g1, _ = _run(cfg, sd, pix, "cls", probe, checkpoint=True, keep=keep)
    assert torch.equal(e0, e1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_ext_null_is_bit_identical_to_the_plain_entry_points(gold):
    """cx_vit_*_ex with ext == NULL on the google/vit fixture == cx_vit_forward / cx_vit_backward (and the hidden pair)."""
    g = gold("vit_tiny")
    d = {k[4:]: g[k].item() for k in g.files if k.startswith("cfg/")}
    cfg, ns = ViTConfig(**d), SimpleNamespace(**d)
    sd = vit_ref.random_state_dict(ns, int(g["seed"]))
    pix = torch.from_numpy(g["pixels"]).to(DEV)
    probe = torch.from_numpy(g["cls/probe"]).to(DEV)
    eng = ViTEngine(cfg, device=DEV, pooling="cls")
    eng.load_reference_state_dict(sd)
    eng.train()
    assert eng._ext is None
    B = pix.shape[0]
    Sq = cfg.n_patch + 1
    cu = eng._cu_seqlens(B, Sq)
    lib = eng.lib
    null = C.POINTER(_C.CxVitExt)()
    outs = []
    for ex in (False, True):
        eng.zero_grad()
        arena = eng._get_arena(B * Sq, B, True)
        emb = torch.empty(B, cfg.n_embd, device=DEV)
        args = (pix.data_ptr(), 0, cu.data_ptr(), B, 3, cfg.img_size, cfg.img_size, cfg.patch_size, 1, emb.data_ptr(), S())
        rc = lib.cx_vit_forward_ex(C.byref(eng._desc), C.byref(arena.desc), null, *args) if ex else \
            lib.cx_vit_forward(C.byref(eng._desc), C.byref(arena.desc), *args)
        _C.check(rc, "fwd")
        bargs = (cu.data_ptr(), B, cfg.n_patch, probe.data_ptr(), emb.data_ptr(), S())
        rc = lib.cx_vit_backward_ex(C.byref(eng._desc), C.byref(arena.desc), null, *bargs) if ex else \
            lib.cx_vit_backward(C.byref(eng._desc), C.byref(arena.desc), *bargs)
        _C.check(rc, "bwd")
        hid = torch.empty(B * Sq, cfg.n_embd, dtype=torch.bfloat16, device=DEV)
        hargs = (pix.data_ptr(), 0, cu.data_ptr(), B, 3, cfg.img_size, cfg.img_size, cfg.patch_size, 1, hid.data_ptr(), S())
        rc = lib.cx_vit_forward_hidden_ex(C.byref(eng._desc), C.byref(arena.desc), null, *hargs) if ex else \
            lib.cx_vit_forward_hidden(C.byref(eng._desc), C.byref(arena.desc), *hargs)
        _C.check(rc, "fwd hidden")
        dh = (hid.float() * 0.01).to(torch.bfloat16)
        hbargs = (cu.data_ptr(), B, cfg.n_patch, dh.data_ptr(), S())
        rc = lib.cx_vit_backward_hidden_ex(C.byref(eng._desc), C.byref(arena.desc), null, *hbargs) if ex else \
            lib.cx_vit_backward_hidden(C.byref(eng._desc), C.byref(arena.desc), *hbargs)
        _C.check(rc, "bwd hidden")
        torch.cuda.synchronize()
        outs.append((emb.clone(), hid.clone(), eng.flat_grad.clone()))
        eng.release_arena(arena)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n_layer", [2, 12])
def test_eva02_b16_vs_fp32_restatement(n_layer):
    """EVA-02 B/16 at 224 -- 2 blocks and the full 12 (where errors accumulate through the rotated attention and the sub-LN),
    B = 3, the 3 x bf16-eager rule."""
    cfg = ViTConfig.eva02_base_patch16_224(n_layer=n_layer)
    ns = SimpleNamespace(**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__})
    sd = eva02_ref.random_state_dict(ns, 9)
    gen = torch.Generator().manual_seed(10)
    pix = torch.randn(3, 3, 224, 224, generator=gen).to(DEV)
    probe = torch.randn(3, cfg.n_embd, generator=gen).to(DEV)
    emb, grads, _ = _run(cfg, sd, pix, "mean", probe)
    ref, sd32 = _oracle(sd, ns, pix, "mean", False)
    ref16, sd16 = _oracle(sd, ns, pix, "mean", True)
    (ref * probe).sum().backward()
    (ref16 * probe).sum().backward()
    e_hip, e_b = max_err(emb, ref), max_err(ref16, ref)
    worst, worst_name = 0.0, ""
    for n, gh in grads.items():
        eh = rel_err(gh.reshape(-1), sd32[n].grad.reshape(-1))
        eb = rel_err(sd16[n].grad.float().reshape(-1), sd32[n].grad.reshape(-1))
        if eh / (eb + 1e-4) > worst:
            worst, worst_name = eh / (eb + 1e-4), n
        assert eh <= 3 * (eb + 1e-4), f"{n}: rel grad err {eh:.4f} vs bf16 eager {eb:.4f}"
    report("eva02_b16", n_layer=n_layer, e_emb_hip=e_hip, e_emb_bf16=e_b, worst_grad_ratio=worst, worst_grad_name=worst_name)
    assert e_hip <= 3 * e_b + 1e-4


def test_map_head_on_the_eva02_tower(gold):
    """`pooling: map` of the recipe: the head of a SwiGLU tower is a GatedMLP head (modeling_biencoder.py:107-115); the
    whole BiEncoder vs the fp32 composition (restated tower + head in torch), gradients through cx_vit_backward_hidden_ex."""
    from contrastors_amd.biencoder import BiEncoder, BiEncoderConfig

    g, cfg, ns = _tiny(gold)
    sd = eva02_ref.random_state_dict(ns, int(g["seed"]))
    tower = BiEncoder(BiEncoderConfig(model_name="eva", pooling="map", trunk_config=cfg, gradient_checkpointing=True,
                                      checkpoint_keep_layers=0), device=DEV, seed=4).train()
    tower.trunk.load_reference_state_dict(sd)
    assert hasattr(tower.selector.mlp, "fc11") and tower.selector.mlp.fc11.out_features == 512
    head = {k: v.detach().clone() for k, v in tower.selector.state_dict().items()}
    pix = torch.from_numpy(g["pixels"]).to(DEV)
    probe = torch.randn(pix.shape[0], cfg.n_embd, generator=torch.Generator().manual_seed(3)).to(DEV)
    tower.trunk.zero_grad()
    emb = tower(input_ids=pix)["embedding"]
    (emb * probe).sum().backward()
    assert tower.trunk._outstanding == 0

    def oracle(bf16):
        sdd = {k: v.detach().to(DEV).requires_grad_() for k, v in sd.items()}
        hd = {k: v.detach().float().requires_grad_() for k, v in head.items()}
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            h = eva02_ref.eva_hidden(sdd, ns, pix)
            B, Sq, d = h.shape
            q = (hd["attn.latent"].expand(B, 1, d) @ hd["attn.Wq.weight"].T + hd["attn.Wq.bias"]).view(B, 1, 4, 64)
            kv = (h @ hd["attn.Wkv.weight"].T + hd["attn.Wkv.bias"]).view(B, Sq, 2, 4, 64)
            att = torch.einsum("bqhd,bkhd->bhqk", q, kv[:, :, 0]) / 8.0
            a = torch.einsum("bhqk,bkhd->bqhd", att.float().softmax(-1).to(kv.dtype), kv[:, :, 1]).reshape(B, 1, d)
            a = a @ hd["attn.out_proj.weight"].T + hd["attn.out_proj.bias"]
            n1 = F.layer_norm(a.float(), (d,), hd["norm1.weight"], hd["norm1.bias"], cfg.layer_norm_epsilon)
            y = n1 @ hd["mlp.fc11.weight"].T + hd["mlp.fc11.bias"]
            gt = n1 @ hd["mlp.fc12.weight"].T + hd["mlp.fc12.bias"]
            m = (F.silu(gt.float()) * y.float()) @ hd["mlp.fc2.weight"].T + hd["mlp.fc2.bias"]
            e = F.normalize((h[:, :1].float() + m.float())[:, 0], dim=-1)
        (e.float() * probe).sum().backward()
        return e.float(), sdd

    ref, sd32 = oracle(False)
    ref16, sd16 = oracle(True)
    e_hip, e_b = max_err(emb, ref), max_err(ref16, ref)
    report("eva02_map", e_emb_hip=e_hip, e_emb_bf16=e_b)
    assert e_hip <= 3 * e_b + 1e-4 and e_hip < 1e-2, (e_hip, e_b)
    grads = tower.trunk.reference_grad_dict()
    for n, gh in grads.items():
        eh, eb = rel_err(gh.reshape(-1), sd32[n].grad.reshape(-1)), rel_err(sd16[n].grad.float().reshape(-1), sd32[n].grad.reshape(-1))
        assert eh <= 3 * eb + 1e-2, f"{n}: rel grad err {eh:.4f} vs bf16 eager {eb:.4f}"


def _eva_map_embedding(sd, head, ns, pix, n_head, eps):
    """torch composition of BiEncoder(EVA-02 trunk, pooling: map): the restated tower, then the attention-pooling head with a
    SwiGLU MLP (modeling_biencoder.py:93-156), then L2 normalisation."""
    h = eva02_ref.eva_hidden(sd, ns, pix)
    B, Sq, d = h.shape
    q = (head["attn.latent"].expand(B, 1, d) @ head["attn.Wq.weight"].T + head["attn.Wq.bias"]).view(B, 1, n_head, 64)
    kv = (h @ head["attn.Wkv.weight"].T + head["attn.Wkv.bias"]).view(B, Sq, 2, n_head, 64)
    att = torch.einsum("bqhd,bkhd->bhqk", q, kv[:, :, 0]) / 8.0
    a = torch.einsum("bhqk,bkhd->bqhd", att.float().softmax(-1).to(kv.dtype), kv[:, :, 1]).reshape(B, 1, d)
    a = a @ head["attn.out_proj.weight"].T + head["attn.out_proj.bias"]
    n1 = F.layer_norm(a.float(), (d,), head["norm1.weight"], head["norm1.bias"], eps)
    y = n1 @ head["mlp.fc11.weight"].T + head["mlp.fc11.bias"]
    gt = n1 @ head["mlp.fc12.weight"].T + head["mlp.fc12.bias"]
    m = (F.silu(gt.float()) * y.float()) @ head["mlp.fc2.weight"].T + head["mlp.fc2.bias"]
    return F.normalize((h[:, :1].float() + m.float())[:, 0], dim=-1)


def test_lit_training_step_of_the_recipe_shape():
    """nomic-embed-vision-v1.5 in miniature through ImageTextTrainer: EVA-02 image tower (tiny sizes) with `pooling: map` and
    gradient checkpointing, a frozen nomic text tower, batch 16.  (1) One forward / backward of the trainer vs the torch
    composition of the same step (fp32 towers, symmetric InfoNCE at the logit scale), with the 3 x bf16-eager rule on every
    image-tower and head gradient; (2) the MLP LayerNorms sit in the no-decay group; (3) a few steps lower the loss, the frozen
    text tower does not move, the image tower (its mlp.norm included) does."""
    from contrastors_amd.config import Config, DataArgs, ModelArgs, TrainArgs
    from contrastors_amd.nomic_bert import NomicBertConfig
    from contrastors_amd.trainers import ImageTextTrainer
    from oracle import encoder_ref
    from oracle.make_golden import TINY_NOMIC

    cfg = Config(train_args=TrainArgs(learning_rate=2e-3, weight_decay=0.01, warmup_steps=0, grad_cache=False,
                                      schedule_type="linear", max_grad_norm=1.0, clamp_logits=True, checkpoint_keep_layers=0),
                 data_args=DataArgs(batch_size=16, seed=7),
                 text_model_args=ModelArgs(logit_scale=20.0, pooling="mean", model_name="tiny-text", freeze=True),
                 vision_model_args=ModelArgs(logit_scale=20.0, pooling="map", model_name="tiny-eva", freeze=False,
                                             trainable_logit_scale=True, gradient_checkpointing=True))
    tc = NomicBertConfig(**{k: v for k, v in TINY_NOMIC.items() if k in NomicBertConfig.__dataclass_fields__})
    vc = ViTConfig.eva02_base_patch16_224(n_embd=256, n_head=4, n_layer=2, n_inner=512, img_size=32, patch_size=8)
    tr = ImageTextTrainer(cfg, torch.bfloat16, device=DEV, text_trunk_config=tc, vision_trunk_config=vc, total_steps=20)
    m = tr.model["model"]
    vis, txt = m.vision, m.text
    assert vis.trunk.gradient_checkpointing and txt.frozen_trunk and vis.trunk._ext is not None
    gen = torch.Generator().manual_seed(3)
    n = 16
    ids = torch.randint(3, 512, (n, 24), generator=gen)
    mask = torch.ones(n, 24, dtype=torch.long)
    pix = torch.randn(n, 3, 32, 32, generator=gen)
    batch = {"text": {"input_ids": ids, "attention_mask": mask}, "vision": {"input_ids": pix}}

    # (1) one forward / backward vs the torch composition
    vsd = {k: v.detach().float().clone() for k, v in vis.trunk.reference_state_dict().items()}
    head = {k: v.detach().float().clone() for k, v in vis.selector.state_dict().items()}
    tsd = {k: v.detach().float().clone() for k, v in txt.trunk.reference_state_dict().items()}
    scale = float(m.logit_scale.logit_scale.detach().exp())
    tr._zero_grads()
    out = tr.forward_step(batch)
    tr.backward(out)
    torch.cuda.synchronize()
    g_trunk = {k: v.clone() for k, v in vis.trunk.reference_grad_dict().items()}
    g_head = {k: p.grad.detach().float().clone() for k, p in vis.selector.named_parameters()}
    assert float(txt.trunk.flat_grad.abs().max()) == 0.0
    with torch.no_grad():
        te = encoder_ref.biencoder_embedding(tsd, SimpleNamespace(**TINY_NOMIC), ids.to(DEV), mask.to(DEV)).float()
    pixd = pix.to(DEV)
    labels = torch.arange(n, device=DEV)

    def composition(bf16):
        # (fresh leaves per call: the two compositions must not accumulate into the same .grad)
        sdd = {k: v.detach().clone().to(DEV).requires_grad_() for k, v in vsd.items()}
        hd = {k: v.detach().clone().to(DEV).requires_grad_() for k, v in head.items()}
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            ve = _eva_map_embedding(sdd, hd, SimpleNamespace(**{k: getattr(vc, k) for k in vc.__dataclass_fields__}), pixd,
                                    vc.n_head, vc.layer_norm_epsilon).float()
        loss = 0.5 * (F.cross_entropy(scale * ve @ te.T, labels) + F.cross_entropy(scale * te @ ve.T, labels))
        loss.backward()
        return float(loss), sdd, hd

    l32, sd32, hd32 = composition(False)
    l16, sd16, hd16 = composition(True)
    e_loss = abs(float(out["loss"].detach()) - l32)
    worst = 0.0
    for mine, r32, r16, what in ((g_trunk, sd32, sd16, "trunk"), (g_head, hd32, hd16, "selector")):
        for k, gh in mine.items():
            eh = rel_err(gh.reshape(-1), r32[k].grad.reshape(-1))
            eb = rel_err(r16[k].grad.float().reshape(-1), r32[k].grad.reshape(-1))
            worst = max(worst, eh / (eb + 1e-4))
            assert eh <= 3 * eb + 1e-2, f"{what}.{k}: rel grad err {eh:.4f} vs bf16 eager {eb:.4f}"
    report("eva02_lit_step", loss=float(out["loss"].detach()), ref=l32, ref_bf16=l16, e_loss=e_loss, worst_grad_ratio=worst)
    assert e_loss < 2e-2 and e_loss <= 3 * abs(l16 - l32) + 2e-3

    # (2) decay groups over the flat buffers: mlp.norm.* in the no-decay segment, pos_embed in the decay one
    lay = vis.trunk._layout
    assert lay["layers.0.mlp.norm.weight"][0] >= vis.trunk.n_decay and lay["layers.1.mlp.norm.bias"][0] >= vis.trunk.n_decay
    assert lay["embeddings.pos_embed"][0] < vis.trunk.n_decay
    wd = {id(p): grp["weight_decay"] for grp in tr.optimizer.param_groups for p in grp["params"]}
    assert wd[id(vis.trunk.flat_nodecay)] == 0.0 and wd[id(vis.trunk.flat_decay)] == 0.01

    # (3) training
    tr._zero_grads()
    v0, t0 = vis.trunk.flat_param.clone(), txt.trunk.flat_param.clone()
    norm0 = vis.trunk.p("layers.0.mlp.norm.weight").clone()
    losses = [float(tr.training_step(batch)) for _ in range(6)]
    assert all(x == x for x in losses) and losses[-1] < losses[0] - 0.05, losses
    assert torch.equal(txt.trunk.flat_param, t0)
    assert float((vis.trunk.flat_param - v0).abs().max()) > 0
    assert not torch.equal(vis.trunk.p("layers.0.mlp.norm.weight"), norm0)


def _to_timm(sd, cfg):
    """Reference keys -> the timm EVA-02 layout (q / v biases without a k bias, fc1_x / fc1_g, a 4-D patch kernel), plus the
    classifier keys a timm checkpoint carries."""
    d, p = cfg.n_embd, cfg.patch_size
    out = {"cls_token": sd["embeddings.cls_token"], "pos_embed": sd["embeddings.pos_embed"],
           "patch_embed.proj.weight": sd["embeddings.proj.weight"].reshape(d, cfg.num_channels, p, p),
           "patch_embed.proj.bias": sd["embeddings.proj.bias"], "head.weight": torch.zeros(7, d), "head.bias": torch.zeros(7),
           "fc_norm.weight": torch.ones(d), "fc_norm.bias": torch.zeros(d)}
    names = {"attn.out_proj": "attn.proj", "mlp.fc11": "mlp.fc1_x", "mlp.fc12": "mlp.fc1_g", "mlp.fc2": "mlp.fc2",
             "mlp.norm": "mlp.norm", "norm1": "norm1", "norm2": "norm2"}
    for l in range(cfg.n_layer):
        a, b = f"layers.{l}.", f"blocks.{l}."
        out[b + "attn.qkv.weight"] = sd[a + "attn.Wqkv.weight"]
        out[b + "attn.q_bias"] = sd[a + "attn.Wqkv.bias"][:d]
        out[b + "attn.v_bias"] = sd[a + "attn.Wqkv.bias"][2 * d:]
        for ours, theirs in names.items():
            for w in ("weight", "bias"):
                out[f"{b}{theirs}.{w}"] = sd[f"{a}{ours}.{w}"]
    return {k: v.contiguous().clone() for k, v in out.items()}


def test_timm_eva02_checkpoint_directory_loads(tmp_path, gold):
    """A local timm-keyed EVA-02 checkpoint (model.safetensors or pytorch_model.bin) into the tower, through the trainer's
    initial-weights path for `pretrained: true`: every parameter lands (k bias zero, as the reference's remap makes it); a key
    the tower has no parameter for, or a missing one, raises."""
    from safetensors.torch import save_file

    from contrastors_amd.biencoder import BiEncoder, BiEncoderConfig
    from contrastors_amd.trainers import _load_initial_weights, load_timm_eva02

    _, cfg, ns = _tiny(gold)
    sd = eva02_ref.random_state_dict(ns, 17)
    d = cfg.n_embd
    for l in range(cfg.n_layer):
        sd[f"layers.{l}.attn.Wqkv.bias"][d:2 * d] = 0.0
    timm = _to_timm(sd, cfg)
    st_dir, bin_dir = tmp_path / "st", tmp_path / "bin"
    st_dir.mkdir()
    bin_dir.mkdir()
    save_file(timm, str(st_dir / "model.safetensors"))
    torch.save(timm, str(bin_dir / "pytorch_model.bin"))
    for where in (st_dir, bin_dir):
        tower = BiEncoder(BiEncoderConfig(model_name=str(where), pooling="cls", trunk_config=cfg), device=DEV, seed=1)
        _load_initial_weights(tower, SimpleNamespace(checkpoint=None, pretrained=True, model_name=str(where)), explicit_arch=False)
        got = tower.trunk.reference_state_dict()
        assert set(got) == set(sd)
        for k, v in sd.items():
            assert torch.equal(got[k].cpu(), v.float()), k
    eng = tower.trunk
    extra = dict(timm, **{"blocks.0.ls1.gamma": torch.ones(d)})
    bad = tmp_path / "extra"
    bad.mkdir()
    save_file(extra, str(bad / "model.safetensors"))
    with pytest.raises(KeyError):
        load_timm_eva02(eng, str(bad))
    missing = {k: v for k, v in timm.items() if k != "blocks.1.mlp.norm.bias"}
    bad2 = tmp_path / "missing"
    bad2.mkdir()
    save_file(missing, str(bad2 / "model.safetensors"))
    with pytest.raises(KeyError):
        load_timm_eva02(eng, str(bad2))
