"""Same-box A/B of whole LIBRARIES (the product .so against variants built by scripts/build_variant.py, or any other build of
the library given by path) on isolated launches of the step's kernels: every library is loaded side by side (ctypes), rounds are
interleaved (lib A, lib B, ..., lib A, ...) so that clock / power drift of the box hits all of them alike, and every library's
output is compared with the first library's (bit-identical or the max relative difference).  usage:
    python scripts/lib_ab.py [--libs base,hi1,hi2] [--cases swiglu_bwd,attn_bwd] [--chunk 2048] [--rounds 7] [--reps 6]
    python scripts/lib_ab.py --libs /path/to/parent.so,/path/to/parent_copy.so,base --cases ln_fwd,ln_bwd_ws [--width 768]
`base` = contrastors_amd/lib/libcontrastors_hip.so; a name with a `/` is the path of a .so; any other name N =
contrastors_amd/lib/variants/libcontrastors_hip_N.so.  Two copies of one build among the libraries give the yardstick for the
others: the ratio between them, and the `spread` column (max - min over the median of the first library's per-round times), are
what the box cannot tell from no change.  Operands are allocated only for the groups of cases selected (GEMM, attention, LayerNorm,
glue kernels).
The LayerNorm cases run at T = chunk * 128 rows of --width columns (the metric's 262144 x 768 by default) and report the bytes they
must move as TB/s; each lists only its deterministic outputs (the atomically accumulated vectors are held to bounds by
tests/test_layernorm_edges_gpu.py).  The glue cases (elementwise.hip, eva.hip, vit.hip, xent.hip, optimizer.hip) run at the step's
sizes too (T rows of I = 3072 or d = 768; cross-entropy on T / 8 rows of the 30528-way MLM vocabulary; AdamW on the parameter count
of nomic-bert-2048) and report TB/s; cx_bias_grad and cx_grad_sq_norm accumulate atomically and are timed only.
    python scripts/lib_ab.py --libs /path/to/parent.so,/path/to/parent_copy.so,base --cases glue"""
import argparse
import ctypes as C
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from contrastors_amd import _C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--libs", type=str, default="base")
ap.add_argument("--cases", type=str, default="")
ap.add_argument("--chunk", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--seq", type=int, default=128)
ap.add_argument("--rotary", type=int, default=1, help="0: no rotation tables (pre-rotated long sequences, image towers)")
ap.add_argument("--width", type=int, default=768, help="LayerNorm cases: row width (256, 512, 768 or 1024)")
a = ap.parse_args()


def load(name):
    path = _C.LIB_PATH if name == "base" else Path(name) if "/" in name else _C.LIB_PATH.parent / "variants" / f"libcontrastors_hip_{name}.so"
    h = C.CDLL(str(path))
    for fn, (res, args) in _C._SIGS.items():
        if hasattr(h, fn):
            f = getattr(h, fn)
            f.restype, f.argtypes = res, args
    return h


names = a.libs.split(",")
labels = {n: Path(n).stem if "/" in n else n for n in names}
libs = {n: load(n) for n in names}
dev = "cuda"
s = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *sh, std=1.0: (torch.randn(*sh, device=dev, generator=g) * std).bfloat16()   # noqa: E731
rf = lambda *sh, std=1.0: torch.randn(*sh, device=dev, generator=g) * std   # noqa: E731
P = lambda t: None if t is None else t.data_ptr()   # noqa: E731
E = lambda *sh, dt=torch.bfloat16: torch.empty(*sh, device=dev, dtype=dt)   # noqa: E731
T, d, I, H, S = a.chunk * 128, 768, 3072, 12, a.seq


# Every group: name -> (work, outputs to compare, call(lib)[, prep()]).  work = flop (GEMM, attention: the TF column) or bytes
# (LayerNorm: TB/s); the outputs are zeroed, then prep() (if any) restores what the call overwrites, before each compared call.
def gemm_cases():
    x, res = rn(T, d), rn(T, d)
    w1, w2t, w2, wo, wqkv = rn(2 * I, d, std=0.05), rn(I, d, std=0.05), rn(d, I, std=0.05), rn(d, d, std=0.05), rn(3 * d, d, std=0.05)
    act, gate = rn(T, I), rn(T, I, std=2.0)
    x3, wqkv_t = rn(T, 3 * d), rn(d, 3 * d, std=0.05)
    x6, w1_t = rn(T, 2 * I), rn(d, 2 * I, std=0.05)
    dyg, out_d, out_3d, out_I, gs = E(T, 2 * I), E(T, d), E(T, 3 * d), E(T, I), E(T, I)
    return {
        "swiglu_bwd": (2.0 * T * I * d, [dyg], lambda L: L.cx_gemm_bf16_swiglu_bwd_gate(P(x), P(w2t), P(act), P(gate), P(dyg), T, I, d, d, d, I, 2 * I, s)),
        "swiglu_fwd_save": (2.0 * T * 2 * I * d, [gs, out_I], lambda L: L.cx_gemm_bf16_swiglu_gate(P(x), P(w1), P(gs), P(out_I), T, I, d, d, d, I, I, s)),
        "swiglu_fwd": (2.0 * T * 2 * I * d, [out_I], lambda L: L.cx_gemm_bf16_swiglu_gate(P(x), P(w1), None, P(out_I), T, I, d, d, d, I, I, s)),
        "qkv_fwd": (2.0 * T * 3 * d * d, [out_3d], lambda L: L.cx_gemm_bf16_nt(P(x), P(wqkv), P(out_3d), None, T, 3 * d, d, d, d, 3 * d, 0, 1, 1.0, s)),
        "out_dgrad": (2.0 * T * d * d, [out_d], lambda L: L.cx_gemm_bf16_nt(P(x), P(wo), P(out_d), None, T, d, d, d, d, d, 0, 1, 1.0, s)),
        "out_fwd_res": (2.0 * T * d * d, [out_d], lambda L: L.cx_gemm_bf16_nt_residual(P(x), P(wo), P(out_d), None, P(res), T, d, d, d, d, d, d, s)),
        "fc2_fwd_res": (2.0 * T * I * d, [out_d], lambda L: L.cx_gemm_bf16_nt_residual(P(act), P(w2), P(out_d), None, P(res), T, d, I, I, I, d, d, s)),
        "qkv_dgrad_res": (2.0 * T * 3 * d * d, [out_d], lambda L: L.cx_gemm_bf16_nt_residual(P(x3), P(wqkv_t), P(out_d), None, P(res), T, d, 3 * d, 3 * d, 3 * d, d, d, s)),
        "fc1_dgrad_res": (2.0 * T * 2 * I * d, [out_d], lambda L: L.cx_gemm_bf16_nt_residual(P(x6), P(w1_t), P(out_d), None, P(res), T, d, 2 * I, 2 * I, 2 * I, d, d, s)),
    }


def attn_cases():
    # attention (S <= 128 single-pass kernels at S = 128; ragged: lengths 64..128)
    B = T // S
    qkv = rn(T, 3 * H * 64, std=0.5)
    cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=dev)
    inv = 1.0 / (1000.0 ** (torch.arange(0, 64, 2, dtype=torch.float32) / 64))
    fr = torch.outer(torch.arange(max(S, 128), dtype=torch.float32), inv)
    cos, sin = torch.cos(fr).to(dev).contiguous(), torch.sin(fr).to(dev).contiguous()
    if not a.rotary:
        cos = sin = None
    att_out, lse, dout = E(T, H * 64), E(H * T, dt=torch.float32), rn(T, H * 64)
    dqkv, delta = torch.empty_like(qkv), E(H * T, dt=torch.float32)
    lens = torch.randint(S // 2, S + 1, (B,), generator=torch.Generator().manual_seed(1))
    cu_r = torch.zeros(B + 1, dtype=torch.int32)
    cu_r[1:] = lens.cumsum(0)
    cu_r = cu_r.to(dev)
    T_r = int(lens.sum())

    def fwd_first(ragged):   # the inputs of a backward: a forward of the first library on the same sequences
        return lambda: libs[names[0]].cx_attn_varlen_fwd(P(qkv), P(cu_r if ragged else cu), P(cos), P(sin), P(att_out), P(lse), B, H,
                                                         T_r if ragged else T, S, 0.125, s)

    def delta_first():   # delta = rowsum(dO * O) into `delta` (H, T): the general (max_seqlen > 128) path computes it first
        fwd_first(False)()
        assert libs[names[0]].cx_attn_varlen_bwd(P(dout), P(qkv), P(att_out), P(lse), P(cu), P(cos), P(sin), P(delta), P(dqkv), B, H, T, S + 1, 0.125, s) == 0
        torch.cuda.synchronize()

    bwd = lambda L: L.cx_attn_varlen_bwd(P(dout), P(qkv), P(att_out), P(lse), P(cu), P(cos), P(sin), P(delta), P(dqkv), B, H, T, S, 0.125, s)   # noqa: E731
    return {
        "attn_fwd": (4.0 * S * S * 64 * B * H, [att_out, lse], lambda L: L.cx_attn_varlen_fwd(P(qkv), P(cu), P(cos), P(sin), P(att_out), P(lse), B, H, T, S, 0.125, s)),
        "attn_bwd": (10.0 * S * S * 64 * B * H, [dqkv], bwd, None, fwd_first(False)),
        # (A/B of CX_ATTN_DELTA_IN builds: `delta` is filled beforehand by the first library's general kernels)
        "attn_bwd_dpre": (10.0 * S * S * 64 * B * H, [dqkv], bwd, None, delta_first),
        "attn_bwd_drop": (10.0 * S * S * 64 * B * H, [dqkv], lambda L: L.cx_attn_varlen_dropout_bwd(P(dout), P(qkv), P(att_out), P(lse), P(cu), P(cos), P(sin), P(delta), P(dqkv), B, H, T, S, 0.125, 0.1, 1234, 0, 0, s), None, fwd_first(False)),
        "attn_fwd_drop": (4.0 * S * S * 64 * B * H, [att_out, lse], lambda L: L.cx_attn_varlen_dropout_fwd(P(qkv), P(cu), P(cos), P(sin), P(att_out), P(lse), B, H, T, S, 0.125, 0.1, 1234, 0, 0, s)),
        "attn_bwd_ragged": (0.0, [dqkv], lambda L: L.cx_attn_varlen_bwd(P(dout), P(qkv), P(att_out), P(lse), P(cu_r), P(cos), P(sin), P(delta), P(dqkv), B, H, T_r, S, 0.125, s), None, fwd_first(True)),
    }


def ln_cases():
    w = a.width
    f32 = torch.float32
    x, r, dout = rn(T, w), rn(T, w), rn(T, w)
    gam, bet = 1 + rf(w, std=0.1), rf(w, std=0.1)
    out, z, dz, dx0 = E(T, w), E(T, w), E(T, w), E(T, w)
    mean_o, rstd_o, mean, rstd = E(T, dt=f32), E(T, dt=f32), E(T, dt=f32), E(T, dt=f32)
    dg, db, cs = E(w, dt=f32), E(w, dt=f32), E(w, dt=f32)
    ws = E(3 * w * 768, dt=f32)
    # the backward cases take x as the stored z, with the first library's statistics of it
    assert libs[names[0]].cx_layernorm_fwd(P(x), None, P(gam), P(bet), P(out), None, P(mean), P(rstd), T, w, 1e-12, s) == 0
    Bq = T // 128                                         # pooled: sequences of 128 rows
    demb, emb, norm = rf(Bq, w), torch.nn.functional.normalize(rf(Bq, w), dim=-1), 0.5 + torch.rand(Bq, device=dev, generator=g)
    cu = torch.arange(0, (Bq + 1) * 128, 128, dtype=torch.int32, device=dev)
    xf, rf_, doutf = x.float(), r.float(), dout.float()   # mixed kernels, every operand fp32
    outf, zf = E(T, w, dt=f32), E(T, w, dt=f32)
    ALL_F32 = 1 | 2 | 4 | 8
    vocab = 30528                                         # embedding: every slot a token, positions 0 .. 127
    ids = torch.randint(0, vocab, (Bq, 128), device=dev, generator=g)
    idx = torch.arange(T, dtype=torch.int32, device=dev)
    word, type_e, pos_e = rf(vocab, w, std=0.5), rf(2, w, std=0.5), rf(128, w, std=0.5)
    sids, perm = torch.sort(ids.flatten().to(torch.int32), stable=True)
    perm = perm.to(torch.int32)
    dword, scratch, dt0, dpos = E(vocab, w, dt=f32), E(T, w, dt=f32), torch.zeros(w, device=dev), torch.zeros(128, w, device=dev)
    inplace = E(T, w)
    Bt, n_ws = 2.0 * T * w, ws.numel()                    # bytes of one bf16 (T, w) operand
    DROP = (0.1, 1234, 0, 3)
    return {
        "ln_fwd": (2 * Bt, [out, mean_o, rstd_o], lambda L: L.cx_layernorm_fwd(P(x), None, P(gam), P(bet), P(out), None, P(mean_o), P(rstd_o), T, w, 1e-12, s)),
        "ln_fwd_res_z": (4 * Bt, [out, z, mean_o, rstd_o], lambda L: L.cx_layernorm_fwd(P(x), P(r), P(gam), P(bet), P(out), P(z), P(mean_o), P(rstd_o), T, w, 1e-12, s)),
        "ln_bwd_ws": (3 * Bt, [dz, dg, db], lambda L: L.cx_layernorm_bwd(P(dout), None, P(x), P(gam), P(mean), P(rstd), None, P(dz), P(dg), P(db), P(ws), n_ws, T, w, s)),
        "ln_bwd_colsum_ws": (3 * Bt, [dz, dg, db, cs], lambda L: L.cx_layernorm_bwd_colsum(P(dout), None, P(x), P(gam), P(mean), P(rstd), None, P(dz), P(dg), P(db), P(cs), P(ws), n_ws, T, w, s)),
        "ln_bwd_atomics": (3 * Bt, [dz], lambda L: L.cx_layernorm_bwd(P(dout), None, P(x), P(gam), P(mean), P(rstd), None, P(dz), P(dg), P(db), None, 0, T, w, s)),
        "ln_pooled_ws": (2 * Bt, [dz, dg, db, cs], lambda L: L.cx_layernorm_bwd_pooled(P(demb), P(emb), P(norm), P(cu), Bq, 0, 1, P(x), P(gam), P(mean), P(rstd), P(dz), P(dg), P(db), P(cs), P(ws), n_ws, T, w, s)),
        "ln_drop_fwd": (4 * Bt, [out, z, mean_o, rstd_o], lambda L: L.cx_dropout_add_layernorm_fwd(P(x), P(r), P(gam), P(bet), P(out), P(z), P(mean_o), P(rstd_o), T, w, 1e-12, *DROP, s)),
        "ln_drop_bwd_colsum_ws": (4 * Bt, [dz, dx0, dg, db, cs], lambda L: L.cx_dropout_add_layernorm_bwd_colsum(P(dout), None, P(x), P(gam), P(mean), P(rstd), P(dz), P(dx0), P(dg), P(db), P(cs), P(ws), n_ws, T, w, *DROP, s)),
        "ln_mixed_fwd_f32": (8 * Bt, [outf, zf, mean_o, rstd_o], lambda L: L.cx_layernorm_fwd_mixed(P(xf), P(rf_), P(gam), P(bet), P(outf), P(zf), P(mean_o), P(rstd_o), T, w, 1e-12, ALL_F32, s)),
        "ln_mixed_bwd_f32": (8 * Bt, [outf, zf], lambda L: L.cx_layernorm_bwd_mixed(P(doutf), P(xf), P(gam), P(mean), P(rstd), None, P(outf), P(zf), P(dg), P(db), T, w, ALL_F32, s)),
        # word rows in fp32 (2 Bt) -> out; backward: dout + word rows -> fp32 row gradients (2 Bt), read back by the scatter
        "embed_fwd": (3 * Bt, [out, mean_o, rstd_o], lambda L: L.cx_embed_ln_fwd(P(ids), P(idx), P(word), P(type_e), P(pos_e), P(gam), P(bet), P(out), P(mean_o), P(rstd_o), T, 128, w, 1e-12, s)),
        "embed_bwd_sorted": (7 * Bt, [scratch, dword], lambda L: L.cx_embed_ln_bwd_sorted(P(dout), None, P(ids), P(idx), P(word), P(type_e), P(pos_e), P(gam), P(mean), P(rstd), P(dword), P(dt0), P(dpos), P(dg), P(db), T, 128, w, 0, vocab, P(sids), P(perm), P(scratch), s)),
        "dropout_scale": (2 * Bt, [inplace], lambda L: L.cx_dropout_scale(P(inplace), T * w, *DROP, s), lambda: inplace.copy_(x)),
    }


def glue_cases():
    f32, i32 = torch.float32, torch.int32
    L0 = libs[names[0]]
    Bt, Bd = 2.0 * T * I, 2.0 * T * d                     # bytes of one bf16 (T, I) / (T, d) operand
    yg, dact, pre, gate = rn(T, 2 * I), rn(T, I), rn(T, I), rn(T, I, std=2.0)
    act, bias = E(T, I), rf(I, std=0.1)
    assert L0.cx_swiglu_fwd(P(yg), P(act), T, I, 1, s) == 0   # the (act, gate) pair of the gate-saving backward
    dyg, o_I = E(T, 2 * I), E(T, I)
    # casts and transposes: the fc1 weight (2I, d) and its 12 layers in one batched launch; the bf16 transpose on (T, d)
    w32, x = rf(2 * I, d, std=0.05), rn(T, d)
    wbf, w_back, wt, wt32, xt = E(2 * I, d), E(2 * I, d, dt=f32), E(d, 2 * I), E(d, 2 * I, dt=f32), E(d, T)
    w12, wt12 = [rf(2 * I, d, std=0.05) for _ in range(12)], [E(d, 2 * I) for _ in range(12)]
    jobs = torch.zeros(12, 3, dtype=torch.int64)
    for k in range(12):
        jobs[k, 0], jobs[k, 1], jobs[k, 2] = w12[k].data_ptr(), wt12[k].data_ptr(), (2 * I) | (d << 32)
    jobs, tiles = jobs.to(dev), ((2 * I + 63) // 64) * ((d + 63) // 64)
    assert L0.cx_cast_f32_to_bf16(P(w32), P(wbf), w32.numel(), s) == 0
    wbf0 = wbf.clone()
    Wb = 4.0 * w32.numel()
    # pooling and rotary: sequences of 128 tokens
    Bq = T // 128
    cu = torch.arange(0, (Bq + 1) * 128, 128, dtype=i32, device=dev)
    emb, norm, demb, dh = E(Bq, d, dt=f32), E(Bq, dt=f32), rf(Bq, d), E(T, d)
    assert L0.cx_pool_normalize_fwd(P(x), P(cu), P(emb), P(norm), Bq, d, 0, 1, s) == 0
    emb0, norm0 = emb.clone(), norm.clone()
    inv = 1.0 / (1000.0 ** (torch.arange(0, 64, 2, dtype=f32) / 64))
    fr = torch.outer(torch.arange(128, dtype=f32), inv)
    cos, sin = torch.cos(fr).to(dev).contiguous(), torch.sin(fr).to(dev).contiguous()
    qkv0 = rn(T, 3 * d, std=0.5)
    qkv = qkv0.clone()
    # EVA-02: sequences of 1 + 256 tokens, 2-D rotary tables of 256 rows; SwiGLU + sub-LayerNorm at I
    Be = T // 257
    Te = Be * 257
    cu_e = torch.arange(0, (Be + 1) * 257, 257, dtype=i32, device=dev)
    cs2, sn2 = torch.cos(rf(256, 32)).contiguous(), torch.sin(rf(256, 32)).contiguous()
    gam, bet = 1 + rf(I, std=0.1), rf(I, std=0.1)
    g_o, a_o, z_o, mean, rstd = E(T, I), E(T, I), E(T, I), E(T, dt=f32), E(T, dt=f32)
    assert L0.cx_swiglu_subln_fwd(P(yg), P(gam), P(bet), P(g_o), P(a_o), P(z_o), P(mean), P(rstd), T, I, 1e-6, s) == 0
    sa, sg, sm, sr = a_o.clone(), g_o.clone(), mean.clone(), rstd.clone()
    dgam, dbet, dbias = E(I, dt=f32), E(I, dt=f32), E(2 * I, dt=f32)
    ws = E(1024 * 4 * I, dt=f32)
    # ViT-B/16 front end: 224 x 224 images, 196 patches of 768 features
    Bv = max(T // 256, 1)
    pix, patches = rf(Bv, 3, 224, 224), E(Bv * 196, 768)
    proj, cls, pos, seq = rn(Bv * 196, d), rf(d), rf(197, d), E(Bv * 197, d)
    dzv, dproj, gcls, gpos = rn(Bv * 197, d), E(Bv * 196, d), E(d, dt=f32), E(197, d, dt=f32)
    # cross-entropy: T / 8 rows of the MLM vocabulary
    N, V = max(T // 8, 1), 30528
    logits, labels = rn(N, V, std=2.0), torch.randint(0, V, (N,), device=dev, generator=g)
    labels[::7] = -100
    loss, lse, dloss, dlogits = E(N, dt=f32), E(N, dt=f32), rf(N), E(N, V)
    assert L0.cx_xent_fwd(P(logits), 1, P(labels), P(loss), P(lse), N, V, V, 1.0, -100, s) == 0
    lse0 = lse.clone()
    # optimizer: the 136.7 M parameters of nomic-bert-2048 (+ 3: the scalar tail runs)
    n = 136_700_003
    p0, gr, m0, v0 = rf(n, std=0.05), rf(n, std=0.01), rf(n, std=3e-3), rf(n, std=0.01) ** 2
    pw, mw, vw, ema = p0.clone(), m0.clone(), v0.clone(), p0.clone()
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    assert L0.cx_grad_sq_norm(P(gr), n, P(sq), s) == 0
    sq_acc = torch.zeros(1, dtype=torch.float64, device=dev)

    def restore(*pairs):
        return lambda: [dst.copy_(src) for dst, src in pairs]

    return {
        "swiglu_fwd_ew": (3 * Bt, [o_I], lambda L: L.cx_swiglu_fwd(P(yg), P(o_I), T, I, 1, s)),
        "swiglu_bwd_ew": (5 * Bt, [dyg], lambda L: L.cx_swiglu_bwd(P(dact), P(yg), P(dyg), T, I, 1, s)),
        "swiglu_bwd_gate_ew": (5 * Bt, [dyg], lambda L: L.cx_swiglu_bwd_gate(P(dact), P(act), P(gate), P(dyg), T, I, s)),
        "bias_gelu_fwd": (2 * Bt, [o_I], lambda L: L.cx_bias_act_fwd(P(pre), P(bias), P(o_I), T, I, 0, s)),
        "bias_qgelu_fwd": (2 * Bt, [o_I], lambda L: L.cx_bias_act_fwd(P(pre), P(bias), P(o_I), T, I, 1, s)),
        "bias_gelu_bwd": (3 * Bt, [o_I], lambda L: L.cx_bias_gelu_bwd(P(dact), P(pre), P(bias), P(o_I), T, I, s)),
        "bias_gelu_bwd_colsum": (3 * Bt, [o_I], lambda L: L.cx_bias_act_bwd_colsum(P(dact), P(pre), P(bias), P(o_I), P(dbet), T, I, 0, s)),
        "bias_qgelu_bwd_colsum": (3 * Bt, [o_I], lambda L: L.cx_bias_act_bwd_colsum(P(dact), P(pre), P(bias), P(o_I), P(dbet), T, I, 1, s)),
        "bias_grad": (Bt, [], lambda L: L.cx_bias_grad(P(dact), P(dbet), T, I, I, s)),
        "cast_f32_bf16": (1.5 * Wb, [wbf], lambda L: L.cx_cast_f32_to_bf16(P(w32), P(wbf), w32.numel(), s)),
        "cast_bf16_f32": (1.5 * Wb, [w_back], lambda L: L.cx_cast_bf16_to_f32(P(wbf0), P(w_back), w32.numel(), s)),
        "cast_transpose": (1.5 * Wb, [wt], lambda L: L.cx_cast_transpose_f32_to_bf16(P(w32), P(wt), 2 * I, d, s)),
        "cast_transpose_x12": (18 * Wb, wt12, lambda L: L.cx_cast_transpose_f32_to_bf16_batched(P(jobs), 12, tiles, s)),
        "transpose_bf16": (2 * Bd, [xt], lambda L: L.cx_transpose_bf16(P(x), P(xt), T, d, d, T, T, s)),
        "transpose_f32": (2 * Wb, [wt32], lambda L: L.cx_transpose_f32(P(w32), P(wt32), 2 * I, d, d, 2 * I, s)),
        "pool_fwd": (Bd, [emb, norm], lambda L: L.cx_pool_normalize_fwd(P(x), P(cu), P(emb), P(norm), Bq, d, 0, 1, s)),
        "pool_bwd": (Bd, [dh], lambda L: L.cx_pool_normalize_bwd(P(demb), P(emb0), P(norm0), P(cu), P(dh), Bq, d, 0, 1, s)),
        "rotary_qkv": (4 * Bd, [qkv], lambda L: L.cx_rotary_qkv_inplace(P(qkv), P(cu), P(cos), P(sin), Bq, H, T, 128, 1, s), restore((qkv, qkv0))),
        "rope2d_qkv": (4 * Bd, [qkv], lambda L: L.cx_rope2d_qkv_inplace(P(qkv), P(cu_e), P(cs2), P(sn2), 256, Be, H, Te, 1, 1, s), restore((qkv, qkv0))),
        "swiglu_subln_fwd": (5 * Bt, [g_o, a_o, z_o, mean, rstd], lambda L: L.cx_swiglu_subln_fwd(P(yg), P(gam), P(bet), P(g_o), P(a_o), P(z_o), P(mean), P(rstd), T, I, 1e-6, s)),
        "swiglu_subln_bwd": (5 * Bt, [dyg, dgam, dbet, dbias], lambda L: L.cx_swiglu_subln_bwd(P(dact), P(sa), P(sg), P(sm), P(sr), P(gam), P(dyg), P(dgam), P(dbet), P(dbias), P(ws), ws.numel(), T, I, s)),
        "vit_patchify": (6.0 * pix.numel(), [patches], lambda L: L.cx_vit_patchify(P(pix), 0, P(patches), Bv, 3, 224, 224, 16, s)),
        "vit_assemble_fwd": (4.0 * proj.numel(), [seq], lambda L: L.cx_vit_assemble_fwd(P(proj), P(cls), P(pos), P(seq), Bv, 196, d, s)),
        "vit_assemble_bwd": (4.0 * dzv.numel(), [dproj, gcls, gpos], lambda L: L.cx_vit_assemble_bwd(P(dzv), P(dproj), P(gcls), P(gpos), Bv, 196, d, s)),
        "xent_fwd": (2.0 * N * V, [loss, lse], lambda L: L.cx_xent_fwd(P(logits), 1, P(labels), P(loss), P(lse), N, V, V, 1.0, -100, s)),
        "xent_bwd": (4.0 * N * V, [dlogits], lambda L: L.cx_xent_bwd(P(dloss), P(logits), 1, P(lse0), P(labels), P(dlogits), N, V, V, V, 1.0, -100, s)),
        "adamw_clip_step": (28.0 * n, [pw, mw, vw], lambda L: L.cx_adamw_clip_step(P(pw), P(gr), P(mw), P(vw), n, 2e-4, 0.9, 0.999, 1e-8, 0.1, 1000, P(sq), 1.0, s),
                            restore((pw, p0), (mw, m0), (vw, v0))),
        "ema_update": (12.0 * n, [ema], lambda L: L.cx_ema_update(P(ema), P(pw), n, 0.999, s), restore((ema, p0), (pw, p0))),
        "grad_sq_norm": (4.0 * n, [], lambda L: L.cx_grad_sq_norm(P(gr), n, P(sq_acc), s)),
    }


GLUE = ("swiglu_fwd_ew", "swiglu_bwd_ew", "swiglu_bwd_gate_ew", "bias_gelu_fwd", "bias_qgelu_fwd", "bias_gelu_bwd", "bias_gelu_bwd_colsum",
        "bias_qgelu_bwd_colsum", "bias_grad", "cast_f32_bf16", "cast_bf16_f32", "cast_transpose", "cast_transpose_x12", "transpose_bf16",
        "transpose_f32", "pool_fwd", "pool_bwd", "rotary_qkv", "rope2d_qkv", "swiglu_subln_fwd", "swiglu_subln_bwd", "vit_patchify",
        "vit_assemble_fwd", "vit_assemble_bwd", "xent_fwd", "xent_bwd", "adamw_clip_step", "ema_update", "grad_sq_norm")
GROUPS = {glue_cases: GLUE, gemm_cases: ("swiglu_bwd", "swiglu_fwd_save", "swiglu_fwd", "qkv_fwd", "out_dgrad", "out_fwd_res", "fc2_fwd_res", "qkv_dgrad_res", "fc1_dgrad_res"),
          attn_cases: ("attn_fwd", "attn_bwd", "attn_bwd_dpre", "attn_bwd_drop", "attn_fwd_drop", "attn_bwd_ragged"),
          ln_cases: ("ln_fwd", "ln_fwd_res_z", "ln_bwd_ws", "ln_bwd_colsum_ws", "ln_bwd_atomics", "ln_pooled_ws", "ln_drop_fwd", "ln_drop_bwd_colsum_ws",
                     "ln_mixed_fwd_f32", "ln_mixed_bwd_f32", "embed_fwd", "embed_bwd_sorted", "dropout_scale")}
want = [c for c in a.cases.split(",") if c] or [c for grp in GROUPS.values() for c in grp]
want = [c for w in want for c in (GLUE if w == "glue" else (w,))]
unknown = [c for c in want if not any(c in grp for grp in GROUPS.values())]
assert not unknown, f"unknown cases {unknown}"
cases = {}
for build, grp in GROUPS.items():
    if any(c in grp for c in want):
        cases.update(build())
first = names[0]
print(f"# T = {T} token rows, seq {S}, LayerNorm width {a.width}; median of {a.rounds} interleaved rounds x {a.reps} launches (us); "
      f"libs: {[labels[n] for n in names]}")
hdr = f"{'case':22s}" + "".join(f"{labels[n] + ' us':>14s}{'T/s':>8s}" for n in names) + f"{'spread':>8s}"
hdr += "".join(f"{labels[n] + '/' + labels[first]:>22s}{'maxrel':>10s}" for n in names[1:])
print(hdr)
for cname in want:
    fl, outs, call, prep, once = (cases[cname] + (None, None))[:5]
    if once:
        once()
    ref, diffs = None, {}
    for n in names:
        for o in outs:
            o.zero_()
        if prep:
            prep()
        rc = call(libs[n])
        assert rc == 0, (cname, n, rc)
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        if ref is None:
            ref = got
        else:
            same = all(torch.equal(x_.view(torch.uint8), y_.view(torch.uint8)) for x_, y_ in zip(got, ref))
            rel = max((float((x_.float() - y_.float()).norm() / (y_.float().norm() + 1e-30)) for x_, y_ in zip(got, ref)), default=0.0)
            diffs[n] = "timed only" if not outs else "bit-ident" if same else f"{rel:.2e}"
    t = {n: [] for n in names}
    for _ in range(a.rounds):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call(libs[n])
            e1.record()
            torch.cuda.synchronize()
            t[n].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
    row = f"{cname:22s}" + "".join(f"{med[n]:14.1f}{(fl / med[n] / 1e6 if fl else 0):8.2f}" for n in names)
    row += f"{(max(t[first]) - min(t[first])) / med[first]:8.3f}"
    row += "".join(f"{med[n] / med[first]:22.3f}{diffs[n]:>10s}" for n in names[1:])
    print(row, flush=True)
