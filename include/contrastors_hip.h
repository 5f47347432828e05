/* contrastors_hip.h -- C-ABI of libcontrastors_hip.so (gfx950 / MI355X only).
 *
 * This is the drop-in boundary of SURVEY.md §8(b): the reference (nomic-ai/contrastors) reaches its native
 * hot path through the python symbol surface of the third-party `flash_attn` package; every entry point
 * below is what that surface binds for ONE op, with the reference call site it replaces.  Rules:
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - bf16 tensors are `uint16_t*` (raw bfloat16 bits), row-major, leading dimension in ELEMENTS;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only enqueues work;
 *   - nothing allocates or frees: outputs and scratch are caller-owned (torch caching allocator upstream);
 *   - return value: CX_OK (0) or a negative CX_ERR_* code; the library never throws and never exits.
 * Reference paths are relative to /root/reference/src/contrastors (abbreviated sc/).
 */
#ifndef CONTRASTORS_HIP_H
#define CONTRASTORS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CX_OK 0
#define CX_ERR_SHAPE (-1)  /* unsupported shape (e.g. K % 64 != 0, head_dim != 64) */
#define CX_ERR_ALIGN (-2)  /* pointer / leading dimension not aligned as required */
#define CX_ERR_ARG (-3)    /* invalid enum / null pointer */
#define CX_ERR_LAUNCH (-4) /* hipGetLastError() != hipSuccess after the launch */

/* ---- library info -------------------------------------------------------------------------------- */
int cx_abi_version(void);          /* bumped on any signature change */
const char* cx_build_info(void);   /* "gfx950 <date> <compiler>" */
const char* cx_error_string(int code);

/* ---- K9  FusedDense  (flash_attn.ops.fused_dense.FusedDense; sc/layers/attention.py:82-85,112-114,243,
 *          sc/layers/mlp.py:24-28,61-83) ----------------------------------------------------------------
 * Out[m][n] = alpha * sum_k X[m][k] * W[n][k] (+ bias[n])          X:(M,K) ldx   W:(N,K) ldw   Out:(M,N) ldo
 * out_mode 0: Out is bf16;  1: Out is fp32 (overwrite).  Accumulating forms: cx_gemm_bf16_nt_accum / _tn_accum
 * (deterministic split-K); `split_k` is ignored here.  Requirements: K % 64 == 0, N % 4 == 0, ldx/ldw % 8 == 0, ldo % 4 == 0.
 * forward: X=act, W=weight.  dgrad: X=dY, W=W^T.  wgrad: X=dY^T, W=act^T (both via cx_transpose_bf16). */
int cx_gemm_bf16_nt(const uint16_t* X, const uint16_t* W, void* Out, const float* bias, int M, int N, int K, int ldx,
                    int ldw, int ldo, int out_mode, int split_k, float alpha, void* stream);
/* Out:(M,N) fp32 (ld = N) += X W^T with split-K through a caller-owned fp32 workspace `ws` (>= M*N floats; more lets
 * more K slices run concurrently) and a fixed-order reduction: the wgrad form (X = dY^T, W = act^T, K = tokens).
 * Deterministic; no atomics. */
int cx_gemm_bf16_nt_accum(const uint16_t* X, const uint16_t* W, float* Out, float* ws, long ws_floats, int M, int N,
                          int K, int ldx, int ldw, void* stream);
/* wgrad in its natural layout, no transposes: G:(O,I) fp32 (ld = I) += dY:(T,O)^T A:(T,I).  The kernel reads
 * round_up(T,64) token rows of both operands: rows T.. of that range must be ZERO.  O % 256 == 0, I % 256 == 0 (else
 * CX_ERR_SHAPE: transpose both operands with cx_transpose_bf16 and use cx_gemm_bf16_nt_accum). */
int cx_gemm_bf16_tn_accum(const uint16_t* dY, const uint16_t* A, float* G, float* ws, long ws_floats, int T, int O, int I,
                          int ld_dy, int ld_a, void* stream);
/* Sampled per-launch timing of this (dominant) kernel for bench.py's roofline: every `stride`-th launch is bracketed by
 * HIP events on its own stream; collect() synchronises them and returns the summed duration (ms) and algorithmic FLOPs
 * (2*M*N*K) of exactly the sampled launches. */
int cx_prof_gemm_config(int enable, int stride);
int cx_prof_gemm_collect(double* total_ms, double* total_flop, long* launches_timed, long* launches_total);
/* Per-box calibration for bench.py (cx_abi_version >= 9; measurement aids, no product kernel calls them): the pool's boxes differ
 * by +-3 % in sustained matrix-core clock at their power limit, so a roofline fraction is also reported against what THIS box
 * sustains.  cx_calib_mfma_bf16: register-only v_mfma_f32_16x16x32_bf16 loop (the GEMMs' instruction), `nwg` workgroups of one wave per SIMD, each wave
 * `iters` x 16 MFMAs (16 KFLOP each) on fragments from seed (1024 x 16 B, random bf16): FLOPs = nwg * 4 * iters * 8 * 32768; cycles (NULL ok):
 * nwg x 4 s_memtime deltas.  cx_calib_copy: 16 B per lane grid-stride copy, bytes % 16 == 0 (HBM stream rate). */
int cx_calib_mfma_bf16(const void* seed_1024x16B, int iters, int nwg, long long* cycles_nwg_x4, float* sink, void* stream);
int cx_calib_copy(const void* src, void* dst, long bytes, void* stream);

/* Out[c][r] = In[r][c] for r < rows, zero for rows <= r < rows_pad (token padding for the wgrad reduction).
 * In:(rows,cols) ld_in, Out:(cols,rows_pad) ld_out.  cols % 8 == 0. */
int cx_transpose_bf16(const uint16_t* In, uint16_t* Out, int rows, int cols, int ld_in, int ld_out, int rows_pad,
                      void* stream);
/* fp32 master weights -> bf16 shadow (row-major copy) and optional transposed bf16 shadow (for dgrad). */
int cx_cast_f32_to_bf16(const float* In, uint16_t* Out, long n, void* stream);
int cx_cast_transpose_f32_to_bf16(const float* In, uint16_t* OutT, int rows, int cols, void* stream);
/* The same for n_jobs matrices in ONE launch (cx_abi_version >= 8): `jobs` is a DEVICE array; max_tiles = the largest
 * ceil(rows / 64) * ceil(cols / 64) among them.  The optimizer step's refresh of the transposed bf16 weight shadows was 48
 * launches of ~11 us each -- 5 % of BASELINE configs[0]'s 11 ms step. */
typedef struct {
    const float* in;    /* (rows, cols) fp32, row-major */
    uint16_t* out_t;    /* (cols, rows) bf16 */
    int rows, cols;
} CxCastJob;
int cx_cast_transpose_f32_to_bf16_batched(const CxCastJob* jobs, int n_jobs, int max_tiles, void* stream);
int cx_cast_bf16_to_f32(const uint16_t* In, float* Out, long n, void* stream);

/* ---- K5/K6  dropout_add_layer_norm / layer_norm  (flash_attn.ops.layer_norm; sc/layers/block.py:309-319,
 *             422-431,453-462; sc/models/encoder/modeling_nomic_bert.py:534; sc/models/vit/vit.py:253-263) ---
 * z = x0 + residual (residual may be NULL); out = (z-mean)*rstd*gamma + beta.  Statistics in fp32.
 * z_out (may be NULL, may alias x0) receives z in bf16 (kept for backward / the pre-norm residual stream).
 * dropout p == 0 only (all five BASELINE configs train with resid_pdrop = 0).  d in {256,512,768,1024}. */
int cx_layernorm_fwd(const uint16_t* x0, const uint16_t* residual, const float* gamma, const float* beta,
                     uint16_t* out, uint16_t* z_out, float* mean, float* rstd, int rows, int d, float eps,
                     void* stream);
/* dout = dout_a + dout_b (dout_b may be NULL); dz_extra (may be NULL) is added to dz (pre-norm residual grad).
 * dz: bf16 (rows,d) (grad of x0 and of residual); dgamma/dbeta: fp32[d], accumulated (+=).  ws (may be NULL): fp32
 * scratch of ws_floats >= 512*d floats enabling the deterministic two-stage reduction (else atomics are used). */
int cx_layernorm_bwd(const uint16_t* dout_a, const uint16_t* dout_b, const uint16_t* z, const float* gamma,
                     const float* mean, const float* rstd, const uint16_t* dz_extra, uint16_t* dz, float* dgamma,
                     float* dbeta, float* ws, long ws_floats, int rows, int d, void* stream);

/* Backward of the LAST LayerNorm of a pooled encoder with the pooling / normalisation backward folded in
 * (sc/models/biencoder/modeling_biencoder.py:79-90,314-319 backward + the LayerNorm backward of sc/layers/block.py:453-462
 * or sc/models/vit/vit.py:253-263): dout[t] = w(t) * g[seq(t)], g = d(pooled vector) from (demb, emb, norm) exactly as
 * cx_pool_normalize_bwd computes it, w = 1/len (pool_mode 0, mean) or [t first token] (pool_mode 1, cls).  dout stays in
 * fp32 registers: the bf16 rounding of a materialised dout showed in the final LayerNorm's bias gradient (3.7 % vs the
 * fp32 oracle on the reference's GradCache fixture, where bf16-eager is 0.5 % off).  rows = total tokens. */
int cx_layernorm_bwd_pooled(const float* demb, const float* emb, const float* norm, const int32_t* cu_seqlens, int B,
                            int pool_mode, int normalize, const uint16_t* z, const float* gamma, const float* mean,
                            const float* rstd, uint16_t* dz, float* dgamma, float* dbeta, float* dz_colsum, float* ws,
                            long ws_floats, int rows, int d, void* stream);
/* cx_layernorm_bwd that also accumulates dz_colsum[n] += sum_t dz[t][n] (fp32[d]; also a trailing argument of the pooled
 * form above, NULL = off): dz is the gradient of (Linear output + residual), so this IS the bias gradient of that Linear
 * (FusedDense backward's db for fc2 / out_proj of the BERT-base and ViT towers) without a second pass over dz.  Needs
 * the workspace (CX_ERR_ARG otherwise: call cx_layernorm_bwd + cx_bias_grad). */
int cx_layernorm_bwd_colsum(const uint16_t* dout_a, const uint16_t* dout_b, const uint16_t* z, const float* gamma,
                            const float* mean, const float* rstd, const uint16_t* dz_extra, uint16_t* dz, float* dgamma,
                            float* dbeta, float* dz_colsum, float* ws, long ws_floats, int rows, int d, void* stream);

/* dropout p > 0 (flash_attn.ops.layer_norm.dropout_add_layer_norm(p > 0), sc/layers/block.py:422-431,453-462 with
 * resid_pdrop > 0): z = dropout_p(x0) + residual, out = LN(z).  The keep-mask is Philox4x32-10(seed; offset + site,
 * element group) -- a pure function of the torch generator's (seed, offset) the host drew for this chunk, so backward and
 * a GradCache re-forward under RandContext (sc/rand_state.py:6-22) regenerate it; nothing is stored.  bwd returns dz
 * (gradient of the residual) AND dx0 = dz * mask / (1 - p) (gradient of x0).  0 < p < 1.  `site` separates the dropout
 * sites of one chunk (2 per block + the embeddings). */
int cx_dropout_add_layernorm_fwd(const uint16_t* x0, const uint16_t* residual, const float* gamma, const float* beta,
                                 uint16_t* out, uint16_t* z_out, float* mean, float* rstd, int rows, int d, float eps,
                                 float p, unsigned long long seed, unsigned long long offset, unsigned int site,
                                 void* stream);
int cx_dropout_add_layernorm_bwd(const uint16_t* dout_a, const uint16_t* dout_b, const uint16_t* z, const float* gamma,
                                 const float* mean, const float* rstd, uint16_t* dz, uint16_t* dx0, float* dgamma,
                                 float* dbeta, float* ws, long ws_floats, int rows, int d, float p,
                                 unsigned long long seed, unsigned long long offset, unsigned int site, void* stream);
/* The same that also accumulates dx0_colsum[n] += sum_t dx0[t][n] (fp32[d], may be NULL: then identical to the call above) -- dx0 is the
 * gradient of the (dropped) sub-layer output, so these are the bias gradient of the Linear that produced it (cx_abi_version >= 10; needs
 * ws >= 3 * d * 256 floats, CX_ERR_ARG otherwise).  Deterministic two-stage reduction, no atomics. */
int cx_dropout_add_layernorm_bwd_colsum(const uint16_t* dout_a, const uint16_t* dout_b, const uint16_t* z, const float* gamma,
                                        const float* mean, const float* rstd, uint16_t* dz, uint16_t* dx0, float* dgamma, float* dbeta,
                                        float* dx0_colsum, float* ws, long ws_floats, int rows, int d, float p, unsigned long long seed,
                                        unsigned long long offset, unsigned int site, void* stream);
/* x <- x * mask / (1 - p) in place, n % 4 == 0 (embedding dropout, sc/models/encoder/modeling_nomic_bert.py:534-535, and
 * its gradient). */
int cx_dropout_scale(uint16_t* x, long n, float p, unsigned long long seed, unsigned long long offset, unsigned int site,
                     void* stream);

/* The same two ops with a dtype per operand, for the flash_attn.ops.layer_norm python surface (`residual_in_fp32`, fp32
 * inputs on the reference's BERT path: embedding LayerNorm fp32 in / fp32 out, layer-0 residual fp32).
 * flags: bit0 x0 is fp32, bit1 residual is fp32, bit2 out is fp32, bit3 z (the saved sum / prenorm residual output) is
 * fp32; clear = bf16 (statistics always use the unrounded fp32 sum); bit4: RMSNorm (flash_attn.ops.rms_norm, K8): out =
 * z * rsqrt(mean(z^2) + eps) * gamma (+ beta, which may then be NULL), `mean` receives 0.  bwd writes
 * dz to dx0 (x0's dtype) and, if not NULL, to dres (the residual's dtype); dout has out's dtype, dz_extra has z's. */
int cx_layernorm_fwd_mixed(const void* x0, const void* residual, const float* gamma, const float* beta, void* out,
                           void* z_out, float* mean, float* rstd, int rows, int d, float eps, int flags, void* stream);
int cx_layernorm_bwd_mixed(const void* dout, const void* z, const float* gamma, const float* mean, const float* rstd,
                           const void* dz_extra, void* dx0, void* dres, float* dgamma, float* dbeta, int rows, int d,
                           int flags, void* stream);

/* ---- a11 BertEmbeddings + K6 embedding LayerNorm, on the unpadded token stream
 *          (sc/layers/embedding.py:594-615, sc/models/encoder/modeling_nomic_bert.py:531-535, K4 unpad_input
 *          sc/models/encoder/modeling_nomic_bert.py:332-333) -------------------------------------------------
 * token t: flat = indices[t] (= b*S + s of the padded batch); id = input_ids[flat]; pos = flat % S.
 * z = word[id] + type[0] (+ pos_emb[pos] if pos_emb != NULL); out = LN(z) in bf16; mean/rstd saved. */
int cx_embed_ln_fwd(const int64_t* input_ids, const int32_t* indices, const float* word, const float* type0,
                    const float* pos_emb, const float* gamma, const float* beta, uint16_t* out, float* mean,
                    float* rstd, int T, int S, int d, float eps, void* stream);
/* backward: scatter-adds into fp32 grads (word rows except padding_idx, type row 0, pos rows), dgamma/dbeta. */
int cx_embed_ln_bwd(const uint16_t* dout_a, const uint16_t* dout_b, const int64_t* input_ids,
                    const int32_t* indices, const float* word, const float* type0, const float* pos_emb,
                    const float* gamma, const float* mean, const float* rstd, float* dword, float* dtype0,
                    float* dpos, float* dgamma, float* dbeta, int T, int S, int d, int padding_idx, void* stream);

/* The same backward with the word-embedding rows reduced WITHOUT atomics: `sorted_ids` = the chunk's T token ids in
 * ascending order (stable), `perm` = the token index each sorted entry came from (both int32[T], prepared by the host
 * with one device sort per chunk), dz_scratch = (T, d) fp32 (the row gradients are not rounded before they are summed).  One workgroup per vocabulary row sums its tokens in token
 * order: deterministic, and ~10x faster than 100 M fp32 atomics per 131072-token chunk.  dpos / dtype0 / dgamma / dbeta as
 * above. */
int cx_embed_ln_bwd_sorted(const uint16_t* dout_a, const uint16_t* dout_b, const int64_t* input_ids,
                           const int32_t* indices, const float* word, const float* type0, const float* pos_emb,
                           const float* gamma, const float* mean, const float* rstd, float* dword, float* dtype0,
                           float* dpos, float* dgamma, float* dbeta, int T, int S, int d, int padding_idx, int vocab,
                           const int32_t* sorted_ids, const int32_t* perm, float* dz_scratch, void* stream);

/* The three entry points above with token-type (segment) ids (sc/layers/embedding.py:607-614; sentence-pair tasks): token t
 * takes row token_type_ids[flat] of `type`:(type_vocab_size, d) -- token_type_ids:(B*S) int64 is indexed with indices[t] exactly
 * like input_ids -- and `dtype`:(type_vocab_size, d) receives both rows' gradients.  type_vocab_size must be 2 (anything else:
 * CX_ERR_SHAPE, nothing launched); an id other than 0 selects row 1.  token_type_ids == NULL calls the untyped entry point with
 * row 0: the same bits, for the output and every gradient.  The backward forms accumulate the type rows in registers per wave
 * and fold the block partials -- of the type rows and of dgamma / dbeta -- through ws (fp32, >= 4 * d floats: [blocks][2][d]
 * twice; the grid is capped by what it holds; CX_ERR_ARG if it holds none) with the LayerNorm backward's second-stage
 * reduction: no atomics on the type rows, dgamma or dbeta, which are the same bits on every run (dpos, and dword in the
 * unsorted form, remain fp32 atomics).
 * Additive: cx_abi_version stays 10. */
int cx_embed_ln_fwd_typed(const int64_t* input_ids, const int64_t* token_type_ids, const int32_t* indices, const float* word,
                          const float* type, int type_vocab_size, const float* pos_emb, const float* gamma, const float* beta,
                          uint16_t* out, float* mean, float* rstd, int T, int S, int d, float eps, void* stream);
int cx_embed_ln_bwd_typed(const uint16_t* dout_a, const uint16_t* dout_b, const int64_t* input_ids,
                          const int64_t* token_type_ids, const int32_t* indices, const float* word, const float* type,
                          int type_vocab_size, const float* pos_emb, const float* gamma, const float* mean, const float* rstd,
                          float* dword, float* dtype, float* dpos, float* dgamma, float* dbeta, float* ws, long ws_floats, int T,
                          int S, int d, int padding_idx, void* stream);
int cx_embed_ln_bwd_sorted_typed(const uint16_t* dout_a, const uint16_t* dout_b, const int64_t* input_ids,
                                 const int64_t* token_type_ids, const int32_t* indices, const float* word, const float* type,
                                 int type_vocab_size, const float* pos_emb, const float* gamma, const float* mean,
                                 const float* rstd, float* dword, float* dtype, float* dpos, float* dgamma, float* dbeta,
                                 float* ws, long ws_floats, int T, int S, int d, int padding_idx, int vocab,
                                 const int32_t* sorted_ids, const int32_t* perm, float* dz_scratch, void* stream);

/* ---- K10 swiglu (flash_attn.ops.activations.swiglu; sc/layers/mlp.py:75) and GELU(erf) (mlp.py:30-34) ----
 * yg:(T, 2*I) holds y = fc11(x) and gate = fc12(x);  act = silu(gate) * y, fp32 math, one rounding.
 * layout 0: yg = [y | gate] concatenated; layout 1: interleaved in groups of 32 columns
 * ([y 0..31 | gate 0..31 | y 32..63 | ...]) -- the layout of the fused fc1 weight and of cx_gemm_bf16_swiglu. */
int cx_swiglu_fwd(const uint16_t* yg, uint16_t* act, int T, int I, int layout, void* stream);
int cx_swiglu_bwd(const uint16_t* dact, const uint16_t* yg, uint16_t* dyg, int T, int I, int layout, void* stream);
/* K9 + K10 fused: Act:(M,I) = silu(X Wg^T) * (X Wy^T) in one pass, W:(2I,K) rows interleaved by 32 as above; YG (may be
 * NULL):(M,2I) receives the pre-activation pair in the interleaved layout (kept for backward). */
/* Projection whose output is the `x0` of `dropout_add_layer_norm(x0, residual, ...)` (sc/layers/block.py:422-431,
 * 453-462: out_proj and fc2 of every block): Out = bf16(bf16(X W^T + bias) + Residual), i.e. the residual add leaves the
 * LayerNorm kernel (call cx_layernorm_fwd with x0 = Out, residual = NULL).  Residual: (M, N) bf16, leading dim ldr.
 * CX_ERR_SHAPE = shape not covered by the fused kernel (use cx_gemm_bf16_nt and pass the residual to the LayerNorm). */
int cx_gemm_bf16_nt_residual(const uint16_t* X, const uint16_t* W, uint16_t* Out, const float* bias,
                             const uint16_t* Residual, int M, int N, int K, int ldx, int ldw, int ldo, int ldr,
                             void* stream);
/* The same projection for FEW output tiles and a LONG K (sc/trainers at small batches: BASELINE configs[0], B = 32, S = 64 is
 * 2048 token rows -- fc2 is 24 tiles of 256 x 256 with 48 K-tiles each): the K range is split into K / 384 slices (at most
 * 16; a function of K alone, so the summation order does not depend on M), fp32 partial slabs go to `ws` (>= slices * M * N
 * floats) and one fixed-order pass writes Out = bf16(bf16(sum + bias) + Residual) (bias, Residual optional).  Deterministic.
 * CX_ERR_SHAPE = not the case this route is for (more than 64 tiles, K < 1536, no room for the slabs): use
 * cx_gemm_bf16_nt / cx_gemm_bf16_nt_residual. */
int cx_gemm_bf16_nt_splitk(const uint16_t* X, const uint16_t* W, uint16_t* Out, const float* bias, const uint16_t* Residual,
                           float* ws, long ws_floats, int M, int N, int K, int ldx, int ldw, int ldo, int ldr, void* stream);
int cx_gemm_bf16_swiglu(const uint16_t* X, const uint16_t* W, uint16_t* YG, uint16_t* Act, int M, int I, int K, int ldx,
                        int ldw, int ld_yg, int ld_act, void* stream);
/* fc1 of the plain MLP (sc/layers/mlp.py:30-34: fc2(gelu(fc1 x)), erf GELU, block.py:181-189) with bias + GELU fused
 * into the GEMM epilogue: Pre (M,N) bf16 = X W^T + bias (optional: NULL in the no-grad pass), Act (M,N) = gelu(Pre).
 * CX_ERR_SHAPE = shape not covered by the fused kernel (run cx_gemm_bf16_nt + cx_bias_gelu_fwd instead). */
int cx_gemm_bf16_bias_gelu(const uint16_t* X, const uint16_t* W, const float* bias, uint16_t* Pre, uint16_t* Act, int M,
                           int N, int K, int ldx, int ldw, int ld_pre, int ld_act, void* stream);
/* The same with the activation selected at run time (sc/layers/mlp.py:8-34 `activation`): act = 0 exact-erf GELU (BERT-base,
 * HF / timm ViTs), 1 quick_gelu = x * sigmoid(1.702 x) (sc/layers/activations.py:4-5: the OpenAI-CLIP image tower,
 * sc/models/vit/clip.py:14-58). */
int cx_gemm_bf16_bias_act(const uint16_t* X, const uint16_t* W, const float* bias, uint16_t* Pre, uint16_t* Act, int M,
                          int N, int K, int ldx, int ldw, int ld_pre, int ld_act, int act, void* stream);
/* fc2 dgrad of the plain MLP with the GELU / quick_gelu backward fused into the epilogue (cx_abi_version >= 10; the reference gets the
 * pair from flash_attn.ops.fused_dense / FusedMLP, sc/layers/mlp.py:30-34): dPre (M, N) = bf16(bf16(dY W^T) * act'(Pre)), Pre = the
 * biased pre-activation saved by cx_gemm_bf16_bias_act, W: (N, K) row-major (the transposed fc2 weight), act as there.  Bit-identical to
 * cx_gemm_bf16_nt + cx_bias_act_bwd_colsum(bias = NULL).  dbias (may be NULL): fp32 [N] += column sums of the bf16 dPre = the fc1 bias
 * gradient, summed in a fixed order through `ws` (>= ceil(M / 128) * N floats): deterministic, no atomics.
 * CX_ERR_SHAPE = not covered (K % 64, N % 8, ld % 8, workspace too small): run the two calls above instead. */
int cx_gemm_bf16_act_bwd(const uint16_t* dY, const uint16_t* W, const uint16_t* Pre, uint16_t* dPre, float* dbias, float* ws,
                         long ws_floats, int M, int N, int K, int ldx, int ldw, int ld_pre, int ld_dpre, int act, void* stream);
/* fc2 dgrad of the gated MLP with the backward of `swiglu` (flash_attn.ops.activations, sc/layers/mlp.py:75) fused into
 * the epilogue: dYG (M, 2I) = d swiglu(YG) applied to dAct = dY W^T, YG / dYG in the interleaved-by-32 layout of
 * cx_gemm_bf16_swiglu; W: (I, K) row-major (the transposed fc2 weight).  dAct is never written to memory.
 * CX_ERR_SHAPE = shape not covered (needs I % 256 == 0, K % 64 == 0): run cx_gemm_bf16_nt + cx_swiglu_bwd instead. */
int cx_gemm_bf16_swiglu_bwd(const uint16_t* dY, const uint16_t* W, const uint16_t* YG, uint16_t* dYG, int M, int I, int K,
                            int ldx, int ldw, int ld_yg, void* stream);
/* Round 3: the compact save of the gated MLP.  The reference's swiglu keeps y and gate for its backward (sc/layers/mlp.py:75,
 * flash_attn.ops.activations.swiglu) and the activation for fc2's: three (M, I) tensors per layer.  y is redundant:
 * act = y * silu(gate), so   d gate = d * y * silu'(g) = d * act * (1 / g + 1 - sigmoid(g)).   cx_gemm_bf16_swiglu_gate
 * saves G: (M, I) = bf16(X Wg^T) in plain column order (may be NULL) next to Act; cx_gemm_bf16_swiglu_bwd_gate is
 * cx_gemm_bf16_swiglu_bwd reading (Act, G) (both leading dimension ld_ag) and writing dYG (M, 2I) in the interleaved-by-32
 * layout; cx_swiglu_bwd_gate is the standalone form for shapes the fused kernel does not cover (CX_ERR_SHAPE as there).
 * The recovered y carries one bf16 rounding (of act), as the saved bf16 y did. */
int cx_gemm_bf16_swiglu_gate(const uint16_t* X, const uint16_t* W, uint16_t* G, uint16_t* Act, int M, int I, int K, int ldx,
                             int ldw, int ld_g, int ld_act, void* stream);
int cx_gemm_bf16_swiglu_bwd_gate(const uint16_t* dY, const uint16_t* W, const uint16_t* Act, const uint16_t* G, uint16_t* dYG,
                                 int M, int I, int K, int ldx, int ldw, int ld_ag, int ld_dyg, void* stream);
int cx_swiglu_bwd_gate(const uint16_t* dact, const uint16_t* act, const uint16_t* gate, uint16_t* dyg, int T, int I,
                       void* stream);
/* act = gelu_erf(pre + bias); bias fp32[I] may be NULL.  backward: dpre = dact * gelu'(pre + bias). */
int cx_bias_gelu_fwd(const uint16_t* pre, const float* bias, uint16_t* act, int T, int I, void* stream);
int cx_bias_gelu_bwd(const uint16_t* dact, const uint16_t* pre, const float* bias, uint16_t* dpre, int T, int I,
                     void* stream);
/* The same backward with the bias gradient of the same pass: dbias[n] += sum_t dpre[t][n] (fp32 atomics; dbias may be NULL).
 * Replaces cx_bias_gelu_bwd + cx_bias_grad (the second kernel re-read dpre: T x I x 2 bytes). */
int cx_bias_gelu_bwd_colsum(const uint16_t* dact, const uint16_t* pre, const float* bias, uint16_t* dpre, float* dbias, int T,
                            int I, void* stream);
/* ... and both directions with the activation selected at run time (act as in cx_gemm_bf16_bias_act). */
int cx_bias_act_fwd(const uint16_t* pre, const float* bias, uint16_t* act_out, int T, int I, int act, void* stream);
int cx_bias_act_bwd_colsum(const uint16_t* dact, const uint16_t* pre, const float* bias, uint16_t* dpre, float* dbias, int T,
                           int I, int act, void* stream);
/* dbias[n] += sum_t dY[t][n]  (fp32 atomic accumulate; bgrad half of FusedDense backward). */
int cx_bias_grad(const uint16_t* dY, float* dbias, int T, int N, int ld, void* stream);

/* ---- K1/K2 + K11  flash_attn_varlen_qkvpacked_func with rotary fused into the Q/K tile load
 *          (sc/layers/attention.py:122-135,172-182; sc/layers/embedding.py:685-706) -------------------------
 * qkv:(T,3,H,64) bf16 packed, cu_seqlens:(B+1) int32, non-causal, softmax in fp32, dropout 0.
 * rot_cos/rot_sin: fp32 (>= max_seqlen, 32) tables for full non-interleaved rotary, or NULL for no rotary
 * (bert-base / ViT).  out:(T,H,64) bf16.  lse:(H,T) fp32 (natural log of the scaled-score softmax denominator). */
int cx_attn_varlen_fwd(const uint16_t* qkv, const int32_t* cu_seqlens, const float* rot_cos, const float* rot_sin,
                       uint16_t* out, float* lse, int B, int H, int T, int max_seqlen, float softmax_scale,
                       void* stream);
/* delta:(H,T) fp32 scratch (rowsum(dO*O)); dqkv:(T,3,H,64) bf16 fully overwritten (dq,dk un-rotated). */
int cx_attn_varlen_bwd(const uint16_t* dout, const uint16_t* qkv, const uint16_t* out, const float* lse,
                       const int32_t* cu_seqlens, const float* rot_cos, const float* rot_sin, float* delta,
                       uint16_t* dqkv, int B, int H, int T, int max_seqlen, float softmax_scale, void* stream);

/* backward for a qkv whose q and k were rotated IN PLACE beforehand (cx_rotary_qkv_inplace; the forward is then
 * cx_attn_varlen_fwd with NULL tables): nothing is rotated at the loads, dq / dk leave through the inverse rotation.  The
 * engine takes this route for max_seqlen > 128 (the streaming kernels would re-rotate every row once per 128-row block). */
int cx_attn_varlen_bwd_prerotated(const uint16_t* dout, const uint16_t* qkv_rotated, const uint16_t* out, const float* lse,
                                  const int32_t* cu_seqlens, const float* rot_cos, const float* rot_sin, float* delta,
                                  uint16_t* dqkv, int B, int H, int T, int max_seqlen, float softmax_scale, void* stream);

/* attention dropout (flash_attn_varlen_qkvpacked_func(dropout_p > 0), attn_pdrop > 0): O = (P * keep / (1 - p)) V with
 * keep(b, h, q, key) = Philox4x32-10(seed; offset + site, (b * H + h, q, key / 4))[key % 4] >= p * 2^32 -- regenerated by
 * the backward and by a GradCache re-forward under RandContext, never stored.  Same arguments as cx_attn_varlen_fwd/_bwd
 * plus (p, seed, offset, site); 0 < p < 1, any max_seqlen < 2^20, B * H < 2^24. */
int cx_attn_varlen_dropout_fwd(const uint16_t* qkv, const int32_t* cu_seqlens, const float* rot_cos, const float* rot_sin,
                               uint16_t* out, float* lse, int B, int H, int T, int max_seqlen, float softmax_scale,
                               float p_drop, unsigned long long seed, unsigned long long offset, unsigned int site,
                               void* stream);
int cx_attn_varlen_dropout_bwd(const uint16_t* dout, const uint16_t* qkv, const uint16_t* out, const float* lse,
                               const int32_t* cu_seqlens, const float* rot_cos, const float* rot_sin, float* delta,
                               uint16_t* dqkv, int B, int H, int T, int max_seqlen, float softmax_scale, float p_drop,
                               unsigned long long seed, unsigned long long offset, unsigned int site, void* stream);

/* ---- K3  flash_attn_kvpacked_func / flash_attn_varlen_kvpacked_func (cross-attention; sc/layers/attention.py:313-433,
 *          FlashAttentionPooling: one latent query per sequence over the sequence's keys) ---
 * q (Tq, H, 64), kv (Tk, 2, H, 64) bf16, batch entry b: queries cu_seqlens_q[b] .. [b+1), keys cu_seqlens_k[b] .. [b+1);
 * out (Tq, H, 64), lse (H, Tq) fp32.  Non-causal, no dropout, no rotary, H_kv == H (the reference: "we don't really
 * support mqa / gqa").  A query with no keys gets out = 0.  bwd: delta = fp32 scratch (H, Tq); dq (Tq, H, 64),
 * dkv (Tk, 2, H, 64) are overwritten. */
int cx_attn_varlen_kvpacked_fwd(const uint16_t* q, const uint16_t* kv, const int32_t* cu_seqlens_q,
                                const int32_t* cu_seqlens_k, uint16_t* out, float* lse, int B, int H, int Tq,
                                int max_seqlen_q, int max_seqlen_k, float softmax_scale, void* stream);
int cx_attn_varlen_kvpacked_bwd(const uint16_t* dout, const uint16_t* q, const uint16_t* kv, const uint16_t* out,
                                const float* lse, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, float* delta,
                                uint16_t* dq, uint16_t* dkv, int B, int H, int Tq, int max_seqlen_q, int max_seqlen_k,
                                float softmax_scale, void* stream);
/* standalone K11 (apply_rotary_emb_func on a packed qkv, in place on q and k; sign=-1 gives the backward). */
int cx_rotary_qkv_inplace(uint16_t* qkv, const int32_t* cu_seqlens, const float* rot_cos, const float* rot_sin,
                          int B, int H, int T, int max_seqlen, int sign, void* stream);

/* apply_rotary_emb_func on one (T,H,64) view with token stride `tok_stride` elements (in place; sign=-1: backward). */
int cx_rotary_apply(uint16_t* x, long tok_stride, const int32_t* cu_seqlens, const float* rot_cos,
                    const float* rot_sin, int B, int H, int T, int max_seqlen, int sign, void* stream);

/* ---- a9 BiEncoder pooling + normalize (sc/models/biencoder/modeling_biencoder.py:79-90,44-49,314-319) -----
 * mode 0 = mean over the sequence's tokens, 1 = cls (first token).  emb:(B,d) fp32 = x / max(||x||, 1e-12);
 * if normalize == 0 the raw pooled vector is written.  norm:(B) fp32 saved for backward. */
int cx_pool_normalize_fwd(const uint16_t* h, const int32_t* cu_seqlens, float* emb, float* norm, int B, int d,
                          int mode, int normalize, void* stream);
int cx_pool_normalize_bwd(const float* demb, const float* emb, const float* norm, const int32_t* cu_seqlens,
                          uint16_t* dh, int B, int d, int mode, int normalize, void* stream);

/* ---- K13 fused InfoNCE (sc/loss.py:76-132 clip_loss; LogitScale sc/models/biencoder/modeling_biencoder.py:30-41)
 * Q:(N,dim) ldq, D:(G,dim) ldd fp32 (D = rank-ordered all-gather of the document embeddings),
 * labels:(N) int64 = (arange(N)+rank*N)*(G/(N*world)) computed by the host exactly as loss.py:108-117.
 * logits = scale * Q D^T are never written: exact-fp32 MFMA tiles feed an online row log-sum-exp.
 * ws: fp32 scratch of cx_infonce_ws_floats(N,G) floats.  Outputs: lse:(N) fp32, loss_rows:(N) fp32
 * (= lse_i - logit_{i,label_i}); the host takes mean * world_size (loss.py:125).  Every label must lie in [0, G): a label
 * outside it leaves that row's positive logit unwritten in ws and its loss_rows undefined (lse and the arg max do not read it). */
long cx_infonce_ws_floats(int N, int G);
int cx_infonce_fwd(const float* Q, const float* D, const int64_t* labels, float scale, float* ws, float* lse,
                   float* loss_rows, int N, int G, int dim, int ldq, int ldd, void* stream);
/* The same forward that also returns every row's arg max over the G columns (cx_abi_version >= 9): argmax:(N) int32 = the
 * FIRST column attaining the row maximum, i.e. `similarity.argmax(dim=1)` of the in-batch accuracy the reference logs
 * (sc/loss.py:127-130), read off the tiles the loss walks anyway -- the (N,G) similarity is not written for it either.
 * ws: cx_infonce_argmax_ws_floats(N,G) floats.  argmax == NULL: exactly cx_infonce_fwd. */
long cx_infonce_argmax_ws_floats(int N, int G);
int cx_infonce_fwd_argmax(const float* Q, const float* D, const int64_t* labels, float scale, float* ws, float* lse,
                          float* loss_rows, int32_t* argmax, int N, int G, int dim, int ldq, int ldd, void* stream);
/* ---- exact inner-product top-k search (faiss IndexFlatIP.search; scripts/text/index_filtering.py:363-391,
 *          scripts/text/get_negatives.py:111-196, scripts/text/mine_beir_negatives_full.py:98-136) ----------------------
 * Q:(M,d) ldq and D:(N,d) ldd bf16 row-major, d % 64 == 0, 64 <= d <= 1024, N <= 2^31 - 129 rows (byte offsets are 64-bit).
 * Per query row: the k (1 <= k <= 1024) largest scores s = q . d^T (fp32 accumulation) and their corpus ids, in descending
 * score order with ties to the lower id; rows with fewer than k admissible documents are padded with (-inf, -1).
 * out_scores:(M,k) fp32, out_ids:(M,k) int64.  Optional per-row filters: excl_ptr:(M+1) / excl_ids int64 = CSR lists of ids
 * the row must not return (absolute offsets into excl_ids), below:(M) fp32 = exclusive upper bound on the score.
 * nsplit = number of corpus ranges searched in parallel (<= 0: chosen from M and N); the result does not depend on it.
 * ws: 16-B aligned scratch of cx_search_ws_bytes(M, N, k, nsplit) bytes (same nsplit), need not be initialised.
 * The (M,N) scores are never written; deterministic, no atomics.  Q, D 16-B aligned and ldq / ldd % 8 == 0 (CX_ERR_ALIGN). */
long cx_search_ws_bytes(int M, long N, int k, int nsplit);
int cx_search_topk(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, int k,
                   const int64_t* excl_ptr, const int64_t* excl_ids, const float* below, int nsplit, void* ws,
                   float* out_scores, int64_t* out_ids, void* stream);
/* ---- top-k inside a per-row id window, and a merge of top-k lists (what an IVF index is made of; csrc/search.hip).
 *          Additive: cx_abi_version stays 10. ------------------------------------------------------------------------------
 * cx_search_window_topk: cx_search_topk (same operands, alignment rules, error codes, order, padding, score bits) where row m
 * admits document n only if min_id[m] < n < end_id[m]; min_id / end_id:(M) int64 device arrays, clamped to [-1, N] and [0, N],
 * NULL = -1 / N everywhere.  excl_ids and out_ids are corpus positions.  A 128-row query tile computes only the corpus tiles
 * [t0, t1), t0 = (min min_id + 1) / 128 and t1 = ceil(max end_id / 128) over its rows with a non-empty window (a tile without
 * one computes nothing), in one workgroup: made for rows sorted by window.  ws: 16-B aligned,
 * cx_search_window_ws_bytes(M, k) bytes, need not be initialised.  Deterministic, no atomics on global memory.
 * cx_topk_merge_lists: scores / ids:(P,k) = P sorted top-k lists padded with (-inf, -1) (a list ends at its first negative
 * id), as the two search entry points write them.  src:(M,L) int64 names the lists of output row m; entries outside [0, P)
 * are skipped; 1 <= L <= 256.  id_map:(N) int64 or NULL: the id reported for position n is id_map[n] (NULL: n; N is read only
 * with id_map).  out_scores / out_ids:(M,k) = the k best entries of the row's lists by (score descending, REPORTED id
 * ascending), padded with (-inf, -1).  The lists of one row must be disjoint and each sorted in that order (true when id_map
 * ascends along every list).  Rank counting: every output slot is written once, no atomics, deterministic. */
long cx_search_window_ws_bytes(int M, int k);
int cx_search_window_topk(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, int k,
                          const int64_t* min_id, const int64_t* end_id, const int64_t* excl_ptr, const int64_t* excl_ids,
                          const float* below, void* ws, float* out_scores, int64_t* out_ids, void* stream);
int cx_topk_merge_lists(const float* scores, const int64_t* ids, long P, int k, const int64_t* src, int M, int L,
                        const int64_t* id_map, long N, float* out_scores, int64_t* out_ids, void* stream);
/* ---- rank of target columns in the rows of the similarity matrix (zero-shot top-k accuracy, retrieval recall@k:
 *          sc/trainers/image_text.py:198-254; csrc/rank.hip).  Additive: cx_abi_version stays 10. ------------------------------
 * Q, D, d, ldq, ldd, N: as cx_search_topk (same alignment rules and error codes).  tgt_ptr:(M+1) / tgt_ids: int64 CSR lists
 * of target ids per query row (device memory; offsets from 0; ids in [0, N) -- the caller checks them before the call; a row
 * may be empty or repeat an id).  For entry e of row m with t = tgt_ids[e]:  out_score[e] = s(m, t)  and
 * out_rank[e] = #{ n in [0, N) : s(m,n) > s(m,t) or (s(m,n) == s(m,t) and n < t) }, the 0-based position of t in
 * cx_search_topk's order, with the bits cx_search_topk gives s(m, t).  The (M,N) scores are never written.  The result does
 * not depend on nsplit (<= 0: chosen); deterministic, no atomics.  ws: 16-B aligned, cx_rank_ws_bytes(M, N, nnz, nsplit)
 * bytes with nnz = tgt_ptr[M], need not be initialised.  M == 0 or N == 0 launches nothing and succeeds. */
long cx_rank_ws_bytes(int M, long N, long nnz, int nsplit);
int cx_rank_targets(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const int64_t* tgt_ptr,
                    const int64_t* tgt_ids, int nsplit, void* ws, int32_t* out_rank, float* out_score, void* stream);
/* ---- exact range search: every document above a per-row bound (faiss IndexFlatIP.range_search; near-duplicate removal,
 *          decontamination, per-row radius queries; csrc/range.hip).  Additive: cx_abi_version stays 10. ----------------------
 * Q, D, d, ldq, ldd, N: as cx_search_topk (same alignment rules and error codes).  radius:(M) fp32, min_id:(M) int64 or NULL
 * (= -1 everywhere), device memory.  Row m admits document n iff s(m,n) > radius[m] (strict) and n > min_id[m], with the bits
 * cx_search_topk gives s(m,n); a NaN radius admits nothing, -inf every finite score.  The (M,N) scores are never written.
 * cx_range_count: counts:(M) int64 = the number of admitted n per row; it also leaves in ws what cx_range_emit needs (partial
 * counts per corpus split, one flag per (query tile, corpus tile) that holds an admitted pair).  Corpus tiles that end at or
 * below the smallest min_id of a 128-row query tile are not computed.
 * cx_range_emit: same arguments, same nsplit, ws as cx_range_count left it; lims:(M+1) int64 = the exclusive prefix sum of
 * counts (computed by the caller, who can refuse the total first).  Row m's admitted (score, id) pairs go to
 * out_scores / out_ids [lims[m], lims[m+1]) in ASCENDING id order; unflagged tiles are not recomputed.
 * Neither result depends on nsplit (<= 0: chosen), on query batching or on scheduling; deterministic, no global atomics.
 * ws: 16-B aligned, cx_range_ws_bytes(M, N, nsplit) bytes, need not be initialised.  M == 0 or N == 0 launches nothing and
 * succeeds. */
long cx_range_ws_bytes(int M, long N, int nsplit);
int cx_range_count(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
                   const int64_t* min_id, int nsplit, void* ws, int64_t* counts, void* stream);
int cx_range_emit(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
                  const int64_t* min_id, int nsplit, const void* ws, const int64_t* lims, float* out_scores, int64_t* out_ids,
                  void* stream);
/* The same search with a WINDOW of ids per row (cluster-scoped near-duplicate search over label-sorted rows: min_id = the row's
 * own position, end_id = its cluster's end; any partition; "neighbours before row r").  Additive: cx_abi_version stays 10.
 * end_id:(M) int64 device memory or NULL (= N everywhere), clamped to [0, N].  Row m admits n iff s(m,n) > radius[m] (strict)
 * and min_id[m] < n < end_id[m]; a NaN radius admits nothing, -inf every id of the window, a window with
 * end_id <= min_id + 1 nothing.  Operands, alignment rules, error codes, the two-pass contract, the output layout (ascending
 * ids per row, unflagged tiles skipped) and the independence of nsplit / batching / scheduling are those of cx_range_count /
 * cx_range_emit; deterministic, no global atomics.
 * The band: query tile tm (rows 128 tm ..) walks corpus tiles [t0, t1) only, t0 = (min min_id + 1) / 128 and
 * t1 = ceil(max end_id / 128) over its rows with a non-empty window (no such row: nothing).  The workspace holds one flag word
 * per band tile: band_ptr:(ceil(M / 128) + 1) int64 DEVICE memory = the exclusive prefix sum of t1 - t0, band_tiles = its last
 * entry, read by the caller.  A walk is cut to band_ptr[tm + 1] - band_ptr[tm] tiles and band_ptr is clamped to
 * [0, band_tiles]: arrays inconsistent with each other give wrong results, never an access outside ws.
 * nsplit divides a query tile's band (<= 0: chosen from the query tiles and the mean band; thousands of query tiles: 1).
 * ws: 16-B aligned, cx_range_window_ws_bytes(M, N, band_tiles, nsplit) bytes -- partial counts + 4 bytes per band tile,
 * nothing proportional to tiles_m x tiles_n -- need not be initialised.  A NULL band_ptr or band_tiles < 0: CX_ERR_ARG. */
long cx_range_window_ws_bytes(int M, long N, long band_tiles, int nsplit);
int cx_range_window_count(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
                          const int64_t* min_id, const int64_t* end_id, const int64_t* band_ptr, long band_tiles, int nsplit,
                          void* ws, int64_t* counts, void* stream);
int cx_range_window_emit(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
                         const int64_t* min_id, const int64_t* end_id, const int64_t* band_ptr, long band_tiles, int nsplit,
                         const void* ws, const int64_t* lims, float* out_scores, int64_t* out_ids, void* stream);
/* ---- k-means over bf16 points: fused assignment and a deterministic centroid update (cluster-scoped curation, clustering
 *          evaluation, coarse quantisers; csrc/kmeans.hip).  Additive: cx_abi_version stays 10. ------------------------------
 * cx_kmeans_assign: X:(N,d) ldx points, C:(K,d) ldc centroids (alignment rules and d as cx_search_topk; N, K <= 2^31 - 129,
 * K >= 1), half_norm:(K) fp32 or NULL.  Per point: label = argmax_c s(x,c) - half_norm[c] (ties to the lower c), best = that
 * value, second:(N) or NULL = the second largest value (-inf for K == 1).  s(x,c) has the bits cx_search_topk gives the pair
 * (X as queries, C as corpus); the bias is subtracted once, in fp32.  No workspace.  N == 0 launches nothing and succeeds.
 * cx_kmeans_partial / cx_kmeans_finish: the update, from a plan the caller builds on the device.  order:(N) int32 = the point
 * ids sorted by label, stable (a cluster is a run of ascending ids); the runs are cut into PIECES of at most
 * CX_KMEANS_PIECE_ROWS entries: piece_start / piece_end:(max_pieces) int32 offsets into order, in run order; piece_ptr:(K+1)
 * int32 = cluster k owns pieces piece_ptr[k] : piece_ptr[k+1]; n_pieces:(1) int32 on the device = piece_ptr[K].  The grids are
 * sized by max_pieces >= n_pieces (ceil(N / CX_KMEANS_PIECE_ROWS) + K always is); workgroups past n_pieces exit.
 * partial:(max_pieces,d) fp32: row p = the sum of piece p's rows of X.  cx_kmeans_finish adds a cluster's partials in piece order
 * and writes counts:(K) int32, centroids:(K,d) fp32 (the mean; spherical != 0: the sum scaled to unit L2 norm), shadow:(K,d) lds
 * = the centroid rounded to bf16, half_norm:(K) = |shadow|^2 / 2 in fp32, summed over ascending dimension (spherical: 0).  An
 * empty cluster gets count 0 and keeps its centroid, shadow and half_norm.  No atomics: the summation order is a function of the
 * labels, N and d only, the result bitwise reproducible. */
#define CX_KMEANS_PIECE_ROWS 256
int cx_kmeans_assign(const uint16_t* X, const uint16_t* C, const float* half_norm, long N, long K, int d, long ldx, long ldc,
                     int32_t* label, float* best, float* second, void* stream);
int cx_kmeans_partial(const uint16_t* X, long N, int d, long ldx, const int32_t* order, const int32_t* piece_start,
                      const int32_t* piece_end, const int32_t* n_pieces, int max_pieces, float* partial, void* stream);
int cx_kmeans_finish(const float* partial, const int32_t* piece_start, const int32_t* piece_end, const int32_t* piece_ptr, long K,
                     int d, int max_pieces, int spherical, int32_t* counts, float* centroids, uint16_t* shadow, long lds,
                     float* half_norm, void* stream);
/* ---- retrieval metrics from target ranks (nDCG / MAP / recall / precision / MRR / hit rate at K cut-offs; trec_eval's
 *          ndcg_cut, map_cut, recall, P and BEIR's MRR; csrc/ir_metrics.hip).  Additive: cx_abi_version stays 10. -------------
 * row_ptr:(M+1) int64 offsets from 0, ranks / gains:(nnz) -- device memory, the CSR rows of cx_rank_targets with the ranks
 * widened to int64.  An entry with gain > 0 is a relevant document of that (linear) gain; an entry with gain == 0 is an
 * EXCLUDED document: it is taken out of the ranking.  Ranks within a row are distinct.  With R = the relevant entries of a row,
 *   a_j = rank_j - #{excluded e : rank_e < rank_j},  before_j = #{relevant i : a_i < a_j},
 *   ipos_j = #{relevant i : gain_i > gain_j or (gain_i == gain_j and i < j)},
 * and for cut-off k = ks[c] (ks: HOST memory, K in [1, 8], every k >= 1), out:(M, K, 6) double holds
 *   ndcg = sum_{a_j<k} gain_j / log2(a_j + 2) / sum_{ipos_j<k} gain_j / log2(ipos_j + 2),  ap = (1/R) sum_{a_j<k} (before_j + 1) / (a_j + 1),
 *   recall = hits / R,  precision = hits / k,  rr = 1 / (min_j a_j + 1) if that minimum is < k else 0,  hit = hits > 0,
 * hits = #{a_j < k}; nrel:(M) int = R.  A row with R == 0 gives zeros; a row of more than CX_IR_MAX_ROW entries is not staged:
 * it gives NaNs and nrel = -1.  fp64 sums in a fixed order, no atomics: bitwise reproducible.  One workgroup per row.
 * CX_ERR_SHAPE: K outside [1, 8], a k < 1, M < 0; CX_ERR_ARG: a null pointer (ks is looked at first); M == 0 launches nothing. */
#define CX_IR_MAX_ROW 4096
#define CX_IR_MAX_K 8
int cx_ir_metrics(const int64_t* row_ptr, const int64_t* ranks, const float* gains, int M, const int* ks, int K, double* out,
                  int* nrel, void* stream);
/* ---- binary (sign-bit) index with exact re-scoring (faiss IndexBinaryFlat, sentence-transformers "ubinary"; the recipes
 *          with `hamming: true`; csrc/search_binary.hip).  Additive: cx_abi_version stays 10. ---------------------------------
 * Sign codes: out:(rows, d/8) bytes, leading dimension ldo BYTES, in the layout of numpy.packbits(x > 0, axis=1) (dimension 0
 * = bit 7 of byte 0; +-0 and NaN give bit 0).  X:(rows,d) with leading dimension ldx ELEMENTS, dtype 0 = fp32, 1 = bf16.
 * d % 64 == 0, 64 <= d <= 1024. */
int cx_pack_sign_bits(const void* X, int dtype, long rows, int d, long ldx, uint8_t* out, long ldo, void* stream);
/* Hamming top-k over packed codes, argument for argument cx_search_topk: Qc:(M,d/8) ldq and Dc:(N,d/8) ldd bytes (leading
 * dimensions in BYTES, % 8 == 0, pointers 8-B aligned: CX_ERR_ALIGN), d = the number of BITS.  Per query row the k smallest
 * distances in ascending order, ties to the lower id, padded with (INT32_MAX, -1): out_dist:(M,k) int32, out_ids:(M,k) int64.
 * excl_ptr / excl_ids as there; max_dist:(M) int32 = INCLUSIVE upper bound on the distance (NULL = none).  The result does
 * not depend on nsplit; ws: 16-B aligned, cx_search_hamming_ws_bytes(M, N, k, nsplit) bytes.  The distances come off the matrix
 * cores (codes expanded to +-64 int8 in the kernel, v_mfma_i32_16x16x64_i8, exact); deterministic, no atomics. */
long cx_search_hamming_ws_bytes(int M, long N, int k, int nsplit);
int cx_search_hamming_topk(const uint8_t* Qc, const uint8_t* Dc, int M, long N, int d, long ldq, long ldd, int k,
                           const int64_t* excl_ptr, const int64_t* excl_ids, const int32_t* max_dist, int nsplit, void* ws,
                           int32_t* out_dist, int64_t* out_ids, void* stream);
/* Exact re-scoring of candidate lists: Q:(M,d) ldq bf16, D:(R,d) ldd bf16, cand:(M,c) int64 row indices into D (entries < 0
 * or >= R are skipped), ids:(M,c) int64 = what to report for each candidate (NULL: the row index).  Per query the k best
 * candidates by (score descending, id ascending), padded with (-inf, -1); below:(M) fp32 = exclusive upper bound on the score
 * (NULL = none).  1 <= c <= 4096, 1 <= k <= min(c, 1024).  The score of a pair has the bits cx_search_topk gives that pair
 * (same instruction, same K order), so coarse search + re-scoring of every candidate equals the exact search. */
int cx_rescore_topk(const uint16_t* Q, const uint16_t* D, const int64_t* cand, const int64_t* ids, int M, long R, int d,
                    long ldq, long ldd, int c, int k, const float* below, float* out_scores, int64_t* out_ids,
                    void* stream);
/* ---- int8 scalar-quantised index (sentence-transformers "int8", faiss SQ8 with one range per row; csrc/quantize_int8.hip,
 *          csrc/search.hip).  Additive: cx_abi_version stays 10. ------------------------------------------------------------
 * cx_quantize_rows_int8: X:(rows,d) with leading dimension ldx ELEMENTS, dtype 0 = fp32, 1 = bf16 (cx_pack_sign_bits'
 * operands; X aligned to its element).  out:(rows,d) int8, leading dimension ldo BYTES % 16 == 0, 16-B aligned; scale:(rows)
 * fp32.  Per row: amax = max_j |x_j| in fp32; amax < 2^-100: codes 0, scale 0; otherwise inv = 127.0f / amax,
 * scale = amax / 127.0f (IEEE divisions), code_j = clamp(rint(x_j * inv), -127, 127) (fp32 product, half to even; never -128).
 * Non-finite input is never an out-of-bounds access; NaN elements are skipped by the maximum and get code -127, an infinite
 * element makes the row's scale inf (finite elements 0, infinite ones -127).  d % 64 == 0, 64 <= d <= 1024. */
int cx_quantize_rows_int8(const void* X, int dtype, long rows, int d, long ldx, int8_t* out, long ldo, float* scale,
                          void* stream);
/* Top-k over such codes, cx_search_topk argument for argument with these differences: Q:(M,d) ldq and D:(N,d) ldd int8, leading
 * dimensions in BYTES, each >= d and % 16 == 0, pointers 16-B aligned (CX_ERR_ALIGN); q_scale:(M) and d_scale:(N) fp32.
 * The score of (m, n):  acc = sum_j Q[m][j] D[n][j] (int32, exact: v_mfma_i32_16x16x64_i8; |acc| <= 127^2 * 1024 < 2^24),
 * s = ((float)acc * d_scale[n]) * q_scale[m] -- two fp32 multiplications in that order, no FMA.  k, the exclusion CSR, below
 * (a strict upper bound on s), nsplit (no effect on the result), the order (s descending, id ascending), the (-inf, -1) padding,
 * the error codes, N == 0 and M == 0: as cx_search_topk.  ws: 16-B aligned, cx_search_int8_ws_bytes(M, N, k, nsplit) bytes. */
long cx_search_int8_ws_bytes(int M, long N, int k, int nsplit);
int cx_search_int8_topk(const int8_t* Q, const int8_t* D, const float* q_scale, const float* d_scale, int M, long N, int d,
                        long ldq, long ldd, int k, const int64_t* excl_ptr, const int64_t* excl_ids, const float* below,
                        int nsplit, void* ws, float* out_scores, int64_t* out_ids, void* stream);
/* The int8 scan of an IVF index (faiss IndexIVFScalarQuantizer, QT_8bit with one range per row).  Additive: cx_abi_version
 * stays 10.  cx_search_int8_topk's operands, score definition, alignment rules and refusals (d % 64 == 0 in [64, 1024], k <= 1024,
 * byte leading dimensions % 16, 16-B aligned pointers, non-null scales) with cx_search_window_topk's window: row m admits
 * document n only if min_id[m] < n < end_id[m] (min_id clamped to [-1, N], end_id to [0, N]; NULL = -1 / N everywhere; a row
 * with end_id <= min_id + 1 has an empty window and is all padding).  A query tile walks the corpus tiles [t0, t1) of its rows'
 * non-empty windows in one workgroup, as there.  Order (s descending, id ascending), (-inf, -1) padding, ids reported as
 * positions, M == 0 and N == 0: as cx_search_window_topk.  ws: 16-B aligned, cx_search_int8_window_ws_bytes(M, k)
 * (== cx_search_window_ws_bytes(M, k)) bytes, need not be initialised.  No value of the window arrays, exclusions or scales
 * causes an access outside the operands; results under non-finite scales are unspecified. */
long cx_search_int8_window_ws_bytes(int M, int k);
int cx_search_int8_window_topk(const int8_t* Q, const int8_t* D, const float* q_scale, const float* d_scale, int M, long N,
                               int d, long ldq, long ldd, int k, const int64_t* min_id, const int64_t* end_id,
                               const int64_t* excl_ptr, const int64_t* excl_ids, const float* below, void* ws,
                               float* out_scores, int64_t* out_ids, void* stream);
/* ---- product-quantised index (faiss IndexPQ, 8 bits per sub-quantiser; csrc/pq.hip, csrc/search.hip).  Additive:
 *          cx_abi_version stays 10. ---------------------------------------------------------------------------------------
 * A row of width d (% 64 == 0 in [64, 1024]) is cut into m = d / dsub sub-vectors, dsub in {8, 16, 32, 64} (CX_ERR_SHAPE
 * otherwise); sub-quantiser s has 256 centroids.  Codebooks: masters:(m,256,dsub) fp32, shadow:(m,256,dsub) bf16 = the
 * masters rounded to nearest even, 16-B aligned, half_norm:(m,256) fp32.  Only the shadow encodes, decodes and scores.  Every
 * step below is one correctly rounded fp32 operation in the order given (tests/pq_ref.py is the contract).
 * cx_pq_half_norm: half_norm[s][c] = 0.5f * h, h = 0, h = fmaf(c_j, c_j, h) for j ascending over the bf16 centroid.
 * cx_pq_assign: X:(n,d) bf16, leading dimension ldx ELEMENTS >= d.  Per row and s: acc = 0, acc = fmaf(x_j, c_j, acc) for j
 * ascending over the sub-vector, score = acc - half_norm[s][c]; code = the arg-max over c, ties to the lower c.  codes:(n,m)
 * uint8, byte leading dimension ldc >= m, any alignment (ldc == m is legal for every m).  A code is in [0, 256) whatever the
 * input; results under non-finite input are otherwise unspecified.
 * cx_pq_update (the second half of a Lloyd step, n <= 2^24): per (s, c) the fp32 sum of the sub-vectors of the rows whose code
 * is c, added element-wise in ASCENDING ROW ORDER; masters[s][c] = sum / count where count > 0, an empty cell keeps its
 * master; shadow and half_norm of every cell are rewritten.  Deterministic, no atomics.
 * Both: n == 0 is CX_OK without a launch (cx_pq_update then leaves shadow and half_norm alone). */
int cx_pq_half_norm(const uint16_t* shadow, int d, int dsub, float* half_norm, void* stream);
int cx_pq_assign(const uint16_t* X, long n, int d, long ldx, const uint16_t* shadow, const float* half_norm, int dsub,
                 uint8_t* codes, long ldc, void* stream);
int cx_pq_update(const uint16_t* X, long n, int d, long ldx, const uint8_t* codes, long ldc, int dsub, float* masters,
                 uint16_t* shadow, float* half_norm, void* stream);
/* Top-k over such codes: cx_search_topk argument for argument with (codes, codebook, dsub, ldc) in place of (D, ldd).
 * Document n is the concatenation of codebook[s][codes[n][s]], s < m; codebook = the bf16 shadow, 16-B aligned
 * (CX_ERR_ALIGN); codes:(N,m) uint8, byte leading dimension ldc >= m (CX_ERR_ALIGN), any alignment.  The score of (m, n) has
 * the bits cx_search_topk gives query m and the decoded row n (the same MFMAs in the same K order), so the whole result is
 * cx_search_topk's over the decoded corpus: k, the exclusion CSR, below, nsplit (no effect on the result), the order, the
 * (-inf, -1) padding, the error codes, N == 0 and M == 0 as there.  ws: 16-B aligned, cx_search_pq_ws_bytes(M, N, k, nsplit)
 * (== cx_search_ws_bytes) bytes.  A code is a byte, so no value of codes reads outside the codebook. */
long cx_search_pq_ws_bytes(int M, long N, int k, int nsplit);
int cx_search_pq_topk(const uint16_t* Q, const uint8_t* codes, const uint16_t* codebook, int M, long N, int d, int dsub,
                      long ldq, long ldc, int k, const int64_t* excl_ptr, const int64_t* excl_ids, const float* below,
                      int nsplit, void* ws, float* out_scores, int64_t* out_ids, void* stream);
/* backward of  coef * sum_i loss_rows[i]:  Gm[i][j] = coef*scale*(softmax_ij - [j==label_i]) is written to
 * Gmat:(N,G) and GmatT:(G,N) fp32 scratch; dQ:(N,dim) = Gm D, dD:(G,dim) = Gm^T Q (overwritten);
 * dscale_accum (may be NULL): += coef * sum_ij (softmax_ij - y_ij) * (Q D^T)_ij   (d loss / d scale).
 * QT:(dim,N) and DT:(dim,G) fp32 scratch for the K-contiguous operands of the two output GEMMs.
 * Requirements: dim % 4 == 0, N % 4 == 0, G % 4 == 0, ldq/ldd % 4 == 0. */
int cx_infonce_bwd(const float* Q, const float* D, const int64_t* labels, const float* lse, float scale, float coef,
                   float* Gmat, float* GmatT, float* QT, float* DT, float* dQ, float* dD, float* dscale_accum,
                   int N, int G, int dim, int ldq, int ldd, void* stream);
/* ---- fused similarity-KL: the `kd` term of the distillation trainer (sc/trainers/distill.py:347-355)
 * F.kl_div(log_softmax(s), softmax(t), reduction="batchmean") * N, row by row, for t = inv_temp * Qt Dt^T (teacher) and
 * s = inv_temp * Qs Ds^T (student):  kl_rows[i] = sum_j p_ij (t_ij - s_ij) - lse_t[i] + lse_s[i],  p = softmax_j t.
 * Qs:(N,dim_s) ldqs, Ds:(G,dim_s) ldds, Qt:(N,dim_t) ldqt, Dt:(G,dim_t) lddt fp32; the widths are independent.  Both products
 * of a 128 x 128 tile run on the exact-fp32 MFMA path of cx_infonce_fwd in one kernel; neither (N,G) matrix is written, no
 * atomics (a repeated call gives the same bits; identical student and teacher operands give kl_rows == 0 exactly).
 * ws: cx_simkl_ws_floats(N,G) floats.  Outputs: lse_s, lse_t, kl_rows:(N) fp32 (natural log).  The host takes sum / N.
 * Requirements: dim_s % 4 == 0, dim_t % 4 == 0 (CX_ERR_SHAPE), every leading dimension % 4 == 0 (CX_ERR_ALIGN).
 * Additive: cx_abi_version stays 10. */
long cx_simkl_ws_floats(int N, int G);
int cx_simkl_fwd(const float* Qs, const float* Ds, const float* Qt, const float* Dt, float inv_temp, float* ws,
                 float* lse_s, float* lse_t, float* kl_rows, int N, int G, int dim_s, int dim_t, int ldqs, int ldds,
                 int ldqt, int lddt, void* stream);
/* backward of  coef * sum_i kl_rows[i]  with respect to the student only (the teacher is a constant, and so is inv_temp: no
 * scale gradient, hence no atomic):  Gm[i][j] = coef * inv_temp * (q_ij - p_ij), q = softmax_j s, is written to Gmat:(N,G) and
 * GmatT:(G,N) fp32 scratch; dQs:(N,dim_s) = Gm Ds, dDs:(G,dim_s) = Gm^T Qs (overwritten).  QsT:(dim_s,N), DsT:(dim_s,G) fp32
 * scratch.  lse_s / lse_t: what cx_simkl_fwd wrote.  Requirements of the forward, and N % 4 == 0, G % 4 == 0 (CX_ERR_SHAPE). */
int cx_simkl_bwd(const float* Qs, const float* Ds, const float* Qt, const float* Dt, const float* lse_s,
                 const float* lse_t, float inv_temp, float coef, float* Gmat, float* GmatT, float* QsT, float* DsT,
                 float* dQs, float* dDs, int N, int G, int dim_s, int dim_t, int ldqs, int ldds, int ldqt, int lddt,
                 void* stream);
/* ---- the sequence-classification head (sc/models/encoder/modeling_nomic_bert.py:398-414 NomicBertPooler, 672-757
 * NomicBertForSequenceClassification): pooled = tanh(X Wp^T + bp); h = dropout(pooled, p); logits = h Wc^T + bc; then
 *   mode 0  cross-entropy: labels:(B) int64, loss_rows[b] = lse(logits[b]) - logits[b][label]; a label outside [0, C) (-100, the
 *           ignore index, among them) gives the row loss 0 and no gradient;
 *   mode 1  MSE: labels:(B, C) fp32, loss_rows[b] = mean_c (logits[b][c] - labels[b][c])^2.
 * The host takes the mean (over the counted rows).  X:(B, d) fp32 with row stride ldx >= d, ldx % 4 == 0 (the engine's cls-pooled,
 * un-normalised output); Wp:(d, d), bp:(d), Wc:(C, d), bc:(C) fp32.  Outputs pooled:(B, d), logits:(B, C), loss_rows:(B) fp32;
 * labels == NULL: logits only.  The dropout mask is dropout_keep4 of (seed, offset) over element b * d + j and is regenerated by
 * the backward, never stored; p = 0 is no dropout.  fp32 accumulation, no atomics, every sum in one fixed order: a repeated call
 * gives the same bits.  d in {256, 512, 768, 1024}, 1 <= C <= 8, 1 <= B <= 4096 (CX_ERR_SHAPE); a NULL required pointer, a mode
 * other than 0 / 1 or p outside [0, 1): CX_ERR_ARG; neither launches anything.  Two launches forward, two backward.
 * Additive: cx_abi_version stays 10. */
long cx_seqcls_ws_floats(int B, int d, int C);
int cx_seqcls_head_fwd(const float* X, long ldx, const float* Wp, const float* bp, const float* Wc, const float* bc,
                       const void* labels, int mode, float p, unsigned long long seed, unsigned long long offset, float* pooled,
                       float* logits, float* loss_rows, int B, int d, int C, void* stream);
/* backward of  coef * sum_b loss_rows[b]:  dWp:(d, d), dbp:(d), dWc:(C, d), dbc:(C), dX:(B, d) fp32 are OVERWRITTEN (dX is the demb
 * of cx_encoder_backward_typed).  pooled / logits: what the forward wrote; ws: cx_seqcls_ws_floats(B, d, C) floats. */
int cx_seqcls_head_bwd(const float* X, long ldx, const float* Wp, const float* Wc, const float* pooled, const float* logits,
                       const void* labels, int mode, float coef, float p, unsigned long long seed, unsigned long long offset,
                       float* ws, long ws_floats, float* dWp, float* dbp, float* dWc, float* dbc, float* dX, int B, int d, int C,
                       void* stream);
/* ---- image crop + resize + normalize of the image-text data path (sc/dataset/transform.py: RandomResizedCrop(S, BICUBIC) or
 * Resize(S, BICUBIC) + CenterCrop(S), then ToTensor + Normalize, which the reference runs with torchvision on PIL images).
 * pixels: one ragged device buffer of HWC uint8 RGB images; image b starts at byte offsets[b] (any alignment) and is
 * sizes[2b] rows x sizes[2b+1] columns.  plan_i[4b..] = (y_lo, y_hi, x_lo, x_hi): the clamp range [lo, hi) of the taps per axis;
 * plan_f[4b..] = (y_origin, y_scale, x_origin, x_scale), float64: output pixel o of an axis is centred at
 * origin + (o + 0.5) * scale source pixels.  The arithmetic is PIL's BICUBIC (a = -0.5, support 2 * max(scale, 1), weights
 * normalised per output pixel): the horizontal pass is rounded half up and clamped to 0..255, the vertical pass runs on those
 * 8-bit values and is rounded and clamped again, then out[b][c][y][x] = (level / 255 - mean[c]) / std[c], (B, 3, S, S) fp32
 * (out_bf16 = 0) or bf16 (out_bf16 = 1).  One launch for the whole batch, the 8-bit intermediate stays in LDS; no atomics, a
 * repeated call gives the same bits.  offsets (B + 1 entries, the last = the end of image B - 1), sizes, plan_i and plan_f are
 * PINNED HOST memory (hipHostMalloc / torch pin_memory): the call reads them on the host -- the served-range check and the
 * launch plan come from them -- and the kernel reads the same bytes through their device mapping, so they must stay unchanged
 * until the launch has completed; pageable or device memory there is CX_ERR_ARG.  mean3 / std3: three host floats each.
 * Served: 1 <= S <= 512, source sides 1..8192, 0 <= lo < hi <= side, scale in (0, 16] per axis (an upsample has no lower limit:
 * its support stays at 2 source pixels), the first and last centre within one `scale` of [lo, hi], and offsets[b + 1] -
 * offsets[b] >= 3 * h * w; anything else is CX_ERR_SHAPE.  A NULL pointer or B <= 0: CX_ERR_ARG.  Neither launches anything.
 * Additive: cx_abi_version stays 10. */
int cx_image_transform(const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, const int32_t* plan_i,
                       const double* plan_f, void* out, int out_bf16, int B, int S, const float* mean3, const float* std3,
                       void* stream);
/* ---- masked-language-model masking on the device (transformers.DataCollatorForLanguageModeling.torch_mask_tokens, the collator
 * of sc/trainers/mlm.py:70,84; contrastors_amd/mlm_data.py): ids (B, S) int32 (ids_i64 = 0) or int64 (ids_i64 = 1) with a row
 * stride of ids_stride >= S elements -> out_ids, labels (B, S) int64, contiguous.  attention_mask (B, S) int64 and special_mask
 * (B, S) uint8 are contiguous and may be NULL; special_ids is a DEVICE array of n_special <= 16 int64 token ids (NULL when 0).
 * The token at flat position g = b * S + s takes one Philox4x32-10 call, counter (lo32(g), hi32(g), lo32(offset), hi32(offset)),
 * key (lo32(seed), hi32(seed)) -> (u0, u1, u2, u3).  A token is special if its attention mask is 0, its special_mask is
 * non-zero or its id is in special_ids.  A non-special token is a target iff u0 < T(p), T(x) = (uint32) fminf(x * 2^32,
 * 4294967040.f); a target becomes mask_token_id iff u1 < T(0.8), else the word (uint64(u2) * random_vocab) >> 32 iff
 * u1 < T(0.9), else keeps its id (u3 is unused).  labels = the original id at targets, -100 elsewhere; out_ids = ids at
 * non-targets.  The result is a pure function of (seed, offset, g, id, specialness): not of the launch geometry, the dtype of
 * ids or its stride; a repeated call gives the same bits.  random_vocab is len(tokenizer), not the padded model vocabulary.
 * out_ids / labels must not overlap the inputs.  B or S < 1, n_special outside 0..16, random_vocab < 1, p outside [0, 1) or
 * ids_stride < S: CX_ERR_SHAPE; a NULL ids / out_ids / labels (or special_ids with n_special > 0): CX_ERR_ARG.  Neither
 * launches anything.  No allocation, no synchronisation.  Additive: cx_abi_version stays 10. */
int cx_mlm_mask(const void* ids, int ids_i64, long ids_stride, const int64_t* attention_mask, const uint8_t* special_mask,
                const int64_t* special_ids, int n_special, long mask_token_id, int random_vocab, float p,
                unsigned long long seed, unsigned long long offset, int64_t* out_ids, int64_t* labels, int B, int S,
                void* stream);
/* ---- the same loss on the fp8 matrix-core path (BASELINE.json configs[4] "fp8 MFMA similarity GEMM"; the reference
 * only carries the `use_fp8` flag, configs/train/contrastive_pretrain.yaml:24).  Rows are quantised to OCP e4m3 with
 * one scale per row, the contraction is v_mfma_scale_f32_32x32x64_f8f6f4 (fp32 accumulate, online fp32 log-sum-exp);
 * the logits are never written.  dim in {256,512,768,1024}.  Scratch, all caller-owned: ws = fp32
 * [cx_infonce_fp8_ws_floats(N,G)]; Q8 (N,dim) / D8 (G,dim) bytes and sq (N) / sd (G) row scales are WRITTEN by fwd and
 * read again by bwd.  bwd writes GmT (G,N) bf16 = coef*scale*(softmax - onehot)^T once and forms dD = GmT Q, dQ = GmT^T D
 * on the bf16 GEMM family (Qb (N,dim), QbT (dim,N), Db (G,dim) bf16 scratch; gws / gws_floats = split-K workspace as for
 * cx_gemm_bf16_tn_accum, >= N*dim floats).  bwd needs N % 256 == 0, G % 64 == 0, dim % 128 == 0 (else CX_ERR_SHAPE:
 * use the exact path).  Tolerance against the fp32 oracle (tests/test_infonce_fp8_gpu.py): e4m3 has 3 mantissa bits. */
long cx_infonce_fp8_ws_floats(int N, int G);
int cx_infonce_fp8_fwd(const float* Q, const float* D, const int64_t* labels, float scale, float* ws, uint8_t* Q8,
                       uint8_t* D8, float* sq, float* sd, float* lse, float* loss_rows, int N, int G, int dim, int ldq,
                       int ldd, void* stream);
int cx_infonce_fp8_bwd(const float* Q, const float* D, const int64_t* labels, const float* lse, float scale, float coef,
                       const uint8_t* Q8, const uint8_t* D8, const float* sq, const float* sd, uint16_t* GmT, uint16_t* Qb,
                       uint16_t* QbT, uint16_t* Db, float* gws, long gws_floats, float* dQ, float* dD,
                       float* dscale_accum, int N, int G, int dim, int ldq, int ldd, void* stream);
/* plain exact-fp32 MFMA GEMM  C[m][n] = sum_k A[m][k] B[n][k]  (K % 4 == 0; lda, ldb % 4 == 0).  Each element has the bits of
 * the fp32 fmaf chain from +0 over k in blocks of 16, inside a block in the order 0 4 1 5 2 6 3 7 8 12 9 13 10 14 11 15; the
 * zero-filled steps of a K tail (K % 16 != 0) add +0, so a sum that underflows to -0 comes out as +0 there. */
int cx_sgemm_nt(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                void* stream);
int cx_transpose_f32(const float* In, float* Out, int rows, int cols, int ld_in, int ld_out, void* stream);

/* ---- native encoder engine (a10-a17: NomicBertModel / NomicBertEncoder / Block / FlashAttention / (Gated)MLP,
 *      sc/models/encoder/modeling_nomic_bert.py:307-395,515-587; sc/layers/block.py:389-463) -----------------
 * One call enqueues a whole chunk forward (embeddings -> L post-norm blocks -> pool -> normalize) or backward on
 * `stream`.  All memory is described by the caller in CxEncoderDesc / CxChunkBuffers. */
typedef struct CxLayerWeights {
    const uint16_t* Wqkv;   /* (3d, d) bf16 */
    const uint16_t* Wout;   /* (d, d) */
    const uint16_t* Wfc1;   /* gated: (2I, d) fc11/fc12 rows interleaved by 32;  plain MLP: (I, d) */
    const uint16_t* Wfc2;   /* (d, I) */
    const uint16_t* WqkvT;  /* transposed bf16 shadows for dgrad: (d, 3d) */
    const uint16_t* WoutT;  /* (d, d) */
    const uint16_t* Wfc1T;  /* (d, 2I) or (d, I) */
    const uint16_t* Wfc2T;  /* (I, d) */
    const float* bqkv;      /* fp32 biases or NULL (nomic-bert has none) */
    const float* bout;
    const float* bfc1;
    const float* bfc2;
    const float* ln1_g; const float* ln1_b; const float* ln2_g; const float* ln2_b;
    /* fp32 gradient accumulators (same shapes as the fp32 master parameters) */
    float* gWqkv; float* gWout; float* gWfc1; float* gWfc2;
    float* gbqkv; float* gbout; float* gbfc1; float* gbfc2;
    float* gln1_g; float* gln1_b; float* gln2_g; float* gln2_b;
} CxLayerWeights;

typedef struct CxEncoderDesc {
    int n_layer, d, n_head, d_inner, gated; /* gated=1: SwiGLU GatedMLP; 0: GELU(erf) MLP */
    int vocab, max_pos, padding_idx;
    float ln_eps, softmax_scale;
    const float* word_emb; const float* type_emb; const float* pos_emb; /* fp32 masters; pos_emb NULL for rotary */
    const float* emb_ln_g; const float* emb_ln_b;
    float* gword_emb; float* gtype_emb; float* gpos_emb; float* gemb_ln_g; float* gemb_ln_b;
    const float* rot_cos; const float* rot_sin; /* NULL when rotary_emb_fraction == 0 */
    const CxLayerWeights* layers;              /* HOST array of n_layer entries (device pointers inside) */
    int pool_mode, normalize;
    /* ---- pre-norm trunks (sc/layers/block.py:293-388) and the ViT image tower (sc/models/vit/vit.py:176-276) ---- */
    int prenorm;                               /* 0: post-norm blocks (BERT family); 1: pre-norm blocks + final LN */
    const float* lnf_g; const float* lnf_b;    /* final LayerNorm ln_f (prenorm only) */
    float* glnf_g; float* glnf_b;
    const uint16_t* Wpatch;                    /* ViT: bf16 (d, patch_dim) patch projection; NULL for text trunks */
    const float* bpatch;                       /* fp32[d] or NULL */
    const float* cls_token;                    /* fp32[d] */
    const float* vit_pos;                      /* fp32 (n_patch + 1, d) */
    float* gWpatch; float* gbpatch; float* gcls_token; float* gvit_pos;
    int patch_dim;                             /* C * p * p */
    /* dropout (post-norm text trunks; 0 = off, the BASELINE configs): on every sub-layer output before the residual add
     * (resid_pdrop, sc/layers/block.py:422-431,453-462) and on the embedding-LayerNorm output (embd_pdrop).  Applied when
     * CxChunkBuffers.drop_active != 0 (training mode). */
    float resid_pdrop, embd_pdrop;
    float attn_pdrop;   /* dropout on the attention probabilities (attn_pdrop, sc/layers/attention.py:158-182); text trunks */
    /* ---- the OpenAI-CLIP flavour of the image tower (sc/models/vit/clip.py:14-58; round 3) ---- */
    int mlp_act;                                   /* plain MLP activation: 0 exact-erf GELU, 1 quick_gelu (cx_gemm_bf16_bias_act) */
    const float* lnpre_g; const float* lnpre_b;    /* `prepre_layernom` (sc/models/vit/vit.py:128-132,180): LayerNorm on the */
    float* glnpre_g; float* glnpre_b;              /* embeddings ahead of the first block; NULL = none */
} CxEncoderDesc;

/* Per-chunk activation arena (device memory owned by the caller).  save_for_backward = 0 lets every layer reuse
 * the layer-0 slots (GradCache pass 1, sc/loss.py:135-146); = 1 keeps per-layer slots (pass 2, loss.py:149-161). */
typedef struct CxChunkBuffers {
    long T_cap;                 /* capacity in tokens of every per-token buffer (>= round_up(T,128)) */
    uint16_t* h0;               /* (T,d) embedding-LN output */
    float* emb_mean; float* emb_rstd;
    /* per layer, n_layer slots each (slot stride = T_cap * width elements): */
    uint16_t* qkv;              /* (T,3d) */
    uint16_t* ctx;              /* (T,d) attention output (pre out_proj) */
    float* lse;                 /* (H,T) */
    uint16_t* z1;               /* (T,d) attn_out + residual (LN1 input) */
    uint16_t* h1;               /* (T,d) LN1 output */
    float* mean1; float* rstd1;
    uint16_t* yg;               /* (T,I) per slot: what fc1 keeps for backward -- the biased pre-activation (plain MLP) or the
                                 * gate alone (gated MLP, cx_abi_version >= 6; it was the (T,2I) (y, gate) pair before) */
    uint16_t* act;              /* (T,I) */
    uint16_t* z2;               /* (T,d) */
    uint16_t* h2;               /* (T,d) LN2 output = layer output */
    float* mean2; float* rstd2;
    float* pool_norm;           /* (B) */
    /* backward scratch (single slot each): */
    uint16_t* g_a; uint16_t* g_b; uint16_t* g_c;   /* (T,d) gradient ping-pong buffers */
    uint16_t* g_wide;           /* (T, max(3d, 2I)) */
    uint16_t* g_act;            /* (T, I) */
    uint16_t* tr_a; uint16_t* tr_b; /* transposed operands for wgrad: (max(3d,2I), T_cap) each.  Only the fallback for feature
                                     * counts that are not multiples of 256 uses them (cx_gemm_bf16_tn_accum declines those
                                     * shapes); may be NULL otherwise (cx_abi_version >= 8) -- 24.6 KB per token at d = 768 */
    float* delta;               /* (H,T) */
    float* ws_f32;              /* split-K workspace for the wgrad GEMMs */
    long ws_floats;
    /* pre-norm trunks: input of / output of the final LayerNorm (single slot), its statistics */
    uint16_t* zf; uint16_t* hf; float* meanf; float* rstdf;
    /* ViT front end: patchified pixels (Bc*n_patch rounded up to 64 rows, patch_dim) and their projection (.., d);
     * patch_proj doubles as the gradient of the projection in backward */
    uint16_t* patch_in; uint16_t* patch_proj;
    /* activation checkpointing (sc/models/encoder/modeling_nomic_bert.py:339-365 gradient_checkpointing,
     * sc/models/vit/vit.py:200-231): != 0 -> a saving forward keeps ONE (T,d) tensor per block -- `h2` (post-norm: the
     * block's output = the next block's input) or `z1` (pre-norm: the residual stream at LN1) has n_layer slots, every
     * other per-layer buffer has a single slot -- and backward recomputes each block from it before differentiating
     * it.  Results are bit-identical to checkpoint = 0; the arena shrinks from ~25 KB to ~1.5 KB per token and layer. */
    int checkpoint;
    /* dropout state of the chunk, set by the host before the forward and read again by the backward: Philox (seed, offset)
     * drawn from the torch generator (so RandContext replays it), the on/off switch, and one more (T,d) gradient buffer
     * (the LayerNorm backward returns two different gradients once a mask sits between x0 and the sum). */
    int drop_active;
    unsigned long long drop_seed, drop_offset;
    uint16_t* g_d;
    /* Optional (NULL = none): HOST array of n_layer + 1 hipEvent_t.  A backward call records layer_events[l] on `stream`
     * right after the last kernel that writes block l's parameter gradients (blocks run L-1 ... 0), and
     * layer_events[n_layer] after the embedding (text) / patch-projection (ViT) gradients, i.e. at the end of the call.
     * The data-parallel gradient reduction of a step's LAST backward starts on block l's slice of the flat gradient as
     * soon as its event fires, overlapped with the blocks still differentiating -- what DDP's bucket hooks do for the
     * reference (sc/trainers/text_text.py:163-170). */
    void* const* layer_events;
    /* image towers with a pre-LayerNorm (CxEncoderDesc.lnpre_g): its input, (T, d), kept for backward; statistics in
     * emb_mean / emb_rstd (the slots the text trunk's embedding LayerNorm uses) */
    uint16_t* zpre;
    /* selective activation checkpointing (cx_abi_version >= 6; meaningful with checkpoint != 0): the TOP ckpt_keep blocks
     * (l >= n_layer - ckpt_keep) keep all their intermediates -- every per-layer buffer then has 1 + ckpt_keep slots, slot 0
     * shared by the recomputed blocks, slot 1 + l - (n_layer - ckpt_keep) owned by kept block l -- and backward recomputes
     * only the blocks below them.  0 = the reference's behaviour (every block recomputed).  A memory knob like
     * `checkpoint` itself: results are bit-identical for every value (tests/test_checkpoint_gpu.py). */
    int ckpt_keep;
    /* PatchDropout of the image tower (cx_abi_version >= 7; sc/layers/embedding.py:415-418, 519-557): NULL = every patch.
     * patch_keep: (Bc, n_keep) int32 device array, the patch indices (0 .. n_patch - 1) each image keeps, in the order their
     * tokens take in the sequence ([cls] first, then patch_keep[b][0 .. n_keep - 1]); patch_inv: (Bc, n_patch) int32, position
     * of a patch among its image's kept ones or -1.  Only the kept patches are gathered, projected and run through the blocks:
     * sequences have n_keep + 1 tokens, cu_seqlens = multiples of n_keep + 1, cx_vit_backward takes n_patch = n_keep;
     * n_patch_all = (H / patch) * (W / patch), the row count of patch_inv (the backward does not see the image size). */
    const int32_t* patch_keep;
    const int32_t* patch_inv;
    int n_keep;
    int n_patch_all;
} CxChunkBuffers;

/* input_ids:(Bc,S) int64 padded batch rows of this chunk; indices:(T) int32; cu_seqlens:(Bc+1) int32.
 * emb_out:(Bc,d) fp32. */
int cx_encoder_forward(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const int64_t* input_ids,
                       const int32_t* indices, const int32_t* cu_seqlens, int Bc, int S, int T, int max_seqlen,
                       int save_for_backward, float* emb_out, void* stream);
/* demb:(Bc,d) fp32 cached embedding gradient (GradCache surrogate, sc/loss.py:158-161). Accumulates every
 * parameter gradient in enc->g* / layers[i].g*.  Must follow a forward with save_for_backward = 1 on `buf`. */
int cx_encoder_backward(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const int64_t* input_ids,
                        const int32_t* indices, const int32_t* cu_seqlens, int Bc, int S, int T, int max_seqlen,
                        const float* demb, const float* emb_out, const int32_t* sort_ids, const int32_t* sort_perm,
                        void* stream);
/* sort_ids / sort_perm (both int32[T], or both NULL): the chunk's token ids in ascending stable order and the permutation
 * that sorts them -- with them the word-embedding gradient is a deterministic segmented reduction
 * (cx_embed_ln_bwd_sorted), without them fp32 atomics. */

/* The pooled pair with token-type ids (sentence-pair tasks): token_type_ids:(Bc,S) int64 segment ids 0 / 1, NULL = the pair
 * above, bit for bit.  enc->type_emb / gtype_emb are the (2, d) table and its gradient.  Routed to cx_embed_ln_*_typed. */
int cx_encoder_forward_typed(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const int64_t* input_ids,
                             const int64_t* token_type_ids, const int32_t* indices, const int32_t* cu_seqlens, int Bc, int S,
                             int T, int max_seqlen, int save_for_backward, float* emb_out, void* stream);
int cx_encoder_backward_typed(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const int64_t* input_ids,
                              const int64_t* token_type_ids, const int32_t* indices, const int32_t* cu_seqlens, int Bc, int S,
                              int T, int max_seqlen, const float* demb, const float* emb_out, const int32_t* sort_ids,
                              const int32_t* sort_perm, void* stream);

/* Token-level variant for heads that read every position (the MLM head of NomicBertForPreTraining,
 * sc/models/encoder/modeling_nomic_bert.py:590-669): hidden_out / dhidden are (T, d) bf16 in unpadded token order
 * (row t = token indices[t] of the padded batch).  Same arenas, same contracts as the pooled pair above. */
int cx_encoder_forward_hidden(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const int64_t* input_ids,
                              const int32_t* indices, const int32_t* cu_seqlens, int Bc, int S, int T, int max_seqlen,
                              int save_for_backward, uint16_t* hidden_out, void* stream);
int cx_encoder_backward_hidden(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const int64_t* input_ids,
                               const int32_t* indices, const int32_t* cu_seqlens, int Bc, int S, int T, int max_seqlen,
                               const uint16_t* dhidden, const int32_t* sort_ids, const int32_t* sort_perm, void* stream);

/* ---- ViT image tower (sc/models/vit/vit.py:176-276 ViTModel.forward, sc/layers/embedding.py:465-516
 *      PatchEmbedding.forward, sc/models/biencoder/modeling_biencoder.py:287-319 pooling): one call per chunk.
 * pixels: (Bc, C, H, W) fp32 or bf16 (pixels_bf16 != 0) device tensor; n_patch = (H/p)*(W/p); sequences have
 * n_patch + 1 tokens ([cls] first); cu_seqlens: (Bc+1) int32 = multiples of n_patch + 1.  desc->prenorm selects the
 * block order (ViT-B/16: 1), desc->Wpatch etc. must be set.  backward accumulates every parameter gradient. */
int cx_vit_patchify(const void* pixels, int pixels_bf16, uint16_t* patches, int B, int C, int H, int W, int patch,
                    void* stream);
int cx_vit_assemble_fwd(const uint16_t* proj, const float* cls_token, const float* pos_embed, uint16_t* out, int B,
                        int P, int d, void* stream);
int cx_vit_assemble_bwd(const uint16_t* dz, uint16_t* dproj, float* gcls, float* gpos, int B, int P, int d,
                        void* stream);
/* the same three with a patch subset (PatchDropout, see CxChunkBuffers.patch_keep): keep (B, n_keep) / inv (B, P_all) int32
 * device arrays, NULL = the plain forms above; with keep, P = n_keep in the assemble calls */
int cx_vit_patchify_gather(const void* pixels, int pixels_bf16, uint16_t* patches, int B, int C, int H, int W, int patch,
                           const int32_t* keep, int n_keep, void* stream);
int cx_vit_assemble_fwd_gather(const uint16_t* proj, const float* cls_token, const float* pos_embed, uint16_t* out, int B,
                               int P, int d, const int32_t* keep, void* stream);
int cx_vit_assemble_bwd_gather(const uint16_t* dz, uint16_t* dproj, float* gcls, float* gpos, int B, int P, int d,
                               const int32_t* inv, int P_all, void* stream);
int cx_vit_forward(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const void* pixels, int pixels_bf16,
                   const int32_t* cu_seqlens, int Bc, int C, int H, int W, int patch, int save_for_backward,
                   float* emb_out, void* stream);
int cx_vit_backward(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const int32_t* cu_seqlens, int Bc,
                    int n_patch, const float* demb, const float* emb_out, void* stream);
/* Token-level twins (as cx_encoder_forward_hidden / _backward_hidden for the text trunk): hidden_out / dhidden are the
 * (Bc * (n_patch + 1), d) bf16 hidden states after ln_f and their gradient -- for poolers that live above the C-ABI
 * (sc/models/biencoder/modeling_biencoder.py:93-156 MultiHeadAttentionPooling, `pooling: map` of the vision recipes). */
int cx_vit_forward_hidden(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const void* pixels, int pixels_bf16,
                          const int32_t* cu_seqlens, int Bc, int Cc, int H, int W, int patch, int save_for_backward,
                          uint16_t* hidden_out, void* stream);
int cx_vit_backward_hidden(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const int32_t* cu_seqlens, int Bc, int n_patch,
                           const uint16_t* dhidden, void* stream);

/* ---- EVA-02 image tower (sc/models/vit/timm_vit.py:71-95 `vit_eva02_base_patch16_224`, the image tower of the
 *      nomic-embed-vision-v1.5 recipe): 2-D RoPE on q / k, SwiGLU with fc1 biases and a LayerNorm inside the MLP, no final
 *      LayerNorm.  Additive to ABI 10: the plain ViT entry points above are unchanged. ----------------------------------
 * cx_rope2d_qkv_inplace: rotates q and k of a packed (T, 3 * n_head * 64) bf16 qkv in place, interleaved pairs (2j, 2j+1)
 *   (RotaryEmbeddingCat / apply_rot_embed_cat, sc/layers/embedding.py:297-360): x * cos + rot(x) * sin, rot(x) = (-x1, x0),
 *   fp32 math, one rounding.  Token t of sequence b (cu_seqlens[b] <= t < cu_seqlens[b + 1]) at offset s uses row s - n_prefix
 *   of the fp32 (n_rope, 32) tables; offsets < n_prefix (the [cls] token) and rows >= n_rope stay untouched, V always.
 *   sign = -1: the inverse rotation = the backward on dq / dk of a (T, 3d) gradient buffer. */
int cx_rope2d_qkv_inplace(uint16_t* qkv, const int32_t* cu_seqlens, const float* rope_cos, const float* rope_sin, int n_rope,
                          int B, int n_head, int T, int n_prefix, int sign, void* stream);
/* GatedMLP with norm_layer (sc/layers/mlp.py:37-83): yg (T, 2I) = the BIASED fc1 output in the interleaved-by-32 layout of the
 * fused fc1 weight; act = bf16(silu(gate) * y) (T, I), gate (T, I) plain column order (may be NULL: the no-grad pass), z =
 * bf16(LN(act) * gamma + beta) (T, I), mean / rstd (T) fp32 over the whole I-wide row.  I % 256 == 0 and I <= 4096
 * (CX_ERR_SHAPE otherwise). */
int cx_swiglu_subln_fwd(const uint16_t* yg, const float* gamma, const float* beta, uint16_t* gate, uint16_t* act, uint16_t* z,
                        float* mean, float* rstd, int T, int I, float eps, void* stream);
/* dz (T, I) = gradient of z -> dyg (T, 2I) interleaved; dgamma / dbeta (I) and dbias (2I, interleaved = the fused fc1 bias)
 * accumulate (+=; each may be NULL).  Per-block fp32 partials in ws (>= 4 I floats, up to 1024 x 4 I used) and a fixed-order
 * reduction: deterministic, no atomics.  Same shape rule as the forward. */
int cx_swiglu_subln_bwd(const uint16_t* dz, const uint16_t* act, const uint16_t* gate, const float* mean, const float* rstd,
                        const float* gamma, uint16_t* dyg, float* dgamma, float* dbeta, float* dbias, float* ws, long ws_floats,
                        int T, int I, void* stream);

typedef struct CxVitSubLN {
    const float* norm_g; const float* norm_b;   /* mlp.norm.weight / .bias, fp32 (I) */
    float* gnorm_g; float* gnorm_b;             /* their gradient accumulators (may be NULL) */
} CxVitSubLN;

/* What a block of the EVA-02 tower adds to CxEncoderDesc / CxChunkBuffers.  The host refreshes the arena pointers before each
 * call (the library reads the struct only while it enqueues). */
typedef struct CxVitExt {
    const float* rope_cos; const float* rope_sin;   /* fp32 (n_rope, 32) per patch, or NULL: no rotary */
    int n_rope, n_prefix;                           /* table rows; leading tokens not rotated ([cls]: 1) */
    int no_final_ln;                                /* != 0: hidden states = the residual stream after the last block */
    float subln_eps;                                /* eps of the LayerNorm inside the MLP (nn.LayerNorm default 1e-5) */
    const CxVitSubLN* sub_ln;                       /* HOST array of n_layer, or NULL: no sub-LN (the plain MLP path) */
    /* arena: per-layer slots (slot stride T_cap rows, the slot mapping of yg / act, single slot under checkpointing) */
    uint16_t* z;                                    /* (slots, T_cap, I) bf16 sub-LN output (the fc2 input) */
    float* zmean; float* zrstd;                     /* (slots, T_cap) */
    uint16_t* yg_wide;                              /* (T_cap, 2I) bf16 scratch for the biased fc1 output; NULL = g_wide */
} CxVitExt;

/* The four ViT entry points with an extension; ext == NULL is exactly the call without the suffix. */
int cx_vit_forward_ex(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const CxVitExt* ext, const void* pixels,
                      int pixels_bf16, const int32_t* cu_seqlens, int Bc, int C, int H, int W, int patch, int save_for_backward,
                      float* emb_out, void* stream);
int cx_vit_backward_ex(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const CxVitExt* ext, const int32_t* cu_seqlens, int Bc,
                       int n_patch, const float* demb, const float* emb_out, void* stream);
int cx_vit_forward_hidden_ex(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const CxVitExt* ext, const void* pixels,
                             int pixels_bf16, const int32_t* cu_seqlens, int Bc, int Cc, int H, int W, int patch,
                             int save_for_backward, uint16_t* hidden_out, void* stream);
int cx_vit_backward_hidden_ex(const CxEncoderDesc* enc, const CxChunkBuffers* buf, const CxVitExt* ext, const int32_t* cu_seqlens,
                              int Bc, int n_patch, const uint16_t* dhidden, void* stream);

/* ---- K12  fused softmax cross-entropy over a vocabulary-sized class axis (flash_attn.losses.cross_entropy.
 *      CrossEntropyLoss, csrc/xentropy; sc/models/encoder/modeling_nomic_bert.py:603-610).  logits: (N, V) bf16
 *      (logits_bf16 != 0) or fp32, row stride ld; labels int64[N] (== ignore_index -> loss 0, zero gradient).
 *      fwd: loss[i] = lse_i - s*logit[i][label_i], lse[i] = log sum_j exp(s*logit[i][j]), s = logit_scale.
 *      bwd: dlogits = dloss[i] * s * (softmax - onehot); dlogits may alias logits (inplace_backward). */
int cx_xent_fwd(const void* logits, int logits_bf16, const int64_t* labels, float* loss, float* lse, int N, int V,
                long ld, float logit_scale, long ignore_index, void* stream);
int cx_xent_bwd(const float* dloss, const void* logits, int logits_bf16, const float* lse, const int64_t* labels,
                void* dlogits, int N, int V, long ld, long ld_d, float logit_scale, long ignore_index, void* stream);

/* ---- fused optimizer tail of training_step (replaces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step as
 *      sc/trainers/base.py:362-385 and sc/optimizer.py:7-47 use them).  fp32, 16-B aligned contiguous buffers.
 *      cx_grad_sq_norm ADDS sum(grad^2) to *sq_norm_accum (device double, zeroed by the caller; call once per gradient
 *      tensor).  cx_adamw_clip_step applies one AdamW step (amsgrad off, decoupled decay, bias correction for the
 *      1-based `step`) to `param` using grad * min(1, max_norm / (sqrt(*sq_norm) + 1e-6)); sq_norm NULL or
 *      max_norm <= 0 = no clipping.  The clip coefficient is derived on the device: no host synchronisation. */
int cx_grad_sq_norm(const float* grad, long n, double* sq_norm_accum, void* stream);
int cx_adamw_clip_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, long step, const double* sq_norm, float max_norm,
                       void* stream);
/* EMA copy of the weights (sc/trainers/base.py:387-391 `self.model["ema"].update(model)`): ema = decay * ema + (1 - decay) *
 * param over a flat fp32 buffer, one pass; 16-B aligned, 0 <= decay <= 1. */
int cx_ema_update(float* ema, const float* param, long n, float decay, void* stream);


/* ---- one-shot exchange over xGMI (sc/distributed.py:5-12 gather_with_grad): receive buffers shared between the
 * per-GPU processes by HIP IPC, every rank stores its shard straight into every peer's buffer (all 7 links at once), one
 * flag exchange.  Host protocol: contrastors_amd/distributed.py::OneShotExchange.
 * cx_ipc_alloc: device memory that can be exported (uncached == 1: hipDeviceMallocUncached, for the flags; == 2: mapped
 *   coherent HOST memory, for the error flag the host polls without synchronising);
 * cx_ipc_export / cx_ipc_open: 64-byte hipIpcMemHandle_t in / mapped pointer out.
 * cx_xgmi_push: peer_bufs_dev[p] + dst_offset_bytes <- src[0 .. bytes) for p = 0 .. world-1 (device array of pointers).
 * cx_xgmi_scatter: peer_bufs_dev[p] + slot * slice_bytes <- src + p * slice_bytes (the reduce-scatter's send side).
 * cx_xgmi_signal_wait: peer_flags_dev[p][rank] = epoch for all p, then wait until my_flags[p] >= epoch for all p
 *   (system-scope release / acquire); gives up after max_spins polls and stores 1 + p in *err_flag (uncached memory).
 * cx_sum_slots_f32: out[i] = sum_w slots[w * n + i], n % 4 == 0.  All sizes / offsets multiples of 16 bytes. */
int cx_ipc_alloc(void** ptr, long bytes, int uncached);
int cx_ipc_free(void* ptr);
int cx_ipc_export(void* ptr, unsigned char* handle64);
int cx_ipc_open(const unsigned char* handle64, void** ptr);
int cx_ipc_close(void* ptr);
int cx_xgmi_push(const void* src, void* const* peer_bufs_dev, long dst_offset_bytes, long bytes, int world, void* stream);
int cx_xgmi_scatter(const void* src, void* const* peer_bufs_dev, int slot, long slice_bytes, int world, void* stream);
int cx_xgmi_signal_wait(unsigned int* const* peer_flags_dev, unsigned int* my_flags, int rank, int world, unsigned int epoch,
                        long max_spins, unsigned int* err_flag, void* stream);
int cx_sum_slots_f32(const float* slots, float* out, long n, int world, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CONTRASTORS_HIP_H */
