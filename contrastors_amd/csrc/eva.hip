// eva.hip -- the three kernels the EVA-02 image tower adds to the ViT block (sc/models/vit/timm_vit.py:71-95 recipe of
// nomic-embed-vision-v1.5):
//   * 2-D rotary position embedding on q and k of the packed qkv, interleaved pairs (RotaryEmbeddingCat /
//     apply_rot_embed_cat, sc/layers/embedding.py:297-360; applied after the prefix tokens, sc/layers/attention.py:136-147);
//   * SwiGLU of the biased fc1 pre-activation followed by the LayerNorm inside the MLP (GatedMLP with norm_layer,
//     sc/layers/mlp.py:37-83), forward and backward;
// All three are one pass over HBM: 16 B per lane, fp32 math, one bf16 rounding per stored value.  The backward reduces its
// column sums (sub-LN gamma / beta, fc1 bias) through per-block fp32 partials and a fixed-order pass: deterministic.
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

namespace {

// ---- 2-D RoPE ------------------------------------------------------------------------------------------------------
// Block (bx, by): row y of the block owns token t = blockIdx.x * by + y, its bx threads walk the 8-column groups of [q | k]
// (4 rotation pairs of one head each).  Token t belongs to the sequence b with cu[b] <= t < cu[b + 1]; the search over
// cu_seqlens runs once per token (lane 0 of its row) and its result goes through LDS.  The offset s in the sequence selects
// table row s - n_prefix.  Prefix tokens and rows past the table are left alone, V is never touched.  sgn = +1:
// x * cos + rot(x) * sin with rot(x) = (-x1, x0) per pair; sgn = -1: the transposed rotation (the backward of the forward
// on dq / dk).  Products and the sum are rounded separately (no contraction into an FMA): the same fp32 operations the
// reference's python performs.
constexpr int ROPE_MAX_ROWS = 16;
__global__ __launch_bounds__(1024) void rope2d_kernel(bf16_t* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                      const float* __restrict__ cs, const float* __restrict__ sn, int n_rope,
                                                      int B, int d, long T, int n_prefix, float sgn) {
#pragma clang fp contract(off)
    __shared__ int row_of[ROPE_MAX_ROWS];
    const long t = (long)blockIdx.x * blockDim.y + threadIdx.y;
    if (threadIdx.x == 0) {
        int p = -1;
        if (t < T) {
            int lo = 0, hi = B;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (cu[mid] <= t) lo = mid;
                else hi = mid;
            }
            p = (int)(t - cu[lo]) - n_prefix;
        }
        row_of[threadIdx.y] = p;
    }
    __syncthreads();
    const int p = row_of[threadIdx.y];
    if (p < 0 || p >= n_rope) return;
    const int per = (2 * d) >> 3;
    for (int k = threadIdx.x; k < per; k += blockDim.x) {
        const int c = k * 8;
        const int j0 = (c & 63) >> 1;
        const float4 c4 = *reinterpret_cast<const float4*>(cs + (size_t)p * 32 + j0);
        const float4 s4 = *reinterpret_cast<const float4*>(sn + (size_t)p * 32 + j0);
        const float co[4] = {c4.x, c4.y, c4.z, c4.w};
        const float si[4] = {sgn * s4.x, sgn * s4.y, sgn * s4.z, sgn * s4.w};
        bf16_t* ptr = qkv + (size_t)t * 3 * d + c;
        float x[8], o[8];
        unpack8(*reinterpret_cast<const uint4*>(ptr), x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x0 = x[2 * j], x1 = x[2 * j + 1];
            o[2 * j] = x0 * co[j] + (-x1) * si[j];   // (fp contract off: two roundings of the products, one of the sum)
            o[2 * j + 1] = x1 * co[j] + x0 * si[j];
        }
        *reinterpret_cast<uint4*>(ptr) = pack8(o);
    }
}

// ---- SwiGLU + sub-LayerNorm ------------------------------------------------------------------------------------------
// One workgroup per row, one thread per 8 columns of the I-wide activation (blockDim = round_up(I / 8, 64) <= 512).
// Row sums: wave sums, then the waves' partials in a fixed order (deterministic, no atomics).
CX_DEVICE float2 block_sum2(float a, float b, float2* red) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = make_float2(a, b);
    __syncthreads();
    float2 s = make_float2(0.f, 0.f);
    for (int k = 0; k < nw; ++k) {
        s.x += red[k].x;
        s.y += red[k].y;
    }
    __syncthreads();   // (red is reused by the next call)
    return s;
}

// a = bf16(silu(gate) * y), z = LN_I(a) * gamma + beta.  The statistics are taken over the ROUNDED a (what the next op of the
// reference reads), two passes in registers.
__global__ __launch_bounds__(512) void swiglu_subln_fwd_kernel(const bf16_t* __restrict__ yg, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, bf16_t* __restrict__ gate_out,
                                                               bf16_t* __restrict__ act_out, bf16_t* __restrict__ z_out,
                                                               float* __restrict__ mean_o, float* __restrict__ rstd_o, int I,
                                                               float eps) {
    __shared__ float2 red[8];
    const long t = blockIdx.x;
    const int c = threadIdx.x * 8;
    const bool has = c < I;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (has) {
        const bf16_t* row = yg + t * (2L * I);
        const uint4 gu = *reinterpret_cast<const uint4*>(row + gcol(c, I, 1));
        float y[8], g[8], o[8];
        unpack8(*reinterpret_cast<const uint4*>(row + ycol(c, I, 1)), y);
        unpack8(gu, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = g[e] * sigmoid_fast(g[e]) * y[e];
        const uint4 au = pack8(o);
        *reinterpret_cast<uint4*>(act_out + t * (long)I + c) = au;
        if (gate_out) *reinterpret_cast<uint4*>(gate_out + t * (long)I + c) = gu;
        unpack8(au, a);
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += a[e];
    const float mean = block_sum2(s, 0.f, red).x / (float)I;
    float v = 0.f;
    if (has) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v += (a[e] - mean) * (a[e] - mean);
    }
    const float rstd = rsqrtf(block_sum2(v, 0.f, red).x / (float)I + eps);
    if (has) {
        float gg[8], bb[8], z[8];
        load8_f32(gamma + c, gg);
        load8_f32(beta + c, bb);
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (a[e] - mean) * rstd * gg[e] + bb[e];
        *reinterpret_cast<uint4*>(z_out + t * (long)I + c) = pack8(z);
    }
    if (threadIdx.x == 0) {
        mean_o[t] = mean;
        rstd_o[t] = rstd;
    }
}

// Backward.  Block b owns the contiguous rows [b * rows_per, min(T, (b + 1) * rows_per)) and keeps, per thread, the column
// sums of its 8 columns: d gamma, d beta and the fc1 bias gradient (the bf16 dy / d gate it stores, summed in fp32).  They go
// to ws[b][4I] = [d gamma (I) | d beta (I) | d bias (2I, interleaved layout)].
__global__ __launch_bounds__(512) void swiglu_subln_bwd_kernel(const bf16_t* __restrict__ dz, const bf16_t* __restrict__ act,
                                                               const bf16_t* __restrict__ gate, const float* __restrict__ mean_i,
                                                               const float* __restrict__ rstd_i, const float* __restrict__ gamma,
                                                               bf16_t* __restrict__ dyg, float* __restrict__ ws, long T, int I,
                                                               long rows_per) {
    __shared__ float2 red[8];
    const int c = threadIdx.x * 8;
    const bool has = c < I;
    const long r0 = (long)blockIdx.x * rows_per;
    const long r1 = r0 + rows_per < T ? r0 + rows_per : T;
    float gg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (has) load8_f32(gamma + c, gg);
    float acc_g[8], acc_b[8], acc_y[8], acc_t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc_g[e] = acc_b[e] = acc_y[e] = acc_t[e] = 0.f;
    for (long t = r0; t < r1; ++t) {
        float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
              g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (has) {
            unpack8(*reinterpret_cast<const uint4*>(dz + t * (long)I + c), d);
            unpack8(*reinterpret_cast<const uint4*>(act + t * (long)I + c), a);
            unpack8(*reinterpret_cast<const uint4*>(gate + t * (long)I + c), g);
        }
        const float mu = mean_i[t], rs = rstd_i[t];
        float xh[8], dxh[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            xh[e] = (a[e] - mu) * rs;
            dxh[e] = d[e] * gg[e];
            s1 += dxh[e];
            s2 += dxh[e] * xh[e];
        }
        const float2 s = block_sum2(s1, s2, red);
        const float m1 = s.x / (float)I, m2 = s.y / (float)I;
        if (!has) continue;
        float dy[8], dg[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc_g[e] += d[e] * xh[e];
            acc_b[e] += d[e];
            const float da = rs * (dxh[e] - m1 - xh[e] * m2);
            swiglu_bwd_from_act(da, a[e], g[e], dy[e], dg[e]);
        }
        const uint4 yu = pack8(dy), gu = pack8(dg);
        bf16_t* orow = dyg + t * (2L * I);
        *reinterpret_cast<uint4*>(orow + ycol(c, I, 1)) = yu;
        *reinterpret_cast<uint4*>(orow + gcol(c, I, 1)) = gu;
        unpack8(yu, dy);
        unpack8(gu, dg);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc_y[e] += dy[e];
            acc_t[e] += dg[e];
        }
    }
    if (!has) return;
    float* w = ws + (size_t)blockIdx.x * 4 * I;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        w[c + e] = acc_g[e];
        w[I + c + e] = acc_b[e];
        w[2 * I + ycol(c, I, 1) + e] = acc_y[e];
        w[2 * I + gcol(c, I, 1) + e] = acc_t[e];
    }
}

// fixed-order sum of the nb partial vectors (4I floats each) into the three accumulators (+=; NULL = skipped)
__global__ __launch_bounds__(256) void swiglu_subln_reduce_kernel(const float* __restrict__ ws, int nb, int I,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                  float* __restrict__ dbias) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 4 * I) return;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s += ws[(size_t)b * 4 * I + j];
    if (j < I) {
        if (dgamma) dgamma[j] += s;
    } else if (j < 2 * I) {
        if (dbeta) dbeta[j - I] += s;
    } else if (dbias) {
        dbias[j - 2 * I] += s;
    }
}

inline bool subln_width_ok(int I) { return I > 0 && I <= 4096 && (I % 256) == 0; }

}  // namespace

extern "C" {

int cx_rope2d_qkv_inplace(uint16_t* qkv, const int32_t* cu_seqlens, const float* rope_cos, const float* rope_sin, int n_rope,
                          int B, int n_head, int T, int n_prefix, int sign, void* stream) {
    if (B <= 0 || T <= 0) return CX_OK;
    if (!qkv || !cu_seqlens || !rope_cos || !rope_sin || n_rope <= 0 || n_prefix < 0 || (sign != 1 && sign != -1))
        return CX_ERR_ARG;
    if (n_head <= 0) return CX_ERR_SHAPE;
    const int d = n_head * 64;
    // a row of threads per token (d = 768: 192 lanes), as many tokens per block as fill ~768 threads
    const int per = (2 * d) >> 3;
    const int bx = per < 256 ? (per + 63) / 64 * 64 : 256;
    int by = 768 / bx;
    if (by < 1) by = 1;
    if (by > ROPE_MAX_ROWS) by = ROPE_MAX_ROWS;
    hipLaunchKernelGGL(rope2d_kernel, dim3((unsigned)((T + by - 1) / by)), dim3(bx, by), 0, (hipStream_t)stream, qkv, cu_seqlens,
                       rope_cos, rope_sin, n_rope, B, d, (long)T, n_prefix, (float)sign);
    return done();
}

int cx_swiglu_subln_fwd(const uint16_t* yg, const float* gamma, const float* beta, uint16_t* gate, uint16_t* act, uint16_t* z,
                        float* mean, float* rstd, int T, int I, float eps, void* stream) {
    if (T <= 0) return CX_OK;
    if (!yg || !gamma || !beta || !act || !z || !mean || !rstd) return CX_ERR_ARG;
    if (!subln_width_ok(I)) return CX_ERR_SHAPE;
    const int threads = ((I / 8) + 63) / 64 * 64;
    hipLaunchKernelGGL(swiglu_subln_fwd_kernel, dim3((unsigned)T), dim3(threads), 0, (hipStream_t)stream, yg, gamma, beta, gate,
                       act, z, mean, rstd, I, eps);
    return done();
}

int cx_swiglu_subln_bwd(const uint16_t* dz, const uint16_t* act, const uint16_t* gate, const float* mean, const float* rstd,
                        const float* gamma, uint16_t* dyg, float* dgamma, float* dbeta, float* dbias, float* ws, long ws_floats,
                        int T, int I, void* stream) {
    if (T <= 0) return CX_OK;
    if (!dz || !act || !gate || !mean || !rstd || !gamma || !dyg || !ws) return CX_ERR_ARG;
    if (!subln_width_ok(I)) return CX_ERR_SHAPE;
    // partial count: a function of (T, I, workspace) only, so a repeated call sums in the same order
    long nb = ws_floats / (4L * I);
    if (nb > 1024) nb = 1024;
    if (nb > T) nb = T;
    if (nb < 1) return CX_ERR_ARG;
    const long rows_per = (T + nb - 1) / nb;
    nb = (T + rows_per - 1) / rows_per;
    const int threads = ((I / 8) + 63) / 64 * 64;
    hipLaunchKernelGGL(swiglu_subln_bwd_kernel, dim3((unsigned)nb), dim3(threads), 0, (hipStream_t)stream, dz, act, gate, mean,
                       rstd, gamma, dyg, ws, (long)T, I, rows_per);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(swiglu_subln_reduce_kernel, dim3((unsigned)((4 * I + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws,
                       (int)nb, I, dgamma, dbeta, dbias);
    return done();
}

}  // extern "C"
