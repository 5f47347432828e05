// xent.hip -- K12: fused softmax cross-entropy over a vocabulary-sized class axis, forward and backward
// (flash_attn.losses.cross_entropy.CrossEntropyLoss, csrc/xentropy in the reference's dependency; call site
// sc/models/encoder/modeling_nomic_bert.py:603-610, `partial(CrossEntropyLoss, inplace_backward=True)`).
// HBM-bound: the forward reads every logit once (online max / sum-exp, one workgroup per row), the backward reads it
// once more and writes the gradient once -- in place when asked to (the 30528-way MLM logits are the largest tensor of
// that path).  Logits may be bf16 or fp32; statistics are fp32.
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

namespace {

constexpr int XB = 256;

template <typename T>
CX_DEVICE float ld_logit(const T* p, long i) {
    if constexpr (sizeof(T) == 4) return p[i];
    else return bf16_to_f32(p[i]);
}
template <typename T>
CX_DEVICE void st_logit(T* p, long i, float v) {
    if constexpr (sizeof(T) == 4) p[i] = v;
    else p[i] = f32_to_bf16(v);
}

CX_DEVICE void online_merge(float& m, float& s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    s = (mm == -INFINITY) ? 0.f : s * __expf(m - mm) + s2 * __expf(m2 - mm);
    m = mm;
}

// 16-byte vector access: 8 bf16 or 4 fp32 per lane when V and the row stride allow it (VEC elements), else scalar.
template <typename T, int VEC>
CX_DEVICE void ld_vec(const T* p, long i, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = ld_logit(p, i);
    } else if constexpr (sizeof(T) == 4) {
        const float4 u = *reinterpret_cast<const float4*>(p + i);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    } else {
        unpack8(*reinterpret_cast<const uint4*>(p + i), v);
    }
}
template <typename T, int VEC>
CX_DEVICE void st_vec(T* p, long i, const float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        st_logit(p, i, v[0]);
    } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *reinterpret_cast<uint4*>(p + i) = pack8(v);
    }
}

// loss[row] = lse - scale * logit[label]  (0 for ignored rows);  lse[row] = log sum_j exp(scale * logit_j)
template <typename T, int VEC>
__global__ __launch_bounds__(XB) void xent_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      float* __restrict__ loss, float* __restrict__ lse_out, int V,
                                                      long ld, float scale, long ignore_index) {
    const int row = blockIdx.x;
    const T* x = logits + (size_t)row * ld;
    float m = -INFINITY, s = 0.f;
    for (int j = threadIdx.x * VEC; j < V; j += XB * VEC) {
        float v[VEC];
        ld_vec<T, VEC>(x, j, v);
        float mm = m;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { v[e] *= scale; mm = fmaxf(mm, v[e]); }
        // every logit seen so far is -inf: s stays 0 (m - mm and v - mm would be -inf - -inf = NaN; online_merge guards the same case)
        if (mm != -INFINITY) {
            float acc = s * __expf(m - mm);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc += __expf(v[e] - mm);
            s = acc;
        }
        m = mm;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        online_merge(m, s, m2, s2);
    }
    __shared__ float sm[XB / 64], ss[XB / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[wave] = m; ss[wave] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float M = sm[0], S = ss[0];
#pragma unroll
        for (int w = 1; w < XB / 64; ++w) online_merge(M, S, sm[w], ss[w]);
        const float lse = M + __logf(S);
        lse_out[row] = lse;
        const long lab = labels[row];
        loss[row] = (lab == ignore_index || lab < 0 || lab >= V) ? 0.f : lse - ld_logit(x, lab) * scale;
    }
}

// dlogits[row][j] = dloss[row] * scale * (exp(scale * logit_j - lse) - [j == label]);  0 for ignored rows
template <typename T, int VEC>
__global__ __launch_bounds__(XB) void xent_bwd_kernel(const float* __restrict__ dloss, const T* logits,
                                                      const float* __restrict__ lse, const int64_t* __restrict__ labels,
                                                      T* dlogits, int V, long ld, long ldd, float scale,
                                                      long ignore_index) {
    const int row = blockIdx.x;
    const T* x = logits + (size_t)row * ld;
    T* dx = dlogits + (size_t)row * ldd;
    const long lab = labels[row];
    const bool ignored = (lab == ignore_index || lab < 0 || lab >= V);
    const float g = ignored ? 0.f : dloss[row] * scale;
    const float l = lse[row];
    for (int j = threadIdx.x * VEC; j < V; j += XB * VEC) {
        float v[VEC];
        if (ignored) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = 0.f;
        } else {
            ld_vec<T, VEC>(x, j, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                v[e] = __expf(v[e] * scale - l);
                if (j + e == lab) v[e] -= 1.f;
                v[e] *= g;
            }
        }
        st_vec<T, VEC>(dx, j, v);
    }
}

// launch(T{}, VEC) with the logit type and the vector width of one launch: 16-byte accesses when `vec16` (every base pointer
// is 16-byte aligned), V and both row strides allow them (the forward has one stride and passes it twice), else scalar
template <typename F>
void pick_kernel(int logits_bf16, bool vec16, int V, long ld, long ld_d, F launch) {
    if (logits_bf16) {
        if (vec16 && (V % 8) == 0 && (ld % 8) == 0 && (ld_d % 8) == 0) launch(bf16_t{}, std::integral_constant<int, 8>{});
        else launch(bf16_t{}, std::integral_constant<int, 1>{});
    } else {
        if (vec16 && (V % 4) == 0 && (ld % 4) == 0 && (ld_d % 4) == 0) launch(float{}, std::integral_constant<int, 4>{});
        else launch(float{}, std::integral_constant<int, 1>{});
    }
}

}  // namespace

extern "C" {

int cx_xent_fwd(const void* logits, int logits_bf16, const int64_t* labels, float* loss, float* lse, int N, int V,
                long ld, float logit_scale, long ignore_index, void* stream) {
    if (N <= 0) return CX_OK;
    if (!logits || !labels || !loss || !lse) return CX_ERR_ARG;
    if (V <= 0 || ld < V) return CX_ERR_SHAPE;
    const bool vec16 = ((uintptr_t)logits % 16) == 0;
    pick_kernel(logits_bf16, vec16, V, ld, ld, [&](auto t, auto vec) {
        using T = decltype(t);
        hipLaunchKernelGGL((xent_fwd_kernel<T, vec()>), dim3(N), dim3(XB), 0, (hipStream_t)stream, (const T*)logits, labels, loss,
                           lse, V, ld, logit_scale, ignore_index);
    });
    return done();
}

int cx_xent_bwd(const float* dloss, const void* logits, int logits_bf16, const float* lse, const int64_t* labels,
                void* dlogits, int N, int V, long ld, long ld_d, float logit_scale, long ignore_index, void* stream) {
    if (N <= 0) return CX_OK;
    if (!dloss || !logits || !lse || !labels || !dlogits) return CX_ERR_ARG;
    if (V <= 0 || ld < V || ld_d < V) return CX_ERR_SHAPE;
    const bool vec16 = ((uintptr_t)logits % 16) == 0 && ((uintptr_t)dlogits % 16) == 0;
    pick_kernel(logits_bf16, vec16, V, ld, ld_d, [&](auto t, auto vec) {
        using T = decltype(t);
        hipLaunchKernelGGL((xent_bwd_kernel<T, vec()>), dim3(N), dim3(XB), 0, (hipStream_t)stream, dloss, (const T*)logits, lse, labels,
                           (T*)dlogits, V, ld, ld_d, logit_scale, ignore_index);
    });
    return done();
}

}  // extern "C"
