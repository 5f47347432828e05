// quantize_int8.hip -- per-row symmetric int8 scalar quantisation (sentence-transformers "int8", faiss SQ8 with one range per
// row): the storage format of Int8FlatIndex / cx_search_int8_topk (search.hip).  Per row x of width d:
//   amax = max_j |x_j| (fp32; bf16 widened exactly);  amax < 2^-100: a zero row, codes 0 and scale 0;  otherwise
//   inv = 127.0f / amax,  scale = amax / 127.0f (IEEE fp32 divisions),  code_j = clamp(rint(x_j * inv), -127, 127)
// with an fp32 product and round-half-to-even; -128 is never produced.  Every step is one correctly rounded fp32 operation, so
// the bytes are those of the same formula in numpy (tests/int8_ref.py).
// A group of G = 16 / 32 / 64 lanes owns a row (64 / G rows per wave for d <= 128); a lane holds up to four quads of
// consecutive elements in registers across the one pass: load, |max| over the group by xor shuffles, scale, pack four codes into a
// dword, store.  Non-finite input: a NaN element is skipped by the maximum and gets code -127; an infinite element makes
// amax = inf, inv = 0 and scale = inf, finite elements of that row get code 0 and the infinite ones -127.  No value is used as an
// index, so nothing is read or written out of bounds whatever the input.
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

namespace {

template <typename T, bool VEC> CX_DEVICE void load_quad(const T* p, float (&v)[4]) {
    if constexpr (sizeof(T) == 4) {
        if constexpr (VEC) {
            const float4 t = *reinterpret_cast<const float4*>(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = p[e];
        }
    } else {
        if constexpr (VEC) {
            const uint2 t = *reinterpret_cast<const uint2*>(p);
            v[0] = bf16lo_to_f32(t.x); v[1] = bf16hi_to_f32(t.x); v[2] = bf16lo_to_f32(t.y); v[3] = bf16hi_to_f32(t.y);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = bf16_to_f32(p[e]);
        }
    }
}

CX_DEVICE uint32_t code_of(float x, float inv) {
    const float c = fminf(fmaxf(rintf(__fmul_rn(x, inv)), -127.f), 127.f);   // (a NaN product comes out as -127)
    return (uint32_t)(int)c & 0xffu;
}

// lg = log2(G); d / 4 <= 4 G quads per row
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const T* __restrict__ X, long ldx, long rows, int d, int lg,
                                                            int8_t* __restrict__ out, long ldo, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63, G = 1 << lg, sub = lane >> lg, j = lane & (G - 1);
    const int rpw = 64 >> lg, nq = d >> 2;
    const long nwaves = (long)gridDim.x * 4;
    for (long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw; r0 < rows; r0 += nwaves * rpw) {   // (wave-uniform)
        const long row = r0 + sub;
        const bool live = row < rows;
        float v[4][4];
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = j + (i << lg);
            if (live && q < nq) {
                load_quad<T, VEC>(X + row * ldx + 4 * q, v[i]);
#pragma unroll
                for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(v[i][e]));
            }
        }
        for (int off = G >> 1; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
        const bool zero = amax < 0x1p-100f;
        const float inv = zero ? 0.f : __fdiv_rn(127.0f, amax);
        const float sc = zero ? 0.f : __fdiv_rn(amax, 127.0f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = j + (i << lg);
            if (live && q < nq) {
                const uint32_t w = zero ? 0u
                                        : code_of(v[i][0], inv) | (code_of(v[i][1], inv) << 8) | (code_of(v[i][2], inv) << 16) |
                                              (code_of(v[i][3], inv) << 24);
                *reinterpret_cast<uint32_t*>(out + row * ldo + 4 * q) = w;
            }
        }
        if (live && j == 0) scale[row] = sc;
    }
}

template <typename T, bool VEC>
void launch(const void* X, long ldx, long rows, int d, int8_t* out, long ldo, float* scale, hipStream_t s) {
    const int quads = d / 4;
    const int lg = quads <= 16 ? 4 : quads <= 32 ? 5 : 6;
    const long waves = (rows + (64 >> lg) - 1) / (64 >> lg);
    const int grid = (int)min((waves + 3) / 4, 1L << 16);
    hipLaunchKernelGGL((quantize_rows_kernel<T, VEC>), dim3(grid), dim3(256), 0, s, (const T*)X, ldx, rows, d, lg, out, ldo, scale);
}

}  // namespace

extern "C" {

int cx_quantize_rows_int8(const void* X, int dtype, long rows, int d, long ldx, int8_t* out, long ldo, float* scale,
                          void* stream) {
    if (rows < 0 || d < 64 || d > 1024 || (d % 64) != 0) return CX_ERR_SHAPE;
    if (dtype != 0 && dtype != 1) return CX_ERR_ARG;
    if (rows == 0) return CX_OK;
    if (!X || !out || !scale) return CX_ERR_ARG;
    if (ldx < d || ldo < d || (ldo % 16) != 0 || ((uintptr_t)out & 15)) return CX_ERR_ALIGN;
    if (((uintptr_t)X & (dtype == 0 ? 3 : 1)) != 0) return CX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    // four elements per load where every quad is aligned for it, element loads otherwise
    const bool vec = (ldx % 4) == 0 && ((uintptr_t)X & (dtype == 0 ? 15 : 7)) == 0;
    if (dtype == 0) {
        if (vec) launch<float, true>(X, ldx, rows, d, out, ldo, scale, s);
        else launch<float, false>(X, ldx, rows, d, out, ldo, scale, s);
    } else {
        if (vec) launch<bf16_t, true>(X, ldx, rows, d, out, ldo, scale, s);
        else launch<bf16_t, false>(X, ldx, rows, d, out, ldo, scale, s);
    }
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

}  // extern "C"
